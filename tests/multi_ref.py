"""A plain reference for main-trace programs with joint COUNT columns (one multiplicity column for several looked-up values, the _multi
entry points): Python integers, one cell at a time.  It shares nothing with MainProgram.evaluate - no numpy, no vectorised op, no
call into the builder beyond reading its lists (ops [(op, a, b)], consts, cols [(kind, num_op, den_op, pad)], periodic_cols).

It knows what the programs of multi_programs hold: ops 0 LOAD, 1 CONST, 2 ADD, 3 SUB, 4 MUL and 6 PERIODIC; VALUE columns without a
denominator, LIMB columns, and COUNT columns of both forms.  A joint column (bit 8 of its pad) is a dictionary of counts over all X_k,
placed on the first row of each table value; a key at or above 2^key_bits raises KeyOutOfRange."""

P = 2**251 + 17 * 2**192 + 1
VALUE, COUNT, LIMB = 0, 6, 8
NO_DEN = 0xFFFFFFFF
LIST_BIT, LIST_END, ALSO = 256, 0xFFFF, 12


class KeyOutOfRange(Exception):
    pass


def list_of(ops, cell):
    """The looked-up values of the list that starts at the op 12 `cell`: X_0 is its a, X_1 the a of its b, and so on."""
    xs = []
    while cell != LIST_END:
        op, a, cell = ops[cell]
        assert op == ALSO
        xs.append(a)
    return xs


def main_table(m, rows):
    """The whole main table, n x main_cols Python ints, of the MainProgram m from its input rows."""
    n, first = len(rows), m.input_cols
    table = [[int(v) % P for v in r] + [None] * len(m.cols) for r in rows]

    def value(t, i, memo):
        if (t, i) in memo:
            return memo[t, i]
        op, a, b = m.ops[t]
        if op == 0:
            v = table[(i + a) % n][b]
            assert v is not None, "a LOAD of a column that is not built yet"
        elif op == 1:
            v = m.consts[a] % P
        elif op == 2:
            v = (value(a, i, memo) + value(b, i, memo)) % P
        elif op == 3:
            v = (value(a, i, memo) - value(b, i, memo)) % P
        elif op == 4:
            v = value(a, i, memo) * value(b, i, memo) % P
        elif op == 6:
            column = m.periodic_cols[b]
            v = int(column[(i + a) % len(column)]) % P
        else:
            raise AssertionError(f"op {t} has the code {op}, which this reference does not know")
        memo[t, i] = v
        return v

    for k, (kind, num_op, den_op, pad) in enumerate(m.cols):
        memo, col = {}, first + k
        if kind == COUNT:
            x_ops, key_bits = (list_of(m.ops, num_op), pad & 255) if pad & LIST_BIT else ([num_op], pad)
            counts = {}
            for x_op in x_ops:
                for j in range(n):
                    key = value(x_op, j, memo)
                    if key >> key_bits:
                        raise KeyOutOfRange(f"X (op {x_op}) on row {j}")
                    counts[key] = counts.get(key, 0) + 1
            seen = set()
            for i in range(n):
                key = value(den_op, i, memo)
                if key >> key_bits:
                    raise KeyOutOfRange(f"T on row {i}")
                table[i][col] = 0 if key in seen else counts.get(key, 0)
                seen.add(key)
        elif kind == LIMB:
            lo, width = pad & 255, (pad >> 8) & 255
            for i in range(n):
                table[i][col] = (value(num_op, i, memo) >> lo) & ((1 << width) - 1)
        elif kind == VALUE and den_op == NO_DEN:
            for i in range(n):
                table[i][col] = value(num_op, i, memo)
        else:
            raise AssertionError(f"derived column {k} has kind {kind}, which this reference does not know")
    return table
