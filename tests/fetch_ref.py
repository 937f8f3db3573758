"""A plain reference for main programs that hold FETCH columns (sp_air_main_column.kind 7, the _fetch entry points): Python integers,
one cell at a time, the table side of a fetch as a dictionary from each key to the first row that holds it.  No numpy, and nothing
shared with MainProgram.evaluate; the op values come from program_ref._Ops.  So that a whole table can be compared it also knows VALUE
and SUM columns, COUNT columns and unlinked CHAIN groups."""
from program_ref import NO_DEN, P, _Ops

VALUE, SUM, CHAIN, COUNT, FETCH = 0, 3, 5, 6, 7


class KeyOutOfRange(ValueError):
    pass


class MissingKey(ValueError):
    pass


def _keys(e, op, n, bits, what):
    keys = [e.val(op, i) for i in range(n)]
    for i, v in enumerate(keys):
        if v >> bits:
            raise KeyOutOfRange(f"{what} on row {i}: {v} >= 2^{bits}")
    return keys


def main_table(program, input_rows):
    """The whole main segment, n x main_cols, of an air.MainProgram (input_cols, ops, consts, cols [(kind, num_op, den_op, pad)],
    periodic_cols) over n x input_cols rows.  KeyOutOfRange for an X or T at or above 2^key_bits - looked for on both sides before
    anything is fetched -, MissingKey for an X that no T equals."""
    n, I, cols = len(input_rows), program.input_cols, program.cols
    table = [[int(v) % P for v in row] + [None] * len(cols) for row in input_rows]
    e = _Ops(program.ops, program.consts, (), program.periodic_cols, n, lambda i, c: table[i][c])
    k = 0
    while k < len(cols):
        kind, num_op, den_op, pad = cols[k]
        c = I + k
        if kind == CHAIN:
            w, period = 1, 1 << (pad & 255)
            assert pad >> 16 == 0, "a linked group: not this reference's business"
            while k + w < len(cols) and cols[k + w][0] == CHAIN and (cols[k + w][3] >> 8) & 255:
                w += 1
            for i in range(n):
                state = [e.val(cols[k + j][2], i) if i % period == 0 else e.val(cols[k + j][1], i - 1) for j in range(w)]
                for j in range(w):
                    table[i][c + j] = state[j]
            k += w
            continue
        if kind == FETCH:
            bits, v_op = pad & 255, (pad >> 8) & 65535
            assert 1 <= bits <= 64 and pad >> 24 == 0 and den_op != NO_DEN
            xs, ts = _keys(e, num_op, n, bits, "X"), _keys(e, den_op, n, bits, "T")
            first = {}
            for j in range(n):
                if ts[j] not in first:
                    first[ts[j]] = j
            for i in range(n):
                if xs[i] not in first:
                    raise MissingKey(f"derived column {k}: X = {xs[i]} on row {i} is in no table row")
                table[i][c] = e.val(v_op, first[xs[i]])
        elif kind == COUNT:
            xs, ts = _keys(e, num_op, n, pad, "X"), _keys(e, den_op, n, pad, "T")
            for i in range(n):
                seen_before = any(ts[j] == ts[i] for j in range(i))
                table[i][c] = 0 if seen_before else sum(1 for v in xs if v == ts[i])
        elif kind in (VALUE, SUM):
            total = 0
            for i in range(n):
                term = e.quotient(num_op, den_op, i)
                table[i][c] = term if kind == VALUE else total
                total = (total + term) % P
        else:
            raise NotImplementedError(f"derived column {k}: kind {kind}")
        k += 1
    return table
