"""A plain reference for main programs that hold LIMB and WORD columns (sp_air_main_column.kind 8 and 9, the _word entry points): Python
integers, one cell at a time - (x >> lo) & ((1 << width) - 1), x & y, x | y, x ^ y.  No numpy, and nothing shared with
MainProgram.evaluate; the op values come from program_ref._Ops.  So that a whole table can be compared it also knows VALUE, BIT and SUM
columns, COUNT and FETCH columns and unlinked CHAIN groups."""
from program_ref import NO_DEN, P, _Ops

VALUE, BIT, SUM, CHAIN, COUNT, FETCH, LIMB, WORD = 0, 2, 3, 5, 6, 7, 8, 9
AND, OR, XOR = range(3)


class WordOutOfRange(ValueError):
    pass


class KeyOutOfRange(ValueError):
    pass


class MissingKey(ValueError):
    pass


def limb(x, lo, width):
    return (x >> lo) & ((1 << width) - 1)


def word(fn, x, y):
    return x & y if fn == AND else x | y if fn == OR else x ^ y


def _keys(e, op, n, bits, what):
    keys = [e.val(op, i) for i in range(n)]
    for i, v in enumerate(keys):
        if v >> bits:
            raise KeyOutOfRange(f"{what} on row {i}: {v} >= 2^{bits}")
    return keys


def main_table(program, input_rows):
    """The whole main segment, n x main_cols, of an air.MainProgram (input_cols, ops, consts, cols [(kind, num_op, den_op, pad)],
    periodic_cols) over n x input_cols rows.  WordOutOfRange for an operand of a WORD column at or above 2^bits, KeyOutOfRange and
    MissingKey as fetch_ref, ZeroDivisionError on a zero denominator."""
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
        if kind == LIMB:
            lo, width = pad & 255, (pad >> 8) & 255
            assert pad >> 16 == 0 and den_op == NO_DEN and width >= 1 and lo + width <= 252
            for i in range(n):
                table[i][c] = limb(e.val(num_op, i), lo, width)
        elif kind == WORD:
            fn, bits = pad & 255, (pad >> 8) & 255
            assert pad >> 16 == 0 and den_op != NO_DEN and fn <= XOR and 1 <= bits <= 251
            for i in range(n):
                x, y = e.val(num_op, i), e.val(den_op, i)
                if x >> bits or y >> bits:
                    raise WordOutOfRange(f"derived column {k}, row {i}: {x} or {y} >= 2^{bits}")
                table[i][c] = word(fn, x, y)
        elif kind == BIT:
            for i in range(n):
                table[i][c] = (e.val(num_op, i) >> pad) & 1
        elif kind == FETCH:
            bits, v_op = pad & 255, (pad >> 8) & 65535
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
            counts, first = {}, {}
            for v in xs:
                counts[v] = counts.get(v, 0) + 1
            for i, v in enumerate(ts):
                first.setdefault(v, i)
                table[i][c] = counts.get(v, 0) if first[v] == i else 0
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
