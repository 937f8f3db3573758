"""A plain reference for main and auxiliary programs (air.MainProgram, air.AuxProgram; sp_air_main_desc, sp_air_aux_desc in
include/stark252_hip.h): Python integers, one cell at a time, from the raw lists a program consists of - ops, consts, cols, the periodic
value lists, the challenges.  It shares nothing with MainProgram.evaluate / AuxProgram.evaluate: no numpy, no vectorised ops, no batch
inversion (every quotient is N * pow(D, P - 2, P) of its own cell), no two-phase evaluation.  An op's value on row i is a memoised
recursive function of (op, i); a cell that is read before it was built is an error of the program, and raises.  A chain group is built
by state instead: its programs run once per row with a memo of that row alone, and a LOAD of the group is the state.  It knows every
column kind of a main program, 0 to 9.  It is slow, and meant for n <= 4096."""
import sys

P = 2**251 + 17 * 2**192 + 1
LOAD, CONST, ADD, SUB, MUL, OUT, PERIODIC, DIV = range(8)
VALUE, INV_OR_ZERO, BIT, SUM, PRODUCT, CHAIN, COUNT, FETCH, LIMB, WORD = range(10)      # sp_air_main_column.kind
AUX_PRODUCT, AUX_SUM, AUX_SORTED = range(3)                          # sp_air_aux_column.kind
AND, OR, XOR = range(3)                                              # the function of a WORD column
NO_DEN = 0xFFFFFFFF
RAP_TAG = 0x8000                                                     # a CONST of the builder's lists that names a challenge


class KeyOutOfRange(ValueError):
    """An X or T of a COUNT or FETCH column, or a sort key, at or above 2^key_bits."""


class MissingKey(ValueError):
    """An X of a FETCH column that no T equals."""


class WordOutOfRange(ValueError):
    """An operand of a WORD column at or above 2^bits."""


class ZeroDenominator(ZeroDivisionError):
    """A column's denominator, or the divisor of an op 7, is zero on some row."""


class _Ops:
    """val(t, i): the value of op t on row i.  cell(i, col) gives a trace cell, or None where it is not built yet."""

    def __init__(self, ops, consts, rap, periodic, n, cell):
        self.ops, self.consts, self.rap, self.n, self.cell = ops, [int(c) % P for c in consts], [int(r) % P for r in rap], n, cell
        self.periodic = [[int(v) % P for v in values] for values in periodic]
        self.memo = [None] * len(ops)
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(ops) + 1000))

    def _op(self, t, i, load, operand):
        """Op t on row i: a LOAD through load(shift, col), the operands of an arithmetic op through operand(t')."""
        op, a, b = self.ops[t]
        if op == LOAD:
            return load(a, b)
        if op == CONST:
            return self.rap[a & ~RAP_TAG] if a & RAP_TAG else self.consts[a]
        if op == PERIODIC:
            values = self.periodic[b]
            return values[(i + a) % len(values)]
        if op not in (ADD, SUB, MUL, DIV):
            raise ValueError(f"op {t}: code {op}")
        u, v = operand(a), operand(b)
        if op == DIV:
            if v == 0:
                raise ZeroDenominator(f"op {t} divides by zero on row {i}")
            return u * pow(v, P - 2, P) % P
        return (u + v if op == ADD else u - v if op == SUB else u * v) % P

    def _cell(self, t, i, shift, col):
        v = self.cell((i + shift) % self.n, col)
        if v is None:
            raise ValueError(f"op {t} reads column {col} on row {(i + shift) % self.n} before it is built")
        return v

    def val(self, t, i):
        row = self.memo[t]
        if row is None:
            row = self.memo[t] = [None] * self.n
        if row[i] is None:
            row[i] = self._op(t, i, lambda a, b: self._cell(t, i, a, b), lambda u: self.val(u, i))
        return row[i]

    def val_in_group(self, t, i, first, state, memo):
        """Op t on row i while a chain group is built: a LOAD of main column first + j, j < len(state), is state[j]; memo is this
        row's own (the state changes from row to row)."""
        if t not in memo:
            def load(a, b):
                if first <= b < first + len(state):
                    assert a == 0, f"op {t} reads a group column at shift {a}"
                    return state[b - first]
                return self._cell(t, i, a, b)
            memo[t] = self._op(t, i, load, lambda u: self.val_in_group(u, i, first, state, memo))
        return memo[t]

    def quotient(self, num_op, den_op, i):
        if den_op == NO_DEN:
            return self.val(num_op, i)
        d = self.val(den_op, i)
        if d == 0:
            raise ZeroDenominator(f"a denominator (op {den_op}) is zero on row {i}")
        return self.val(num_op, i) * pow(d, P - 2, P) % P

    def keys(self, op, bits, what):
        """Op `op` on every row, as lookup or sort keys below 2^bits."""
        keys = [self.val(op, i) for i in range(self.n)]
        for i, v in enumerate(keys):
            if v >> bits:
                raise KeyOutOfRange(f"{what}: a key is out of range (row {i}: {v} >= 2^{bits})")
        return keys


def _scan(kind_is_sum, term, n):
    """z_0 = 0 / 1, z_i = z_(i-1) + / * term(i - 1)."""
    out, z = [], 0 if kind_is_sum else 1
    for i in range(n):
        out.append(z)
        z = (z + term(i)) % P if kind_is_sum else z * term(i) % P
    return out


def limb(x, lo, width):
    return (x >> lo) & ((1 << width) - 1)


def word(fn, x, y):
    return x & y if fn == AND else x | y if fn == OR else x ^ y


def main_table(program, input_rows):
    """The whole main segment, n x main_cols, of a MainProgram (or anything with input_cols, ops, consts, cols [(kind, num_op, den_op,
    pad)], periodic_cols) over n x input_cols input rows.  ZeroDenominator on a zero denominator or divisor; KeyOutOfRange for an X or T
    of a COUNT or FETCH column at or above 2^key_bits - looked for on both sides before anything is counted or fetched -, MissingKey
    for an X of a FETCH column that no T equals, WordOutOfRange for an operand of a WORD column at or above 2^bits."""
    n, I, cols = len(input_rows), program.input_cols, program.cols
    table = [[int(v) % P for v in row] + [None] * len(cols) for row in input_rows]
    assert all(len(row) == I + len(cols) for row in table)
    e = _Ops(program.ops, program.consts, (), program.periodic_cols, n, lambda i, c: table[i][c])
    k = 0
    while k < len(cols):
        kind, num_op, den_op, pad = cols[k]
        c = I + k
        if kind == CHAIN:   # pad = l + 256 j + 65536 k: blocks of 2^l rows, column j of its group, runs of 2^k blocks
            w, s, link = 1, 1 << (pad & 255), 1 << (pad >> 16)
            while k + w < len(cols) and cols[k + w][0] == CHAIN and (cols[k + w][3] >> 8) & 255:
                w += 1
            for run in range(0, n, s * link):
                state = [0] * w               # the carry in front of a run
                for block in range(run, run + s * link, s):
                    # the seeds: in a linked group a LOAD of the group is the carry, in an unlinked one the trace
                    memo, carry = {}, state if link > 1 else []
                    state = [e.val_in_group(cols[k + j][2], block, c, carry, memo) for j in range(w)]
                    table[block][c:c + w] = state
                    for i in range(block, block + s - 1):
                        # every column of the step from the state on row i, then all assigned together
                        memo = {}
                        state = [e.val_in_group(cols[k + j][1], i, c, state, memo) for j in range(w)]
                        table[i + 1][c:c + w] = state
            k += w
            continue
        if kind == COUNT:
            xs, ts = e.keys(num_op, pad, f"derived column {k}, X"), e.keys(den_op, pad, f"derived column {k}, T")
            counts, first = {}, {}
            for v in xs:
                counts[v] = counts.get(v, 0) + 1
            for i, v in enumerate(ts):
                first.setdefault(v, i)
                table[i][c] = counts.get(v, 0) if first[v] == i else 0
        elif kind == FETCH:
            bits, v_op = pad & 255, (pad >> 8) & 65535
            assert 1 <= bits <= 64 and pad >> 24 == 0 and den_op != NO_DEN
            xs, ts = e.keys(num_op, bits, f"derived column {k}, X"), e.keys(den_op, bits, f"derived column {k}, T")
            first = {}
            for j, v in enumerate(ts):
                first.setdefault(v, j)
            for i in range(n):
                if xs[i] not in first:
                    raise MissingKey(f"derived column {k}: X = {xs[i]} on row {i} is in no table row")
                table[i][c] = e.val(v_op, first[xs[i]])
        elif kind == LIMB:
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
        elif kind == VALUE:
            for i in range(n):
                table[i][c] = e.quotient(num_op, den_op, i)
        elif kind == INV_OR_ZERO:
            for i in range(n):
                x = e.val(num_op, i)
                table[i][c] = pow(x, P - 2, P) if x else 0
        elif kind == BIT:
            for i in range(n):
                table[i][c] = (e.val(num_op, i) >> pad) & 1
        elif kind in (SUM, PRODUCT):
            for i, z in enumerate(_scan(kind == SUM, lambda i: e.quotient(num_op, den_op, i), n)):
                table[i][c] = z
        else:
            raise ValueError(f"derived column {k}: kind {kind}")
        k += 1
    return table


def aux_table(program, main_rows, rap, periodic):
    """The auxiliary segment, n x len(cols), of an AuxProgram (main_cols, ops, consts, cols, key_bits) over the whole main segment,
    under the challenges `rap`; periodic: the value lists an op 6 reads.  Columns in index order; a sorted column is row pi(i) of its
    expression, pi the stable order of the rows by the key's integer (sorted() is stable)."""
    n, M, cols = len(main_rows), program.main_cols, program.cols
    main = [[int(v) % P for v in row] for row in main_rows]
    out = [[None] * len(cols) for _ in range(n)]
    e = _Ops(program.ops, program.consts, rap, periodic, n, lambda i, c: main[i][c] if c < M else out[i][c - M])
    orders = {}
    for k, (kind, num_op, den_op) in enumerate(cols):
        if kind == AUX_SORTED:
            if den_op not in orders:
                keys = e.keys(den_op, program.key_bits.get(k, 64), f"auxiliary column {k}")
                orders[den_op] = sorted(range(n), key=lambda i: keys[i])
            for i, src in enumerate(orders[den_op]):
                out[i][k] = e.val(num_op, src)
        elif kind in (AUX_SUM, AUX_PRODUCT):
            for i, z in enumerate(_scan(kind == AUX_SUM, lambda i: e.quotient(num_op, den_op, i), n)):
                out[i][k] = z
        else:
            raise ValueError(f"auxiliary column {k}: kind {kind}")
    return out
