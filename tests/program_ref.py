"""A plain reference for main and auxiliary programs (air.MainProgram, air.AuxProgram; sp_air_main_desc, sp_air_aux_desc in
include/stark252_hip.h): Python integers, one cell at a time, from the raw lists a program consists of - ops, consts, cols, the periodic
value lists, the challenges.  It shares nothing with MainProgram.evaluate / AuxProgram.evaluate: no numpy, no vectorised ops, no batch
inversion (every quotient is N * pow(D, P - 2, P) of its own cell), no two-phase evaluation.  An op's value on row i is a memoised
recursive function of (op, i); a cell that is read before it was built is an error of the program, and raises.  It is slow, and meant
for n <= 4096."""
import sys

P = 2**251 + 17 * 2**192 + 1
LOAD, CONST, ADD, SUB, MUL, OUT, PERIODIC = range(7)
VALUE, INV_OR_ZERO, BIT, SUM, PRODUCT, CHAIN, COUNT = range(7)      # sp_air_main_column.kind
AUX_PRODUCT, AUX_SUM, AUX_SORTED = range(3)                          # sp_air_aux_column.kind
NO_DEN = 0xFFFFFFFF
RAP_TAG = 0x8000                                                     # a CONST of the builder's lists that names a challenge


class _Ops:
    """val(t, i): the value of op t on row i.  cell(i, col) gives a trace cell, or None where it is not built yet."""

    def __init__(self, ops, consts, rap, periodic, n, cell):
        self.ops, self.consts, self.rap, self.n, self.cell = ops, [int(c) % P for c in consts], [int(r) % P for r in rap], n, cell
        self.periodic = [[int(v) % P for v in values] for values in periodic]
        self.memo = [None] * len(ops)
        sys.setrecursionlimit(max(sys.getrecursionlimit(), 4 * len(ops) + 1000))

    def val(self, t, i):
        row = self.memo[t]
        if row is None:
            row = self.memo[t] = [None] * self.n
        v = row[i]
        if v is not None:
            return v
        op, a, b = self.ops[t]
        if op == LOAD:
            v = self.cell((i + a) % self.n, b)
            if v is None:
                raise ValueError(f"op {t} reads column {b} on row {(i + a) % self.n} before it is built")
        elif op == CONST:
            v = self.rap[a & ~RAP_TAG] if a & RAP_TAG else self.consts[a]
        elif op == ADD:
            v = (self.val(a, i) + self.val(b, i)) % P
        elif op == SUB:
            v = (self.val(a, i) - self.val(b, i)) % P
        elif op == MUL:
            v = self.val(a, i) * self.val(b, i) % P
        elif op == PERIODIC:
            values = self.periodic[b]
            v = values[(i + a) % len(values)]
        else:
            raise ValueError(f"op {t}: code {op}")
        row[i] = v
        return v

    def quotient(self, num_op, den_op, i):
        if den_op == NO_DEN:
            return self.val(num_op, i)
        d = self.val(den_op, i)
        if d == 0:
            raise ZeroDivisionError(f"a denominator (op {den_op}) is zero on row {i}")
        return self.val(num_op, i) * pow(d, P - 2, P) % P


def _scan(kind_is_sum, term, n):
    """z_0 = 0 / 1, z_i = z_(i-1) + / * term(i - 1)."""
    out, z = [], 0 if kind_is_sum else 1
    for i in range(n):
        out.append(z)
        z = (z + term(i)) % P if kind_is_sum else z * term(i) % P
    return out


def main_table(program, input_rows):
    """The whole main segment, n x main_cols, of a MainProgram (or anything with input_cols, ops, consts, cols, periodic_cols) over
    n x input_cols input rows.  ZeroDivisionError on a zero denominator, ValueError on a lookup key at or above 2^key_bits."""
    n, I, cols = len(input_rows), program.input_cols, program.cols
    table = [[int(v) % P for v in row] + [None] * len(cols) for row in input_rows]
    assert all(len(row) == I + len(cols) for row in table)
    e = _Ops(program.ops, program.consts, (), program.periodic_cols, n, lambda i, c: table[i][c])
    k = 0
    while k < len(cols):
        kind, num_op, den_op, pad = cols[k]
        c = I + k
        if kind == CHAIN:
            w, period = 1, 1 << (pad & 255)
            while k + w < len(cols) and cols[k + w][0] == CHAIN and cols[k + w][3] >> 8:
                w += 1
            for r0 in range(0, n, period):
                for i in range(r0, r0 + period):
                    # every column of the step from the row before, then all assigned together
                    state = [e.val(cols[k + j][2], i) if i == r0 else e.val(cols[k + j][1], i - 1) for j in range(w)]
                    for j in range(w):
                        table[i][c + j] = state[j]
            k += w
            continue
        if kind == COUNT:
            xs, ts = [e.val(num_op, j) for j in range(n)], [e.val(den_op, i) for i in range(n)]
            for v in xs + ts:
                if v >> pad:
                    raise ValueError(f"derived column {k}: a lookup key is out of range ({v} >= 2^{pad})")
            counts, first = {}, {}
            for v in xs:
                counts[v] = counts.get(v, 0) + 1
            for i, v in enumerate(ts):
                first.setdefault(v, i)
                table[i][c] = counts.get(v, 0) if first[v] == i else 0
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
                keys, bits = [e.val(den_op, i) for i in range(n)], program.key_bits.get(k, 64)
                for i, v in enumerate(keys):
                    if v >> bits:
                        raise ValueError(f"auxiliary column {k}: a sort key is out of range (row {i}: {v} >= 2^{bits})")
                orders[den_op] = sorted(range(n), key=lambda i: keys[i])
            for i, src in enumerate(orders[den_op]):
                out[i][k] = e.val(num_op, src)
        elif kind in (AUX_SUM, AUX_PRODUCT):
            for i, z in enumerate(_scan(kind == AUX_SUM, lambda i: e.quotient(num_op, den_op, i), n)):
                out[i][k] = z
        else:
            raise ValueError(f"auxiliary column {k}: kind {kind}")
    return out
