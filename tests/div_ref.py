"""A plain reference for main programs whose chain groups divide: one cell at a time over the op lists, a memoised recursion per row,
every quotient its own pow(d, P - 2, P).  It shares no code with MainProgram.evaluate (which runs an op over all blocks at once and
inverts in batches).  Knows ops 0 - 4, 6 and 7, CHAIN columns - linked or not - and, so that a whole table can be compared, VALUE and
SUM columns.  Beside it an affine elliptic-curve adder and the table of air.ec_subset_sum written with it."""
P = 2**251 + 17 * 2**192 + 1
LOAD, CONST, ADD, SUB, MUL, PERIODIC, DIV = 0, 1, 2, 3, 4, 6, 7
VALUE, SUM, CHAIN = 0, 3, 5
NO_DEN = 0xFFFFFFFF


class ZeroDenominator(Exception):
    pass


def table(input_cols, main_cols, ops, consts, cols, periodic, rows):
    """The whole main segment: ops [(op, a, b)], consts [int], cols [(kind, num_op, den_op, pad)] with pad = l + 256 j + 65536 k on
    a CHAIN column, periodic [[int]], rows n x input_cols.  Only the ops a column names are evaluated, on the rows it names them on."""
    n = len(rows)
    m = [[int(v) % P for v in row] + [None] * (main_cols - input_cols) for row in rows]

    def value(t, i, first, state, memo):
        """Op t on row i; a LOAD of main column first + j is state[j] (state None: no group is being built)."""
        if t in memo:
            return memo[t]
        op, a, b = ops[t]
        if op == LOAD:
            if state is not None and first <= b < first + len(state):
                assert a == 0
                r = state[b - first]
            else:
                r = m[(i + a) % n][b]
                assert r is not None, (t, i, b)
        elif op == CONST:
            r = consts[a] % P
        elif op == PERIODIC:
            r = periodic[b][(i + a) % len(periodic[b])] % P
        elif op in (ADD, SUB, MUL, DIV):
            u, v = value(a, i, first, state, memo), value(b, i, first, state, memo)
            if op == DIV:
                if v == 0:
                    raise ZeroDenominator((t, i))
                r = u * pow(v, P - 2, P) % P
            else:
                r = (u + v if op == ADD else u - v if op == SUB else u * v) % P
        else:
            raise ValueError(f"op {t}: code {op}")
        memo[t] = r
        return r

    k = 0
    while k < len(cols):
        kind, num_op, den_op, pad = cols[k]
        col = input_cols + k
        if kind == CHAIN:
            w = 1
            while k + w < len(cols) and cols[k + w][0] == CHAIN and (cols[k + w][3] >> 8) & 255:
                w += 1
            s, link = 1 << (pad & 255), 1 << (pad >> 16)
            for run in range(0, n, s * link):
                state = [0] * w
                for block in range(run, run + s * link, s):
                    memo = {}
                    state = [value(cols[k + j][2], block, col, state if link > 1 else [], memo) for j in range(w)]
                    for j in range(w):
                        m[block][col + j] = state[j]
                    for i in range(block, block + s - 1):
                        memo = {}
                        state = [value(cols[k + j][1], i, col, state, memo) for j in range(w)]
                        for j in range(w):
                            m[i + 1][col + j] = state[j]
            k += w
            continue
        if kind not in (VALUE, SUM):
            raise NotImplementedError(f"column kind {kind}")
        terms = []
        for i in range(n):
            memo = {}
            t = value(num_op, i, 0, None, memo)
            if den_op != NO_DEN:
                d = value(den_op, i, 0, None, memo)
                if d == 0:
                    raise ZeroDenominator((den_op, i))
                t = t * pow(d, P - 2, P) % P
            terms.append(t)
        total = 0
        for i in range(n):
            m[i][col] = terms[i] if kind == VALUE else total
            total = (total + terms[i]) % P
        k += 1
    return m


def table_of(main, rows):
    """table() of an air.MainProgram."""
    return table(main.input_cols, main.main_cols, main.ops, main.consts, main.cols, main.periodic_cols, rows)


# ---- affine points of y^2 = x^3 + x + beta ----------------------------------------------------------------------------------------
def ec_add(p, q):
    """p + q for affine points with different x."""
    if (p[0] - q[0]) % P == 0:
        raise ZeroDenominator("the chord of two points with one x")
    lam = (q[1] - p[1]) * pow(q[0] - p[0], P - 2, P) % P
    x = (lam * lam - p[0] - q[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def ec_subset_sum_table(rows, s, points, shift):
    """The main segment of air.ec_subset_sum over the bits `rows`: [b, x, y, lambda, lambda^2, b lambda] on every row, the accumulator
    moved by ec_add and the slope computed from the two points it joins."""
    out = []
    for i, (bit,) in enumerate(rows):
        t = i % s
        if t == 0:
            acc = (shift[0] % P, shift[1] % P)
        elif out[i - 1][0]:
            acc = ec_add(acc, points[t - 1])
        px, py = points[t]
        if (acc[0] - px) % P == 0:
            raise ZeroDenominator(i)
        lam = (acc[1] - py) * pow(acc[0] - px, P - 2, P) % P
        out.append([int(bit) % P, acc[0], acc[1], lam, lam * lam % P, int(bit) * lam % P])
    return out
