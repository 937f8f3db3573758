"""Program AIRs whose chain groups divide (air.MainProgram.div, op 7, sp_air_prove_div) for the tests, beside the worked example
air.ec_subset_sum.  Each comes with a helper that returns its INPUT rows only; hand_table gives the whole main segment of `mixed` from
plain loops written without the builder, without the op lists and without MainProgram.evaluate."""
import div_ref
from lambdaworks_cairo_prover_amd import air

P = air.P
K1_PERIOD, K2_PERIOD = 4, 64
WIDE = 16

# The Stark curve y^2 = x^3 + x + BETA over this field and its generator, as StarkWare publishes them; no file of the repository holds
# them, and ec_case checks that G lies on the curve.
EC_BETA = 0x6f21413efbe40de150e596d72f7a8c5609ad26c15c915c1f4cdfcb99cee9e89
EC_G = (0x1ef15c18599971b7beced415a40f0c7deacfd9b0d1819e03d723d8bc943cfca, 0x5668060aa49730b7be4801df46ec62de53ecd11abe43a32873000c36e8dc1f)


class ZeroDenominator(Exception):
    pass


def inv(d):
    """1 / d by the extended Euclid of Python's pow (a tenth of the time of pow(d, P - 2, P), which program_ref uses: hand_table is what the
    tests can afford at 8192 rows)."""
    if d % P == 0:
        raise ZeroDenominator
    return pow(d, -1, P)


def periodic_columns(rng):
    """Two periodic columns: period 4 (below the block lengths 8 and 64, above 2) and period 64."""
    return [[rng.randrange(P) for _ in range(K1_PERIOD)], [rng.randrange(P) for _ in range(K2_PERIOD)]]


def mixed(s, link, periodic):
    """Inputs a (column 0) and c (column 1); periodic columns K1 (period 4) and K2 (period 64).  cX is the carry of column X: its value
    on the last row of the block before, zero on the first block of a run of `link` blocks (with link = 1 every block stands alone
    and the carries are the constant zero).  q / d is op 7.

    dead = a / (a - a): a DIV over a denominator that is zero on every row, which no column reaches - it is never evaluated.
    group A, columns 2 .. 4, every block on its own, DIV in the steps only, K1 and K2:
        seeds   x0 = a + K1,   x1 = c,   x2 = a(i + 3) + 1
        steps   t = x0 / (x1 + K1)   - one quotient shared by two next values, and the numerator of a third -
                x0' = t + x2,   x1' = t x1 + K2(i + 1),   x2' = t / (x2 + a(i + 3))   - a quotient of a quotient
    group B, columns 5 and 6, linked, DIV in a seed that reads a carry, no op 6 and no DIV in the steps:
        seeds   y0 = (cy1 + a) / (cy0 + c + 1),   y1 = cy1 + 1
        steps   y0' = y0 y1 + x0(i + 1),   y1' = y1 + y0^2
    group C, columns 7 and 8, polynomial, no op 7 anywhere: the launch of before inside a program of the _div entry points:
        seeds   z0 = y0,   z1 = c
        steps   z0' = z0 z1 + K1,   z1' = z1 + z0^2
    group D, columns 9 .. 24, linked, the full width of sixteen, every seed and every next value a quotient, K2:
        seeds   w_j = (cw_((j + 1) mod 16) + a + j) / (c + j + 1)
        steps   w_j' = (w_j + K2) / (w_((j + 1) mod 16) + a(i + 3) + j)
    then v = y0 x1(i + 1) + w_15 + K2 (VALUE, column 25) and r = the running sum of x0 + w_0 (SUM, column 26).
    y1 = cy1 + 1 is 1 on a run's first block whatever the run before left.  One trivial constraint: the tests of the table need a
    well-formed AIR around the program.  Returns (builder, {name: main column})."""
    b = air.AirBuilder(11 + WIDE, [0], 1, periodic=periodic, main_inputs=2)
    m = b.main
    a, a3, c = m.load(0, 0), m.load(3, 0), m.load(0, 1)
    k1, k2, k2n = m.periodic(0, 0), m.periodic(0, 1), m.periodic(1, 1)
    m.div(a, a - a)
    ga = m.chain(s, [a + k1, c, a3 + 1])
    x0, x1, x2 = ga.state(0), ga.state(1), ga.state(2)
    t = x0 / (x1 + k1)
    ga.step([t + x2, t * x1 + k2n, t / (x2 + a3)])
    carry = (lambda g, j: g.carry(j)) if link > 1 else (lambda g, j: m.const(0))
    gb = m.chain(s, None, width=2, link=link)
    gb.seed([(carry(gb, 1) + a) / (carry(gb, 0) + c + 1), carry(gb, 1) + 1])
    y0, y1 = gb.state(0), gb.state(1)
    gb.step([y0 * y1 + m.load(1, ga.cols[0]), y1 + y0 * y0])
    gc = m.chain(s, [m.load(0, gb.cols[0]), c])
    z0, z1 = gc.state(0), gc.state(1)
    gc.step([z0 * z1 + k1, z1 + z0 * z0])
    gd = m.chain(s, None, width=WIDE, link=link)
    gd.seed([(carry(gd, (j + 1) % WIDE) + a + j) / (c + (j + 1)) for j in range(WIDE)])
    w = [gd.state(j) for j in range(WIDE)]
    gd.step([(w[j] + k2) / (w[(j + 1) % WIDE] + a3 + j) for j in range(WIDE)])
    v = m.value(m.load(0, gb.cols[0]) * m.load(1, ga.cols[1]) + m.load(0, gd.cols[WIDE - 1]) + k2)
    r = m.running_sum(m.load(0, ga.cols[0]) + m.load(0, gd.cols[0]))
    x = b.load(0, 0)
    b.constraint(x - x, degree=1, exemptions=0)
    return b, {"x0": ga.cols[0], "x1": ga.cols[1], "x2": ga.cols[2], "y0": gb.cols[0], "y1": gb.cols[1], "z0": gc.cols[0], "w0": gd.cols[0], "v": v, "r": r}


def hand_table(rows, s, link, periodic):
    """The main segment of mixed(s, link, periodic) over the input rows, cell by cell in plain integers; ZeroDenominator where a
    quotient that some column reaches has none."""
    n = len(rows)
    k1 = lambda i: periodic[0][i % K1_PERIOD]
    k2 = lambda i: periodic[1][i % K2_PERIOD]
    a = lambda i: rows[i % n][0]
    c = lambda i: rows[i % n][1]
    x = [[0, 0, 0] for _ in range(n)]
    y = [[0, 0] for _ in range(n)]
    z = [[0, 0] for _ in range(n)]
    w = [[0] * WIDE for _ in range(n)]
    for block in range(n // s):
        i = block * s
        x[i] = [(a(i) + k1(i)) % P, c(i) % P, (a(i + 3) + 1) % P]
        for t in range(s - 1):
            i = block * s + t
            x0, x1, x2 = x[i]
            q = x0 * inv(x1 + k1(i)) % P
            x[i + 1] = [(q + x2) % P, (q * x1 + k2(i + 1)) % P, q * inv(x2 + a(i + 3)) % P]
    for block in range(n // s):
        i = block * s
        first = block % link == 0
        cy = [0, 0] if first else y[i - 1]
        cw = [0] * WIDE if first else w[i - 1]
        y[i] = [(cy[1] + a(i)) * inv(cy[0] + c(i) + 1) % P, (cy[1] + 1) % P]
        w[i] = [(cw[(j + 1) % WIDE] + a(i) + j) * inv(c(i) + j + 1) % P for j in range(WIDE)]
        for t in range(s - 1):
            i = block * s + t
            y0, y1 = y[i]
            y[i + 1] = [(y0 * y1 + x[(i + 1) % n][0]) % P, (y1 + y0 * y0) % P]
            w[i + 1] = [(w[i][j] + k2(i)) * inv(w[i][(j + 1) % WIDE] + a(i + 3) + j) % P for j in range(WIDE)]
    for block in range(n // s):
        i = block * s
        z[i] = [y[i][0], c(i) % P]
        for t in range(s - 1):
            i = block * s + t
            z0, z1 = z[i]
            z[i + 1] = [(z0 * z1 + k1(i)) % P, (z1 + z0 * z0) % P]
    table, total = [], 0
    for i in range(n):
        table.append([a(i) % P, c(i) % P] + x[i] + y[i] + z[i] + w[i] + [(y[i][0] * x[(i + 1) % n][1] + w[i][WIDE - 1] + k2(i)) % P, total])
        total = (total + x[i][0] + w[i][0]) % P
    return table


def mixed_inputs(n, s, link, periodic, rng):
    """(input rows, their hand_table): rows from rng on which no quotient of mixed(s, link, periodic) meets a zero - drawn again
    until hand_table says so (with elements of a 252-bit field the first draw does), and asserted."""
    for _ in range(8):
        rows = [[rng.randrange(P), rng.randrange(P)] for _ in range(n)]
        try:
            return rows, hand_table(rows, s, link, periodic)
        except ZeroDenominator:
            continue
    raise AssertionError("mixed_inputs: eight draws in a row met a zero denominator")


def plain_div(s):
    """No periodic column and no stride, so the CPU oracle can prove the same table: input a; a group of two columns with seeds x0 = a,
    x1 = a(i + 1) / (a + 2) and steps x0' = x0 / (x1 + 1) + a(i + 1), x1' = x0 x1 + 3; then v = x0 x1 (VALUE).  One real constraint on
    every row, v - x0 x1 = 0 (degree 2 under degree_bound_factor 1, as in air.dummy)."""
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    a, a1 = m.load(0, 0), m.load(1, 0)
    g = m.chain(s, [a, a1 / (a + 2)])
    x0, x1 = g.state(0), g.state(1)
    g.step([x0 / (x1 + 1) + a1, x0 * x1 + 3])
    v = m.value(m.load(0, g.cols[0]) * m.load(0, g.cols[1]))
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) * b.load(0, g.cols[1]), degree=2, exemptions=0)
    return b


def poly_only(s):
    """A program without any op 7 (through the _rec entry points): what runs between two calls of a dividing one."""
    b = air.AirBuilder(3, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(s, [m.load(0, 0)])
    g.step([g.state(0) * g.state(0) + m.load(1, 0)])
    v = m.value(m.load(0, g.cols[0]) * 3)
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) * 3, degree=1, exemptions=0)
    return b


# ---- the worked example -----------------------------------------------------------------------------------------------------------
def ec_double(p):
    lam = (3 * p[0] * p[0] + 1) * inv(2 * p[1]) % P
    x = (lam * lam - 2 * p[0]) % P
    return x, (lam * (p[0] - x) - p[1]) % P


def ec_points(s):
    """([2 G, 4 G, .., 2^s G], the shift G + P_0 + P_1) on the Stark curve."""
    assert (EC_G[1] ** 2 - EC_G[0] ** 3 - EC_G[0] - EC_BETA) % P == 0
    points, q = [], EC_G
    for _ in range(s):
        q = ec_double(q)
        assert (q[1] ** 2 - q[0] ** 3 - q[0] - EC_BETA) % P == 0
        points.append(q)
    return points, div_ref.ec_add(div_ref.ec_add(EC_G, points[0]), points[1])


def ec_case(n, s, rng, wrong=0):
    """(builder, input rows, points, shift, result) of air.ec_subset_sum with the true sum of block 0 (+ `wrong` in its x)."""
    points, shift = ec_points(s)
    rows = air.ec_subset_sum_inputs(n, rng)
    result = air.ec_subset_sum_result([r[0] for r in rows[:s]], points, shift)
    return air.ec_subset_sum(n, s, points, shift, ((result[0] + wrong) % P, result[1])), rows, points, shift, result
