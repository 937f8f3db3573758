"""Program AIRs whose main program holds chain groups (air.MainProgram.chain, sp_air_prove_rec) for the tests, beside the worked example
air.mimc_blocks.  Each comes with a helper that returns its INPUT rows only, and hand_table gives the whole main segment of `mixed`
from a double loop written without the builder."""
from lambdaworks_cairo_prover_amd import air

P = air.P
K1_PERIOD, K2_PERIOD = 8, 64


def periodic_columns(rng):
    """Two periodic columns of different periods: 8 (below most block lengths) and 64 (above them)."""
    return [[rng.randrange(P) for _ in range(K1_PERIOD)], [rng.randrange(P) for _ in range(K2_PERIOD)]]


def mixed(s, periodic):
    """Inputs a (column 0) and c (column 1); periodic columns K1 (period 8) and K2 (period 64).

    group A, columns 2 .. 4, blocks of s rows, whose steps read each other's state:
        seeds   x0 = a,   x1 = a(i + 3) + K1,   x2 = c K2
        steps   x0' = (x0 + K1)^3 + x1,   x1' = x1 x2 + a(i + 3) + K2(i + 1),   x2' = x2^2 + x0 c + 5
    group B, columns 5 and 6, adjacent to A with the same block length; it reads A as any earlier column, at a shift too:
        seeds   y0 = x0,   y1 = c
        steps   y0' = y0 y1 + x2(i + 1),   y1' = y1 + y0^2 + K1
    then v = y0 x1(i + 1) + K2 (VALUE, column 7) and r = the running sum of x0 (SUM, column 8).
    a is read at shifts 0 and 3: on the last three rows the read wraps to the first rows.  One trivial constraint: the tests of the
    table need a well-formed AIR around the program.  Returns (builder, {name: main column})."""
    b = air.AirBuilder(9, [0], 1, periodic=periodic, main_inputs=2)
    m = b.main
    a, a3, c = m.load(0, 0), m.load(3, 0), m.load(0, 1)
    k1, k2, k2n = m.periodic(0, 0), m.periodic(0, 1), m.periodic(1, 1)
    ga = m.chain(s, [a, a3 + k1, c * k2])
    x0, x1, x2 = ga.state(0), ga.state(1), ga.state(2)
    t = x0 + k1
    ga.step([t * t * t + x1, x1 * x2 + a3 + k2n, x2 * x2 + x0 * c + 5])
    gb = m.chain(s, [m.load(0, ga.cols[0]), c])
    y0, y1 = gb.state(0), gb.state(1)
    gb.step([y0 * y1 + m.load(1, ga.cols[2]), y1 + y0 * y0 + k1])
    v = m.value(m.load(0, gb.cols[0]) * m.load(1, ga.cols[1]) + k2)
    r = m.running_sum(m.load(0, ga.cols[0]))
    x = b.load(0, 0)
    b.constraint(x - x, degree=1, exemptions=0)
    return b, {"x0": ga.cols[0], "x1": ga.cols[1], "x2": ga.cols[2], "y0": gb.cols[0], "y1": gb.cols[1], "v": v, "r": r}


def mixed_inputs(n, rng):
    return [[rng.randrange(P), rng.randrange(P)] for _ in range(n)]


def hand_table(rows, s, periodic):
    """The main segment of mixed(s, periodic) over the input rows, row by row and block by block in plain integers."""
    n = len(rows)
    k1 = lambda i: periodic[0][i % K1_PERIOD]
    k2 = lambda i: periodic[1][i % K2_PERIOD]
    a = lambda i: rows[i % n][0]
    c = lambda i: rows[i % n][1]
    x = [[0, 0, 0] for _ in range(n)]
    for block in range(n // s):
        i = block * s
        x[i] = [a(i) % P, (a(i + 3) + k1(i)) % P, c(i) * k2(i) % P]
        for t in range(s - 1):
            i = block * s + t
            x0, x1, x2 = x[i]
            x[i + 1] = [(pow(x0 + k1(i), 3, P) + x1) % P, (x1 * x2 + a(i + 3) + k2(i + 1)) % P, (x2 * x2 + x0 * c(i) + 5) % P]
    y = [[0, 0] for _ in range(n)]
    for block in range(n // s):
        i = block * s
        y[i] = [x[i][0], c(i) % P]
        for t in range(s - 1):
            i = block * s + t
            y0, y1 = y[i]
            y[i + 1] = [(y0 * y1 + x[(i + 1) % n][2]) % P, (y1 + y0 * y0 + k1(i)) % P]
    table, total = [], 0
    for i in range(n):
        table.append([a(i) % P, c(i) % P] + x[i] + y[i] + [(y[i][0] * x[(i + 1) % n][1] + k2(i)) % P, total])
        total = (total + x[i][0]) % P
    return table


def plain_pair(s):
    """No periodic column and no stride, so the CPU oracle can prove the same table: input a; a group of two columns in blocks of s
    rows, x0 = a and x1 = a(i + 1) on a block's first row, x0' = x0^2 + x1 and x1' = x0 x1 + 3; then v = x0 x1 (VALUE).  One real
    constraint on every row, v - x0 x1 = 0 (degree 2 under degree_bound_factor 1, as in air.dummy)."""
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(s, [m.load(0, 0), m.load(1, 0)])
    x0, x1 = g.state(0), g.state(1)
    g.step([x0 * x0 + x1, x0 * x1 + 3])
    v = m.value(m.load(0, g.cols[0]) * m.load(0, g.cols[1]))
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) * b.load(0, g.cols[1]), degree=2, exemptions=0)
    return b


def chain_permutation(s):
    """A chain beside an auxiliary program: input a, the one-column chain x (seed a, step x^2 + a(i + 1)), d_i = x_(i+1) (VALUE of a
    shifted load of the chain column, wrapping) and the grand product z_0 = 1, z' (gamma - d) = z (gamma - x) on every row - the last
    wraps to z_0 = 1, so d is a permutation of x.  The second constraint ties d to the next row's x."""
    b = air.AirBuilder(3, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, main_inputs=1)
    m = b.main
    g = m.chain(s, [m.load(0, 0)])
    x = g.state(0)
    g.step([x * x + m.load(1, 0)])
    xc = g.cols[0]
    d = m.value(m.load(1, xc))
    gamma = b.rap(0)
    b.constraint(b.load(1, 3) * (gamma - b.load(0, d)) - b.load(0, 3) * (gamma - b.load(0, xc)), degree=2, exemptions=0)
    b.constraint(b.load(0, d) - b.load(1, xc), degree=1, exemptions=0)
    b.boundary(3, 0, 1)
    gm = b.aux.rap(0)
    b.aux.product(gm - b.aux.load(0, xc), gm - b.aux.load(0, d))
    return b


def mimc_case(n, s, rng, width=1):
    """(builder, input rows, keys) of air.mimc_blocks with the true digest of block 0."""
    keys = [rng.randrange(P) for _ in range(s)]
    rows = air.mimc_blocks_inputs(n, s, rng)
    return air.mimc_blocks(n, s, keys, air.mimc_blocks_digest([rows[0][0]], s, keys, width), width), rows, keys
