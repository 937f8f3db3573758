"""Program AIRs whose main program holds lookup multiplicities (air.MainProgram.multiplicity, sp_air_prove_lk) for the tests, beside the
worked examples air.table_lookup_main and air.xor_lookup.  Each comes with a helper that returns its INPUT rows only, and hand_table
gives the whole main segment of `mixed` from a double loop written without the builder."""
from lambdaworks_cairo_prover_amd import air

P = air.P
MIXED_PERIOD = 8


def trivial(b):
    """One constraint that every trace satisfies: the tests of the table need a well-formed AIR around the program."""
    x = b.load(0, 0)
    b.constraint(x - x, degree=1, exemptions=0)
    return b


def mixed(periodic, key_bits=64):
    """Inputs a (column 0) and c (column 1); periodic column K (period 8).

        v = a + 3                         VALUE, column 2
        m = multiplicity(X, T, key_bits)  COUNT, column 3:  X = v + a(i + 1),  T = K + c   (X reads a VALUE column and an input at a
                                          shift, which wraps on the last row; T a periodic column and an input)
        r = running sum of m(i + 1)       SUM, column 4: it reads the COUNT column at shift 1

    Returns (builder, {name: main column})."""
    b = air.AirBuilder(5, [0], 1, periodic=[periodic], main_inputs=2)
    m = b.main
    v = m.value(m.load(0, 0) + 3)
    mult = m.multiplicity(m.load(0, v) + m.load(1, 0), m.periodic(0, 0) + m.load(0, 1), key_bits)
    r = m.running_sum(m.load(1, mult))
    return trivial(b), {"v": v, "m": mult, "r": r}


def mixed_inputs(n, periodic, rng, small=40):
    """a small, so that sums of two of them collide often; c such that T = K + c hits some of those sums, repeats some of its own values
    and misses others."""
    rows = [[rng.randrange(small), 0] for _ in range(n)]
    for i in range(n):
        want = rng.choice([rows[j][0] + 3 + rows[(j + 1) % n][0] for j in range(n)] + [5 * small + rng.randrange(small)])
        rows[i][1] = (want - periodic[i % MIXED_PERIOD]) % P
    return rows


def hand_table(rows, periodic):
    """The main segment of mixed(periodic) over the input rows: a double loop over table rows and looked-up rows in plain integers."""
    n = len(rows)
    x = [(rows[j][0] + 3 + rows[(j + 1) % n][0]) % P for j in range(n)]
    t = [(periodic[i % MIXED_PERIOD] + rows[i][1]) % P for i in range(n)]
    m = []
    for i in range(n):
        first = all(t[k] != t[i] for k in range(i))
        m.append(sum(1 for j in range(n) if x[j] == t[i]) if first else 0)
    table, total = [], 0
    for i in range(n):
        table.append([rows[i][0] % P, rows[i][1] % P, (rows[i][0] + 3) % P, m[i], total])
        total = (total + m[(i + 1) % n]) % P
    return table


def plain_count(key_bits=64):
    """The smallest program with a COUNT column: inputs a (column 0) and t (column 1), m = multiplicity(a, t, key_bits) (column 2)."""
    b = air.AirBuilder(3, [0], 1, main_inputs=2)
    b.main.multiplicity(b.main.load(0, 0), b.main.load(0, 1), key_bits)
    return trivial(b)


def periodic_count(table, key_bits):
    """Input a (column 0), m = multiplicity(a, T, key_bits) (column 1) with T periodic column 0 - air.table_lookup_main's main program
    without the argument around it, so that the table may hold any trace: X outside the table, a column of zeros."""
    b = air.AirBuilder(2, [0], 1, periodic=[table], main_inputs=1)
    b.main.multiplicity(b.main.load(0, 0), b.main.periodic(0, 0), key_bits)
    return trivial(b)


def two_counts(s, periodic):
    """Two COUNT columns of different key widths with a chain group between them (the workspace is used by each in turn): inputs a and
    c; m1 = multiplicity(a, T, 16) with T periodic column 0 (column 2); the chain x (blocks of s rows, seed a + m1, step x^2 + c,
    column 3); m2 = multiplicity(c, a(i + 2), 64) (column 4); v = m1 + m2 x (VALUE, column 5)."""
    b = air.AirBuilder(6, [0], 1, periodic=[periodic], main_inputs=2)
    m = b.main
    m1 = m.multiplicity(m.load(0, 0), m.periodic(0, 0), 16)
    g = m.chain(s, [m.load(0, 0) + m.load(0, m1)])
    g.step([g.state(0) * g.state(0) + m.load(0, 1)])
    m2 = m.multiplicity(m.load(0, 1), m.load(2, 0), 64)
    m.value(m.load(0, m1) + m.load(0, m2) * m.load(0, g.cols[0]))
    return trivial(b)


def input_table_lookup():
    """air.table_lookup with the table as an input column and not a periodic one, so that the CPU oracle - which takes no periodic
    columns - can prove the same table: inputs a and t, m = multiplicity(a, t) (column 2), the LogUp running sum s (auxiliary column 3)
    with s_0 = 0 and s' = s + m / (gamma - t) - 1 / (gamma - a), no exempted row."""
    b = air.AirBuilder(3, [0, 1], 2, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, main_inputs=2)
    b.main.multiplicity(b.main.load(0, 0), b.main.load(0, 1))
    gamma = b.rap(0)
    ga, gt = gamma - b.load(0, 0), gamma - b.load(0, 1)
    b.constraint((b.load(1, 3) - b.load(0, 3)) * gt * ga - b.load(0, 2) * ga + gt, degree=3, exemptions=0)
    b.boundary(3, 0, 0)
    g = b.aux.rap(0)
    xa, xt = g - b.aux.load(0, 0), g - b.aux.load(0, 1)
    b.aux.running_sum(b.aux.load(0, 2) * xa - xt, xt * xa)
    return b


def input_table_rows(n, rng, distinct=24):
    """(n, 2) rows [a, t]: t draws from `distinct` random field elements' low 64 bits with repeats, a from the values t holds."""
    pool = [rng.randrange(1 << 64) for _ in range(distinct)]
    t = [rng.choice(pool) for _ in range(n)]
    return [[rng.choice(t), t[i]] for i in range(n)]


def lookup_case(n, period, key_bits, rng):
    """(builder, input rows, table) of air.table_lookup_main: a table of `period` values below 2^key_bits with one value repeated
    inside the period (when the period and the key width leave room for it)."""
    table = [rng.randrange(1 << key_bits) for _ in range(period)]
    if period > 2:
        table[period - 1] = table[1]
    return air.table_lookup_main(n, table, key_bits), air.table_lookup_main_inputs(n, table, rng), table
