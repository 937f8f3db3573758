"""Program AIRs whose main program holds looked-up values (air.MainProgram.fetch / fetch_many, sp_air_prove_fetch) for the tests, beside
the worked examples air.xor_fetch and air.rom_reads.  Each comes with a helper that returns its INPUT rows only."""
from lambdaworks_cairo_prover_amd import air
from lookup_airs import trivial

P = air.P


def periodic_fetch(keys, values, key_bits):
    """Input x (column 0); the table is periodic: column 0 the keys, columns 1 .. w the values (`values`: w lists as long as `keys`).
    Columns 1 .. w = fetch_many(x, keys, values): one run."""
    w = len(values)
    b = air.AirBuilder(1 + w, [0], 1, periodic=[keys] + list(values), main_inputs=1)
    m = b.main
    m.fetch_many(m.load(0, 0), m.periodic(0, 0), [m.periodic(0, 1 + j) for j in range(w)], key_bits)
    return trivial(b)


def periodic_table(period, w, key_bits, rng):
    """(keys, values) for periodic_fetch: keys below 2^key_bits with both ends of the range and a duplicate (whose values differ)."""
    top = (1 << key_bits) - 1
    if key_bits == 1:
        keys = [rng.randrange(2) for _ in range(period)]
        keys[0], keys[1] = 1, 0
    else:
        keys = [rng.randrange(top + 1) for _ in range(period)]
        keys[1], keys[2], keys[period - 1] = top, 0, keys[3 % period]
    return keys, [[rng.randrange(P) for _ in range(period)] for _ in range(w)]


def input_fetch(w, key_bits=64):
    """Inputs x, t and v (columns 0 - 2): the table is a pair of input columns.  Columns 3 .. 2 + w = fetch_many(x, t, [(j + 1) v + j]),
    one run of w columns."""
    b = air.AirBuilder(3 + w, [0], 1, main_inputs=3)
    m = b.main
    m.fetch_many(m.load(0, 0), m.load(0, 1), [m.load(0, 2) * (j + 1) + j for j in range(w)], key_bits)
    return trivial(b)


def input_rows(n, key_bits, rng, distinct=None):
    """(n, 3) rows [x, t, v]: t draws from `distinct` keys below 2^key_bits with repeats - equal keys carry different v -, among them
    both ends of the range; x from the keys t holds, the smallest and the largest among them."""
    distinct = distinct or max(2, n // 3)
    top = (1 << key_bits) - 1
    pool = [0, top] + [rng.randrange(top + 1) for _ in range(max(0, distinct - 2))]
    t = [pool[i] if i < len(pool) and i < 2 else rng.choice(pool) for i in range(n)]
    rng.shuffle(t)
    rows = [[rng.choice(t), t[i], rng.randrange(P)] for i in range(n)]
    rows[0][0], rows[n - 1][0] = min(t), max(t)
    return rows


def chain_fetch(s):
    """Inputs x, t and v.  Column 3 is a chain c in blocks of s rows (seed v, step c^2 + t); column 4 = fetch(x + 0 c(i + 1), t,
    c(i + 1) + v): X and V read the chain column at shift 1, which wraps on the last row."""
    b = air.AirBuilder(5, [0], 1, main_inputs=3)
    m = b.main
    g = m.chain(s, [m.load(0, 2)])
    g.step([g.state(0) * g.state(0) + m.load(0, 1)])
    c = g.cols[0]
    m.fetch(m.load(0, 0) + m.load(1, c) * 0, m.load(0, 1), m.load(1, c) + m.load(0, 2), 64)
    return trivial(b)


def count_and_fetch(key_bits=64):
    """Inputs x, t and v: m = multiplicity(x, t) (column 3) and f = fetch(x, t, v) (column 4) on one table, and their product as a VALUE
    (column 5)."""
    b = air.AirBuilder(6, [0], 1, main_inputs=3)
    m = b.main
    mult = m.multiplicity(m.load(0, 0), m.load(0, 1), key_bits)
    f = m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), key_bits)
    m.value(m.load(0, mult) * f)
    return trivial(b)


def mixed(s, key_bits=64):
    """Inputs x, t and v: f = fetch(x, t, v) (column 3); a chain c in blocks of s rows that reads it (seed f + x, step c^2 + f(i + 1),
    column 4); m = multiplicity(x, t) on the same table (column 5); a second fetch of c through the same keys (column 6), which is a
    chunk of its own since a chain group and a COUNT column lie between; the running sum of m f2 (column 7)."""
    b = air.AirBuilder(8, [0], 1, main_inputs=3)
    m = b.main
    f = m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), key_bits)
    g = m.chain(s, [f + m.load(0, 0)])
    g.step([g.state(0) * g.state(0) + m.load(1, 3)])
    mult = m.multiplicity(m.load(0, 0), m.load(0, 1), key_bits)
    f2 = m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, g.cols[0]), key_bits)
    m.running_sum(m.load(0, mult) * f2)
    return trivial(b)


def separated(w):
    """The columns of input_fetch(w) with a VALUE column (x + 1) between the first half and the second: two runs, the same FETCH cells.
    Returns (builder, the main columns of the w FETCH columns)."""
    b = air.AirBuilder(4 + w, [0], 1, main_inputs=3)
    m = b.main
    values = [m.load(0, 2) * (j + 1) + j for j in range(w)]
    half = w // 2
    m.fetch_many(m.load(0, 0), m.load(0, 1), values[:half], 64)
    m.value(m.load(0, 0) + 1)
    m.fetch_many(m.load(0, 0), m.load(0, 1), values[half:], 64)
    return trivial(b), list(range(3, 3 + half)) + list(range(4 + half, 4 + w))


def zero_den_beside_a_fetch():
    """Inputs x, t and v: a VALUE 1 / (v - 5) (column 3) and f = fetch(x, t, v) with 8 key bits (column 4)."""
    b = air.AirBuilder(5, [0], 1, main_inputs=3)
    m = b.main
    m.value(1, m.load(0, 2) - 5)
    m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), 8)
    return trivial(b)
