"""Seeded main-trace programs with joint COUNT columns (b.main.multiplicity_many, the _multi entry points), through the builder, and
their input rows.  case(n, L, key_bits, shape, seed) covers the shapes of SHAPES; the other builders are the small programs single
tests want."""
import random

from lambdaworks_cairo_prover_amd import air

P = air.P
SHAPES = ("hot", "distinct", "period", "unlooked", "limb", "periodic")


def pool(rng, key_bits, size):
    """`size` distinct keys below 2^key_bits (all 2^key_bits of them where there are fewer); at 64 bits every other one has bit 63 set."""
    if (1 << key_bits) <= size:
        keys = list(range(1 << key_bits))
        rng.shuffle(keys)
        return keys
    keys = set()
    while len(keys) < size:
        v = rng.randrange(1 << key_bits)
        if key_bits == 64 and len(keys) % 2:
            v |= 1 << 63
        keys.add(v)
    keys = sorted(keys)
    rng.shuffle(keys)
    return keys


def _cycled(keys, count):
    return [keys[i % len(keys)] for i in range(count)]


def _trivial_constraint(b):
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)


def case(n, L, key_bits, shape, seed):
    """(builder, input rows) of one joint COUNT column over L looked-up values:
    hot       every X_k on every row is one table value, which two table rows hold (the combining path; a zero behind the head)
    distinct  the table keys are all different where 2^key_bits allows, every X_k a permutation of them
    period    the table keys repeat with period n / 4: the multiplicity on the first row, zeros behind it
    unlooked  half of the table values are looked up by nobody, and half of the X values are in no table row
    limb      X_k reads a LIMB column at the wrapping shift k mod 8; the table is an input column
    periodic  the table is a periodic column of n / 2 values"""
    rng = random.Random(f"{seed}/{n}/{L}/{key_bits}/{shape}")
    if shape == "limb":
        width = min(key_bits, 12)
        b = air.AirBuilder(4, [0], 1, main_inputs=2)
        m = b.main
        c = m.limb(m.load(0, 0), 3, width)
        shifts = [k % 8 if k < 8 else (3 * k + 1) % 8 for k in range(L)]
        m.multiplicity_many([m.load(s, c) for s in shifts], m.load(0, 1), key_bits)
        _trivial_constraint(b)
        values = pool(rng, width, n)
        return b, [[rng.randrange(P), values[rng.randrange(len(values))]] for _ in range(n)]
    if shape == "periodic":
        period = max(1, n // 2)
        table = _cycled(pool(rng, key_bits, period), period)
        b = air.AirBuilder(L + 1, [0], 1, periodic=[table], main_inputs=L)
        m = b.main
        m.multiplicity_many([m.load(0, k) for k in range(L)], m.periodic(0, 0), key_bits)
        _trivial_constraint(b)
        return b, [[table[rng.randrange(period)] for _ in range(L)] for _ in range(n)]
    b = air.AirBuilder(L + 2, [0], 1, main_inputs=L + 1)
    m = b.main
    m.multiplicity_many([m.load(0, k) for k in range(L)], m.load(0, L), key_bits)
    _trivial_constraint(b)
    if shape == "hot":
        keys = pool(rng, key_bits, n)
        t = [keys[rng.randrange(len(keys))] for _ in range(n)]
        hot = keys[0]
        t[n // 3] = t[n - 1] = hot
        return b, [[hot] * L + [t[i]] for i in range(n)]
    if shape == "distinct":
        keys = _cycled(pool(rng, key_bits, n), n)
        xs = []
        for _ in range(L):
            perm = list(keys)
            rng.shuffle(perm)
            xs.append(perm)
        t = list(keys)
        rng.shuffle(t)
        return b, [[xs[k][i] for k in range(L)] + [t[i]] for i in range(n)]
    if shape == "period":
        q = max(1, n // 4)
        values = _cycled(pool(rng, key_bits, q), q)
        return b, [[values[rng.randrange(q)] for _ in range(L)] + [values[i % q]] for i in range(n)]
    if shape == "unlooked":
        keys = pool(rng, key_bits, 2 * n)
        half, quarter = max(1, len(keys) // 2), len(keys) // 4
        table, looked = _cycled(keys[:half], n), keys[quarter:quarter + half]     # (they share the second quarter of the keys)
        rng.shuffle(table)
        return b, [[looked[rng.randrange(len(looked))] for _ in range(L)] + [table[i]] for i in range(n)]
    raise ValueError(shape)


def single(joint, key_bits=16):
    """Inputs x and t and one COUNT column of x in t: a list of one (joint) or the plain multiplicity column - the same table."""
    b = air.AirBuilder(3, [0], 1, main_inputs=2)
    m = b.main
    if joint:
        m.multiplicity_many([m.load(0, 0)], m.load(0, 1), key_bits)
    else:
        m.multiplicity(m.load(0, 0), m.load(0, 1), key_bits)
    _trivial_constraint(b)
    return b


def old_only():
    """Inputs x, y and t and two COUNT columns of the old form, the second over a shifted read of the first: nothing demands _multi."""
    b = air.AirBuilder(5, [0], 1, main_inputs=3)
    m = b.main
    c = m.multiplicity(m.load(0, 0), m.load(0, 2), 16)
    m.multiplicity(m.load(0, 1) + m.load(1, c), m.load(0, 2), 20)
    _trivial_constraint(b)
    return b


def lookup_rows(n, cols, key_bits, rng, span=None):
    """(n, cols) keys below 2^key_bits out of a pool of `span` (default n / 2) values: lookups that mostly hit."""
    keys = pool(rng, key_bits, span or max(1, n // 2))
    return [[keys[rng.randrange(len(keys))] for _ in range(cols)] for _ in range(n)]


def plain_joint():
    """No periodic column, no stride and no auxiliary segment, so the CPU oracle can prove the same table: inputs x0, x1 and the table
    value t; m = the joint multiplicity of (x0, x1 + 1) in t under 16 key bits, then v = x0 x1 (VALUE).  One real constraint on every
    row, v - x0 x1 = 0 (degree 2 under degree_bound_factor 1, as in air.dummy)."""
    b = air.AirBuilder(5, [0], 1, main_inputs=3)
    m = b.main
    x0, x1, t = m.load(0, 0), m.load(0, 1), m.load(0, 2)
    m.multiplicity_many([x0, x1 + 1], t, 16)
    v = m.value(x0 * x1)
    b.constraint(b.load(0, v) - b.load(0, 0) * b.load(0, 1), degree=2, exemptions=0)
    return b
