"""Seeded chain groups with integer ops (air.MainProgram.int_limb / int_and / int_or / int_xor, ops 8 .. 11, sp_air_prove_int), drawn
through the public builder API: widths 1 .. 16, integer ops in seeds and in steps, beside op 7 and periodic reads or without them,
linked and unlinked.  The LIMB immediates come from EDGES - funnel shifts across a limb boundary, whole-limb shifts by 4, 2 and 1
limbs, the widest limb -, the AND / OR / XOR operands include 2^251 - 1, and the inputs are drawn again until the plain reference
(int_chain_ref) meets no error on them.  Beside them a program the CPU oracle can prove (plain_int) and the case of the worked example
air.arx_chain."""
import random

import int_chain_ref as R
from lambdaworks_cairo_prover_amd import air

P = air.P
# (lo, width): bit 0, the last bit of limb 0, the first and second of limb 1, the top bit, the whole value, a funnel shift out of limb 0
# into limb 2, a whole-limb shift by 7 = 4 + 2 + 1 limbs, by 3 = 2 + 1 with 64 bits, by 5 = 4 + 1 with 91
EDGES = [(0, 1), (31, 1), (32, 1), (33, 1), (251, 1), (0, 252), (30, 40), (224, 28), (96, 64), (160, 91)]
TOP = (1 << 251) - 1             # the largest operand of AND, OR and XOR
K1_PERIOD, K2_PERIOD = 4, 64
SEEDS = list(range(16))          # the CPU tests' seed list: seed -> width seed + 1, every width once


def periodic_columns(rng):
    """Two periodic columns below 2^251: period 4 (below the block lengths 8 and 64, above 2) and period 64."""
    return [[rng.randrange(TOP + 1) for _ in range(K1_PERIOD)], [rng.randrange(TOP + 1) for _ in range(K2_PERIOD)]]


def group(seed, s, link=1, periodic=None, div=False, width=None):
    """One chain group of `width` columns (seed % 16 + 1 when None) in blocks of s rows, runs of `link` blocks, over the inputs a (column
    0) and c (column 1); periodic: the two value lists of periodic_columns, or None for a program without op 6; div: op 7 beside the
    integer ops.  Every seed and every next value goes through an integer op, which recipe by the seed's own generator; the LIMB
    immediates walk EDGES from an offset the seed gives, so a group of ten columns meets them all and sixteen seeds meet each often.
    Behind the group a VALUE column reads it (a row-local column behind integer ops' results, not behind the ops).  One trivial
    constraint: the table tests need a well-formed AIR around the program.  Returns the builder."""
    rng = random.Random(0x1a7 + seed)
    w = seed % 16 + 1 if width is None else width
    b = air.AirBuilder(3 + w, [0], 1, periodic=periodic or (), main_inputs=2)
    m = b.main
    a, a3, c = m.load(0, 0), m.load(3, 0), m.load(0, 1)
    k1 = m.periodic(0, 0) if periodic else m.const(rng.randrange(TOP + 1))
    k2n = m.periodic(1, 1) if periodic else m.const(rng.randrange(TOP + 1))
    top = m.const(TOP)
    edge = lambda j: EDGES[(seed + j) % len(EDGES)]

    def recipe(x, y, j, extra, always=False):
        """A value built from x, y (values of the state, the carry or the inputs) with at least one integer op; extra: a field value
        that keeps the state from collapsing onto a few small integers; always: with div, divide whatever the generator says (the
        step of column 0: a group with div holds an op 7 at every width)."""
        pick = rng.randrange(6)
        lo, width = edge(j)
        if pick == 0:
            v = m.int_limb(x * y + extra, lo, width) + extra
        elif pick == 1:
            v = m.int_xor(x, y) * 3 + extra
        elif pick == 2:
            v = m.int_and(x, top) + m.int_or(y, m.int_limb(extra, lo, width))
        elif pick == 3:
            v = m.int_rotl(m.int_limb(x, 0, 64), 7 + j, 64) + m.int_add(y, extra, 250)
        elif pick == 4:
            v = m.int_or(m.int_limb(x, lo, width), m.int_and(y, extra)) + x
        else:
            v = m.int_xor(m.int_limb(x + y, 0, 251), top) - extra
        if div and (rng.randrange(2) or always):
            v = v / (m.int_limb(y, 0, 250) + (j + 1))      # a quotient over an integer op, zero with the probability of a field element
            if rng.randrange(2):
                v = m.int_limb(v, lo, width) + extra       # ... and an integer op over a quotient
        return v

    if link > 1:
        g = m.chain(s, None, width=w, link=link)
        g.seed([recipe(g.carry(j) + a, g.carry((j + 1) % w) + c, j, a3 + j) for j in range(w)])
    else:
        g = m.chain(s, [recipe(a + j, c, j, a3 + k1) for j in range(w)])
    x = [g.state(j) for j in range(w)]
    g.step([recipe(x[j], x[(j + 1) % w] + a3, j + 3, k1 + k2n * (j + 1), always=j == 0) for j in range(w)])
    m.value(m.load(0, g.cols[0]) * m.load(1, g.cols[w - 1]) + k1)
    v = b.load(0, 0)
    b.constraint(v - v, degree=1, exemptions=0)
    return b


def inputs(b, n, rng):
    """(input rows, the reference's table): rows from rng on which the reference meets no error - drawn again until it says so (with
    elements of a 252-bit field the first draw does: an operand reaches 2^251 with probability 2^-55), and asserted."""
    for _ in range(8):
        rows = [[rng.randrange(P), rng.randrange(P)] for _ in range(n)]
        try:
            return rows, R.main_table(b.main, rows)
        except (R.WordOutOfRange, R.ZeroDenominator):
            continue
    raise AssertionError("int_chain_programs.inputs: eight draws in a row met an error")


def poly_only(s):
    """A program without integer ops (through the _rec entry points): what runs between two calls of one with them."""
    b = air.AirBuilder(3, [0], 1, main_inputs=1)
    m = b.main
    g = m.chain(s, [m.load(0, 0)])
    g.step([g.state(0) * g.state(0) + m.load(1, 0)])
    v = m.value(m.load(0, g.cols[0]) * 3)
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) * 3, degree=1, exemptions=0)
    return b


def plain_int(s, div=False):
    """No periodic column and no stride, so the CPU oracle can prove the same table: input a; a group of two columns with seeds
    x0 = limb(a, 0, 128), x1 = a xor a(i + 1), steps x0' = rotl(x0, 9) over 128 bits xor limb(x1, 64, 128), x1' = (x0 + x1 + a(i + 1)) and
    (2^251 - 1) (with div: x1' over x0 + 2 first); then v = x0 x1 (VALUE).  One real constraint on every row, v - x0 x1 = 0 (degree 2
    under degree_bound_factor 1, as in air.dummy)."""
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    a, a1 = m.load(0, 0), m.load(1, 0)
    g = m.chain(s, [m.int_limb(a, 0, 128), m.int_xor(m.int_limb(a, 0, 251), m.int_limb(a1, 0, 251))])
    x0, x1 = g.state(0), g.state(1)
    total = x0 + x1 + a1
    g.step([m.int_xor(m.int_rotl(x0, 9, 128), m.int_limb(x1, 64, 128)), m.int_and(m.int_limb(total / (x0 + 2) if div else total, 0, 251), TOP)])
    v = m.value(m.load(0, g.cols[0]) * m.load(0, g.cols[1]))
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) * b.load(0, g.cols[1]), degree=2, exemptions=0)
    return b


def range_case(s):
    """An input a; a one-column group with seed a and step x' = (x and a(i + 1)) + 1 - the AND's second operand is the input of the next
    row, so one input cell decides whether one row of one block is in range - and a second group y with seed a, step y' = 1 / (y - 7):
    a zero denominator where a block's seed is 7.  A VALUE behind them."""
    b = air.AirBuilder(4, [0], 1, main_inputs=1)
    m = b.main
    a, a1 = m.load(0, 0), m.load(1, 0)
    g = m.chain(s, [m.int_limb(a, 0, 250)])
    g.step([m.int_and(g.state(0), a1) + 1])
    h = m.chain(s, [a])
    h.step([m.const(1) / (h.state(0) - 7)])
    v = m.value(m.load(0, g.cols[0]) + m.load(0, h.cols[0]))
    b.constraint(b.load(0, v) - b.load(0, g.cols[0]) - b.load(0, h.cols[0]), degree=1, exemptions=0)
    return b


def arx_case(n, s, rng, wrong=0, bits=16):
    """(builder, input rows, keys, digest) of air.arx_chain with the true digest of block 0 (+ `wrong`)."""
    keys = [rng.randrange(1 << bits) for _ in range(s)]
    rows = air.arx_chain_inputs(n, s, rng, bits)
    digest = air.arx_chain_digest(rows[0], s, keys, bits)
    return air.arx_chain(n, s, keys, (digest + wrong) % P, bits), rows, keys, digest
