"""Program AIRs whose main program holds limbs and bitwise words (air.MainProgram.limb / limbs / word_and / word_or / word_xor,
sp_air_prove_word) for the tests, beside the worked examples air.limb_range_check and air.word_ops.  Each comes with a helper that
returns its INPUT rows only."""
from lambdaworks_cairo_prover_amd import air
from lookup_airs import trivial

P = air.P

# (lo, width) of one LIMB group: single bits at both ends of a 32-bit limb, a limb boundary inside a 2-bit limb, whole 32-bit limbs, 64
# bits out of three source limbs, the top of the integer, the last bit, the whole value and the whole value but its lowest bit
LIMB_SPECS = [(0, 1), (31, 1), (31, 2), (0, 32), (32, 32), (31, 64), (16, 16), (200, 52), (251, 1), (0, 252), (1, 251)]
BIT_POSITIONS = [0, 31, 251]
DISTINCT_LIMBS = sum(v << (32 * l) for l, v in enumerate([0x01234567, 0x12345678, 0x23456789, 0x3456789a, 0x456789ab, 0x56789abc, 0x6789abcd, 0x0789abce]))
# rows 0 .. 5 and n - 1
LIMB_OPERANDS = [0, 1, P - 1, 1 << 251, (1 << 251) - 1, (17 << 192) + 1, DISTINCT_LIMBS]


def limb_group(specs=LIMB_SPECS, bit_positions=BIT_POSITIONS):
    """Input x (column 0); columns 1 .. len(specs) the LIMB columns of `specs` on x - one group -, then a BIT column of x per position."""
    b = air.AirBuilder(1 + len(specs) + len(bit_positions), [0], 1, main_inputs=1)
    m = b.main
    x = m.load(0, 0)
    for lo, width in specs:
        m.limb(x, lo, width)
    for j in bit_positions:
        m.bit(x, j)
    return trivial(b)


def limb_rows(n, rng):
    """(n, 1) rows: LIMB_OPERANDS on rows 0 .. 5 and n - 1, the rest from the whole field."""
    rows = [[rng.randrange(P)] for _ in range(n)]
    for i, v in enumerate(LIMB_OPERANDS[:-1]):
        rows[i] = [v]
    rows[n - 1] = [LIMB_OPERANDS[-1]]
    assert DISTINCT_LIMBS < P and len({(DISTINCT_LIMBS >> (32 * l)) & 0xffffffff for l in range(8)}) == 8
    return rows


def word_groups(bits, other):
    """Inputs x, y, u and v (columns 0 - 3): AND, OR and XOR of (x, y) over `bits` bits (columns 4 - 6, one group) and of (u, v) over
    `other` bits (columns 7 - 9, a second group)."""
    b = air.AirBuilder(10, [0], 1, main_inputs=4)
    m = b.main
    for first, width in ((0, bits), (2, other)):
        p, q = m.load(0, first), m.load(0, first + 1)
        m.word_and(p, q, width); m.word_or(p, q, width); m.word_xor(p, q, width)
    return trivial(b)


def word_rows(n, bits, other, rng):
    """(n, 4) rows below 2^bits and 2^other: rows 0, 1 and n - 1 hold (all ones, 0), (all ones, all ones) and (0, 0) in both pairs."""
    rows = [[rng.randrange(1 << bits), rng.randrange(1 << bits), rng.randrange(1 << other), rng.randrange(1 << other)] for _ in range(n)]
    for i, (p, q) in ((0, (1, 0)), (1, (1, 1)), (n - 1, (0, 0))):
        rows[i] = [p * ((1 << bits) - 1), q * ((1 << bits) - 1), p * ((1 << other) - 1), q * ((1 << other) - 1)]
    return rows


def many_limbs(count):
    """Input x; `count` LIMB columns of width 1 on x, bits 0 .. count - 1: one group, unless the chunk size cuts it."""
    b = air.AirBuilder(1 + count, [0], 1, main_inputs=1)
    b.main.limbs(b.main.load(0, 0), 1, count)
    return trivial(b)


SPLIT_SPECS = [(0, 16), (16, 16), (40, 60), (100, 152)]


def split_group(split):
    """Input x; the LIMB columns of SPLIT_SPECS on x.  With `split` a VALUE column (3 limb + 1) stands behind the second of them and reads
    it, which ends the chunk: the group is built in two parts.  Returns (builder, the main columns of the LIMB columns)."""
    b = air.AirBuilder(1 + len(SPLIT_SPECS) + (1 if split else 0), [0], 1, main_inputs=1)
    m = b.main
    x = m.load(0, 0)
    cols = []
    for j, (lo, width) in enumerate(SPLIT_SPECS):
        cols.append(m.limb(x, lo, width))
        if split and j == 1:
            m.value(m.load(0, cols[-1]) * 3 + 1)
    return trivial(b), cols


MIXED_BITS = 3


def mixed(s):
    """Inputs x, t and v (columns 0 - 2), t the keys 0 .. 7 of a table and v its values:

        l0, l1 = limb(x, 0, 3), limb(x, 100, 3)      LIMB, columns 3 and 4: one group
        w = word_xor(l0, l1, 3)                      WORD, column 5: reads both limbs (a chunk of its own)
        c: seed w + t, step c^2 + l1                 CHAIN in blocks of s rows, column 6: seeded from the WORD column
        m = multiplicity(l0, t, 3)                   COUNT, column 7: X is a limb
        r = running_sum(l0(i + 3))                   SUM, column 8: a limb at a shift that wraps on the last three rows
        f = fetch(l1, t, v, 3)                       FETCH, column 9: keyed by a limb"""
    b = air.AirBuilder(10, [0], 1, main_inputs=3)
    m = b.main
    x = m.load(0, 0)
    l0, l1 = m.limb(x, 0, MIXED_BITS), m.limb(x, 100, MIXED_BITS)
    w = m.word_xor(m.load(0, l0), m.load(0, l1), MIXED_BITS)
    g = m.chain(s, [m.load(0, w) + m.load(0, 1)])
    g.step([g.state(0) * g.state(0) + m.load(0, l1)])
    m.multiplicity(m.load(0, l0), m.load(0, 1), MIXED_BITS)
    m.running_sum(m.load(3, l0))
    m.fetch(m.load(0, l1), m.load(0, 1), m.load(0, 2), MIXED_BITS)
    return trivial(b)


def mixed_rows(n, rng):
    """(n, 3) rows [x, t, v]: x from the whole field, t = i mod 8 (every 3-bit key is in the table from 8 rows on), v from the field."""
    return [[rng.randrange(P), i % (1 << MIXED_BITS), rng.randrange(P)] for i in range(n)]


def verdicts():
    """Inputs x, t, v and y (columns 0 - 3): a VALUE 1 / (v - 5) (column 4), f = fetch(x, t, v) with 8 key bits (column 5) and a =
    word_and(x, y, 8) (column 6): a zero denominator, a missing key and a word operand out of range can meet in one call."""
    b = air.AirBuilder(7, [0], 1, main_inputs=4)
    m = b.main
    m.value(1, m.load(0, 2) - 5)
    m.fetch(m.load(0, 0), m.load(0, 1), m.load(0, 2), 8)
    m.word_and(m.load(0, 0), m.load(0, 3), 8)
    return trivial(b)


def verdicts_rows(n):
    """(n, 4) valid rows for verdicts(): keys i mod 50 on both sides, values 6 + i (never 5), y below 2^8."""
    return [[i % 50, i % 50 if i < 50 else 7, 6 + i, (3 * i) % 256] for i in range(n)]
