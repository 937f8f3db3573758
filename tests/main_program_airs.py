"""Program AIRs with a main-trace program (AirBuilder(..., main_inputs=I)) for the tests, beside the two worked examples of air.py:
every kind of derived column in one program, bits of chosen operands, and statements that put a main program beside an auxiliary
program and beside periodic columns with a stride.  Each comes with a helper that returns its INPUT rows only."""
from lambdaworks_cairo_prover_amd import air

P = air.P


def _trivial_constraint(b):
    """The table-only tests need a well-formed AIR around their main program, not a meaningful one."""
    x = b.load(0, 0)
    b.constraint(x - x, degree=1, exemptions=0)


def all_kinds():
    """Two inputs x (with zeros) and y (never zero), sixteen derived columns in three dependency levels - every kind, VALUE / SUM /
    PRODUCT with and without a denominator, shifts 0, 1 and 7 (7 wraps around the last rows), a run of four scanned columns of both
    kinds, and columns that read scanned columns of the level before at a shift.  Returns (builder, {name: main column})."""
    b = air.AirBuilder(18, [0], 1, main_inputs=2)
    m = b.main
    x, y = m.load(0, 0), m.load(0, 1)
    c = {}
    c["v0"] = m.value(x * y + m.load(7, 0))
    c["v1"] = m.value(x, y)
    c["iz"] = m.inv_or_zero(x)
    c["b0"] = m.bit(x, 0)
    c["b5"] = m.bit(x, 5)
    c["by"] = m.bit(y, 200)
    c["s0"] = m.running_sum(x)
    c["s1"] = m.running_sum(x, y)
    c["p0"] = m.product(y)
    c["p1"] = m.product(y + 3, m.load(1, 1))
    # level 2: reads level 1, scanned columns at a shift among them
    c["w"] = m.value(m.load(7, c["s1"]) * m.load(0, c["p1"]) + m.load(0, c["b5"]))
    c["iz2"] = m.inv_or_zero(m.load(0, c["iz"]))
    c["s2"] = m.running_sum(m.load(7, c["v0"]), m.load(0, c["p0"]))
    # level 3: reads level 2
    c["u"] = m.value(m.load(7, c["w"]) - m.load(0, c["s2"]))
    c["p2"] = m.product(m.load(0, c["iz2"]) + 1)
    c["b2"] = m.bit(m.load(7, c["s2"]), 100)
    _trivial_constraint(b)
    return b, c


def all_kinds_inputs(n, rng):
    """x zero on rows 0, n - 1 and every ninth row, y never zero."""
    return [[0 if i in (0, n - 1) or i % 9 == 4 else rng.randrange(P), 1 + rng.randrange(P - 1)] for i in range(n)]


BIT_OPERANDS = (0, 1, 1 << 63, (1 << 64) - 1, 1 << 192, P - 1, 1 << 251, (1 << 32) | (1 << 31))
BIT_POSITIONS = (0, 31, 32, 63, 64, 191, 192, 251)


def chosen_bits():
    """One input column (BIT_OPERANDS, one per row) and the bits BIT_POSITIONS of it."""
    b = air.AirBuilder(1 + len(BIT_POSITIONS), [0], 1, main_inputs=1)
    x = b.main.load(0, 0)
    for j in BIT_POSITIONS:
        b.main.bit(x, j)
    _trivial_constraint(b)
    return b


def reciprocal():
    """One input x, one derived column 1 / x: VALUE(1, x) - a zero x is a zero denominator."""
    b = air.AirBuilder(2, [0], 1, main_inputs=1)
    b.main.value(1, b.main.load(0, 0))
    b.constraint(b.load(0, 0) * b.load(0, 1) - 1, degree=2, exemptions=0)
    return b


def rotation_permutation():
    """A main program beside an auxiliary program: input x, derived d_i = x_(i+1) (VALUE of a shifted load, wrapping), and the grand
    product z_0 = 1, z' (gamma - d) = z (gamma - x) on every row - the last wraps to z_0 = 1, so d is a permutation of x.  The second
    constraint ties d to the next row's x."""
    b = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, main_inputs=1)
    d = b.main.value(b.main.load(1, 0))
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (gamma - b.load(0, d)) - b.load(0, 2) * (gamma - b.load(0, 0)), degree=2, exemptions=0)
    b.constraint(b.load(0, d) - b.load(1, 0), degree=1, exemptions=0)
    b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(g - b.aux.load(0, 0), g - b.aux.load(0, d))
    return b


STRIDE = 4


def strided_square_chain(n, x0, keys):
    """A main program beside a periodic column and a stride (through sp_air_ext): input x, derived s = x^2; on the rows = 0 (mod 4)
    x' = s + K_(i mod period) with the last row of that progression exempt, the rows between free; s = x x on every row."""
    b = air.AirBuilder(2, [0, 1], 2, periodic=[keys], main_inputs=1)
    xm = b.main.load(0, 0)
    s = b.main.value(xm * xm)
    b.constraint(b.load(1, 0) - (b.load(0, s) + b.periodic(0, 0)), degree=1, exemptions=1, period=STRIDE, offset=0)
    b.constraint(b.load(0, s) - b.load(0, 0) * b.load(0, 0), degree=2, exemptions=0)
    b.boundary(0, 0, x0)
    return b


def strided_square_chain_inputs(n, x0, keys, rng):
    rows, x = [], x0 % P
    for i in range(n):
        rows.append([x])
        x = (x * x + keys[i % len(keys)]) % P if i % STRIDE == 0 else rng.randrange(P)
    return rows
