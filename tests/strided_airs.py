"""AIRs with strided transition constraints (AirBuilder.constraint(..., period, offset)) for the stride tests, with traces that satisfy
the constraints on the enforced rows only and hold random values elsewhere, the cells whose change breaks one enforced row, only
non-enforced rows, or only an exempted tail row of a progression, and the zerofier / exemption product in Python integers."""
import collections
import random

from lambdaworks_cairo_prover_amd import air

P = air.P
SIZES = [16, 64, 256]
OPTIONS = [(4, 3, 3, 1), (8, 3, 3, 1), (4, 4, 3, 2)]
# the field's 2^192-th root of unity (lambdaworks TWO_ADIC_PRIMITVE_ROOT_OF_UNITY), squared down to the order wanted
_ROOT_2_192 = 0x5282db87529cfa3f0464519c8b0fa5ad187148e11a61616070024f42f8ef94


def root(log_order):
    return pow(_ROOT_2_192, 1 << (192 - log_order), P)


def to_bytes(rows):
    return air.ints_to_bytes(rows)


def keys(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(count)]


Case = collections.namedtuple("Case", "builder rows enforced_cell enforced_row free_cell tail_cell")
# enforced_cell: (row, col) read on exactly one enforced row (enforced_row, by constraint 0 of the worked example / 1 of two_class)
# free_cell: read on non-enforced rows only;  tail_cell: read on an exempted tail row of a progression and otherwise on none enforced


def mimc(n, seed=1):
    """air.strided_mimc_chain (the worked example: stride (4, 0), one exempted row) with 8 random keys and random free rows."""
    rng = random.Random(seed)
    k = keys(seed + 1000, 8)
    b = air.strided_mimc_chain(n, 3, k)
    rows = air.strided_mimc_chain_trace(n, 3, k, lambda: rng.randrange(P))
    # cell x_5 is the "next" cell of row 4 (enforced) and the "current" cell of row 5 (free); x_6 touches rows 5, 6; x_(n-3) the
    # exempted row n - 4 and the free row n - 3
    return Case(b, rows, (5, 0), 4, (6, 0), (n - 3, 0))


def mimc_selector(n, seed=1):
    """The same statement and the same trace through the [1, 0, 0, 0] selector column."""
    c = mimc(n, seed)
    return air.strided_mimc_chain(n, 3, keys(seed + 1000, 8), selector=True), c.rows


def two_class(n, seed=2):
    """Frame offsets [0, 1, 4], degree bound n, two columns, three constraints:
      0  every row but the last:           b' = 2 b                              (column 1)
      1  rows = 1 (mod 4), one exempted:   a_(i+4) = a_i + a_(i+1)               (column 0)
      2  row n - 1 alone (period n):       a_3 = a_0 + a_(n-1)  - its frame wraps: rows n - 1, 0, 3
    Column 0 is random wherever no enforced row fixes it."""
    rng = random.Random(seed)
    b = air.AirBuilder(2, [0, 1, 4], 1)
    b.constraint(b.load(1, 1) - b.load(0, 1) * 2, degree=1, exemptions=1)
    b.constraint(b.load(2, 0) - b.load(0, 0) - b.load(1, 0), degree=1, exemptions=1, period=4, offset=1)
    b.constraint(b.load(2, 0) - b.load(0, 0) - b.load(1, 0), degree=1, exemptions=0, period=n, offset=n - 1)
    a = [rng.randrange(P) for _ in range(n)]
    for i in range(1, n - 4, 4):                      # the progression 1, 5, ... without its last row n - 3
        a[i + 4] = (a[i] + a[i + 1]) % P
    a[3] = (a[0] + a[n - 1]) % P
    b.boundary(0, 0, a[0]); b.boundary(1, 0, 7)
    rows = [[a[i], 7 * pow(2, i, P) % P] for i in range(n)]
    # a_6 is read on row 5 (enforced: i + 1) and on rows 6 and 2 (neither = 1 mod 4); a_7 on rows 7, 6, 3 only;
    # a_(n-2) on row n - 3 (the exempted tail of the progression) and on rows n - 2, n - 6
    return Case(b, rows, (6, 0), 5, (7, 0), (n - 2, 0))


def rap_with_stride(n, seed=3):
    """The shape of periodic_airs.rap_with_selector with the selector replaced by a stride: a_(i+2) = a_(i+1) + a_i K_i on the rows
    = 0 (mod 4) - K a period-8 periodic column -, the rows between free; b is a rotated by one row; the permutation column
    z_0 = 1, z_(i+1) (b_i + gamma) = z_i (a_i + gamma) comes from an auxiliary program on the device.  Degree bound 2n: a strided
    constraint of degree 2 needs degree_bound_factor 2."""
    rng = random.Random(seed)
    k = keys(seed + 1000, 8)
    b = air.AirBuilder(2, [0, 1, 2], 2, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, num_transition_exemptions=2, periodic=[k])
    b.constraint(b.load(2, 0) - b.load(1, 0) - b.load(0, 0) * b.periodic(0, 0), degree=2, exemptions=1, period=4, offset=0)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 1)
    b.boundary(0, 0, 1); b.boundary(0, 1, 1); b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(b.aux.load(0, 0) + g, b.aux.load(0, 1) + g)
    a = [1, 1] + [rng.randrange(P) for _ in range(n - 2)]
    for i in range(0, n - 4, 4):
        a[i + 2] = (a[i + 1] + a[i] * k[i % 8]) % P
    return b, [[a[i], a[(i + 1) % n]] for i in range(n)]


def changed(rows, cell):
    """A copy of the trace rows with one cell changed (+1)."""
    out = [list(r) for r in rows]
    out[cell[0]][cell[1]] = (out[cell[0]][cell[1]] + 1) % P
    return out


def with_strides(desc, strides):
    """Attaches sp_air_stride_desc `strides` ([(period, offset), ...], or None: removes it) to a built descriptor; returns the keepalive."""
    if strides is None:
        if hasattr(desc, "stride_desc"):
            del desc.stride_desc
        return None
    desc.stride_desc, keep = air.stride_desc(strides)
    return keep


def degenerate(desc):
    """All strides (1, 0) on a built descriptor: the _ext entry points, today's statement."""
    return with_strides(desc, [(1, 0)] * desc.n_transitions)


def zerofier(period, offset, n, x):
    """Z(x) = x^(n/s) - g^(o n/s) in Python integers."""
    g = root(n.bit_length() - 1)
    return (pow(x, n // period, P) - pow(g, offset * (n // period), P)) % P


def exemption_product(period, offset, e, n, x):
    """E(x) = prod_{t<e} (x - g^(o + s (n/s - 1 - t))) in Python integers."""
    g, out = root(n.bit_length() - 1), 1
    for t in range(e):
        out = out * (x - pow(g, offset + period * (n // period - 1 - t), P)) % P
    return out


def malformed_stride_descs(b, n):
    """[(label, [(period, offset), ...] or a callable patching a built desc)]: every malformed stride descriptor of the C ABI for
    builder b (whose constraint 0 carries a stride) on n rows."""
    t = len(b.degrees)
    base = list(b._strides())

    def first(s):
        return [s] + base[1:]
    out = [("period not a power of two", first((6, 0))), ("period zero", first((0, 0))), ("period above n", first((2 * n, 0))),
           ("period 2^31", first((1 << 31, 0))), ("offset >= period", first((4, 4))), ("n != transitions", base + [(1, 0)]),
           ("n != transitions (fewer)", base[:-1] if t > 1 else [])]
    return out


def golden_case():
    """The AIR and trace of tests/golden/strided_n64.proof: the worked example on 64 rows, x0 = 3, keys and free rows of seed 64."""
    return mimc(64, seed=64)
