"""AIRs with periodic columns for the periodic-column tests, their trace generators, and the rewrite of such an AIR whose periodic
columns hold one value each into the same AIR over constants (what the CPU oracle, which has no periodic columns, can prove)."""
import random

from lambdaworks_cairo_prover_amd import air

P = air.P


def keys(seed, period):
    rng = random.Random(seed)
    return [rng.randrange(P) for _ in range(period)]


def to_bytes(rows):
    return air.ints_to_bytes(rows)


def mimc(n, period, seed=1, same=False):
    """(builder, trace rows): air.mimc_chain with random keys, or with one random key `period` times (same=True)."""
    k = keys(seed, 1) * period if same else keys(seed, period)
    return air.mimc_chain(n, period, 3, k), air.mimc_chain_trace(n, 3, k)


def linear(n, k0, k1):
    """Two columns, degree-1 constraints, composition degree bound n: a' = a + K0(row 0), b' = b + a + K1(row 1) - K1 is read at
    the NEXT row's point."""
    b = air.AirBuilder(2, [0, 1], 1, periodic=[k0, k1])
    b.constraint(b.load(1, 0) - b.load(0, 0) - b.periodic(0, 0), degree=1, exemptions=1)
    b.constraint(b.load(1, 1) - b.load(0, 1) - b.load(0, 0) - b.periodic(1, 1), degree=1, exemptions=1)
    b.boundary(0, 0, 5); b.boundary(1, 0, 7)
    rows, x, y = [], 5, 7
    for i in range(n):
        rows.append([x, y])
        x, y = (x + k0[i % len(k0)]) % P, (y + x + k1[(i + 1) % len(k1)]) % P
    return b, rows


SELECTOR = [1, 0, 0, 0]


def wrap(n, k):
    """One column over the frame rows (i, i + 2, i + 5): x_(i+5) = x_(i+2) + K_i x_i + K_(i+5) + S_(i+2) x_(i+2) with the period-4
    selector S = (1, 0, 0, 0): K is read at frame rows 0 and 2, S at frame row 1, so (row + offset) mod period wraps."""
    b = air.AirBuilder(1, [0, 2, 5], 1, periodic=[k, SELECTOR])
    x0, x2, x5 = b.load(0, 0), b.load(1, 0), b.load(2, 0)
    b.constraint(x5 - x2 - b.periodic(0, 0) * x0 - b.periodic(2, 0) - b.periodic(1, 1) * x2, degree=2, exemptions=5)
    xs = [2, 3, 5, 7, 11]
    for i, v in enumerate(xs):
        b.boundary(0, i, v)
    for i in range(n - 5):
        xs.append((xs[i + 2] + k[i % len(k)] * xs[i] + k[(i + 5) % len(k)] + SELECTOR[(i + 2) % 4] * xs[i + 2]) % P)
    return b, [[v] for v in xs]


def rap_with_selector(n):
    """fibonacci_rap_program's permutation column (an aux program on the device) beside a transition constraint that reads a periodic
    selector: a_(i+2) = a_(i+1) + a_i (1 + S_i); b is a rotated by one row; z_0 = 1, z_(i+1) (b_i + gamma) = z_i (a_i + gamma)."""
    b = air.AirBuilder(2, [0, 1, 2], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, num_transition_exemptions=2, periodic=[SELECTOR])
    a0 = b.load(0, 0)
    b.constraint(b.load(2, 0) - b.load(1, 0) - a0 * (b.periodic(0, 0) + 1), 2, 2)
    gamma = b.rap(0)
    b.constraint(b.load(1, 2) * (b.load(0, 1) + gamma) - b.load(0, 2) * (b.load(0, 0) + gamma), 2, 1)
    b.boundary(0, 0, 1); b.boundary(0, 1, 1); b.boundary(2, 0, 1)
    g = b.aux.rap(0)
    b.aux.product(b.aux.load(0, 0) + g, b.aux.load(0, 1) + g)
    a = [1, 1]
    for i in range(n - 2):
        a.append((a[i + 1] + a[i] * (1 + SELECTOR[i % 4])) % P)
    return b, [[a[i], a[(i + 1) % n]] for i in range(n)]


def with_constants(b):
    """The same AIR with every periodic read replaced by a constant: the value the column holds everywhere (its values must be equal)."""
    c = air.AirBuilder(b.main_cols, b.offsets, b.degree_bound_factor, aux_cols=b.aux_cols, n_rap=b.n_rap, aux_kind=b.aux_kind,
                       num_transition_exemptions=b.num_transition_exemptions, aux_builder=b.aux_builder)
    c.consts, c.degrees, c.exemptions, c.bcs = list(b.consts), list(b.degrees), list(b.exemptions), list(b.bcs)
    for op, x, y in b.ops:
        if op == air.OP_PERIODIC:
            values = b.periodic_cols[y]
            assert len(set(values)) == 1
            if values[0] not in c.consts:
                c.consts.append(values[0])
            c.ops.append((air.OP_CONST, c.consts.index(values[0]), 0))
        else:
            c.ops.append((op, x, y))
    return c


def changed(b, column=0, index=0):
    """A copy of the builder's periodic columns with one value changed (+1)."""
    cols = [list(v) for v in b.periodic_cols]
    cols[column][index] = (cols[column][index] + 1) % P
    return cols
