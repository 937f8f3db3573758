"""AIRs with public data inside a randomized argument for the sp_air_prove_pub tests: the two worked examples of air.py with traces,
a lookup with a shifted table read and a second auxiliary column, the rewrites that take such an AIR back to what the older entry
points and the CPU oracle prove (table reads as constants, boundary values frozen under known challenges, the auxiliary program as a
recording callback), and random boundary-value programs."""
import random

import periodic_airs
from lambdaworks_cairo_prover_amd import air

P = air.P
OPTIONS = (4, 3, 3, 1)


def keys(seed, count):
    rng = random.Random(seed)
    return [rng.randrange(1, P) for _ in range(count)]


def to_bytes(rows):
    return air.ints_to_bytes(rows)


# ---- the worked examples with traces ---------------------------------------------------------------------------------------------
def table_lookup(n, period, seed=1, same=False):
    """(builder, rows): air.table_lookup over `period` random table values (same=True: one value `period` times) and n random picks."""
    rng = random.Random(seed)
    table = keys(seed + 1000, 1) * period if same else keys(seed + 1000, period)
    return air.table_lookup(n, table), air.table_lookup_trace(n, table, [rng.choice(table) for _ in range(n)])


def public_permutation(n, length, seed=2, public=None):
    """(builder, rows): air.public_permutation with `length` random public values (or the list `public`); the trace is that of the seed's
    own list either way, so another `public` gives the statement a trace that does not satisfy it."""
    rng = random.Random(seed)
    own = keys(seed + 2000, length)
    order = list(range(n - 1))
    rng.shuffle(order)
    rows = air.public_permutation_trace(n, own, keys(seed + 3000, n - 1 - length), order)
    return air.public_permutation(n, own if public is None else public), rows


def changed(rows, cell):
    """A copy of the trace rows with one cell changed (+1)."""
    out = [list(r) for r in rows]
    out[cell[0]][cell[1]] = (out[cell[0]][cell[1]] + 1) % P
    return out


# ---- a lookup that reads the table `shift` rows ahead, beside an auxiliary column that reads no table --------------------------------
def shifted_lookup(n, period, shift, seed=3, same=False):
    """(builder, rows).  Main columns a, m; auxiliary columns s (main_cols + 0) and w (main_cols + 1):
      s' = s + m / (gamma - T_(i+shift)) - 1 / (gamma - a)   every row (it wraps and closes the sum), s_0 = 0
      w' = w + a                                              all rows but the last, w_0 = 0 - no table read, no denominator
    m_i counts the look-ups of table[(i + shift) mod period]: each distinct value's multiplicity on the first row that meets it."""
    rng = random.Random(seed)
    table = keys(seed + 1000, 1) * period if same else keys(seed + 1000, period)
    offsets = [0, 1] if shift == 0 else [0, 1, shift]
    b = air.AirBuilder(2, offsets, 2, aux_cols=2, n_rap=1, aux_kind=air.AUX_PROGRAM, periodic=[table])
    gamma = b.rap(0)
    ga, gt = gamma - b.load(0, 0), gamma - b.periodic(0 if shift == 0 else 2, 0)
    b.constraint((b.load(1, 2) - b.load(0, 2)) * gt * ga - b.load(0, 1) * ga + gt, degree=3, exemptions=0)
    # (declared quadratic: with one exempted row a term of declared degree 1 has 2n - 1 + 1 + 1 coefficients under the bound 2n, one
    # too many for the 2n-point path)
    b.constraint(b.load(1, 3) - b.load(0, 3) - b.load(0, 0), degree=2, exemptions=1)
    b.boundary(2, 0, 0); b.boundary(3, 0, 0)
    g = b.aux.rap(0)
    xa, xt = g - b.aux.load(0, 0), g - b.aux.table(shift, 0)
    b.aux.running_sum(b.aux.load(0, 1) * xa - xt, xt * xa)
    b.aux.running_sum(b.aux.load(0, 0))
    a = [rng.choice(table) for _ in range(n)]
    m = [0] * n
    for v in a:
        m[(table.index(v) - shift) % n] += 1
    return b, [[a[i], m[i]] for i in range(n)]


# ---- rewrites -------------------------------------------------------------------------------------------------------------------
def _copy(b, aux_kind, aux_builder=None, periodic=True):
    c = air.AirBuilder(b.main_cols, b.offsets, b.degree_bound_factor, aux_cols=b.aux_cols, n_rap=b.n_rap, aux_kind=aux_kind,
                       num_transition_exemptions=b.num_transition_exemptions, aux_builder=aux_builder,
                       periodic=b.periodic_cols if periodic else None)
    c.ops, c.consts, c.degrees, c.exemptions, c.bcs, c.strides = list(b.ops), list(b.consts), list(b.degrees), list(b.exemptions), list(b.bcs), list(b.strides)
    return c


def with_constants(b):
    """periodic_airs.with_constants (every periodic read of the constraint program becomes the constant its column holds) with the
    auxiliary program's table reads rewritten the same way: an AIR without periodic columns, which the CPU oracle proves."""
    c = periodic_airs.with_constants(b)
    p = c.aux
    p.consts, p.cols = list(b.aux.consts), list(b.aux.cols)
    p._const_at = {v: i for i, v in enumerate(p.consts)}
    for op, x, y in b.aux.ops:
        if op == air.OP_PERIODIC:
            values = b.periodic_cols[y]
            assert len(set(values)) == 1
            if values[0] not in p._const_at:
                p._const_at[values[0]] = len(p.consts)
                p.consts.append(values[0])
            p.ops.append((air.OP_CONST, p._const_at[values[0]], 0))
        else:
            p.ops.append((op, x, y))
    return c


def frozen(b, rap):
    """The same AIR with its boundary_from values as constants: those of b.resolve_boundary(rap).  What sp_air_prove_aux proves."""
    c = _copy(b, b.aux_kind)
    c.aux.ops, c.aux.consts, c.aux.cols, c.aux._const_at = list(b.aux.ops), list(b.aux.consts), list(b.aux.cols), dict(b.aux._const_at)
    c.bcs = b.resolved_bcs(rap)
    return c


def recording(b, rows, seen):
    """The same AIR through aux_kind AUX_CALLBACK - the existing path - with a callback that appends the challenges it is given to
    `seen` and evaluates b's auxiliary program in Python; boundary_from values stay the placeholder 0 (the challenges depend on the
    main commitment and the options only, so the proof this AIR yields need not verify to tell them)."""
    def build_aux(rap):
        seen.append(list(rap))
        return b.aux.evaluate(rows, rap)
    return _copy(b, air.AUX_CALLBACK, aux_builder=build_aux)


def sampled_rap(ctx, b, rows, options):
    """The RAP challenges a proof of (b, rows) under `options` samples, by proving recording(b, ...) on the existing entry points."""
    from lambdaworks_cairo_prover_amd import api
    seen = []
    desc, keep = recording(b, rows, seen).build()
    assert not air.needs_pub(desc)
    ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert len(seen) == 1 and len(seen[0]) == b.n_rap
    return seen[0]


# ---- a boundary value whose denominator a challenge can make zero --------------------------------------------------------------------
def boundary_over_difference(n, v):
    """(builder, rows): air.fibonacci_rap_program with the permutation column's first cell stated as z_0 = (gamma - v) / (gamma - v): 1
    under every challenge but v, where D = gamma - v is zero.  Column b repeats column a, so z is 1 on every row."""
    b = air.fibonacci_rap_program(n, n - 4)
    b.bcs.pop()                                             # z_0 = 1 as a constant ...
    d = b.public.rap(0) - v
    b.boundary_from(2, 0, d, d)                             # ... becomes (gamma - v) / (gamma - v)
    a = [1, 1]
    for i in range(n - 2):
        a.append((a[i] + a[i + 1]) % P)
    return b, [[a[i], a[i]] for i in range(n)]


# ---- random boundary-value programs ------------------------------------------------------------------------------------------------
def random_values_builder(seed, n_rap=3, n_ops=40, n_values=6):
    """An AirBuilder whose b.public is a random program (constants, challenges, + - *) and whose boundary_from entries name random ops
    of it, every other one without a denominator."""
    rng = random.Random(seed)
    b = air.AirBuilder(1, [0, 1], 1, n_rap=n_rap)
    vals = [b.public.const(rng.randrange(P)), b.public.rap(0)]
    while len(b.public.ops) < n_ops:
        kind = rng.randrange(5)
        if kind == 0:
            vals.append(b.public.const(rng.randrange(P)))
        elif kind == 1:
            vals.append(b.public.rap(rng.randrange(n_rap)))
        else:
            x, y = rng.choice(vals), rng.choice(vals)
            vals.append(x + y if kind == 2 else x - y if kind == 3 else x * y)
    for j in range(n_values):
        # (a denominator like x - x is zero under every challenge: a random constant on top makes that a 2^-251 event)
        b.boundary_from(0, j, rng.choice(vals), None if j % 2 else rng.choice(vals) + rng.randrange(1, P))
    return b
