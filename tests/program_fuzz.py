"""Seeded generators of valid main and auxiliary programs (air.MainProgram, air.AuxProgram), built through the public builder API only,
with inputs under which the plain reference (program_ref) meets no error, and - computed from the program alone - the set of features a
program contains: the combinations of the host scheduler's paths (csrc/prover_programs.cpp: build_main_program, commit_aux_program) that no
hand-written AIR holds.

    random_main(seed, n) -> (AirBuilder with main_inputs=I, input rows, features)
    random_aux(seed, n)  -> (AirBuilder with aux_kind=AUX_PROGRAM, main rows, features)

One seed at one size is always the same program: random.Random seeded with a string.  A draw is rejected and drawn again (with the next
attempt number in the seed string) when more than 64 values would be alive at once, or when a denominator is zero on some row.
main_table(seed, n) / aux_columns(seed, n, rap) give the expected cells: program_ref up to 4096 rows, the Python model beyond (the CPU
tests hold the model to program_ref at small sizes).  To look at one seed: `python -c "import program_fuzz as F; print(F.describe_main(17, 64))"`
from tests/."""
import functools
import random

import lookup_airs as L
import program_ref as R
from lambdaworks_cairo_prover_amd import air

P = air.P
MAX_LIVE = 64                        # AIR_MAX_LIVE: the device's slot file
CHUNK_ELEMS = 1 << 22                # AUXP_CHUNK_ELEMS: a chunk holds max(1, 2^22 / n) columns
REF_MAX_N = 4096
KEY_BITS = (1, 8, 9, 16, 17, 64)
BIT_POSITIONS = (0, 31, 32, 63, 64, 250, 251)     # across all eight 32-bit limbs' ends
SHIFTS = (0, 0, 0, 1, 1, 2, 3, 5, 7)
GEN_RAP = (0x1234567, 0x89abcdef01, 3)            # the challenges the generator checks the denominators under
ATTEMPTS = 40

# The fixed seed lists.  test_air_program_fuzz.py holds the models to the reference over MAIN_SEEDS / AUX_SEEDS at 8, 64 and 256 rows and
# checks that they contain every combination below; test_gpu_air_program_fuzz.py runs them on the device at 8 and 64 rows (main), 64
# and 256 (auxiliary), and the few *_LARGE ones - chosen for short references - at the sizes where the sorts and scans take more blocks.
MAIN_SEEDS = list(range(24))
AUX_SEEDS = list(range(16))
MAIN_SEEDS_LARGE = {2048: [12, 14, 2], 4096: [6, 8, 15], 16384: [3, 2, 4]}
AUX_SEEDS_LARGE = {2048: [6, 5], 4096: [11, 8], 16384: [1, 3]}

# what the coverage test asks of the fixed seed lists (the combinations of the issue's point 6, by name)
MAIN_FEATURES = ("bits_split_by_chunk_end_beside_inv_or_zero", "scan_directly_behind_bit_group", "count_reads_chain_at_wrapping_shift",
                 "periodic_read_in_one_chunk_not_the_next", "constant_shared_by_chunks")
MAIN_SHAPES = ("no_periodic_columns", "three_dependency_levels", "chain_width_16", "chain_block_length_n")
AUX_FEATURES = ("sort_groups_of_different_key_bits_read_together", "constant_shared_by_chunks", "periodic_read_in_one_chunk_not_the_next")


# ---- what the host makes of a program: live values, chunks ------------------------------------------------------------------
def max_live(ops, roots=None):
    """An upper bound of the slots air_assign_slots needs for any selection of this op list: every value lives from its definition to
    its last use by an op (a column's OUT stands directly behind its op), operands that die at an op free their slots before its result
    takes one, and no op is dropped.  The host only drops values, so no program it derives for a chunk needs more.  With roots - the
    ops whose values are stored - the count for that selection itself: what no root needs is dropped, as the host drops it."""
    kept = set(range(len(ops))) if roots is None else closure(ops, roots)
    last = list(range(len(ops)))
    for t, (op, a, b) in enumerate(ops):
        if t in kept and op in (air.OP_ADD, air.OP_SUB, air.OP_MUL):
            last[a], last[b] = t, t
    dying = [0] * len(ops)
    for t in kept:
        if last[t] != t:
            dying[last[t]] += 1
    most = alive = 0
    for t in sorted(kept):
        alive += 1 - dying[t]            # (values whose last use is op t are read before its result is written)
        most = max(most, alive)
        if last[t] == t:                 # a value no op reads takes a slot until it is stored
            alive -= 1
    return most


def closure(ops, roots):
    """The ops the values `roots` depend on."""
    seen, stack = set(), [r for r in roots if r != air.AUX_NO_DEN]
    while stack:
        t = stack.pop()
        if t in seen:
            continue
        seen.add(t)
        if ops[t][0] in (air.OP_ADD, air.OP_SUB, air.OP_MUL):
            stack += [ops[t][1], ops[t][2]]
    return seen


def main_chunks(m, n):
    """The chunks build_main_program cuts the derived columns into: [(kind, k0, kc)], kind "chain", "count" or "rows".  A chain group
    and a COUNT column are chunks of their own; a row-local chunk ends at max(1, 2^22 / n) columns and before a column that reads a
    derived column of the chunk itself (at any shift)."""
    K, reads = len(m.cols), m.reads()
    size = max(1, min(K, CHUNK_ELEMS // n))
    col_reads = [max(reads[num], reads[den] if den != air.AUX_NO_DEN else 0) for _, num, den, _ in m.cols]
    chunks, k0 = [], 0
    while k0 < K:
        kind = m.cols[k0][0]
        kc = 1
        if kind == air.MAIN_CHAIN:
            while k0 + kc < K and m.cols[k0 + kc][0] == air.MAIN_CHAIN and m.cols[k0 + kc][3] >> 8:
                kc += 1
            chunks.append(("chain", k0, kc))
        elif kind == air.MAIN_COUNT:
            chunks.append(("count", k0, 1))
        else:
            kc = 0
            while kc < size and k0 + kc < K and col_reads[k0 + kc] <= k0 and m.cols[k0 + kc][0] not in (air.MAIN_CHAIN, air.MAIN_COUNT):
                kc += 1
            chunks.append(("rows", k0, kc))
        k0 += kc
    return chunks


def _chunk_ops(ops, cols, k0, kc):
    return closure(ops, [t for c in cols[k0:k0 + kc] for t in c[1:3]])


def _seam_features(ops, per_chunk):
    """From the op sets of consecutive chunks: a constant two chunks share, a periodic read that one chunk has and the next has not."""
    found = set()
    consts = [{ops[t][1] for t in s if ops[t][0] == air.OP_CONST} for s in per_chunk]
    if any(consts[i] & consts[j] for i in range(len(consts)) for j in range(i)):
        found.add("constant_shared_by_chunks")
    per = [any(ops[t][0] == air.OP_PERIODIC for t in s) for s in per_chunk]
    if any(per[i] and not per[i + 1] for i in range(len(per) - 1)):
        found.add("periodic_read_in_one_chunk_not_the_next")
    return found


def main_features(m, n):
    """Which of MAIN_FEATURES and MAIN_SHAPES the main program holds, from its lists alone."""
    I, ops, cols = m.input_cols, m.ops, m.cols
    chunks = main_chunks(m, n)
    per_chunk = [_chunk_ops(ops, cols, k0, kc) for _, k0, kc in chunks]
    found = _seam_features(ops, per_chunk)
    if not m.periodic_cols:
        found.add("no_periodic_columns")
    chunk_of = {k: i for i, (_, k0, kc) in enumerate(chunks) for k in range(k0, k0 + kc)}
    # BIT columns on one N in two chunks, one of which also holds an INV_OR_ZERO
    by_num = {}
    for k, (kind, num, _, _) in enumerate(cols):
        if kind == air.MAIN_BIT:
            by_num.setdefault(num, set()).add(chunk_of[k])
    with_inv = {chunk_of[k] for k, c in enumerate(cols) if c[0] == air.MAIN_INV_OR_ZERO}
    if any(len(where) > 1 and where & with_inv for where in by_num.values()):
        found.add("bits_split_by_chunk_end_beside_inv_or_zero")
    for k in range(1, len(cols)):
        if cols[k][0] in (air.MAIN_SUM, air.MAIN_PRODUCT) and cols[k - 1][0] == air.MAIN_BIT and chunk_of[k] == chunk_of[k - 1]:
            found.add("scan_directly_behind_bit_group")
    chain_cols = {I + k for k, c in enumerate(cols) if c[0] == air.MAIN_CHAIN}
    for kind, num, _, _ in cols:
        if kind == air.MAIN_COUNT and any(ops[t][0] == air.OP_LOAD and ops[t][1] > 0 and ops[t][2] in chain_cols for t in closure(ops, [num])):
            found.add("count_reads_chain_at_wrapping_shift")
    level = []
    for k, c in enumerate(cols):
        read = {ops[t][2] - I for t in closure(ops, c[1:3]) if ops[t][0] == air.OP_LOAD and I <= ops[t][2] < I + k}
        level.append(1 + max((level[j] for j in read), default=0))
    if max(level) >= 3:
        found.add("three_dependency_levels")
    for kind, k0, kc in chunks:
        if kind == "chain":
            if kc == air.MAIN_CHAIN_MAX_WIDTH:
                found.add("chain_width_16")
            if 1 << (cols[k0][3] & 255) == n:
                found.add("chain_block_length_n")
    return found


def aux_chunks(x, n):
    """The chunks commit_aux_program cuts the products and sums into: [(k0, kc)] - runs between sorted columns, at most a chunk long."""
    K = len(x.cols)
    size = max(1, min(K, CHUNK_ELEMS // n))
    chunks, k0 = [], 0
    while k0 < K:
        if x.cols[k0][0] == air.AUX_SORTED:
            k0 += 1
            continue
        kc = 0
        while kc < size and k0 + kc < K and x.cols[k0 + kc][0] != air.AUX_SORTED:
            kc += 1
        chunks.append((k0, kc))
        k0 += kc
    return chunks


def aux_features(x, n):
    ops, cols = x.ops, x.cols
    found = _seam_features(ops, [_chunk_ops(ops, cols, k0, kc) for k0, kc in aux_chunks(x, n)])
    group_of = {k: key for key, members in x.sort_groups().items() for k in members}
    for kind, num, den in cols:
        if kind == air.AUX_SORTED:
            continue
        read = {group_of[ops[t][2] - x.main_cols] for t in closure(ops, [num, den]) if ops[t][0] == air.OP_LOAD and ops[t][2] >= x.main_cols}
        if len({x.key_bits[x.sort_groups()[key][0]] for key in read}) > 1:
            found.add("sort_groups_of_different_key_bits_read_together")
    return found


# ---- expressions -----------------------------------------------------------------------------------------------------------
class _Exprs:
    """Expression DAGs over leaves and a bounded pool of earlier values, each value with the highest column (+ 1) it depends on."""

    def __init__(self, rng, leaf, pool_size=16):
        self.rng, self.leaf, self.pool, self.pool_size = rng, leaf, [], pool_size

    def keep(self, v, top):
        self.pool.append((v, top))
        if len(self.pool) > self.pool_size:
            self.pool.pop(self.rng.randrange(len(self.pool)))

    def value(self, depth, below):
        """A value that reads columns < below only."""
        rng = self.rng
        usable = [e for e in self.pool if e[1] <= below]
        if depth == 0 or rng.random() < 0.2:
            if usable and rng.random() < 0.35:
                return rng.choice(usable)
            return self.leaf(below)
        (a, ta), (b, tb) = self.value(depth - 1, below), self.value(depth - 1, below)
        v = rng.choice([lambda: a + b, lambda: a - b, lambda: a * b, lambda: a * b])()
        if rng.random() < 0.5:
            self.keep(v, max(ta, tb))
        return v, max(ta, tb)


def _constant(rng):
    return rng.choice([0, 1, P - 1, 2, 3, rng.randrange(1 << 16), rng.randrange(P), rng.randrange(P)])


def _periodic_columns(rng, n, most):
    out = []
    for _ in range(rng.randint(0, most)):
        period = 1 << rng.randint(0, min(n.bit_length() - 1, 6))
        out.append([rng.choice([0, 1, rng.randrange(P), rng.randrange(1 << 20)]) for _ in range(period)])
    return out


# ---- main programs -----------------------------------------------------------------------------------------------------------
def _main_inputs(rng, n, I, kb):
    """Column 0: looked-up values below 2^kb with duplicates and both ends of the range; column 1: table values, some of them never
    looked up, and not all looked-up values; column 2: field elements.  The column INV_OR_ZERO operands are multiples of (2 when there
    is one, else 0) is zero on rows 0, n - 1 and on the rows 64 .. 127 when the trace has them."""
    top = (1 << kb) - 1
    both = [0, top] + [rng.randrange(top + 1) for _ in range(4)]
    only_x = [rng.randrange(top + 1) for _ in range(3)]
    only_t = [rng.randrange(top + 1) for _ in range(3)]
    rows = []
    for _ in range(n):
        row = [rng.choice(both + only_x), rng.choice(both + both + only_t), rng.randrange(P)][:I]
        rows.append(row)
    zc = 2 if I == 3 else 0
    for i in [0, n - 1] + (list(range(64, 128)) if n >= 128 else []):
        rows[i][zc] = 0
    return rows, zc


def _draw_main(rng, n):
    I, K = rng.randint(1, 3), rng.randint(4, 40)
    periodic = _periodic_columns(rng, n, 3)
    kb = rng.choice(KEY_BITS)
    b = air.AirBuilder(I + K, [0], 1, periodic=periodic, main_inputs=I)
    m = b.main
    rows, zc = _main_inputs(rng, n, I, kb)
    state = {"limit": None}          # a chain step reads columns before its group at shifts != 0, its own at shift 0 (g.state)

    def ncols():
        return I + len(m.cols) if state["limit"] is None else state["limit"]

    def leaf(below):
        r = rng.random()
        if r < 0.6:
            col = rng.randrange(min(below, ncols()))
            return m.load(rng.choice(SHIFTS), col), col + 1
        if r < 0.8 or not periodic:
            return m.const(_constant(rng)), 0
        return m.periodic(rng.choice(SHIFTS), rng.randrange(len(periodic))), 0

    ex = _Exprs(rng, leaf)
    base = I                          # the first column of the chunk being filled: a column that reads at or above it starts the next
    small_chains = []                 # chain columns that hold values below 2^kb (rotations of looked-up inputs)
    bit_operands = []
    n_count = 0

    def room():
        return K - len(m.cols)

    def below():
        """Mostly the columns before the chunk (the column joins it); sometimes all of them (a dependency ends the chunk)."""
        return base if rng.random() < 0.7 else I + len(m.cols)

    def placed(top):
        nonlocal base
        if top > base:
            base = I + len(m.cols) - 1

    def denominator(lim):
        d, top = ex.value(rng.randint(0, 2), lim)
        return d + m.const(rng.randrange(1, P)), top

    while room() > 0:
        lim = below()
        kind = rng.choice(["value", "value", "value_d", "value_d", "inv", "bits", "bits", "sum", "sum_d", "product", "product_d", "chain", "count"])
        if kind in ("value", "sum", "product", "value_d", "sum_d", "product_d"):
            num, top = ex.value(rng.randint(0, 3), lim)
            den = None
            if kind.endswith("_d"):
                den, dtop = denominator(lim)
                top = max(top, dtop)
            {"v": m.value, "s": m.running_sum, "p": m.product}[kind[0]](num, den)
            placed(top)
        elif kind == "inv":
            x, top = ex.value(rng.randint(0, 2), lim)
            m.inv_or_zero(m.load(0, zc) * x if rng.random() < 0.8 else m.load(0, zc))
            placed(top)
        elif kind == "bits":
            if bit_operands and rng.random() < 0.4:
                x, top = rng.choice(bit_operands)     # an N that BIT columns further up hold already
            else:
                x, top = ex.value(rng.randint(0, 2), lim)
                bit_operands.append((x, top))
            for j in rng.sample(BIT_POSITIONS + tuple(range(1, 9)), min(room(), rng.randint(1, 8))):
                m.bit(x, j)
                placed(top)
        elif kind == "chain":
            width = min(room(), rng.choice([1, 1, 2, 3, 4, 8, 16, 16]))
            log = rng.choice([1, 1, 2, 3, n.bit_length() - 1, n.bit_length() - 1, rng.randint(1, n.bit_length() - 1)])
            first = I + len(m.cols)
            if rng.random() < 0.4:           # values below 2^kb, for a COUNT column to look up: a rotation of looked-up inputs
                g = m.chain(1 << log, [m.load(rng.choice(SHIFTS), 0) for _ in range(width)])
                g.step([g.state((j + 1) % width) for j in range(width)])
                small_chains += g.cols
            else:
                g = m.chain(1 << log, [ex.value(rng.randint(0, 2), first)[0] for _ in range(width)])
                state["limit"] = first
                nexts = []
                for j in range(width):
                    s, other = g.state(j), g.state(rng.randrange(width))
                    nexts.append(s * s + other * ex.value(1, first)[0] + ex.value(0, first)[0])
                g.step(nexts)
                state["limit"] = None
            base = I + len(m.cols)
        elif kind == "count" and n_count < 3:
            bits = kb if rng.random() < 0.5 else rng.choice([k for k in KEY_BITS if k >= kb])
            wide = bits >= kb + 2             # room for the sum of two looked-up values and a small constant
            if small_chains and rng.random() < 0.6:
                x = m.load(rng.choice([1, 2, 3, 5, 7]), rng.choice(small_chains))
            elif wide and rng.random() < 0.5:
                x = m.load(rng.choice(SHIFTS), 0) + m.load(rng.choice(SHIFTS), min(1, I - 1)) + rng.randrange(4)
            else:
                x = m.load(rng.choice(SHIFTS), 0)
            t = m.load(rng.choice(SHIFTS), min(1, I - 1))
            if wide and rng.random() < 0.5:
                t = t + m.load(rng.choice(SHIFTS), 0) + rng.randrange(4)
            m.multiplicity(x, t, bits)
            n_count += 1
            base = I + len(m.cols)
    return L.trivial(b), rows


def _accept(ops):
    return max_live(ops) <= MAX_LIVE


@functools.lru_cache(maxsize=None)
def _main(seed, n):
    for attempt in range(ATTEMPTS):
        b, rows = _draw_main(random.Random(f"main {seed} {n} {attempt}"), n)
        if not _accept(b.main.ops):
            continue
        try:
            table = R.main_table(b.main, rows) if n <= REF_MAX_N else [[int(v) for v in row] for row in b.main.evaluate(rows)]
        except (ZeroDivisionError, ValueError) as e:
            if "denominator" not in str(e):
                raise
            continue
        return b, rows, frozenset(main_features(b.main, n)), table
    raise RuntimeError(f"main seed {seed} at n = {n}: no valid program in {ATTEMPTS} draws")


def random_main(seed, n):
    return _main(seed, n)[:3]


def main_table(seed, n):
    """The expected main segment of random_main(seed, n): program_ref up to 4096 rows, MainProgram.evaluate beyond."""
    return _main(seed, n)[3]


def describe_main(seed, n):
    b, rows, features, _ = _main(seed, n)
    names = ["VALUE", "INV_OR_ZERO", "BIT", "SUM", "PRODUCT", "CHAIN", "COUNT"]
    lines = [f"main seed {seed}, n = {n}: {b.main.input_cols} inputs, {len(b.main.cols)} derived, {len(b.main.ops)} ops, "
             f"periods {[len(v) for v in b.periodic_cols]}, features {sorted(features)}", f"chunks {main_chunks(b.main, n)}"]
    lines += [f"  column {b.main.input_cols + k}: {names[c[0]]} N op {c[1]} D op {c[2]} pad {c[3]}" for k, c in enumerate(b.main.cols)]
    return "\n".join(lines)


# ---- auxiliary programs ------------------------------------------------------------------------------------------------------
def _aux_rows(rng, n, M, kb):
    """Column 0: sort keys below 2^kb with duplicates and both ends; column 1: 64-bit keys, 0 and 2^64 - 1 several times; field elements."""
    top = (1 << kb) - 1
    small = [0, top] + [rng.randrange(top + 1) for _ in range(6)]
    wide = [0, (1 << 64) - 1] + [rng.randrange(1 << 64) for _ in range(max(4, n // 4))]
    return [([rng.choice(small), rng.choice(wide)] + [rng.randrange(P) for _ in range(M - 2)]) for _ in range(n)]


def _draw_aux(rng, n, pinned):
    M, n_rap = rng.randint(2, 6), rng.randint(1, 3)
    periodic = _periodic_columns(rng, n, 2)
    kb = rng.choice([1, 8, 9, 16])
    # the plan first: the column count decides where the sorted columns lie behind the main columns
    plan = ["scan"] * rng.randint(3, 40) + [("sort", rng.randint(0, 4)) for _ in range(rng.randint(1, 4))]
    rng.shuffle(plan)
    K = sum(1 if p == "scan" else 1 + p[1] for p in plan)
    b = air.AirBuilder(M + (K if pinned else 0), [0], 1, aux_cols=K, n_rap=n_rap, aux_kind=air.AUX_PROGRAM, periodic=periodic)
    x = b.aux
    rows = _aux_rows(rng, n, M, kb)
    sorted_cols = []
    state = {"sorted": True}

    def leaf(below):
        r = rng.random()
        if r < 0.45:
            return x.load(rng.choice(SHIFTS), rng.randrange(M)), 0
        if r < 0.6:
            return x.const(_constant(rng)), 0
        if r < 0.75:
            return x.rap(rng.randrange(n_rap)), 0
        if r < 0.85 and periodic:
            return x.table(rng.choice(SHIFTS), rng.randrange(len(periodic))), 0
        if sorted_cols and state["sorted"]:
            return x.sorted_load(rng.choice(SHIFTS), rng.choice(sorted_cols)), 1
        return x.load(rng.choice(SHIFTS), rng.randrange(M)), 0

    ex = _Exprs(rng, leaf)
    for p in plan:
        if p == "scan":
            num = ex.value(rng.randint(0, 3), 1)[0]
            den = ex.value(rng.randint(0, 2), 1)[0] + x.const(rng.randrange(1, P)) if rng.random() < 0.5 else None
            (x.product if rng.random() < 0.5 else x.running_sum)(num, den)
            continue
        state["sorted"] = False        # key and carried values read the main trace only: `below` 0 keeps the pool's sorted reads out
        if rng.random() < 0.5:
            key, bits = x.load(rng.choice([0, 0, 1, 3]), 1) + 0, 64
        else:
            bits = rng.choice([k for k in KEY_BITS if k >= kb])
            key = x.load(rng.choice([0, 0, 2, 7]), 0)
            key = key + rng.randrange(1, 4) if bits >= kb + 2 and rng.random() < 0.5 else key + 0
        carry = [ex.value(rng.randint(0, 2), 0)[0] for _ in range(p[1])]
        sorted_cols += x.sorted(key, carry, bits)
        state["sorted"] = True
    if pinned:                         # auxiliary column k equals main column M + k, one degree-1 constraint a column
        for k in range(K):
            b.constraint(b.load(0, M + K + k) - b.load(0, M + k), degree=1, exemptions=0)
        return b, rows
    return L.trivial(b), rows


@functools.lru_cache(maxsize=None)
def _aux(seed, n, pinned):
    for attempt in range(ATTEMPTS):
        b, rows = _draw_aux(random.Random(f"aux {seed} {n} {attempt}"), n, pinned)
        if not _accept(b.aux.ops):
            continue
        K = len(b.aux.cols)
        padded = [row + [0] * K for row in rows] if pinned else rows
        try:
            if n <= REF_MAX_N:
                columns = R.aux_table(b.aux, padded, GEN_RAP[:b.n_rap], b.periodic_cols)
            else:
                columns = [[int(v) for v in row] for row in b.aux.evaluate(padded, GEN_RAP[:b.n_rap])]
        except (ZeroDivisionError, ValueError) as e:
            if "denominator" not in str(e):
                raise
            continue
        return b, rows, frozenset(aux_features(b.aux, n)), columns
    raise RuntimeError(f"aux seed {seed} at n = {n}: no valid program in {ATTEMPTS} draws")


def random_aux(seed, n):
    return _aux(seed, n, False)[:3]


def pinned_aux(seed, n):
    """(builder, whole main rows, rap): random_aux(seed, n)'s program in an AIR whose main segment holds, behind the program's main
    columns, the expected auxiliary columns E_k under `rap`, with one constraint aux_k - E_k a column.  The rows satisfy it."""
    b, rows, _, columns = _aux(seed, n, True)
    return b, [row + list(extra) for row, extra in zip(rows, columns)], list(GEN_RAP[:b.n_rap])


def aux_columns(seed, n):
    """The expected auxiliary segment of random_aux(seed, n) under GEN_RAP: program_ref up to 4096 rows, AuxProgram.evaluate beyond."""
    return _aux(seed, n, False)[3]


def describe_aux(seed, n):
    b, rows, features, _ = _aux(seed, n, False)
    names = ["PRODUCT", "SUM", "SORTED"]
    lines = [f"aux seed {seed}, n = {n}: {b.main_cols} main, {len(b.aux.cols)} auxiliary, {len(b.aux.ops)} ops, {b.n_rap} challenges, "
             f"periods {[len(v) for v in b.periodic_cols]}, features {sorted(features)}", f"chunks {aux_chunks(b.aux, n)}"]
    lines += [f"  column {k}: {names[c[0]]} N op {c[1]} D op {c[2]} key_bits {b.aux.key_bits.get(k)}" for k, c in enumerate(b.aux.cols)]
    return "\n".join(lines)
