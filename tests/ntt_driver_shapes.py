"""The shapes tests/test_gpu_ntt_drivers.py runs, and why: every class of launch the transform drivers can make inside an envelope
of sizes is covered by one of them.  The classes come from sp_ntt_plan - the host code that launches the passes - so a change to the
plan (geometry(), the tile rules) that moves a shape off its path makes tests/test_ntt_plan_cover.py fail and name the class.

A shape is (driver, k, logb, shard_log, batch); what else a test varies (rank, post_table, src, the input) changes no launch."""
from collections import namedtuple

from lambdaworks_cairo_prover_amd import api

Shape = namedtuple("Shape", "driver k logb shard_log batch")

FOOTPRINT_THRESHOLD = 64 << 20      # geometry(): 1024-element tiles for transforms that touch more than this, 512 below
FOOTPRINT_CAP = 128 << 20           # the envelope's largest batch
MAX_K, MAX_LOGB = 20, 4
LDE_DRIVERS = ("lde_natural", "lde_coset_major")
CLASS_FIELDS = ("driver", "dif", "load", "store", "contig", "gtw", "stage_tw", "tile_log", "r", "radix4", "xcd_map", "weak_out",
                "place", "many_cosets", "sharded", "g_is_s")


def footprint(shape):
    """bytes the batched transform touches, as the drivers hand them to geometry()"""
    logs = shape.k + (shape.logb - shape.shard_log if shape.driver in LDE_DRIVERS else 0)
    return (shape.batch << logs) * 32


def pass_classes(shape):
    """the class of every pass the shape launches (tuples over CLASS_FIELDS), in execution order"""
    plan = api.ntt_plan(shape.driver, shape.k, shape.logb, shape.shard_log, shape.batch)
    out = []
    for i, p in enumerate(plan):
        tile_log = p["r"] + p["g"]
        r = p["r"]
        out.append((shape.driver, p["dif"], p["load"], p["store"], p["contig"], p["gtw"], p["stage_tw"],
                    "<=8" if tile_log <= 8 else str(tile_log),
                    str(r) if r <= 2 else ("odd>=3" if r & 1 else "even>=4"),
                    p["radix4"], p["xcd_map"], p["weak_out"],
                    "only" if len(plan) == 1 else "first" if i == 0 else "last" if i + 1 == len(plan) else "middle",
                    int(p["coset_count"] > 1), int(shape.shard_log > 0), int(p["g"] == p["s"])))
    return out


def envelope(drivers):
    """every shape of the envelope: k <= 20, logb <= 4, every shard_log <= logb, batches 1 and 3 and the two on either side of the
    64 MiB threshold, as far as the footprint stays within 128 MiB"""
    for driver in drivers:
        lde = driver in LDE_DRIVERS
        for k in range(MAX_K + 1):
            for logb in range(MAX_LOGB + 1) if lde else (0,):
                for shard_log in range(logb + 1):
                    per_vector = footprint(Shape(driver, k, logb, shard_log, 1))
                    below = FOOTPRINT_THRESHOLD // per_vector
                    for batch in sorted({1, 3, below, below + 1}):
                        shape = Shape(driver, k, logb, shard_log, batch)
                        if batch >= 1 and footprint(shape) <= FOOTPRINT_CAP:
                            yield shape


def greedy_cover(candidates, have=()):
    """the rows that cover every class of `candidates` not already in `have`: smallest footprint first, a shape is taken when it
    launches a class nothing before it did.  Returns (rows, classes covered by have + rows)."""
    covered = set(have)
    rows = []
    for shape in sorted(set(candidates), key=lambda s: (footprint(s), s)):
        new = set(pass_classes(shape)) - covered
        if new:
            rows.append(shape)
            covered |= new
    return rows, covered


def classes_of(shapes):
    return set(c for s in shapes for c in pass_classes(s))


def describe(cls):
    return ", ".join(f"{name}={value}" for name, value in zip(CLASS_FIELDS, cls))


# ---------------------------------------------------------------------------------------------- shapes every table holds
def _coset_major_required():
    """k in {0, 1, 5, 8, 10, 11, 13, 16, 17, 18}, blowup in {2, 4, 8}, batches of 1 and 3: all of them together wherever the output stays
    within 64 MiB; beyond that (k = 17 at blowup 8, k = 18 at blowup 4 and 8, with 3 columns) only k = 17 x blowup 8 x 3, which the issue
    names on its own - 2^18 x 8 x 3 would be 192 MiB, above the envelope and heavier than the 2^22 transform of
    test_ntt_dev_batched_device_entry_point.  Then k = 12 with 65 columns at blowup 8 (more than 512 vectors, just over 64 MiB)."""
    rows = [Shape("lde_coset_major", k, logb, 0, batch) for k in (0, 1, 5, 8, 10, 11, 13, 16, 17, 18) for logb in (1, 2, 3) for batch in (1, 3)
            if footprint(Shape("lde_coset_major", k, logb, 0, batch)) <= FOOTPRINT_THRESHOLD]
    rows += [Shape("lde_coset_major", 12, 3, 0, 65), Shape("lde_coset_major", 17, 3, 0, 3)]
    return rows


def _natural_required():
    """every (shard_log, rank) for blowup 2 and 4 at k in {0, 3, 9, 12, 17} (a test runs every rank of a row); shard_log = logb is
    among them: one coset per rank, first pass at local stride 0"""
    return [Shape("lde_natural", k, logb, shard_log, 1) for k in (0, 3, 9, 12, 17) for logb in (1, 2) for shard_log in range(logb + 1)]


def _inverse_required():
    """k in {0, 1, 2, 7, 10, 11, 15, 16, 18}, batches of 1 and 5 (a test runs a row with and without post_table and src)"""
    return [Shape("intt_bitrev", k, 0, 0, batch) for k in (0, 1, 2, 7, 10, 11, 15, 16, 18) for batch in (1, 5)]


REQUIRED = _coset_major_required() + _natural_required() + _inverse_required()
DRIVER_TABLE_DRIVERS = ("intt_bitrev", "lde_natural", "lde_coset_major")

# What greedy_cover(envelope(DRIVER_TABLE_DRIVERS), classes_of(REQUIRED)) adds to REQUIRED (tests/test_ntt_plan_cover.py recomputes it).
COVER = [
    Shape("lde_coset_major", 0, 0, 0, 1), Shape("lde_coset_major", 0, 1, 1, 1), Shape("lde_coset_major", 0, 2, 1, 1),
    Shape("lde_coset_major", 1, 0, 0, 1), Shape("lde_coset_major", 1, 1, 1, 1), Shape("lde_natural", 1, 0, 0, 1),
    Shape("lde_natural", 1, 1, 1, 1), Shape("lde_coset_major", 1, 2, 1, 1), Shape("lde_coset_major", 2, 0, 0, 1),
    Shape("lde_coset_major", 2, 1, 1, 1), Shape("lde_natural", 1, 1, 0, 1), Shape("lde_natural", 2, 0, 0, 1),
    Shape("lde_natural", 2, 1, 1, 1), Shape("lde_coset_major", 2, 1, 0, 1), Shape("lde_coset_major", 2, 2, 1, 1),
    Shape("lde_coset_major", 3, 0, 0, 1), Shape("lde_coset_major", 3, 1, 1, 1), Shape("lde_natural", 0, 3, 0, 1),
    Shape("lde_natural", 0, 4, 1, 1), Shape("lde_natural", 2, 1, 0, 1), Shape("lde_natural", 3, 0, 0, 1),
    Shape("intt_bitrev", 4, 0, 0, 1), Shape("lde_coset_major", 3, 2, 1, 1), Shape("lde_coset_major", 4, 0, 0, 1),
    Shape("lde_coset_major", 4, 1, 1, 1), Shape("lde_natural", 4, 0, 0, 1), Shape("lde_natural", 4, 1, 1, 1),
    Shape("lde_coset_major", 4, 2, 1, 1), Shape("lde_natural", 4, 1, 0, 1), Shape("intt_bitrev", 9, 0, 0, 1),
    Shape("lde_coset_major", 9, 0, 0, 1), Shape("lde_coset_major", 9, 1, 1, 1), Shape("lde_natural", 5, 4, 0, 1),
    Shape("lde_natural", 6, 3, 0, 1), Shape("lde_natural", 6, 4, 1, 1), Shape("lde_natural", 7, 3, 1, 1),
    Shape("lde_natural", 9, 0, 0, 1), Shape("lde_coset_major", 9, 1, 0, 1), Shape("lde_coset_major", 9, 2, 1, 1),
    Shape("lde_coset_major", 10, 0, 0, 1), Shape("lde_coset_major", 10, 1, 1, 1), Shape("lde_natural", 6, 4, 0, 1),
    Shape("lde_natural", 7, 3, 0, 1), Shape("lde_natural", 7, 4, 1, 1), Shape("lde_natural", 8, 2, 0, 1),
    Shape("lde_natural", 8, 3, 1, 1), Shape("lde_natural", 10, 0, 0, 1), Shape("lde_coset_major", 10, 2, 1, 1),
    Shape("lde_coset_major", 11, 0, 0, 1), Shape("lde_coset_major", 11, 1, 1, 1), Shape("lde_natural", 8, 3, 0, 1),
    Shape("lde_natural", 8, 4, 1, 1), Shape("lde_natural", 11, 0, 0, 1), Shape("lde_natural", 11, 1, 1, 1),
    Shape("lde_coset_major", 11, 2, 1, 1), Shape("lde_coset_major", 12, 0, 0, 1), Shape("lde_coset_major", 12, 1, 1, 1),
    Shape("lde_natural", 12, 0, 0, 1), Shape("lde_coset_major", 12, 2, 1, 1), Shape("lde_coset_major", 13, 0, 0, 1),
    Shape("lde_coset_major", 13, 1, 1, 1), Shape("lde_natural", 9, 4, 0, 1), Shape("lde_natural", 10, 3, 0, 1),
    Shape("lde_natural", 10, 4, 1, 1), Shape("lde_natural", 13, 0, 0, 1), Shape("lde_coset_major", 13, 2, 1, 1),
    Shape("lde_natural", 10, 4, 0, 1), Shape("lde_natural", 14, 0, 0, 1), Shape("lde_natural", 13, 3, 1, 1),
    Shape("lde_coset_major", 16, 0, 0, 1), Shape("lde_coset_major", 16, 1, 1, 1), Shape("lde_natural", 13, 3, 0, 1),
    Shape("lde_natural", 13, 4, 1, 1), Shape("lde_natural", 14, 2, 0, 1), Shape("lde_natural", 14, 3, 1, 1),
    Shape("lde_natural", 16, 1, 1, 1), Shape("lde_coset_major", 16, 2, 1, 1), Shape("lde_coset_major", 17, 0, 0, 1),
    Shape("lde_coset_major", 17, 1, 1, 1), Shape("lde_natural", 14, 3, 0, 1), Shape("lde_natural", 14, 4, 1, 1),
    Shape("lde_natural", 16, 1, 0, 1), Shape("lde_coset_major", 17, 2, 1, 1), Shape("lde_coset_major", 18, 0, 0, 1),
    Shape("lde_coset_major", 18, 1, 1, 1), Shape("lde_natural", 18, 0, 0, 1), Shape("lde_coset_major", 18, 2, 1, 1),
    Shape("lde_natural", 19, 0, 0, 1), Shape("lde_natural", 20, 0, 0, 1), Shape("lde_natural", 7, 3, 0, 2049),
    Shape("lde_natural", 7, 4, 1, 2049), Shape("lde_natural", 9, 1, 0, 2049), Shape("lde_natural", 9, 2, 1, 2049),
    Shape("intt_bitrev", 11, 0, 0, 1025), Shape("lde_coset_major", 11, 0, 0, 1025), Shape("lde_coset_major", 11, 1, 1, 1025),
    Shape("lde_natural", 7, 4, 0, 1025), Shape("lde_natural", 9, 2, 0, 1025), Shape("lde_natural", 9, 3, 1, 1025),
    Shape("lde_natural", 11, 0, 0, 1025), Shape("lde_natural", 11, 1, 1, 1025), Shape("intt_bitrev", 12, 0, 0, 513),
    Shape("lde_coset_major", 11, 1, 0, 513), Shape("lde_coset_major", 11, 2, 1, 513), Shape("lde_coset_major", 12, 0, 0, 513),
    Shape("lde_coset_major", 12, 1, 1, 513), Shape("lde_natural", 11, 1, 0, 513), Shape("lde_natural", 12, 0, 0, 513),
    Shape("lde_coset_major", 12, 2, 1, 257), Shape("lde_coset_major", 13, 0, 0, 257), Shape("lde_coset_major", 13, 1, 1, 257),
    Shape("lde_natural", 11, 2, 0, 257), Shape("lde_natural", 11, 3, 1, 257), Shape("lde_natural", 13, 0, 0, 257),
    Shape("intt_bitrev", 14, 0, 0, 129), Shape("lde_coset_major", 13, 1, 0, 129), Shape("lde_coset_major", 13, 2, 1, 129),
    Shape("intt_bitrev", 16, 0, 0, 33), Shape("lde_natural", 13, 3, 0, 33), Shape("lde_natural", 13, 4, 1, 33),
    Shape("intt_bitrev", 17, 0, 0, 17), Shape("lde_coset_major", 17, 0, 0, 17), Shape("lde_coset_major", 17, 1, 1, 17),
    Shape("lde_natural", 13, 4, 0, 17), Shape("lde_natural", 17, 1, 1, 17), Shape("lde_coset_major", 17, 2, 1, 9),
    Shape("lde_coset_major", 18, 0, 0, 9), Shape("lde_coset_major", 18, 1, 1, 9), Shape("lde_natural", 17, 1, 0, 9),
    Shape("lde_coset_major", 18, 1, 0, 5), Shape("lde_coset_major", 18, 2, 1, 5), Shape("lde_natural", 19, 0, 0, 5),
    Shape("lde_natural", 20, 0, 0, 3),
]

def _parametrised(fn):
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return list(mark.args[1])


def existing_ntt_cases():
    """(k, batch) of every sp_ntt / sp_ntt_dev case of tests/test_gpu_fine_grained.py and tests/test_gpu_ntt_stage_tables.py (both
    directions each), read from the parametrised lists of the test functions themselves; only test_batch_of_three_at_2_19 and the
    sizes test_ntt_edge_inputs and the table-reuse tests write in their bodies are spelt out"""
    import test_gpu_fine_grained as fine
    import test_gpu_ntt_stage_tables as stage
    cases = [(k, 1) for k in _parametrised(fine.test_ntt_forward_inverse_matches_oracle)]
    cases += [(k, 1) for k in _parametrised(fine.test_ntt_coset_variants)]
    cases += [tuple(kb) for kb in _parametrised(fine.test_ntt_dev_batched_device_entry_point)]
    cases += [(k, 1) for k in _parametrised(fine.test_ntt_extreme_values_across_passes)]
    cases += [(k, 1) for k in _parametrised(stage.test_forward_and_inverse_at_every_size_with_two_strided_passes)]
    return sorted(set(cases + [(19, 3), (11, 1), (12, 1), (14, 1), (20, 1), (22, 1)]))


NTT_DRIVERS = ("forward_natural", "inverse_natural")
# What greedy_cover(envelope(NTT_DRIVERS), classes_of(existing_ntt_shapes())) adds: the sp_ntt_dev cases of tests/test_gpu_ntt_drivers.py.
NTT_DEV_EXTRA = [
    Shape("forward_natural", 11, 0, 0, 1025), Shape("inverse_natural", 11, 0, 0, 1025), Shape("forward_natural", 12, 0, 0, 513),
    Shape("inverse_natural", 12, 0, 0, 513), Shape("forward_natural", 13, 0, 0, 257), Shape("inverse_natural", 13, 0, 0, 257),
    Shape("forward_natural", 17, 0, 0, 17), Shape("inverse_natural", 17, 0, 0, 17),
]


def existing_ntt_shapes():
    return [Shape(d, k, 0, 0, batch) for d in NTT_DRIVERS for k, batch in existing_ntt_cases()]


def table():
    """every row the driver tests run"""
    return REQUIRED + COVER
