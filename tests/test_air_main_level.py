"""air.MainLevel against the library, without a GPU: every level's four entry points are exported, and for every level above MAIN the
smallest worked example that needs it is routed there and passes that level's decoder.  A new level adds one line to STATEMENTS."""
import random

import pytest

import chain_airs as C
import div_airs as D
import link_airs as L
from lambdaworks_cairo_prover_amd import air, api

# The shortest trace the seeded GPU tests prove.  Every constructor below admits it: the largest of their own lower bounds is
# mimc_sponge's s * link = 4, and zero_count, table_lookup_main and rom_reads have none.
N = 8
TABLE = [3, 5, 5, 9]


def _zero_count(rng):
    zeros = (1, 4, N - 1)
    return air.zero_count(N, sum(1 for i in zeros if i < N - 1)), air.zero_count_inputs(N, zeros, rng)


# (the level, the example, rng -> (builder, input rows)): each example needs its level and nothing above it
STATEMENTS = [
    (air.MainLevel.MAIN, "zero_count", _zero_count),
    (air.MainLevel.REC, "mimc_blocks", lambda rng: C.mimc_case(N, 2, rng)[:2]),
    (air.MainLevel.LK, "table_lookup_main", lambda rng: (air.table_lookup_main(N, TABLE, 8), air.table_lookup_main_inputs(N, TABLE, rng))),
    (air.MainLevel.LINK, "mimc_sponge", lambda rng: L.sponge_case(N, 2, 2, rng)[:2]),
    (air.MainLevel.DIV, "ec_subset_sum", lambda rng: D.ec_case(N, 2, rng)[:2]),
    (air.MainLevel.FETCH, "rom_reads", lambda rng: (air.rom_reads(N, 16), air.rom_reads_inputs(N, 16, rng))),
]


def test_the_levels_are_those_of_the_library_in_its_order():
    assert [(int(level), level.suffix) for level in air.MainLevel] == [(0, "main"), (1, "rec"), (2, "lk"), (3, "link"), (4, "div"), (5, "fetch")]
    assert [level for level, _, _ in STATEMENTS] == list(air.MainLevel)


@pytest.mark.parametrize("level", list(air.MainLevel), ids=[level.suffix for level in air.MainLevel])
def test_the_library_exports_the_entry_points_of_the_level(hip_lib, level):
    s = level.suffix
    host = ("sp_air_main_trace", "sp_air_main_check") if level == air.MainLevel.MAIN else (f"sp_air_main_trace_{s}", f"sp_air_main_check_{s}")
    for name in (f"sp_air_prove_{s}", f"sp_air_check_trace_{s}") + host:
        assert hasattr(hip_lib, name), name


@pytest.mark.parametrize("level,make", [(c[0], c[2]) for c in STATEMENTS], ids=[c[1] for c in STATEMENTS])
def test_the_smallest_example_of_the_level_is_routed_to_it_and_accepted(hip_lib, level, make):
    b, rows = make(random.Random(int(level)))
    assert len(rows) == N
    desc, keep = b.build()
    assert air.main_level(desc) == level
    assert air.route(desc, "prove")[0] == f"sp_air_prove_{level.suffix}"
    api.air_main_check(desc, N)
