"""sp_air_prove beyond 64 columns and 3 boundary rows on the device (many_column_air.py): the oracle's proof bytes, and both
verifiers accept - up to 1024 columns, 300 boundary constraints on 64 rows, violating traces, several shapes on one context,
2^16 rows x 256 columns, and two ranks."""
import pytest

import many_column_air as M
import oracle_lib as O
from lambdaworks_cairo_prover_amd import air, api
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

# (n, main, aux, frame rows, boundary rows, boundary constraints on main columns, options); with aux columns one more constraint
# pins each of them on row 0 (200 main + 8 aux: 292 + 8 = 300 constraints on 64 rows)
SHAPES = {
    "96_columns": (1 << 8, 96, 0, 2, 4, None, (4, 3, 3, 1)),
    "200_plus_8_aux": (1 << 10, 200, 8, 3, 64, 292, (8, 5, 3, 2)),
    "1024_columns": (1 << 6, 1024, 0, 2, 4, None, (2, 3, 3, 0)),
    "64_columns_40_rows": (1 << 8, 64, 0, 2, 40, 120, (4, 3, 3, 1)),
}


def _shape(name, **kw):
    n, m, a, r, rows, total, options = SHAPES[name]
    b = M.build(n, m, aux_cols=a, frame_rows=r, boundary_row_count=rows, boundary_total=total, **kw)
    return n, m, b, options


def _prove_and_check(ctx, desc, trace, options, valid=True):
    want = O.program_air_prove(desc, trace, options)
    got = ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert O.program_air_verify(desc, got, options) == valid
    assert api.air_verify(got, desc, api.ProofOptions(*options)) == valid
    return got


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_bytes_equal_oracle(hip_ctx, oracle, name):
    n, m, b, options = _shape(name)
    desc, keep = b.build()
    _prove_and_check(hip_ctx, desc, M.main_trace(n, m), options)


def test_violating_boundary_value_at_a_middle_row(hip_ctx, oracle):
    n, m, _, options = _shape("96_columns")
    b = M.build(n, m, boundary_row_count=4, value_offset=(2, 1))    # constraint 2 sits on a middle row
    assert 0 < b.bcs[2][1] < n - 1
    desc, keep = b.build()
    _prove_and_check(hip_ctx, desc, M.main_trace(n, m), options, valid=False)


def test_violating_transition_at_one_row(hip_ctx, oracle):
    n, m, b, options = _shape("96_columns")
    desc, keep = b.build()
    trace = M.main_trace(n, m).copy()
    trace[n // 2 + 1, 50, 31] ^= 1          # (row n/2 + 1 carries no boundary constraint of this shape)
    assert all(step != n // 2 + 1 for _, step, _ in b.bcs)
    _prove_and_check(hip_ctx, desc, trace, options, valid=False)


def test_context_reuse_across_shapes(hip_ctx, oracle):
    for name in ("200_plus_8_aux", "1024_columns"):
        n, m, b, options = _shape(name)
        desc, keep = b.build()
        _prove_and_check(hip_ctx, desc, M.main_trace(n, m), options)
    trace = O.example_trace("fibonacci_2_columns", 64, (1, 1))
    desc, keep = air.fibonacci_2_columns(1, 1).build()
    options = (4, 3, 3, 1)
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == O.example_prove("fibonacci_2_columns", trace, options, (1, 1), 0)


def test_2p16_rows_256_columns(hip_ctx):
    """No oracle leg (the CPU oracle takes too long at this size): the host verifier accepts, and a fresh context gives the same bytes."""
    n, m, options = 1 << 16, 256, (4, 8, 3, 1)
    desc, keep = M.build(n, m, boundary_row_count=64, boundary_total=512).build()
    trace = M.main_trace(n, m)
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert api.air_verify(got, desc, api.ProofOptions(*options))
    with api.Context(device=0) as fresh:
        assert fresh.air_prove(desc, trace, api.ProofOptions(*options)) == got


def _air_body(rank, world):
    n, m, a, r, rows, total, options = SHAPES["200_plus_8_aux"]
    desc, keep = M.build(n, m, aux_cols=a, frame_rows=r, boundary_row_count=rows, boundary_total=total).build()
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    proof = ctx.air_prove(desc, M.main_trace(n, m), api.ProofOptions(*options))
    ctx.close()
    return proof


def test_sharded_200_columns_world_2(hip_ctx):
    n, m, b, options = _shape("200_plus_8_aux")
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, M.main_trace(n, m), api.ProofOptions(*options))
    got = run_ranks(2, _air_body, timeout=300)
    for r in range(2):
        assert got[r] == want, (r, got[r][:400])
