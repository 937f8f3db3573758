"""Quotients in chain steps on the device (sp_air_prove_div, sp_air_check_trace_div, sp_air_main_trace_div): the columns equal the
Python-integer model and the plain references cell for cell, and a proof from the input columns has the bytes of the proof from the
model's whole table through the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import div_airs as D
import div_ref as R
import oracle_lib as O
import program_ref
from air_device_checks import OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, to_bytes, two_ranks_give_the_one_rank_bytes
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
DIV_OPTIONS = (4, 4, 3, 2)      # (degree_bound_factor 2: the composition has 2n coefficients)


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s,link", [(64, 2, 1), (64, 64, 1), (64, 8, 4), (4096, 4, 4), (8192, 2, 2)])
def test_table_equals_the_model_and_the_references_cell_for_cell(hip_ctx, n, s, link):
    """(64, 2, 1): 32 lanes in a half-empty wave, one step a block.  (64, 64, 1): one lane, the whole trace one block, the input read at
    shift 3 wraps on its last rows.  (64, 8, 4): linked.  (4096, 4, 4): 256 lanes, four work-groups.  (8192, 2, 2): 2048 lanes.
    The program (div_airs.mixed): DIV in steps only, DIV in a linked seed that reads a carry, a polynomial group beside them - the
    launch without a flag -, a group of sixteen quotients, a quotient of a quotient, one shared by two next values, a dead DIV over
    zero, op 6 in some groups and none in others, a VALUE and a SUM behind them.  The hand table is the reference that chose the inputs;
    the per-cell evaluator program_ref, one modular exponentiation a quotient, joins it at 64 rows (at 8192 it alone takes ten seconds).
    Twice on one context with a polynomial-only program between: the kept workspace, and the launch with a null flag pointer."""
    rng = random.Random(n + s + link)
    periodic = D.periodic_columns(rng)
    b, cols = D.mixed(s, link, periodic)
    rows, hand = D.mixed_inputs(n, s, link, periodic, rng)
    desc, keep = b.build()
    assert air.main_suffix(desc) == "div"
    want = model_ints(b, rows)
    assert want == hand
    if n == 64:
        assert want == program_ref.main_table(b.main, rows)
    poly = D.poly_only(s)
    poly_desc, poly_keep = poly.build()
    poly_rows = [[r[0]] for r in rows]
    for attempt in range(2):
        got = hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert got.shape == (n, b.main_cols, 32)
        got = table_ints(got)
        for i in range(n):
            assert got[i] == want[i], (attempt, i)
        for first in range(0, n, s * link):
            assert got[first][cols["y1"]] == 1, first
        assert table_ints(hip_ctx.air_main_trace(poly_desc, to_bytes(poly_rows))) == model_ints(poly, poly_rows)


# ---- the worked example ---------------------------------------------------------------------------------------------------------
def test_ec_subset_sum_table_proof_and_check(hip_ctx):
    n, s = 256, 8
    b, rows, points, shift, result = D.ec_case(n, s, random.Random(40))
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    got = table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows)))
    assert got == model_ints(b, rows) == R.ec_subset_sum_table(rows, s, points, shift)
    options = api.ProofOptions(*DIV_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)
    assert api.air_verify(proof, desc, options)
    full = to_bytes(model_ints(b, rows))
    assert proof == prove_full(hip_ctx, desc, full, DIV_OPTIONS, "ext") == prove_full(hip_ctx, desc, full, DIV_OPTIONS, "pub")
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == proof      # the kept workspace, a second time
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == []


def test_wrong_result_is_proved_rejected_and_reported(hip_ctx):
    n, s = 256, 8
    wrong, rows, points, shift, result = D.ec_case(n, s, random.Random(41), wrong=1)
    desc, keep = wrong.build()
    options = api.ProofOptions(*DIV_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)           # as the reference: a proof all the same ...
    assert not api.air_verify(proof, desc, options)                    # ... which no verifier accepts
    want = wrong.check_trace(rows)
    assert want == [air.Violation(air.BOUNDARY, 0, 1, s - 1, s - 1, result[0])]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == want


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
def test_plain_div_proof_bytes_equal_the_oracles(hip_ctx, oracle, options):
    """plain_div has no periodic column and no stride: the CPU oracle, which takes the descriptor alone, proves the same table."""
    n, s = 64, 4
    b = D.plain_div(s)
    rng = random.Random(8)
    rows = [[rng.randrange(P)] for _ in range(n)]
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    assert model_ints(b, rows) == program_ref.main_table(b.main, rows)
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    b, rows = D.ec_case(256, 8, random.Random(13))[:2]
    device_inputs_give_the_same_bytes(hip_ctx, b, rows, api.ProofOptions(*DIV_OPTIONS))


# ---- what is refused ----------------------------------------------------------------------------------------------------------
def test_a_zero_denominator_is_zero_inverse_and_the_context_goes_on(hip_ctx):
    """a + 2 = 0 on the first row of block 2 alone: the seed x1 = a(i + 1) / (a + 2) of that one block has no value.  The same value on
    a row where no seed is evaluated is no error."""
    n, s, options = 64, 4, api.ProofOptions(4, 3, 3, 1)
    b = D.plain_div(s)
    rng = random.Random(29)
    rows = [[rng.randrange(P)] for _ in range(n)]
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    quiet = [list(r) for r in rows]
    quiet[5] = [P - 2]
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(quiet))) == model_ints(b, quiet)
    bad = [list(r) for r in rows]
    bad[8] = [P - 2]
    for call in (lambda: hip_ctx.air_prove(desc, to_bytes(bad), options), lambda: hip_ctx.air_main_trace(desc, to_bytes(bad)),
                 lambda: hip_ctx.air_check_trace(desc, to_bytes(bad), options)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_ZERO_INVERSE and "denominator is zero on some row" in str(e.value)
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want


def test_malformed_dividing_program_is_refused_and_the_context_goes_on(hip_ctx):
    n, s, options = 64, 4, api.ProofOptions(4, 3, 3, 1)
    rng = random.Random(30)
    rows = [[rng.randrange(P)] for _ in range(n)]
    b = D.plain_div(s)
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    quotient = next(t for t, o in enumerate(b.main.ops) if o[0] == air.OP_DIV)
    num_op = desc.main_desc.cols[2].num_op
    desc.main_desc.cols[2].num_op = quotient          # the VALUE column behind the chain group, now N = a quotient
    for call in (lambda: hip_ctx.air_prove(desc, to_bytes(rows), options), lambda: hip_ctx.air_main_trace(desc, to_bytes(rows)),
                 lambda: hip_ctx.air_check_trace(desc, to_bytes(rows), options)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG and "derived column 2 depends on a quotient (op 7)" in str(e.value)
    desc.main_desc.cols[2].num_op = num_op
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    # and through the entry points that were there before op 7 is the malformed op it always was
    lib, opt = _lib.load(), options.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = to_bytes(rows)
    for name in ("sp_air_prove_main", "sp_air_prove_rec", "sp_air_prove_lk", "sp_air_prove_link"):
        rc = getattr(lib, name)(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
        assert rc == _lib.SP_E_INVALID_ARG and f"malformed op {quotient} " in lib.sp_last_error().decode(), name
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_case(n, s):
    return D.ec_case(n, s, random.Random(31))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds every column itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rank_case, (4096, 8), DIV_OPTIONS)
