"""Block recurrences on the device (sp_air_prove_rec, sp_air_check_trace_rec, sp_air_main_trace_rec): the chain columns equal the
Python-integer model cell for cell, and a proof from the input columns has the bytes of the proof from the model's whole table through
the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import chain_airs as C
import oracle_lib as O
from air_device_checks import OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, to_bytes, two_ranks_give_the_one_rank_bytes
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,s", [(64, 2), (64, 64), (4096, 4), (8192, 32)])
def test_table_equals_the_model_cell_for_cell(hip_ctx, n, s):
    """(64, 2): 32 lanes, half a wave, one step a block.  (64, 64): one lane, the whole trace one block, the input read at shift 3
    wraps on its last rows.  (4096, 4): 1024 lanes, 16 work-groups.  (8192, 32): 4 waves, the periodic columns' periods 8 < s < 64.
    The program: a group of three whose steps read each other, a second group beside it, a VALUE and a SUM that read them."""
    rng = random.Random(n + s)
    periodic = C.periodic_columns(rng)
    b, cols = C.mixed(s, periodic)
    rows = C.mixed_inputs(n, rng)
    desc, keep = b.build()
    got = hip_ctx.air_main_trace(desc, to_bytes(rows))
    assert got.shape == (n, b.main_cols, 32)
    got, want = table_ints(got), model_ints(b, rows)
    if n == 64:
        assert want == C.hand_table(rows, s, periodic)
    for i in range(n):
        assert got[i] == want[i], i


def test_mimc_blocks_table(hip_ctx):
    """The worked example, one column and the widened group: a VALUE that reads op 6 beside the chain (the periodic terms kernel)."""
    n, s = 256, 16
    for width in (1, 3):
        b, rows, keys = C.mimc_case(n, s, random.Random(40 + width), width)
        desc, keep = b.build()
        assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == model_ints(b, rows), width


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
def test_proof_bytes_equal_those_from_the_whole_table(hip_ctx, oracle, options):
    """plain_pair has no periodic column and no stride: the CPU oracle, which takes the descriptor alone, proves the same table."""
    n, s = 64, 8
    b = C.plain_pair(s)
    rng = random.Random(7)
    rows = [[rng.randrange(P)] for _ in range(n)]
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub")
    assert got == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)               # and the CPU oracle's, from the same table
    assert hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options)) == got   # the kept workspace, a second time
    assert api.air_verify(got, desc, api.ProofOptions(*options))


@pytest.mark.parametrize("options", OPTIONS)
def test_proof_bytes_with_periodic_reads(hip_ctx, options):
    """The program of the table tests (op 6 in seeds, steps and a VALUE) under both option sets; its AIR carries periodic columns,
    which the oracle's entry point has no argument for."""
    n, s = 64, 8
    rng = random.Random(8)
    b, cols = C.mixed(s, C.periodic_columns(rng))
    rows = C.mixed_inputs(n, rng)
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    assert hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options)) == got
    assert api.air_verify(got, desc, api.ProofOptions(*options))


MIMC_OPTIONS = (4, 4, 3, 2)      # (degree_bound_factor 2: the composition has 2n coefficients, which needs a blowup above 2)


def test_mimc_blocks_proves_verifies_and_checks_clean(hip_ctx):
    n, s = 256, 16
    b, rows, keys = C.mimc_case(n, s, random.Random(11))
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    options = api.ProofOptions(*MIMC_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)
    assert api.air_verify(proof, desc, options)
    full = to_bytes(model_ints(b, rows))
    assert proof == prove_full(hip_ctx, desc, full, MIMC_OPTIONS, "ext") == prove_full(hip_ctx, desc, full, MIMC_OPTIONS, "pub")
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == []


def test_wrong_digest_is_proved_rejected_and_reported(hip_ctx):
    n, s = 256, 16
    b, rows, keys = C.mimc_case(n, s, random.Random(12))
    digest = air.mimc_blocks_digest([rows[0][0]], s, keys)
    wrong = air.mimc_blocks(n, s, keys, digest + 1)
    desc, keep = wrong.build()
    options = api.ProofOptions(*MIMC_OPTIONS)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)           # as the reference: a proof all the same ...
    assert not api.air_verify(proof, desc, options)                    # ... which no verifier accepts
    want = wrong.check_trace(rows)
    assert want == [air.Violation(air.BOUNDARY, 0, 1, s - 1, s - 1, digest)]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == want


def test_chain_beside_an_auxiliary_program(hip_ctx, oracle):
    """A grand product over the chain column: the auxiliary program reads what the main program built."""
    n, s, options = 128, 8, (4, 3, 3, 1)
    rng = random.Random(9)
    b = C.chain_permutation(s)
    rows = [[rng.randrange(P)] for _ in range(n)]
    assert b.check_trace(rows, rap=[12345]) == []
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=full)
    assert got == O.program_air_prove(cb_desc, full, options)
    assert api.air_verify(got, desc, api.ProofOptions(*options))
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), rap=[12345]) == []


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    b, rows, keys = C.mimc_case(256, 16, random.Random(13))
    device_inputs_give_the_same_bytes(hip_ctx, b, rows, api.ProofOptions(*MIMC_OPTIONS))


def test_malformed_chain_is_refused_and_the_context_goes_on(hip_ctx):
    n, s, options = 64, 8, api.ProofOptions(4, 3, 3, 1)
    rng = random.Random(29)
    rows = [[rng.randrange(P)] for _ in range(n)]
    desc, keep = C.plain_pair(s).build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    pad = desc.main_desc.cols[1].pad
    desc.main_desc.cols[1].pad = 2 + 256            # the second column of the group in blocks of 4 rows, the first in blocks of 8
    for call in (lambda: hip_ctx.air_prove(desc, to_bytes(rows), options), lambda: hip_ctx.air_main_trace(desc, to_bytes(rows)),
                 lambda: hip_ctx.air_check_trace(desc, to_bytes(rows), options)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG and "differs from its chain group in l" in str(e.value)
    desc.main_desc.cols[1].pad = pad
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    # and through the entry points that were there before the same program is no program at all
    lib, opt = _lib.load(), options.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = to_bytes(rows)
    rc = lib.sp_air_prove_main(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                               ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    assert rc == _lib.SP_E_INVALID_ARG and "unknown kind" in lib.sp_last_error().decode()


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_case(n, s):
    return C.mimc_case(n, s, random.Random(31))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds every chain column itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rank_case, (4096, 8), MIMC_OPTIONS)
