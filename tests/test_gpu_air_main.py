"""Main-trace programs on the device (sp_air_prove_main, sp_air_check_trace_main, sp_air_main_trace): the derived columns equal the
Python-integer model cell for cell, and a proof from the input columns has the bytes of the proof from the model's whole table through
the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import main_program_airs as M
import oracle_lib as O
from air_device_checks import OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, to_bytes, two_ranks_give_the_one_rank_bytes
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P


def examples(n, rng):
    """(name, builder, input rows) of the two worked examples at n rows."""
    zeros = {0, 1, n // 2, n - 2, n - 1} | {rng.randrange(n) for _ in range(n // 8)}
    return [("bit_range_check", air.bit_range_check(n, 20), air.bit_range_check_inputs(n, 20, rng)),
            ("zero_count", air.zero_count(n, len([i for i in zeros if i < n - 1])), air.zero_count_inputs(n, zeros, rng))]


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_table_equals_the_model_cell_for_cell(hip_ctx, n):
    """n = 64: the last (only) block of every launch is a quarter full; n = 4096: two scan blocks of 2048.  The all-kinds program
    builds in three chunks: its levels read each other at shifts that wrap."""
    rng = random.Random(n)
    b, cols = M.all_kinds()
    assert max(b.main.reads()) == cols["s2"] - b.main.input_cols + 1      # (level 3 reads s2, which reads v0 and p0 of level 1)
    cases = examples(n, rng) + [("all_kinds", b, M.all_kinds_inputs(n, rng))]
    for name, builder, rows in cases:
        desc, keep = builder.build()
        got = hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert got.shape == (n, builder.main_cols, 32), name
        want = model_ints(builder, rows)
        got = table_ints(got)
        for i in range(n):
            assert got[i] == want[i], (name, i)


def test_chunk_boundary_forced_by_size(hip_ctx):
    """2^16 rows x 65 derived columns: a chunk holds 2^22 / 2^16 = 64, so bit 64 is built by a second chunk (its group evaluated again)."""
    n, bits = 1 << 16, 65
    rng = random.Random(65)
    b = air.bit_range_check(n, bits)
    rows = air.bit_range_check_inputs(n, bits, rng)
    for i, v in ((0, (1 << bits) - 1), (1, 1 << 64), (2047, (1 << 64) - 1), (2048, 1 | (1 << 63) | (1 << 64)), (n - 1, 0b101 << 62)):
        rows[i] = [v]
    desc, keep = b.build()
    inputs = to_bytes(rows)
    table = hip_ctx.air_main_trace(desc, inputs)
    for i in (0, 1, 2047, 2048, n - 1, rng.randrange(n)):
        v = rows[i][0]
        assert table_ints(table[i:i + 1])[0] == [v] + [(v >> j) & 1 for j in range(bits)], i
    # the last two derived columns (one on either side of the seam), every row
    seam = air.trace_to_ints(table[:, bits - 1:, :])
    assert [int(x) for x in seam[:, 0]] == [(r[0] >> 63) & 1 for r in rows] and [int(x) for x in seam[:, 1]] == [(r[0] >> 64) & 1 for r in rows]
    options = api.ProofOptions(2, 3, 3, 0)
    proof = hip_ctx.air_prove(desc, inputs, options)
    assert api.air_verify(proof, desc, options)


def test_bit_operands_and_positions(hip_ctx):
    b = M.chosen_bits()
    desc, keep = b.build()
    got = table_ints(hip_ctx.air_main_trace(desc, to_bytes([[v] for v in M.BIT_OPERANDS])))
    for v, row in zip(M.BIT_OPERANDS, got):
        assert row == [v] + [(v >> j) & 1 for j in M.BIT_POSITIONS], hex(v)


def test_inv_or_zero_with_zeros_on_the_edges_and_on_a_whole_wave(hip_ctx):
    n = 256
    rng = random.Random(5)
    zeros = {0, n - 1} | set(range(64, 128))
    rows = air.zero_count_inputs(n, zeros, rng)
    b = air.zero_count(n, len(zeros) - 1)
    desc, keep = b.build()
    got = table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows)))     # no error: a zero is no zero denominator here
    assert got == model_ints(b, rows)
    for i in range(n):
        x, inv, flag, before = got[i]
        assert (inv, flag) == ((0, 1) if i in zeros else (pow(x, P - 2, P), 0)) and before == len([z for z in zeros if z < i])
    options = api.ProofOptions(4, 3, 3, 1)
    assert api.air_verify(hip_ctx.air_prove(desc, to_bytes(rows), options), desc, options)


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("which", [0, 1], ids=["bit_range_check", "zero_count"])
def test_proof_bytes_equal_those_from_the_whole_table(hip_ctx, oracle, which, options):
    n = 64
    name, b, rows = examples(n, random.Random(7))[which]
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub")
    assert got == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)               # and the CPU oracle's, from the same table
    assert hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options)) == got   # the kept workspace, a second time
    opt = api.ProofOptions(*options).to_c()
    assert _lib.load().sp_air_verify(got, ctypes.c_uint64(len(got)), ctypes.byref(desc), ctypes.byref(opt)) == 1
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_main_program_beside_an_auxiliary_program(hip_ctx, oracle):
    n, options = 128, (4, 3, 3, 1)
    rng = random.Random(9)
    b = M.rotation_permutation()
    rows = [[rng.randrange(P)] for _ in range(n)]
    assert b.check_trace(rows, rap=[12345]) == []
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=full)
    assert got == O.program_air_prove(cb_desc, full, options)
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_main_program_beside_a_periodic_column_and_a_stride(hip_ctx):
    n, options = 128, (4, 4, 3, 2)       # (degree_bound_factor 2: the composition has 2n coefficients, which needs a blowup above 2)
    rng = random.Random(10)
    keys = [rng.randrange(P) for _ in range(8)]
    b = M.strided_square_chain(n, 5, keys)
    rows = M.strided_square_chain_inputs(n, 5, keys, rng)
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    assert desc.stride_desc is not None and desc.periodic_desc is not None
    full = to_bytes(model_ints(b, rows))
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "ext") == prove_full(hip_ctx, desc, full, options, "pub")
    assert api.air_verify(got, desc, api.ProofOptions(*options))
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), api.ProofOptions(*options)) == []


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    for name, b, rows in examples(256, random.Random(13)):
        device_inputs_give_the_same_bytes(hip_ctx, b, rows, api.ProofOptions(4, 3, 3, 1), name)


# ---- traces and statements that are wrong -------------------------------------------------------------------------------------
def test_violating_inputs_are_proved_rejected_and_reported(hip_ctx):
    n, bits, options = 64, 20, api.ProofOptions(4, 3, 3, 1)
    rng = random.Random(17)
    b = air.bit_range_check(n, bits)
    rows = air.bit_range_check_inputs(n, bits, rng)
    rows[9], rows[40] = [1 << bits], [(1 << bits) + 3]
    desc, keep = b.build()
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)          # as the reference: a proof all the same ...
    assert proof == prove_full(hip_ctx, desc, to_bytes(model_ints(b, rows)), (4, 3, 3, 1), "pub")
    assert not api.air_verify(proof, desc, options)                   # ... which no verifier accepts
    gamma = 0xabcdef
    want = b.check_trace(rows, rap=[gamma])
    assert want == [air.Violation(air.TRANSITION, 1, 2, 9, 40, (-(1 << bits)) % P)]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), rap=[gamma]) == want
    # zero_count with a public count that is one too high: the last boundary constraint finds the true count
    zeros = {3, 4, 30, n - 1}
    rows = air.zero_count_inputs(n, zeros, rng)
    b = air.zero_count(n, 4)
    desc, keep = b.build()
    want = b.check_trace(rows)
    assert want == [air.Violation(air.BOUNDARY, 1, 1, n - 1, n - 1, 3)]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), options) == want
    assert not api.air_verify(hip_ctx.air_prove(desc, to_bytes(rows), options), desc, options)
    good, good_keep = air.zero_count(n, 3).build()
    assert hip_ctx.air_check_trace(good, to_bytes(rows), options) == []


def test_zero_denominator_and_recovery(hip_ctx):
    n, options = 64, api.ProofOptions(4, 3, 3, 1)
    rng = random.Random(19)
    b = M.reciprocal()
    desc, keep = b.build()
    rows = [[1 + rng.randrange(P - 1)] for _ in range(n)]
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    assert api.air_verify(want, desc, options)
    bad = [list(r) for r in rows]
    bad[37] = [0]
    for call in (lambda: hip_ctx.air_prove(desc, to_bytes(bad), options), lambda: hip_ctx.air_main_trace(desc, to_bytes(bad)),
                 lambda: hip_ctx.air_check_trace(desc, to_bytes(bad), options)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_ZERO_INVERSE and "zero" in str(e.value)
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want   # the same context, right after


@pytest.mark.parametrize("kind", [air.AUX_FIBONACCI_RAP, air.AUX_CALLBACK])
def test_host_built_auxiliary_kinds_are_unsupported(hip_ctx, kind):
    n, options = 64, api.ProofOptions(4, 3, 3, 1)
    rows = air.zero_count_inputs(n, {1}, random.Random(23))
    desc, keep = air.zero_count(n, 1).build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    desc.aux_kind = kind
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_prove(desc, to_bytes(rows), options)
    assert e.value.code == _lib.SP_E_UNSUPPORTED
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_check_trace(desc, to_bytes(rows), options)
    assert e.value.code == _lib.SP_E_UNSUPPORTED
    desc.aux_kind = air.AUX_NONE
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want


def test_malformed_program_is_refused_by_the_prover(hip_ctx):
    n, options = 64, api.ProofOptions(4, 3, 3, 1)
    rows = air.zero_count_inputs(n, {1}, random.Random(29))
    desc, keep = air.zero_count(n, 1).build()
    desc.main_desc.cols[0].den_op = 0            # a denominator on INV_OR_ZERO
    for call in (lambda: hip_ctx.air_prove(desc, to_bytes(rows), options), lambda: hip_ctx.air_main_trace(desc, to_bytes(rows)),
                 lambda: hip_ctx.air_check_trace(desc, to_bytes(rows), options)):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _zero_count_case(n):
    zeros = set(range(0, n, 7)) | {n - 1}
    return air.zero_count(n, len([z for z in zeros if z < n - 1])), air.zero_count_inputs(n, zeros, random.Random(31))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds every derived column itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _zero_count_case, (4096,), (4, 3, 3, 1))
