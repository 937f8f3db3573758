"""Limbs and bitwise words on the device (sp_air_prove_word, sp_air_check_trace_word, sp_air_main_trace_word): the LIMB and WORD
columns equal the plain reference of program_ref cell for cell, grouping and chunking change no cell, and a proof from the input columns
has the bytes of the proof from the whole table through the entry points that existed before.  Every comparison is exact."""
import ctypes
import functools
import random

import numpy as np
import pytest

import air_device_checks
import oracle_lib as O
import program_ref as R
import word_airs as W
from air_device_checks import (LK_OPTIONS, OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, three_calls, to_bytes,
                               two_ranks_give_the_one_rank_bytes)
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "a word operand is out of range on some row (both operands of a WORD column must be below 2^bits as canonical integers)"
MISSING = "a fetched key is in no table row"
OTHER_BITS = {1: 251, 32: 33, 33: 32, 64: 17, 251: 1}


same_table = functools.partial(air_device_checks.same_table, suffix="word")


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 512])
def test_limbs_equal_the_reference_cell_for_cell(hip_ctx, n):
    """n = 64: a quarter of one 256-lane block; 512: two blocks.  One group on one N holds every (lo, width) of W.LIMB_SPECS; rows 0 .. 5
    and n - 1 hold W.LIMB_OPERANDS, the rest the whole field.  The limbs of width 1 equal the BIT columns of the same program."""
    rows = W.limb_rows(n, random.Random(n))
    want = same_table(hip_ctx, W.limb_group(), rows)
    at = {spec: 1 + j for j, spec in enumerate(W.LIMB_SPECS)}
    bit_at = {j: 1 + len(W.LIMB_SPECS) + k for k, j in enumerate(W.BIT_POSITIONS)}
    for r in want:
        assert all(r[at[(j, 1)]] == r[bit_at[j]] for j in W.BIT_POSITIONS) and r[at[(0, 252)]] == r[0]
    assert [r[0] for r in want[:6]] + [want[-1][0]] == W.LIMB_OPERANDS


@pytest.mark.parametrize("bits", [1, 32, 33, 64, 251])
@pytest.mark.parametrize("n", [64, 512])
def test_words_equal_the_reference_cell_for_cell(hip_ctx, n, bits):
    """AND, OR and XOR of one pair over `bits` bits - one group - and of a second pair over another width - a second group; rows 0, 1
    and n - 1 hold (all ones, 0), (all ones, all ones) and (0, 0)."""
    other = OTHER_BITS[bits]
    rows = W.word_rows(n, bits, other, random.Random(1000 * bits + n))
    want = same_table(hip_ctx, W.word_groups(bits, other), rows)
    top = (1 << bits) - 1
    assert want[0][:2] == [top, 0] and want[0][4:7] == [0, top, top] and want[1][4:7] == [top, top, 0] and want[n - 1][4:10] == [0] * 6


# ---- groups split by chunks ---------------------------------------------------------------------------------------------------
def test_chunk_boundary_forced_by_size(hip_ctx):
    """2^16 rows x 65 derived columns: a chunk holds 2^22 / 2^16 = 64, so limb 64 is built by a second chunk (its group evaluated again)."""
    n, count = 1 << 16, 65
    rng = random.Random(65)
    b = W.many_limbs(count)
    rows = [[rng.randrange(P)] for _ in range(n)]
    for i, v in ((0, (1 << count) - 1), (1, 1 << 64), (2047, (1 << 64) - 1), (2048, 1 | (1 << 63) | (1 << 64)), (n - 1, 0b101 << 62)):
        rows[i] = [v]
    desc, keep = b.build()
    table = hip_ctx.air_main_trace(desc, to_bytes(rows))
    for i in (0, 1, 2047, 2048, n - 1, rng.randrange(n)):
        v = rows[i][0]
        assert table_ints(table[i:i + 1])[0] == [v] + [(v >> j) & 1 for j in range(count)], i
    # the last two derived columns (one on either side of the seam), every row
    seam = air.trace_to_ints(table[:, count - 1:, :])
    assert [int(x) for x in seam[:, 0]] == [(r[0] >> 63) & 1 for r in rows] and [int(x) for x in seam[:, 1]] == [(r[0] >> 64) & 1 for r in rows]


@pytest.mark.parametrize("n", [64, 512])
def test_a_group_split_by_a_value_column_equals_the_unsplit_group(hip_ctx, n):
    rows = W.limb_rows(n, random.Random(n + 1))
    one_b, one_cols = W.split_group(False)
    two_b, two_cols = W.split_group(True)
    one, two = same_table(hip_ctx, one_b, rows), same_table(hip_ctx, two_b, rows)
    for i in range(n):
        assert [two[i][c] for c in two_cols] == [one[i][c] for c in one_cols], i


@pytest.mark.parametrize("n", [64, 4096])
def test_mixed_program_twice_on_one_context(hip_ctx, n):
    """Limbs of an input, a WORD of two limbs, a chain group seeded from it, a COUNT and a FETCH keyed by limbs and a SUM of a limb at a
    wrapping shift: the workspace is used by row-local chunks, the COUNT column and the FETCH group in turn."""
    b = W.mixed(8)
    for seed in (n + 3, n + 4):
        rows = W.mixed_rows(n, random.Random(seed))
        want = same_table(hip_ctx, b, rows)
        assert want == model_ints(b, rows)


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("n", [64, 1024])
def test_word_ops_proves_as_its_whole_table_and_as_the_oracle(hip_ctx, oracle, options, n):
    opt = api.ProofOptions(*options)
    b = air.word_ops(n, 8)
    rows = air.word_ops_inputs(n, 8, random.Random(n))
    full = to_bytes(air.word_ops_trace(rows, 8))
    desc, keep = b.build()
    assert air.route(desc, "prove")[0] == "sp_air_prove_word"
    got = hip_ctx.air_prove(desc, to_bytes(rows), opt)
    assert got == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)                        # and the CPU oracle's, from the same table
    assert api.air_verify(got, desc, opt)


@pytest.mark.parametrize("options", LK_OPTIONS)
@pytest.mark.parametrize("n,limb_bits", [(64, 4), (1024, 8)])
def test_limb_range_check_proves_as_its_whole_table(hip_ctx, options, n, limb_bits):
    """(degree_bound_factor 2: the option set with blowup 2 runs with blowup 4, as for every lookup argument)"""
    opt = api.ProofOptions(*options)
    b = air.limb_range_check(n, limb_bits, 2)
    rows = air.limb_range_check_inputs(n, limb_bits, 2, random.Random(n))
    full = air.limb_range_check_trace(rows, limb_bits, 2)
    assert b.check_trace(rows, rap=[12345]) == []
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, to_bytes(rows), opt)
    assert got == prove_full(hip_ctx, desc, to_bytes(full), options, "pub")
    with pytest.raises(api.SpError, match="PERIODIC only through sp_air_prove_pub"):  # (the LogUp sums read the table: as table_lookup_main, _pub alone takes them)
        prove_full(hip_ctx, desc, to_bytes(full), options, "ext")
    assert hip_ctx.air_prove(desc, to_bytes(rows), opt) == got                    # the kept workspace, a second time
    assert api.air_verify(got, desc, opt)
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), opt) == []
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == full


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    device_inputs_give_the_same_bytes(hip_ctx, air.limb_range_check(256, 4, 2), air.limb_range_check_inputs(256, 4, 2, random.Random(13)), api.ProofOptions(*LK_OPTIONS[0]))


# ---- operands that break the call ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1 << 8, P - 1], ids=["two-to-the-bits", "p-minus-1"])
@pytest.mark.parametrize("side", [0, 1], ids=["x", "y"])
def test_operand_out_of_range_is_refused_and_the_context_goes_on(hip_ctx, side, value):
    """On row n - 1 alone (the last lane of the second block), from prove, from main_trace and from check_trace."""
    n, bits, options = 512, 8, api.ProofOptions(*OPTIONS[0])
    b = air.word_ops(n, bits)
    rows = air.word_ops_inputs(n, bits, random.Random(n))
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    bad = [list(r) for r in rows]
    bad[n - 1][side] = value
    with pytest.raises(ValueError, match="a word operand is out of range on some row"):
        b.main.evaluate(bad)
    for call in three_calls(hip_ctx, desc, bad, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == INVALID and OUT_OF_RANGE in str(e.value), str(e.value)
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    assert api.air_verify(want, desc, options)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == air.word_ops_trace(rows, bits)


def test_the_verdict_comes_behind_a_missing_key_and_before_a_zero_denominator(hip_ctx):
    n = 64
    b = W.verdicts()
    desc, keep = b.build()
    good = W.verdicts_rows(n)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == R.main_table(b.main, good)

    def changed(zero=False, missing=False, wide=False):
        rows = [list(r) for r in good]
        if zero:
            rows[9][2] = 5
        if missing:
            rows[40][0] = 200
        if wide:
            rows[n - 1][3] = 1 << 8
        return to_bytes(rows)

    with pytest.raises(api.SpError) as e:
        hip_ctx.air_main_trace(desc, changed(zero=True))
    assert e.value.code == _lib.SP_E_ZERO_INVERSE and "denominator is zero" in str(e.value)
    for data in (changed(wide=True), changed(wide=True, zero=True)):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_main_trace(desc, data)
        assert e.value.code == INVALID and OUT_OF_RANGE in str(e.value), str(e.value)
    for data in (changed(missing=True, wide=True), changed(missing=True, wide=True, zero=True)):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_main_trace(desc, data)
        assert e.value.code == INVALID and MISSING in str(e.value), str(e.value)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == R.main_table(b.main, good)


def test_the_older_entry_points_call_kinds_8_and_9_unknown(hip_ctx):
    n, options = 64, api.ProofOptions(*OPTIONS[0])
    lib, opt = _lib.load(), options.to_c()
    for b, rows in ((W.limb_group(), W.limb_rows(n, random.Random(29))), (W.word_groups(8, 9), W.word_rows(n, 8, 9, random.Random(30)))):
        desc, keep = b.build()
        out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
        a = to_bytes(rows)
        rc = lib.sp_air_prove_fetch(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                    ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
        assert rc == INVALID and "derived column 0 has an unknown kind" in lib.sp_last_error().decode()
        table = np.zeros((n, b.main_cols, 32), dtype=np.uint8)
        rc = lib.sp_air_main_trace_fetch(hip_ctx._h, ctypes.byref(desc), None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                                         table.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)))
        assert rc == INVALID and "derived column 0 has an unknown kind" in lib.sp_last_error().decode() and not table.any()
        assert table_ints(hip_ctx.air_main_trace(desc, a)) == R.main_table(b.main, rows)


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_case(n):
    return air.limb_range_check(n, 4, 2), air.limb_range_check_inputs(n, 4, 2, random.Random(n))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds the LIMB and COUNT columns itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rank_case, (256,), LK_OPTIONS[0])
