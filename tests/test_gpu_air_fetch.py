"""Looked-up values on the device (sp_air_prove_fetch, sp_air_check_trace_fetch, sp_air_main_trace_fetch): the FETCH columns equal the
plain reference of program_ref cell for cell, grouping changes no cell, and a proof from the input columns has the bytes of the proof from
the whole table through the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import fetch_airs as F
import program_ref as R
from air_device_checks import (LK_OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, same_table, table_ints, three_calls, to_bytes,
                               two_ranks_give_the_one_rank_bytes)
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "a lookup key is out of range on some row"
MISSING = "a fetched key is in no table row"


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits", [1, 8, 9, 64])
@pytest.mark.parametrize("n", [64, 256, 4096, 8192])
def test_table_equals_the_reference_cell_for_cell(hip_ctx, n, key_bits):
    """n = 64: a quarter of one 256-lane group, one sort tile; 256: one whole group; 4096: two sort tiles of 2048; 8192: four.  key_bits 1
    and 8: one radix pass; 9: two passes, the result in the other ping-pong buffer; 64: eight passes, with the keys 2^64 - 1 and 0.  The
    table is a pair of input columns with duplicate keys whose values differ; rows 0 and n - 1 look up the smallest and the largest key."""
    rng = random.Random(1000 * key_bits + n)
    rows = F.input_rows(n, key_bits, rng, distinct=min(n // 3, 1 << key_bits))
    t = [r[1] for r in rows]
    assert rows[0][0] == min(t) == 0 and rows[-1][0] == max(t) == (1 << key_bits) - 1 and len(set(t)) < n
    want = same_table(hip_ctx, F.input_fetch(2, key_bits), rows)
    first = {}
    for j, key in enumerate(t):
        first.setdefault(key, j)
    assert all(want[i][3] == rows[first[rows[i][0]]][2] for i in range(n))        # the lowest row wins


@pytest.mark.parametrize("n", [64, 4096])
def test_every_row_looks_up_one_key_and_a_periodic_table(hip_ctx, n):
    keys = [7, 300, 300, 9, 511, 0, 12, 100]
    values = [[11 * j + 1 for j in range(8)], [P - 1 - j for j in range(8)]]
    b = F.periodic_fetch(keys, values, 9)
    want = same_table(hip_ctx, b, [[300]] * n)                                    # the first of the two rows that hold 300
    assert all(r[1:] == [12, P - 2] for r in want)
    want = same_table(hip_ctx, b, [[keys[(5 * i) % 8]] for i in range(n)])
    assert {r[1] for r in want} == {1, 12, 34, 45, 56, 67, 78}                    # (every value but that of the second 300)


# ---- grouping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 4096])
def test_a_run_of_sixteen_equals_two_runs_around_a_value_column(hip_ctx, n):
    rows = F.input_rows(n, 64, random.Random(n + 2))
    one = same_table(hip_ctx, F.input_fetch(16), rows)
    b, cols = F.separated(16)
    two = same_table(hip_ctx, b, rows)
    for i in range(n):
        assert [two[i][c] for c in cols] == one[i][3:], i


def test_a_run_of_seventeen_splits(hip_ctx):
    n = 256
    rows = F.input_rows(n, 64, random.Random(17))
    want = same_table(hip_ctx, F.input_fetch(17), rows)
    assert all(want[i][3 + 16] == (17 * want[i][3] + 16) % P for i in range(n))      # column 3 + j holds (j + 1) v + j of the fetched row


@pytest.mark.parametrize("n", [64, 4096])
def test_mixed_program_twice_on_one_context(hip_ctx, n):
    """A FETCH, a chain group that reads it, a COUNT on the same table, a second FETCH of the chain column and a SUM: the workspace is
    used by the FETCH group, the COUNT column and the row-local chunk in turn."""
    b = F.mixed(8)
    for seed in (n + 3, n + 4):
        rows = F.input_rows(n, 64, random.Random(seed))
        want = same_table(hip_ctx, b, rows)
        assert want == model_ints(b, rows)
    same_table(hip_ctx, F.chain_fetch(8), F.input_rows(n, 64, random.Random(n + 5)))
    same_table(hip_ctx, F.count_and_fetch(8), F.input_rows(n, 8, random.Random(n + 6)))


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", LK_OPTIONS)
@pytest.mark.parametrize("n", [256, 1024])
def test_xor_fetch_proves_as_xor_lookup(hip_ctx, options, n):
    opt = api.ProofOptions(*options)
    b, whole = air.xor_fetch(n, 4), air.xor_lookup(n, 4)
    desc, keep = b.build()
    whole_desc, whole_keep = whole.build()
    assert air.route(desc, "prove")[0] == "sp_air_prove_fetch" and air.route(whole_desc, "prove")[0] == "sp_air_prove_lk"
    got = hip_ctx.air_prove(desc, to_bytes(air.xor_fetch_inputs(n, 4, random.Random(n))), opt)
    assert got == hip_ctx.air_prove(whole_desc, to_bytes(air.xor_lookup_inputs(n, 4, random.Random(n))), opt)
    assert api.air_verify(got, whole_desc, opt) and api.air_verify(got, desc, opt)
    assert hip_ctx.air_check_trace(desc, to_bytes(air.xor_fetch_inputs(n, 4, random.Random(n))), opt) == []


@pytest.mark.parametrize("options", LK_OPTIONS)
@pytest.mark.parametrize("n,key_bits", [(64, 8), (1024, 64)])
def test_rom_reads_proves_as_its_whole_table(hip_ctx, options, n, key_bits):
    opt = api.ProofOptions(*options)
    b = air.rom_reads(n, key_bits)
    rows = air.rom_reads_inputs(n, key_bits, random.Random(n))
    full = air.rom_reads_trace(rows)
    assert b.check_trace(rows, rap=[12345, 678]) == []
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, to_bytes(rows), opt)
    for entry in ("pub", "ext"):
        assert got == prove_full(hip_ctx, desc, to_bytes(full), options, entry), entry
    assert hip_ctx.air_prove(desc, to_bytes(rows), opt) == got                    # the kept workspace, a second time
    assert api.air_verify(got, desc, opt)
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), opt) == []
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == full


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    device_inputs_give_the_same_bytes(hip_ctx, air.xor_fetch(256, 4), air.xor_fetch_inputs(256, 4, random.Random(13)), api.ProofOptions(*LK_OPTIONS[0]))


# ---- keys that break the call ------------------------------------------------------------------------------------------------------
def _rom_case(n):
    """rom_reads with 16 key bits whose written addresses lie in 1000 .. 1000 + n - 1: keys above and below every table key exist."""
    rng = random.Random(n)
    addrs = list(range(1000, 1000 + n))
    rng.shuffle(addrs)
    return air.rom_reads(n, 16), [[addrs[i], rng.randrange(P), addrs[rng.randrange(n // 2)]] for i in range(n)]


@pytest.mark.parametrize("key", [999, 1000 + 4096, 0, (1 << 16) - 1], ids=["just-below", "just-above", "zero", "top"])
def test_missing_key_is_refused_and_the_context_goes_on(hip_ctx, key):
    """On one row of 4096 (the second sort tile): a key below every table key (the search ends on position 0) and one above them all (it
    ends on n, where nothing is read), from prove, from main_trace and from check_trace."""
    n, options = 4096, api.ProofOptions(*LK_OPTIONS[0])
    b, rows = _rom_case(n)
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    bad = [list(r) for r in rows]
    bad[3000][2] = key
    with pytest.raises(ValueError, match=MISSING):
        b.main.evaluate(bad)
    for call in three_calls(hip_ctx, desc, bad, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == INVALID and MISSING in str(e.value), str(e.value)
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    assert api.air_verify(want, desc, options)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == air.rom_reads_trace(rows)


@pytest.mark.parametrize("side", ["x", "t"])
def test_key_out_of_range_keeps_its_message_beside_a_missing_key(hip_ctx, side):
    n, options = 4096, api.ProofOptions(*LK_OPTIONS[0])
    b, rows = _rom_case(n)
    desc, keep = b.build()
    bad = [list(r) for r in rows]
    bad[17][2] = 5                                                                 # in range, in no table row
    bad[3000][2 if side == "x" else 0] = (1 << 16) if side == "x" else P - 1       # out of range (and, on X, in no table row either)
    for call in three_calls(hip_ctx, desc, bad, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == INVALID and OUT_OF_RANGE in str(e.value), str(e.value)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == air.rom_reads_trace(rows)


def test_zero_denominator_keeps_its_verdict_and_yields_to_a_missing_key(hip_ctx):
    n = 64
    b = F.zero_den_beside_a_fetch()
    desc, keep = b.build()
    good = [[i % 50, i % 50 if i < 50 else 7, 6 + i] for i in range(n)]
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == R.main_table(b.main, good)
    zero, missing, both = [list(r) for r in good], [list(r) for r in good], [list(r) for r in good]
    zero[9][2] = both[9][2] = 5
    missing[40][0] = both[40][0] = 200
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_main_trace(desc, to_bytes(zero))
    assert e.value.code == _lib.SP_E_ZERO_INVERSE and "denominator is zero" in str(e.value)
    for rows in (missing, both):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert e.value.code == INVALID and MISSING in str(e.value), str(e.value)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == R.main_table(b.main, good)


def test_the_older_entry_points_call_kind_7_unknown(hip_ctx):
    n, options = 64, api.ProofOptions(*LK_OPTIONS[0])
    b, rows = F.input_fetch(1, 8), F.input_rows(64, 8, random.Random(29))
    desc, keep = b.build()
    lib, opt = _lib.load(), options.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = to_bytes(rows)
    rc = lib.sp_air_prove_div(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                              ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    assert rc == INVALID and "derived column 0 has an unknown kind" in lib.sp_last_error().decode()
    assert table_ints(hip_ctx.air_main_trace(desc, a)) == R.main_table(b.main, rows)


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds the FETCH and COUNT columns itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rom_case, (4096,), LK_OPTIONS[0])
