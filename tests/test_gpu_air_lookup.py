"""Lookup multiplicities on the device (sp_air_prove_lk, sp_air_check_trace_lk, sp_air_main_trace_lk): the COUNT columns equal the
Python-integer model cell for cell, and a proof from the input columns has the bytes of the proof from the model's whole table through
the entry points that existed before.  Every comparison is exact."""
import ctypes
import functools
import random

import numpy as np
import pytest

import air_device_checks
import lookup_airs as L
import oracle_lib as O
from air_device_checks import (LK_OPTIONS, device_inputs_give_the_same_bytes, model_ints, prove_full, table_ints, three_calls, to_bytes,
                               two_ranks_give_the_one_rank_bytes)
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
INVALID = _lib.SP_E_INVALID_ARG
OUT_OF_RANGE = "a lookup key is out of range on some row"
same_table = functools.partial(air_device_checks.same_table, model=True)      # the plain reference, and the Python model beside it


# ---- cell equality ----------------------------------------------------------------------------------------------------------
def count_data(n, key_bits, rng):
    """(table, looked-up values): a table of period 16 < n - every value repeats n / 16 times down the trace and only its first row
    counts - with a duplicate inside the period, both ends of the key range, values that are never looked up (the second half of the
    period) and looked-up values that no table entry holds; one key bit leaves room for a table of [1, 1] and looked-up bits."""
    top = (1 << key_bits) - 1
    if key_bits == 1:
        return [1, 1], [rng.randrange(2) for _ in range(n)]
    table = [rng.randrange(top + 1) for _ in range(16)]
    table[0], table[3], table[5] = top, 0, table[2]
    absent = [v for v in (rng.randrange(top + 1) for _ in range(64)) if v not in table] or [1]
    return table, [rng.choice(table[:8]) if rng.randrange(4) else rng.choice(absent) for _ in range(n)]


@pytest.mark.parametrize("key_bits", [1, 8, 9, 64])
@pytest.mark.parametrize("n", [64, 4096, 8192])
def test_column_equals_the_model_cell_for_cell(hip_ctx, n, key_bits):
    """n = 64: one wave, one sort tile; 4096: two tiles of 2048; 8192: four.  key_bits 1 and 8: one radix pass; 9: two passes, the result
    in the other ping-pong buffer; 64: eight passes, with keys at 2^64 - 1 and 0."""
    rng = random.Random(1000 * key_bits + n)
    table, xs = count_data(n, key_bits, rng)
    want = same_table(hip_ctx, L.periodic_count(table, key_bits), [[x] for x in xs])
    total = sum(r[1] for r in want)
    assert 0 < total < n and all(r[1] == 0 for r in want[len(table):])


@pytest.mark.parametrize("n", [64, 4096])
def test_one_value_everywhere_and_nothing_in_the_table(hip_ctx, n):
    table = [7, 300, 300, 9, 511, 0, 12, 100]
    want = same_table(hip_ctx, L.periodic_count(table, 9), [[300]] * n)           # every X one value: z = n on its first row
    assert [r[1] for r in want[:8]] == [0, n, 0, 0, 0, 0, 0, 0]
    want = same_table(hip_ctx, L.periodic_count(table, 9), [[1 + i % 5] for i in range(n)])   # no X in the table: all zero
    assert all(r[1] == 0 for r in want)


@pytest.mark.parametrize("n", [64, 4096])
def test_mixed_program_table(hip_ctx, n):
    """X reads a VALUE column and an input at shift 1 (wrapping), T a periodic column and an input; a SUM reads the COUNT column."""
    rng = random.Random(n)
    periodic = [rng.randrange(P) for _ in range(L.MIXED_PERIOD)]
    b, cols = L.mixed(periodic)
    rows = L.mixed_inputs(n, periodic, rng)
    want = same_table(hip_ctx, b, rows)
    if n == 64:
        assert want == L.hand_table(rows, periodic)


@pytest.mark.parametrize("n", [256, 4096])
def test_two_count_columns_with_a_chain_group_between(hip_ctx, n):
    """The second COUNT column uses the workspace the first left behind, with other key bits (16, then 64)."""
    rng = random.Random(n + 1)
    periodic = [rng.randrange(1 << 16) for _ in range(32)]
    a = [rng.choice(periodic[:20]) if rng.randrange(3) else rng.randrange(1 << 16) for _ in range(n)]
    rows = [[a[i], rng.choice(a) if rng.randrange(3) else rng.randrange(1 << 64)] for i in range(n)]
    want = same_table(hip_ctx, L.two_counts(8, periodic), rows)
    assert 0 < sum(r[2] for r in want) < n and 0 < sum(r[4] for r in want) < n


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
def proves_as_the_whole_table(ctx, b, rows, options, entries):
    assert b.check_trace(rows, rap=[12345]) == []
    desc, keep = b.build()
    full = to_bytes(model_ints(b, rows))
    opt = api.ProofOptions(*options)
    got = ctx.air_prove(desc, to_bytes(rows), opt)
    for entry in entries:
        assert got == prove_full(ctx, desc, full, options, entry), entry
    assert ctx.air_prove(desc, to_bytes(rows), opt) == got                  # the kept workspace, a second time
    assert api.air_verify(got, desc, opt)
    assert ctx.air_check_trace(desc, to_bytes(rows), opt) == []
    return desc, full, got


@pytest.mark.parametrize("options", LK_OPTIONS)
@pytest.mark.parametrize("n,period,key_bits", [(64, 8, 8), (512, 16, 64)])
def test_table_lookup_main_proof_bytes(hip_ctx, options, n, period, key_bits):
    """The auxiliary program of the lookup reads the table with op 6, which sp_air_prove_pub takes and sp_air_prove_ext refuses for the
    whole table too: the comparison with _ext is test_input_table_lookup_gives_the_oracle_bytes, whose table is an input column."""
    b, rows, table = L.lookup_case(n, period, key_bits, random.Random(n))
    desc, full, got = proves_as_the_whole_table(hip_ctx, b, rows, options, ["pub"])
    assert table_ints(air.ints_to_bytes(np.array(air.table_lookup_trace(n, table, [r[0] for r in rows]), dtype=object))) == table_ints(full)
    with pytest.raises(api.SpError):
        prove_full(hip_ctx, desc, full, options, "ext")


@pytest.mark.parametrize("options", LK_OPTIONS)
@pytest.mark.parametrize("n", [256, 1024])
def test_xor_lookup_proof_bytes(hip_ctx, options, n):
    b = air.xor_lookup(n, 4)
    proves_as_the_whole_table(hip_ctx, b, air.xor_lookup_inputs(n, 4, random.Random(n)), options, ["pub"])


@pytest.mark.parametrize("options", LK_OPTIONS)
def test_input_table_lookup_gives_the_oracle_bytes(hip_ctx, oracle, options):
    """The table is an input column, so the statement has no periodic column: _pub and _ext both prove the whole table, and so does the
    CPU oracle, with the model's auxiliary column from a callback."""
    n = 128
    b = L.input_table_lookup()
    rows = L.input_table_rows(n, random.Random(9))
    desc, full, got = proves_as_the_whole_table(hip_ctx, b, rows, options, ["pub", "ext"])
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=full)
    assert got == O.program_air_prove(cb_desc, full, options)


# ---- traces that break the statement, keys that break the call ---------------------------------------------------------------
def test_value_outside_the_table_is_proved_rejected_and_reported(hip_ctx):
    n, options = 64, api.ProofOptions(*LK_OPTIONS[0])
    b, rows, table = L.lookup_case(n, 8, 8, random.Random(17))
    rows[20] = [next(v for v in range(256) if v not in table)]
    desc, keep = b.build()
    proof = hip_ctx.air_prove(desc, to_bytes(rows), options)           # as the reference: a proof all the same ...
    assert not api.air_verify(proof, desc, options)                    # ... which no verifier accepts
    want = b.check_trace(rows, rap=[0x5eed])
    assert [(v.kind, v.index, v.first_row) for v in want] == [(air.TRANSITION, 0, n - 1)]
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), rap=[0x5eed]) == want


@pytest.mark.parametrize("side", ["x", "t"])
def test_key_out_of_range_is_refused_and_the_context_goes_on(hip_ctx, side):
    """On X only and on T only, on one row of 4096 (the second sort tile); the sorts and the searches ran on the low bits, in bounds."""
    n, options = 4096, api.ProofOptions(*LK_OPTIONS[0])
    rng = random.Random(23)
    b = L.plain_count(8)
    rows = [[rng.randrange(256), rng.randrange(256)] for _ in range(n)]
    desc, keep = b.build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    bad = [list(r) for r in rows]
    bad[3000][0 if side == "x" else 1] = 256 if side == "x" else P - 1
    for call in three_calls(hip_ctx, desc, bad, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == INVALID and OUT_OF_RANGE in str(e.value), str(e.value)
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == model_ints(b, rows)


@pytest.mark.parametrize("count_first", [False, True])
def test_key_range_and_zero_denominator_keep_their_verdicts(hip_ctx, count_first):
    """A VALUE with the denominator a - 5 before or behind the COUNT column: a zero denominator alone is SP_E_ZERO_INVERSE, a key out
    of range alone the refusal above, and both together the key range."""
    n = 64
    b = air.AirBuilder(4, [0], 1, main_inputs=2)
    m = b.main
    if count_first:
        m.multiplicity(m.load(0, 0), m.load(0, 1), 8)
    m.value(1, m.load(0, 0) - 5)
    if not count_first:
        m.multiplicity(m.load(0, 0), m.load(0, 1), 8)
    desc, keep = L.trivial(b).build()
    good = [[6 + i % 100, 6 + i % 50] for i in range(n)]
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == model_ints(b, good)
    zero, key, both = [list(r) for r in good], [list(r) for r in good], [list(r) for r in good]
    zero[9][0] = both[9][0] = 5
    key[40][1] = both[40][1] = 1 << 8
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_main_trace(desc, to_bytes(zero))
    assert e.value.code == _lib.SP_E_ZERO_INVERSE and "denominator is zero" in str(e.value)
    for rows in (key, both):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert e.value.code == INVALID and OUT_OF_RANGE in str(e.value), str(e.value)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(good))) == model_ints(b, good)


def test_malformed_count_is_refused_and_the_context_goes_on(hip_ctx):
    n, options = 64, api.ProofOptions(*LK_OPTIONS[0])
    rng = random.Random(29)
    rows = [[rng.randrange(256), rng.randrange(256)] for _ in range(n)]
    desc, keep = L.plain_count(8).build()
    want = hip_ctx.air_prove(desc, to_bytes(rows), options)
    desc.main_desc.cols[0].pad = 65
    for call in three_calls(hip_ctx, desc, rows, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == INVALID and "COUNT column with key_bits = 65" in str(e.value)
    desc.main_desc.cols[0].pad = 8
    assert hip_ctx.air_prove(desc, to_bytes(rows), options) == want
    # and through the entry points that were there before the same program has an unknown kind
    lib, opt = _lib.load(), options.to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = to_bytes(rows)
    rc = lib.sp_air_prove_rec(hip_ctx._h, ctypes.byref(desc), None, None, ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(n),
                              ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    assert rc == INVALID and "derived column 0 has an unknown kind" in lib.sp_last_error().decode()


def test_inputs_in_device_memory_give_the_same_bytes(hip_ctx):
    device_inputs_give_the_same_bytes(hip_ctx, air.xor_lookup(256, 4), air.xor_lookup_inputs(256, 4, random.Random(13)), api.ProofOptions(*LK_OPTIONS[0]))


# ---- two ranks ------------------------------------------------------------------------------------------------------------------
def _rank_case(n):
    return L.lookup_case(n, 64, 16, random.Random(31))


def test_two_ranks_give_the_one_rank_bytes(hip_ctx):
    """Every rank ingests the inputs and builds the COUNT column itself: no exchange before the commitment."""
    two_ranks_give_the_one_rank_bytes(hip_ctx, _rank_case, (4096,), LK_OPTIONS[0])
