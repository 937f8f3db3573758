"""One multiplicity column for several looked-up columns on the device (sp_air_prove_multi, sp_air_check_trace_multi,
sp_air_main_trace_multi): the joint COUNT column equals the plain reference (multi_ref) cell for cell, and a proof from the input
columns has the bytes of the proof from the whole table through the entry points that existed before.  Every comparison is exact."""
import ctypes
import random

import pytest

import multi_programs as G
import multi_ref as R
import oracle_lib as O
from air_device_checks import LK_OPTIONS, OPTIONS, model_ints, prove_full, table_ints, three_calls, to_bytes
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu
P = air.P
OUT_OF_RANGE = "a lookup key is out of range on some row"


# ---- cell equality ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key_bits", [1, 16, 64])
@pytest.mark.parametrize("L", [1, 2, 3, 16])
@pytest.mark.parametrize("n", [8, 64, 512, 4096])
def test_table_equals_the_reference_cell_for_cell(hip_ctx, n, L, key_bits):
    """n = 8: part of one wave; 64: one wave; 512: two work-groups of the store kernel; 4096 x 16: 256 work-groups of the search.  Every
    shape of multi_programs.SHAPES: all lanes on one counter, all keys distinct, a table of period n / 4, table values nobody looks up
    and looked-up values in no table row, looked-up values that read a LIMB column at wrapping shifts, a periodic table.  At 64 key
    bits half of the keys have bit 63 set."""
    for shape in G.SHAPES:
        b, rows = G.case(n, L, key_bits, shape, 1)
        desc, keep = b.build()
        assert air.main_suffix(desc) == "multi"
        want = R.main_table(b.main, rows)
        got = hip_ctx.air_main_trace(desc, to_bytes(rows))
        assert got.shape == (n, b.main_cols, 32)
        got = table_ints(got)
        for i in range(n):
            assert got[i] == want[i], (shape, i)


def test_a_list_of_one_gives_the_plain_columns_table(hip_ctx):
    for n, key_bits in ((64, 16), (4096, 64)):
        rows = G.lookup_rows(n, 2, key_bits, random.Random(n))
        tables = []
        for joint in (True, False):
            desc, keep = G.single(joint, key_bits).build()
            assert air.main_suffix(desc) == ("multi" if joint else "lk")
            tables.append(table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))))
        assert tables[0] == tables[1] == R.main_table(G.single(True, key_bits).main, rows)


def test_old_form_columns_give_the_same_table_through_multi_as_through_lk(hip_ctx):
    lib = _lib.load()
    n = 512
    b = G.old_only()
    rows = G.lookup_rows(n, 3, 16, random.Random(3))
    desc, keep = b.build()
    assert air.main_suffix(desc) == "lk"
    a, ext = to_bytes(rows), air.ext_of(desc)
    tables = []
    for name in ("sp_air_main_trace_multi", "sp_air_main_trace_lk"):
        table = (ctypes.c_uint8 * (n * b.main_cols * 32))()
        _lib.check(getattr(lib, name)(hip_ctx._h, ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(desc.main_desc), a.ctypes.data_as(ctypes.c_void_p),
                                      ctypes.c_uint64(n), table))
        tables.append(bytes(table))
    assert tables[0] == tables[1] == hip_ctx.air_main_trace(desc, a).tobytes()
    assert table_ints(hip_ctx.air_main_trace(desc, a)) == R.main_table(b.main, rows)


def test_the_same_context_twice_with_other_inputs_one_large_program_and_one_small_in_turn(hip_ctx):
    """The counters are zeroed on the stream on every run: a second table on the same context does not see the first one's counts, and a
    small program behind a large one does not see the large one's workspace."""
    large, small = G.case(4096, 16, 16, "hot", 7), G.case(64, 2, 16, "period", 7)
    for attempt in range(2):
        for (b, rows), n in ((large, 4096), (small, 64), (large, 4096)):
            rng = random.Random(attempt * 100 + n)
            rows = [list(r) for r in rows]
            if attempt:                           # other inputs: the looked-up values move to another table value
                other = rows[rng.randrange(n)][-1]
                rows = [[other] * (len(r) - 1) + [r[-1]] for r in rows]
            desc, keep = b.build()
            assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == R.main_table(b.main, rows), (attempt, n)


@pytest.mark.parametrize("value", [1 << 16, P - 1], ids=["2^16", "p-1"])
def test_a_key_out_of_range_is_invalid_arg_and_the_context_goes_on(hip_ctx, value):
    """One cell of the last looked-up value, X_(L-1), on one row."""
    n, L, options = 512, 3, api.ProofOptions(4, 3, 3, 1)
    b, rows = G.case(n, L, 16, "period", 9)
    desc, keep = b.build()
    want = R.main_table(b.main, rows)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == want
    bad = [list(r) for r in rows]
    bad[301][L - 1] = value
    with pytest.raises(R.KeyOutOfRange):
        R.main_table(b.main, bad)
    for call in three_calls(hip_ctx, desc, bad, options):
        with pytest.raises(api.SpError) as e:
            call()
        assert e.value.code == _lib.SP_E_INVALID_ARG and OUT_OF_RANGE in str(e.value), str(e.value)
    message = _lib.load().sp_last_error().decode()
    assert "X and T of a COUNT column must be below 2^key_bits as canonical integers" in message, message
    quiet = [list(r) for r in rows]
    quiet[301][L - 1] = (1 << 16) - 1           # in range and in no table row: counted nowhere
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(quiet))) == R.main_table(b.main, quiet)
    other, other_rows = G.case(64, 2, 64, "distinct", 9)
    other_desc, other_keep = other.build()
    assert table_ints(hip_ctx.air_main_trace(other_desc, to_bytes(other_rows))) == R.main_table(other.main, other_rows)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == want


# ---- the worked example ---------------------------------------------------------------------------------------------------------
def test_limb_range_check_joint_table_proof_and_check(hip_ctx):
    n, limb_bits, count = 1 << 10, 4, 4
    options = LK_OPTIONS[0]
    b = air.limb_range_check_joint(n, limb_bits, count)
    rng = random.Random(21)
    rows = air.limb_range_check_joint_inputs(n, limb_bits, count, rng)
    table = air.limb_range_check_joint_trace(rows, limb_bits, count)
    desc, keep = b.build()
    assert air.main_suffix(desc) == "multi" and (b.main_cols, b.aux_cols) == (6, 3)
    assert table_ints(hip_ctx.air_main_trace(desc, to_bytes(rows))) == table == R.main_table(b.main, rows) == model_ints(b, rows)
    proof = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))          # sp_air_prove_multi from the input column
    assert proof == prove_full(hip_ctx, desc, to_bytes(table), options, "pub")            # sp_air_prove_pub from the whole table
    assert api.air_verify(proof, desc, api.ProofOptions(*options))                        # sp_air_verify_pub
    assert air.route(desc, "verify")[0] == "sp_air_verify_pub"
    assert hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options)) == proof   # the kept workspace, a second time
    # a table with one m cell changed: a proof all the same, which the verifier rejects
    wrong = [list(r) for r in table]
    wrong[3][count + 1] += 1
    forged = prove_full(hip_ctx, desc, to_bytes(wrong), options, "pub")
    assert forged != proof and not api.air_verify(forged, desc, api.ProofOptions(*options))
    # the trace check: nothing on the honest inputs, the recomposition (constraint 0) for an x out of range
    assert hip_ctx.air_check_trace(desc, to_bytes(rows), api.ProofOptions(*options)) == []
    bad = [list(r) for r in rows]
    bad[77] = [(1 << (limb_bits * count)) + 5]
    report = hip_ctx.air_check_trace(desc, to_bytes(bad), api.ProofOptions(*options))
    assert [(v.kind, v.index, v.rows, v.first_row, v.last_row) for v in report] == [(air.TRANSITION, 0, 1, 77, 77)], report
    out_of_range = hip_ctx.air_prove(desc, to_bytes(bad), api.ProofOptions(*options))
    assert not api.air_verify(out_of_range, desc, api.ProofOptions(*options))


# ---- proof bytes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
def test_plain_joint_proof_bytes_equal_the_oracles(hip_ctx, oracle, options):
    """plain_joint has no periodic column, no stride and no auxiliary segment - the table is an input column -: the CPU oracle, which
    takes the descriptor alone, proves the same table."""
    n = 64
    b = G.plain_joint()
    rows = G.lookup_rows(n, 3, 15, random.Random(8), span=24)
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    assert air.main_suffix(desc) == "multi"
    want = R.main_table(b.main, rows)
    assert model_ints(b, rows) == want and 0 < sum(r[3] for r in want) < 2 * n
    full = to_bytes(want)
    got = hip_ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert got == prove_full(hip_ctx, desc, full, options, "pub") == prove_full(hip_ctx, desc, full, options, "ext")
    assert got == O.program_air_prove(desc, full, options)
    assert api.air_verify(got, desc, api.ProofOptions(*options))
