"""Sorted auxiliary columns built on the device (SP_AIR_AUX_SORTED: key pass, radix sort, gather): the proof bytes of the CPU oracle
for the two worked examples and a mixed AIR; past one sort tile and one scan segment against the host callback path; a violating trace;
the trace report against the model; the key-range error and the decoder's refusals, with recovery; a sharded context."""
import ctypes

import pytest

import oracle_lib as O
import sorted_airs as X
from lambdaworks_cairo_prover_amd import _lib, air, api
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu

P = api.P
CASES = {"range_check": X.range_check, "memory": X.memory, "mixed": X.mixed}


@pytest.mark.parametrize("options", X.OPTION_SETS)
@pytest.mark.parametrize("n", [64, 256])
@pytest.mark.parametrize("name", list(CASES))
def test_sorted_columns_give_the_oracle_bytes(hip_ctx, oracle, name, n, options):
    b, rows = CASES[name](n)
    trace = X.to_bytes(rows)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = O.program_air_prove(cb_desc, trace, options)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_past_one_sort_tile_and_one_scan_segment(hip_ctx):
    """2^14 rows: 8 tiles of 2048 pairs and 2 segments of the histogram scan.  The mixed AIR - full-range 64-bit keys with 0 and
    2^64 - 1 several times each, and a 16-bit group - against the same AIR through aux_kind 2 (the Python model as the callback) on
    the same device; a second proof on the kept workspace."""
    n = 1 << 14
    b, rows = X.mixed(n)
    assert sum(r[1] == 0 for r in rows) >= 3 and sum(r[1] == X.U64 for r in rows) >= 3
    trace = X.to_bytes(rows)
    options = api.ProofOptions(4, 8, 3, 1)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = hip_ctx.air_prove(cb_desc, trace, options)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, options)
    assert got == want
    assert hip_ctx.air_prove(desc, trace, options) == want
    assert api.air_verify(got, desc, options)


def test_violating_trace_gives_the_oracle_bytes(hip_ctx, oracle):
    """One changed value of a memory cell: still a proof, the oracle's bytes, and both verifiers refuse it."""
    options = (4, 3, 3, 1)
    b, rows = X.memory(64)
    bad, position = X.flipped_memory(rows)
    trace = X.to_bytes(bad)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = O.program_air_prove(cb_desc, trace, options)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert not O.program_air_verify(cb_desc, got, options)
    assert not api.air_verify(got, desc, api.ProofOptions(*options))


def test_check_trace_equals_the_model(hip_ctx):
    n = 64
    mb, mrows = X.memory(n)
    mbad, position = X.flipped_memory(mrows)
    rb, rrows = X.range_check(n)
    rbad = X.changed(rrows, (9, 0), to=max(r[0] for r in rrows) + 1)        # one value beyond the range
    for label, b, rows, given, clean in (("memory", mb, mrows, [7, 11], True), ("memory, one value changed", mb, mbad, [7, 11], False),
                                         ("range check", rb, rrows, [5], True), ("range check, one value beyond", rb, rbad, [5], False)):
        desc, keep = b.build()
        want = b.check_trace(rows, given)
        assert (want == []) == clean, label
        assert hip_ctx.air_check_trace(desc, X.to_bytes(rows), rap=given) == want, label
    want = mb.check_trace(mbad, [7, 11])
    assert [(v.kind, v.index, v.first_row, v.last_row) for v in want] == [(air.TRANSITION, 2, position - 1, position)]


def _proves_the_oracle_bytes(hip_ctx, b, rows):
    trace = X.to_bytes(rows)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    desc, keep = b.build()
    assert hip_ctx.air_prove(desc, trace, api.ProofOptions(4, 3, 3, 1)) == O.program_air_prove(cb_desc, trace, (4, 3, 3, 1))


def test_a_key_out_of_range_is_an_error_and_the_context_recovers(hip_ctx, oracle):
    options = api.ProofOptions(4, 3, 3, 1)
    rb, rrows = X.range_check(64)
    mb, mrows = X.memory(64)
    for b, rows in ((rb, X.changed(rrows, (17, 0), to=1 << 16)),          # 2^16 under 16 key bits
                    (mb, X.changed(mrows, (40, 0), to=P - 1))):          # a "negative" address under 64 key bits
        desc, keep = b.build()
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_prove(desc, X.to_bytes(rows), options)
        assert e.value.code == _lib.SP_E_INVALID_ARG
        assert "key" in str(e.value) and "out of range" in str(e.value)
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_check_trace(desc, X.to_bytes(rows), rap=[3] * b.n_rap)
        assert e.value.code == _lib.SP_E_INVALID_ARG
        _proves_the_oracle_bytes(hip_ctx, rb, rrows)
        _proves_the_oracle_bytes(hip_ctx, mb, mrows)


def _first_sorted_load(desc, main_cols):
    return [i for i in range(desc.aux_desc.n_ops) if desc.aux_desc.ops[i].op == air.OP_LOAD and desc.aux_desc.ops[i].b >= main_cols][0]


def test_hand_edited_descriptors_are_refused(hip_ctx, oracle):
    """memory_consistency's columns: 0 addr' and 1 val' (sorted by op `key`), 2 the product."""
    options = api.ProofOptions(4, 3, 3, 1)
    b, rows = X.memory(64)
    trace = X.to_bytes(rows)

    def kind_3(x): x.cols[1].kind = 3
    def no_key(x): x.cols[1].den_op = air.AUX_NO_DEN
    def pad_65(x): x.cols[0].pad = x.cols[1].pad = 65
    def load_of_a_product(x): x.ops[_first_sorted_load(b.build()[0], b.main_cols)].b = b.main_cols + 2
    def key_reads_a_sorted_column(x): x.cols[1].den_op = _first_sorted_load(b.build()[0], b.main_cols)
    def groups_disagree(x): x.cols[1].pad = 16
    for patch in (kind_3, no_key, pad_65, load_of_a_product, key_reads_a_sorted_column, groups_disagree):
        desc, keep = b.build()
        patch(desc.aux_desc)
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_prove(desc, trace, options)
        assert e.value.code == _lib.SP_E_INVALID_ARG, patch.__name__
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_check_trace(desc, trace, rap=[7, 11])
        assert e.value.code == _lib.SP_E_INVALID_ARG, patch.__name__
    # pad is ignored for products and sums; 0 means 64 for a sorted column
    desc, keep = b.build()
    desc.aux_desc.cols[2].pad = 65
    desc.aux_desc.cols[0].pad = desc.aux_desc.cols[1].pad = 0
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = O.program_air_prove(cb_desc, trace, (4, 3, 3, 1))
    assert hip_ctx.air_prove(desc, trace, options) == want
    # sp_air_prove keeps answering SP_E_UNSUPPORTED for aux_kind 3
    good, good_keep = b.build()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    opt = options.to_c()
    rc = _lib.load().sp_air_prove(hip_ctx._h, ctypes.byref(good), trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(64),
                                  ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    assert rc == _lib.SP_E_UNSUPPORTED
    assert hip_ctx.air_prove(good, trace, options) == want


def _body(rank, world, n, options):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    proofs = []
    for make in (X.range_check, X.memory, X.mixed):
        b, rows = make(n)
        desc, keep = b.build()
        proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
    ctx.close()
    return proofs


def test_sharded_contexts_give_the_one_gpu_bytes(hip_ctx):
    """Every rank holds the whole main trace and sorts it itself: no exchange, the one-GPU bytes on both ranks."""
    world, n, options = 2, 64, (4, 3, 3, 1)
    want = []
    for make in (X.range_check, X.memory, X.mixed):
        b, rows = make(n)
        desc, keep = b.build()
        want.append(hip_ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
    got = run_ranks(world, _body, (n, options), timeout=600)
    for r in range(world):
        assert got[r] == want, (r, "proof bytes differ")
