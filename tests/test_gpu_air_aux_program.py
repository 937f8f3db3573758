"""Auxiliary columns built on the device from an aux program (sp_air_prove_aux): the proof bytes of the oracle - the reference's
fibonacci_rap example, the callback-built test AIRs, a permutation argument and a LogUp lookup - on one GPU and on sharded
contexts; the same bytes as the host callback path at 2^16 rows; and the errors."""
import ctypes

import pytest

import aux_program_airs as X
import oracle_lib as O
from lambdaworks_cairo_prover_amd import _lib, air, api
from rank_procs import run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("length", [16, 100])
@pytest.mark.parametrize("options", [(4, 3, 3, 1), (8, 5, 3, 2), (2, 4, 7, 0)])
def test_fibonacci_rap_program_gives_the_example_bytes(hip_ctx, oracle, length, options):
    """The oracle's hand-written fibonacci_rap class is the anchor: the device-built column must give its bytes."""
    trace = O.example_trace("fibonacci_rap", length, (1, 1))
    n = trace.shape[0]
    want = O.example_prove("fibonacci_rap", trace, options, (1, 1), length)
    desc, keep = air.fibonacci_rap_program(n, length).build()
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert O.example_verify("fibonacci_rap", got, options, (1, 1), length)
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_wide_air_program_gives_the_callback_bytes(hip_ctx, oracle):
    import wide_air
    from test_wide_air import to_bytes
    for n, options in ((64, (4, 3, 3, 1)), (128, (8, 4, 3, 2))):
        trace = to_bytes(wide_air.main_trace(n))
        cb_desc, cb_keep = wide_air.build(n).build()
        want = O.program_air_prove(cb_desc, trace, options)
        desc, keep = X.wide_air_program(n).build()
        got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
        assert got == want, n
        assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_many_column_air_program_gives_the_callback_bytes(hip_ctx, oracle):
    import many_column_air
    n, main_cols, aux_cols, options = 64, 64, 40, (4, 3, 3, 1)
    trace = many_column_air.main_trace(n, main_cols)
    cb_desc, cb_keep = many_column_air.build(n, main_cols, aux_cols).build()
    want = O.program_air_prove(cb_desc, trace, options)
    desc, keep = X.many_column_air_program(n, main_cols, aux_cols).build()
    assert desc.aux_desc.n_cols == 40
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert api.air_verify(got, desc, api.ProofOptions(*options))


@pytest.mark.parametrize("name,builder,n,options", [
    ("permutation", X.permutation_air, 64, (4, 3, 3, 1)),
    ("permutation", X.permutation_air, 256, (8, 4, 3, 2)),
    ("logup", X.logup_air, 64, (4, 3, 3, 1)),
    ("logup", X.logup_air, 128, (2, 6, 7, 0)),
    ("both", lambda n: X.rap_air(n, perm_shifts=range(8), logup_shifts=(1, 5, 7), extra_cols=2), 64, (4, 3, 3, 1)),
])
def test_permutation_and_logup_give_the_oracle_bytes(hip_ctx, oracle, name, builder, n, options):
    b = builder(n)
    trace = X.main_trace(n, b.main_cols - X.BASE_COLS)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = O.program_air_prove(cb_desc, trace, options)
    assert O.program_air_verify(cb_desc, want, options)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert api.air_verify(got, desc, api.ProofOptions(*options))


def test_device_program_equals_the_device_callback_at_2_16_rows(hip_ctx):
    """2^16 rows, 16 auxiliary columns (8 grand products, 8 LogUp sums, every shift 0 .. 7): sp_air_prove_aux against the same AIR
    through aux_kind 2 (the Python evaluator as the callback) on the same device."""
    n = 1 << 16
    b = X.rap_air(n, perm_shifts=range(8), logup_shifts=range(8))
    trace = X.main_trace(n)
    options = api.ProofOptions(4, 8, 3, 1)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=trace)
    want = hip_ctx.air_prove(cb_desc, trace, options)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, options)
    assert got == want
    assert hip_ctx.air_prove(desc, trace, options) == want          # the kept workspace, a second time
    assert api.air_verify(got, desc, options)


def _aux_body(rank, world, n, options):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    desc, keep = X.rap_air(n, perm_shifts=(0, 3), logup_shifts=(1, 6)).build()
    proof = ctx.air_prove(desc, X.main_trace(n), api.ProofOptions(*options))
    ctx.close()
    return proof


@pytest.mark.parametrize("world,n,options", [(2, 64, (4, 3, 3, 1)), (4, 256, (4, 4, 3, 2))])
def test_sharded_contexts_give_the_one_gpu_bytes(hip_ctx, world, n, options):
    """Every rank holds the whole main trace and builds the same columns: no exchange, the one-GPU bytes on every rank."""
    desc, keep = X.rap_air(n, perm_shifts=(0, 3), logup_shifts=(1, 6)).build()
    want = hip_ctx.air_prove(desc, X.main_trace(n), api.ProofOptions(*options))
    got = run_ranks(world, _aux_body, (n, options), timeout=600)
    for r in range(world):
        assert got[r] == want, (r, got[r][:400])


def test_errors_and_recovery(hip_ctx):
    n, options = 64, api.ProofOptions(4, 3, 3, 1)
    trace = X.main_trace(n)
    # a denominator that is zero on row 0 (t_0 = 0)
    b = X.rap_air(n, perm_shifts=(0,))
    b.aux.cols.clear()
    b.aux.product(1, b.aux.load(0, X.T))
    desc, keep = b.build()
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_prove(desc, trace, options)
    assert e.value.code == _lib.SP_E_ZERO_INVERSE
    assert "zero" in str(e.value)
    # the same context proves a valid AIR right after
    good, good_keep = X.permutation_air(n).build()
    cb_desc, cb_keep = X.permutation_air(n).build(aux_as_callback=True, main_trace=trace)
    assert hip_ctx.air_prove(good, trace, options) == O.program_air_prove(cb_desc, trace, (4, 3, 3, 1))
    # a malformed program: a LOAD of a column beyond the main trace, then an operand that refers to a later op
    bad, bad_keep = X.permutation_air(n).build()
    bad.aux_desc.ops[2].b = X.BASE_COLS                 # op 2: LOAD(0, a)
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_prove(bad, trace, options)
    assert e.value.code == _lib.SP_E_INVALID_ARG
    bad2, bad2_keep = X.permutation_air(n).build()
    bad2.aux_desc.ops[3].op, bad2.aux_desc.ops[3].a = air.OP_ADD, 9
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_prove(bad2, trace, options)
    assert e.value.code == _lib.SP_E_INVALID_ARG
    bad3, bad3_keep = X.permutation_air(n).build()
    bad3.aux_desc.cols[0].den_op = 10000
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_prove(bad3, trace, options)
    assert e.value.code == _lib.SP_E_INVALID_ARG
    # sp_air_prove keeps answering SP_E_UNSUPPORTED for aux_kind 3
    lib = _lib.load()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    opt = options.to_c()
    rc = lib.sp_air_prove(hip_ctx._h, ctypes.byref(good), trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(n),
                          ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    assert rc == _lib.SP_E_UNSUPPORTED
    assert hip_ctx.air_prove(good, trace, options) == O.program_air_prove(cb_desc, trace, (4, 3, 3, 1))


def test_violating_trace_gives_the_oracle_bytes(hip_ctx, oracle):
    """One flipped cell: the example still yields a (non-verifying) proof; the device-built column gives the same bytes."""
    length = 20
    trace = O.example_trace("fibonacci_rap", length).copy()
    trace[trace.shape[0] // 2, 0, 31] ^= 1
    n = trace.shape[0]
    options = (4, 3, 3, 1)
    want = O.example_prove("fibonacci_rap", trace, options, (1, 1), length)
    desc, keep = air.fibonacci_rap_program(n, length).build()
    got = hip_ctx.air_prove(desc, trace, api.ProofOptions(*options))
    assert got == want
    assert not O.example_verify("fibonacci_rap", got, options, (1, 1), length)
    assert not api.air_verify(got, desc, api.ProofOptions(*options))
