"""Strided transition constraints on the device (sp_air_prove_ext, sp_air_check_trace_ext, sp_air_stride_table).  The CPU oracle has no
strides, so the checks are: the oracle's bytes where every stride is (1, 0), the 1 / Z table against Python integers, completeness on
the 2n-point path and soundness through the library's verifier - whose zerofier and exemption product the CPU tests pin
(tests/test_air_stride.py) -, and the trace report against the Python-integer model."""
import ctypes

import numpy as np
import pytest

import check_trace_airs as E
import oracle_lib as O
import periodic_airs as XP
import strided_airs as X
from lambdaworks_cairo_prover_amd import _lib, air, api
from rank_procs import run_child, run_ranks

pytestmark = pytest.mark.gpu

P = api.P
CASES = {"mimc": X.mimc, "two_class": X.two_class}


def _flipped(trace):
    t = trace.copy()
    t[t.shape[0] // 2, 0, 31] ^= 1
    return t


# ---- 1. all strides (1, 0): the oracle's bytes through sp_air_prove_ext -----------------------------------------------------------
def _degenerate_cases():
    out = {}
    for name, n in (("mimc1", 64), ("mimc8", 16), ("linear", 64)):            # the AIRs of periodic_airs the oracle can prove
        if name.startswith("mimc"):
            b, rows = XP.mimc(n, int(name[4:]), seed=11, same=True)
        else:
            b, rows = XP.linear(n, XP.keys(12, 1), XP.keys(13, 1) * 8)
        out[name] = (b, XP.with_constants(b), XP.to_bytes(rows), None)
    for name in ("simple_fibonacci", "fibonacci_2_columns", "quadratic", "dummy", "fibonacci_rap"):   # the five example AIRs
        b, rows = E.EXAMPLES[name](16)
        out[name] = (b, b, None, rows)
    return out


@pytest.mark.parametrize("name", ["mimc1", "mimc8", "linear", "simple_fibonacci", "fibonacci_2_columns", "quadratic", "dummy", "fibonacci_rap"])
def test_degenerate_strides_give_the_oracle_bytes(hip_ctx, oracle, name):
    """Every constraint on (1, 0) is today's statement: byte for byte the oracle's proof, for a valid trace (2n-point path) and a
    one-cell-flipped one (whole domain, deg H >= 2n)."""
    b, oracle_builder, trace, rows = _degenerate_cases()[name]
    if trace is None:
        trace = X.to_bytes([r[:b.main_cols] for r in rows])
    desc, keep = b.build()
    odesc, okeep = oracle_builder.build()
    skeep = X.degenerate(desc)
    assert desc.stride_desc.n == desc.n_transitions
    options = (4, 3, 3, 1)
    flipped = trace.copy()
    flipped[trace.shape[0] // 2, 1 if name == "dummy" else 0, 31] ^= 1
    for t, path in ((trace, 1), (flipped, 3)):
        want = O.program_air_prove(odesc, t, options)
        got = hip_ctx.air_prove(desc, t, api.ProofOptions(*options))
        assert got == want, (name, path)
        assert hip_ctx.last_proof_info()["composition_path"] == path


@pytest.mark.parametrize("name", ["mimc8", "wrap", "rap_with_selector"])
def test_degenerate_strides_beside_real_periods_give_the_unstrided_bytes(hip_ctx, name):
    """The AIRs of periodic_airs whose columns really vary are beyond the oracle: there sp_air_prove_ext with every stride (1, 0) must
    give the bytes of sp_air_prove_periodic, which tests/test_gpu_air_periodic.py holds against the verifier."""
    n = 64
    b, rows = {"mimc8": lambda: XP.mimc(n, 8, seed=22), "wrap": lambda: XP.wrap(n, XP.keys(21, 8)), "rap_with_selector": lambda: XP.rap_with_selector(n)}[name]()
    desc, keep = b.build()
    opt = api.ProofOptions(4, 3, 3, 1)
    trace = XP.to_bytes(rows)
    for t in (trace, _flipped(trace)):
        X.with_strides(desc, None)
        want = hip_ctx.air_prove(desc, t, opt)
        path = hip_ctx.last_proof_info()["composition_path"]
        skeep = X.degenerate(desc)
        assert hip_ctx.air_prove(desc, t, opt) == want
        assert hip_ctx.last_proof_info()["composition_path"] == path


# ---- 2. the table seam ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 256])
def test_stride_table_against_python_integers(hip_ctx, n):
    """out[k] = 1 / Z(h w_N^k) for one period (period x blowup points).  Period n at blowup 8 and n = 256 is 2048 entries: more than one
    256-thread block of the table kernel."""
    h = 3
    for period in (2, 8, n):
        for blowup in (2, 4, 8):
            w = X.root((n * blowup).bit_length() - 1)
            for offset in (0, period - 1):
                got = hip_ctx.air_stride_table(period, offset, n, blowup, h)
                assert got.shape == (period * blowup, 32)
                have = [int.from_bytes(bytes(r), "big") for r in got]
                x = h
                for k in range(period * blowup):
                    assert have[k] * X.zerofier(period, offset, n, x) % P == 1, (n, period, blowup, offset, k)
                    x = x * w % P


# ---- 3. completeness on the 2n-point path, 4. soundness -------------------------------------------------------------------------
@pytest.mark.parametrize("options", X.OPTIONS)
@pytest.mark.parametrize("n", X.SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_strided_airs_prove_on_the_2n_point_path_and_verify(hip_ctx, name, n, options):
    c = CASES[name](n)
    assert c.builder.check_trace(c.rows) == []
    desc, keep = c.builder.build()
    opt = api.ProofOptions(*options)
    proof = hip_ctx.air_prove(desc, X.to_bytes(c.rows), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(proof, desc, opt)


@pytest.mark.parametrize("options", X.OPTIONS)
@pytest.mark.parametrize("n", X.SIZES)
@pytest.mark.parametrize("name", list(CASES))
def test_strided_airs_soundness(hip_ctx, name, n, options):
    c = CASES[name](n)
    b = c.builder
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    proof = hip_ctx.air_prove(desc, X.to_bytes(c.rows), opt)
    assert api.air_verify(proof, desc, opt)
    # a flip on an enforced row: the reference-style proof of a violating trace, which the verifier refuses
    bad = hip_ctx.air_prove(desc, X.to_bytes(X.changed(c.rows, c.enforced_cell)), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 3
    assert not api.air_verify(bad, desc, opt)
    # a flip on the exempted tail row of the progression: still a satisfying trace
    tail = hip_ctx.air_prove(desc, X.to_bytes(X.changed(c.rows, c.tail_cell)), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(tail, desc, opt)
    # the statement includes the strides
    strided = next(k for k, s in enumerate(b.strides) if s[0] > 1)
    period, offset = b.strides[strided]
    for other in ((period * 2 if period * 2 <= n else period // 2, offset % max(1, period // 2) if period * 2 > n else offset),
                  (period, (offset + 1) % period)):
        strides = list(b.strides)
        strides[strided] = other
        skeep = X.with_strides(desc, strides)
        assert not api.air_verify(proof, desc, opt), other
    X.with_strides(desc, None)
    assert not api.air_verify(proof, desc, opt)
    desc, keep = b.build()
    assert hip_ctx.air_prove(desc, X.to_bytes(c.rows), opt) == proof          # the kept buffers, a second time


# ---- 5. the trace report -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_trace_report_equals_the_model(hip_ctx, name):
    """The three model cases of the CPU test and the clean trace, field for field.  n = 256 is four waves of one 256-row block of the
    report kernel; n = 512 adds the second block."""
    for n in (256, 512):
        c = CASES[name](n)
        desc, keep = c.builder.build()
        opt = api.ProofOptions(4, 3, 3, 1)
        for cell, count in ((c.free_cell, 0), (c.enforced_cell, 1), (c.tail_cell, 0), (None, 0)):
            rows = c.rows if cell is None else X.changed(c.rows, cell)
            want = c.builder.check_trace(rows)
            assert len(want) == count
            got = hip_ctx.air_check_trace(desc, X.to_bytes(rows), opt)
            assert got == want, (name, n, cell)
            if count:
                assert (got[0].rows, got[0].first_row, got[0].last_row) == (1, c.enforced_row, c.enforced_row)


# ---- 6. with the other extensions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,options", [(64, (4, 3, 3, 1)), (16, (8, 3, 3, 1))])
def test_aux_program_and_periodic_column_beside_a_stride(hip_ctx, n, options):
    b, rows = X.rap_with_stride(n)
    desc, keep = b.build()
    assert desc.aux_desc.n_cols == 1 and desc.periodic_desc.n_cols == 1 and desc.stride_desc.n == 2
    opt = api.ProofOptions(*options)
    trace = X.to_bytes(rows)
    proof = hip_ctx.air_prove(desc, trace, opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(proof, desc, opt)
    assert hip_ctx.air_check_trace(desc, trace, opt) == []
    skeep = X.with_strides(desc, [(4, 1), (1, 0)])
    assert not api.air_verify(proof, desc, opt)


# ---- 7. Poseidon trees -----------------------------------------------------------------------------------------------------------------
def test_poseidon_backend(hip_ctx):
    c = X.two_class(64, seed=41)
    desc, keep = c.builder.build()
    opt = api.ProofOptions(4, 3, 3, 1)
    hip_ctx.set_option(api.SP_OPT_MERKLE_BACKEND, api.SP_MERKLE_POSEIDON)
    try:
        proof = hip_ctx.air_prove(desc, X.to_bytes(c.rows), opt)
    finally:
        hip_ctx.set_option(api.SP_OPT_MERKLE_BACKEND, api.SP_MERKLE_KECCAK256)
    assert api.air_verify(proof, desc, opt, api.SP_MERKLE_POSEIDON)
    assert not api.air_verify(proof, desc, opt)


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_prover_refuses_malformed_stride_descriptors(hip_ctx):
    n, opt = 16, api.ProofOptions(4, 3, 3, 1)
    c = X.mimc(n)
    trace = X.to_bytes(c.rows)
    good, keep = c.builder.build()

    def code(desc, call=None):
        with pytest.raises(api.SpError) as e:
            (call or hip_ctx.air_prove)(desc, trace, opt)
        return e.value.code

    for label, strides in X.malformed_stride_descs(c.builder, n):
        desc, k = c.builder.build()
        skeep = X.with_strides(desc, strides)
        assert code(desc) == _lib.SP_E_INVALID_ARG, label
        assert code(desc, hip_ctx.air_check_trace) == _lib.SP_E_INVALID_ARG, label
    desc, k = c.builder.build()
    desc.exemptions[0] = n // 4                                                       # e >= n / s
    assert code(desc) == _lib.SP_E_INVALID_ARG
    desc, k = c.builder.build()
    desc.stride_desc.strides = None
    assert code(desc) == _lib.SP_E_INVALID_ARG
    desc, k = c.builder.build()
    desc.degrees[0] = 3                                                               # degree f + 1 on a stride
    assert code(desc) == _lib.SP_E_INVALID_ARG
    # five classes
    many = air.AirBuilder(1, [0, 1], 1)
    for o in range(5):
        many.constraint(many.load(1, 0) - many.load(0, 0), 1, 0, period=8, offset=o)
    many.check_limits = lambda: None
    desc, k = many.build()
    assert code(desc) == _lib.SP_E_INVALID_ARG
    # a wrong struct size in sp_air_ext
    ext = air.ext_of(good)
    ext.size += 8
    out, ln, o = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(), opt.to_c()
    a = np.ascontiguousarray(trace)
    rc = hip_ctx._lib.sp_air_prove_ext(hip_ctx._h, ctypes.byref(good), ctypes.byref(ext), a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(n),
                                       ctypes.byref(o), ctypes.byref(out), ctypes.byref(ln))
    assert rc == _lib.SP_E_INVALID_ARG
    assert api.air_verify(hip_ctx.air_prove(good, trace, opt), good, opt)              # and the context still proves


# ---- 9. sharded contexts -------------------------------------------------------------------------------------------------------------------
def _body(rank, world, n, options):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    c = X.two_class(n)
    desc, keep = c.builder.build()
    proof = ctx.air_prove(desc, X.to_bytes(c.rows), api.ProofOptions(*options))
    try:
        ctx.air_check_trace(desc, X.to_bytes(c.rows), api.ProofOptions(*options))
        report = 0
    except api.SpError as e:
        report = e.code
    ctx.close()
    return proof, report


def _single_body(n, options):
    with api.Context(device=0) as ctx:
        c = X.two_class(n)
        desc, keep = c.builder.build()
        proof = ctx.air_prove(desc, X.to_bytes(c.rows), api.ProofOptions(*options))
        assert ctx.last_proof_info()["composition_path"] == 1
    return proof


def test_sharded_contexts_give_the_one_gpu_bytes():
    """World 2 over the gloo-staged all-gather, ranks sharing the GPU: every rank builds all b cosets of the classes' tables and indexes
    them by the global LDE index.  The one-GPU proof comes from a child that has ended before the ranks start."""
    world, n, options = 2, 64, (4, 3, 3, 1)
    want = run_child(_single_body, (n, options), timeout=600)
    desc, keep = X.two_class(n).builder.build()
    assert api.air_verify(want, desc, api.ProofOptions(*options))
    got = run_ranks(world, _body, (n, options), timeout=600)
    for r in range(world):
        assert got[r] == (want, _lib.SP_E_UNSUPPORTED), (r, "proof bytes or report code differ")
