"""Public data inside a randomized argument on the device (sp_air_prove_pub, sp_air_check_trace_pub): an auxiliary program that reads a
periodic column against the same AIR with the column built by the Python model on the host (the existing sp_air_prove_periodic) and,
for a table of equal values, against the CPU oracle; boundary values computed from the challenges against the AIR frozen under the
recorded challenges (the existing sp_air_prove_aux, and the oracle); the trace report against the model; the refusals; a sharded context."""
import ctypes

import pytest

import oracle_lib as O
import public_airs as X
import strided_airs
from lambdaworks_cairo_prover_amd import _lib, air, api
from rank_procs import run_child, run_ranks

pytestmark = pytest.mark.gpu

P = api.P
OPT = api.ProofOptions(*X.OPTIONS)


# ---- 1. op 6 in the auxiliary program ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,period,shift", [(16, 1, 0), (16, 4, 0), (16, 16, 0), (512, 8, 0), (512, 8, 7)])
def test_table_reads_give_the_host_model_bytes(hip_ctx, n, period, shift):
    """A lookup whose table read is `shift` rows ahead, beside an auxiliary column without a table read: the device-built columns give,
    byte for byte, the proof of the same AIR whose columns the Python model builds in a host callback (sp_air_prove_periodic).  512 rows:
    two 256-lane blocks; period 4 and 8: (i + shift) mod period wraps many times; period 1 and n: both ends."""
    b, rows = X.shifted_lookup(n, period, shift)
    trace = X.to_bytes(rows)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=rows)
    assert not air.needs_pub(cb_desc) and cb_desc.periodic_desc.n_cols == 1
    want = hip_ctx.air_prove(cb_desc, trace, OPT)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    desc, keep = b.build()
    assert air.needs_pub(desc) and desc.aux_desc.n_cols == 2
    got = hip_ctx.air_prove(desc, trace, OPT)
    assert got == want
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(got, desc, OPT)
    assert hip_ctx.air_prove(desc, trace, OPT) == want           # the kept buffers, a second time


@pytest.mark.parametrize("n,period", [(16, 4), (512, 8)])
def test_worked_example_lookup(hip_ctx, n, period):
    b, rows = X.table_lookup(n, period)
    trace = X.to_bytes(rows)
    cb_desc, cb_keep = b.build(aux_as_callback=True, main_trace=rows)
    want = hip_ctx.air_prove(cb_desc, trace, OPT)
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, OPT)
    assert got == want
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(got, desc, OPT)
    desc.periodic_desc, other_keep = air.periodic_desc([[(v + (j == period - 1)) % P for j, v in enumerate(b.periodic_cols[0])]])
    assert not api.air_verify(got, desc, OPT)                    # the table is part of the statement


def test_equal_table_gives_the_oracle_bytes(hip_ctx, oracle):
    """A table of equal values is a constant: the CPU oracle proves the AIR with every table read - the constraint program's and the
    auxiliary program's - rewritten to that constant, and the device must give its bytes."""
    n = 16
    for b, rows in (X.table_lookup(n, 4, same=True), X.shifted_lookup(n, 4, 7, same=True)):
        trace = X.to_bytes(rows)
        c = X.with_constants(b)
        assert not c.periodic_cols and not c.aux.reads_table()
        cdesc, ckeep = c.build(aux_as_callback=True, main_trace=rows)
        want = O.program_air_prove(cdesc, trace, X.OPTIONS)
        # (the oracle's verifier takes the frame rows of its DEEP check as consecutive, so it is asked about offsets [0, 1] only; its
        # prover reads the offsets themselves, and the library's verifier checks its proof of offsets [0, 1, 7])
        assert b.offsets != [0, 1] or O.program_air_verify(cdesc, want, X.OPTIONS)
        assert api.air_verify(want, cdesc, OPT)
        desc, keep = b.build()
        assert hip_ctx.air_prove(desc, trace, OPT) == want
        assert hip_ctx.last_proof_info()["composition_path"] == 1


# ---- 2. boundary values computed from the challenges ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64])
def test_boundary_from_equals_the_frozen_air(hip_ctx, oracle, n):
    b, rows = X.public_permutation(n, 5)
    trace = X.to_bytes(rows)
    rap = X.sampled_rap(hip_ctx, b, rows, X.OPTIONS)             # (from the main commitment and the options alone)
    assert b.check_trace(rows, rap) == []
    f = X.frozen(b, rap)
    assert f.bcs[3][2] == b.resolve_boundary(rap)[0] != 0 and not f.bvalues
    fdesc, fkeep = f.build()
    assert not air.needs_pub(fdesc)
    want = hip_ctx.air_prove(fdesc, trace, OPT)                   # sp_air_prove_aux
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    desc, keep = b.build()
    got = hip_ctx.air_prove(desc, trace, OPT)
    assert got == want
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(got, desc, OPT) and api.air_verify(got, fdesc, OPT)
    if n == 16:
        cdesc, ckeep = f.build(aux_as_callback=True, main_trace=rows)
        assert O.program_air_prove(cdesc, trace, X.OPTIONS) == got
    # another public list: the same proof is refused, and the verifier got there through the challenge it replayed
    public = X.keys(2 + 2000, 5)
    public[0] = (public[0] + 1) % P
    other, okeep = air.public_permutation(n, public).build()
    assert not api.air_verify(got, other, OPT)


# ---- 3. the trace report ---------------------------------------------------------------------------------------------------------------
def test_check_trace_equals_the_model(hip_ctx):
    n, given = 16, [0x5eed]
    look, lrows = X.table_lookup(n, 4)
    perm, prows = X.public_permutation(n, 5)
    public = X.keys(2 + 2000, 5)
    public[2] = (public[2] + 1) % P
    other = air.public_permutation(n, public)
    cases = [("lookup", look, lrows, 0), ("lookup, one a changed", look, X.changed(lrows, (5, 0)), 1),
             ("permutation", perm, prows, 0), ("permutation, one public value changed", other, prows, 1)]
    for label, b, rows, count in cases:
        desc, keep = b.build()
        trace = X.to_bytes(rows)
        assert hip_ctx.air_check_trace(desc, trace, rap=given) == b.check_trace(rows, given), label
        sampled = X.sampled_rap(hip_ctx, b, rows, X.OPTIONS)
        want = b.check_trace(rows, sampled)
        assert len(want) == count, label
        assert hip_ctx.air_check_trace(desc, trace, options=OPT) == want, label
    assert [(v.kind, v.index) for v in want] == [(air.BOUNDARY, 3)]


def test_zero_denominator_of_a_boundary_value(hip_ctx):
    b, rows = X.boundary_over_difference(16, 77)
    desc, keep = b.build()
    trace = X.to_bytes(rows)
    assert hip_ctx.air_check_trace(desc, trace, rap=[78]) == b.check_trace(rows, [78]) == []
    with pytest.raises(api.SpError) as e:
        hip_ctx.air_check_trace(desc, trace, rap=[77])
    assert e.value.code == _lib.SP_E_ZERO_INVERSE
    assert api.air_verify(hip_ctx.air_prove(desc, trace, OPT), desc, OPT)        # and the context still proves


# ---- 4. refusals, and the old entry points ---------------------------------------------------------------------------------------------
def _prove(lib, ctx, name, desc, trace, *middle):
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    opt = OPT.to_c()
    code = getattr(lib, name)(ctx._h, ctypes.byref(desc), *middle, trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(trace.shape[0]),
                              ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    if code != _lib.SP_OK:
        return code
    proof = ctypes.string_at(out, ln.value)
    lib.sp_free(out)
    return proof


def test_old_entry_points_refuse_and_pub_without_public_data_is_ext(hip_lib, hip_ctx):
    b, rows = X.table_lookup(16, 4)
    desc, keep = b.build()
    trace = X.to_bytes(rows)
    ext = air.ext_of(desc)
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_ext", desc, trace, ctypes.byref(ext)) == _lib.SP_E_INVALID_ARG
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_periodic", desc, trace, ctypes.byref(desc.aux_desc), ctypes.byref(desc.periodic_desc)) == _lib.SP_E_INVALID_ARG
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_aux", desc, trace, ctypes.byref(desc.aux_desc)) == _lib.SP_E_INVALID_ARG
    # through _pub: a table read needs ext->periodic, and a column that is there
    assert isinstance(_prove(hip_lib, hip_ctx, "sp_air_prove_pub", desc, trace, ctypes.byref(ext), None), bytes)
    ext.periodic = None
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_pub", desc, trace, ctypes.byref(ext), None) == _lib.SP_E_INVALID_ARG
    desc, keep = b.build()
    at = [i for i in range(desc.aux_desc.n_ops) if desc.aux_desc.ops[i].op == air.OP_PERIODIC][0]
    desc.aux_desc.ops[at].b = 1
    ext = air.ext_of(desc)
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_pub", desc, trace, ctypes.byref(ext), None) == _lib.SP_E_INVALID_ARG
    # malformed boundary values: SP_E_INVALID_ARG from the prover and the trace check
    perm, prows = X.public_permutation(16, 5)
    ptrace = X.to_bytes(prows)
    for patch in (lambda d: setattr(d.values[0], "boundary", 4), lambda d: setattr(d, "ops", None), lambda d: setattr(d.ops[0], "op", 0),
                  lambda d: setattr(d.values[0], "num_op", d.n_ops)):
        desc, keep = perm.build()
        patch(desc.boundary_desc)
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_prove(desc, ptrace, OPT)
        assert e.value.code == _lib.SP_E_INVALID_ARG
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_check_trace(desc, ptrace, rap=[5])
        assert e.value.code == _lib.SP_E_INVALID_ARG
    # without bvals and without a table read, _pub is _ext: aux program + periodic column + stride
    sb, srows = strided_airs.rap_with_stride(64)
    sdesc, skeep = sb.build()
    assert not air.needs_pub(sdesc) and sdesc.stride_desc.n == 2
    strace = strided_airs.to_bytes(srows)
    want = hip_ctx.air_prove(sdesc, strace, OPT)                  # sp_air_prove_ext
    sext = air.ext_of(sdesc)
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_ext", sdesc, strace, ctypes.byref(sext)) == want
    assert _prove(hip_lib, hip_ctx, "sp_air_prove_pub", sdesc, strace, ctypes.byref(sext), None) == want


# ---- 5. a sharded context ----------------------------------------------------------------------------------------------------------------
def _cases(n):
    return [X.table_lookup(n, 8, seed=71), X.public_permutation(n, 5, seed=72)]


def _body(rank, world, n):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    proofs = []
    for b, rows in _cases(n):
        desc, keep = b.build()
        proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*X.OPTIONS)))
    ctx.close()
    return proofs


def _single_body(n):
    proofs = []
    with api.Context(device=0) as ctx:
        for b, rows in _cases(n):
            desc, keep = b.build()
            proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*X.OPTIONS)))
            assert ctx.last_proof_info()["composition_path"] == 1
    return proofs


def test_sharded_context_gives_the_one_gpu_bytes():
    """Every rank builds the whole auxiliary column from its whole copy of the main trace and resolves the boundary values itself: both
    ranks return the one-GPU bytes of both worked examples.  The one-GPU child has ended before the ranks start."""
    world, n = 2, 64
    want = run_child(_single_body, (n,), timeout=600)
    for (b, rows), proof in zip(_cases(n), want):
        desc, keep = b.build()
        assert api.air_verify(proof, desc, OPT)
    got = run_ranks(world, _body, (n,), timeout=600)
    for r in range(world):
        assert got[r] == want, (r, "proof bytes differ")
