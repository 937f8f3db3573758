"""What the device tests of main-trace programs share (test_gpu_air_*.py): the conversions between rows of integers and the library's
bytes, the proof of a whole table through the entry points without a main program, the device's table of a builder against the plain
reference (program_ref), the three calls that build a main segment, and the two checks every feature repeats on its own worked example -
inputs in device memory, and two ranks."""
import ctypes

import numpy as np

import program_ref
from lambdaworks_cairo_prover_amd import _lib, air, api
from rank_procs import run_ranks

OPTIONS = [(4, 3, 3, 1), (2, 4, 7, 0)]
# A lookup argument's constraint has degree 3 under degree_bound_factor 2: the composition has 2n coefficients, which needs a blowup
# above 2 (test_gpu_air_chain.MIMC_OPTIONS) - the option set with blowup 2 runs with blowup 4 there.
LK_OPTIONS = [o if o[0] > 2 else (4,) + tuple(o[1:]) for o in OPTIONS]


def to_bytes(rows):
    return air.ints_to_bytes(np.array(rows, dtype=object))


def table_ints(table):
    return [[int(x) for x in row] for row in air.trace_to_ints(table)]


def model_ints(builder, rows):
    return [[int(x) for x in row] for row in builder.main.evaluate(rows)]


def prove_full(ctx, desc, full, options, entry):
    """The proof of the whole table through sp_air_prove_pub or sp_air_prove_ext: the descriptor's parts, no main program."""
    lib = _lib.load()
    ext = air.ext_of(desc)
    opt = api.ProofOptions(*options).to_c()
    out, ln = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64()
    a = np.ascontiguousarray(full, dtype=np.uint8)
    assert a.shape[1] == desc.main_cols
    ptr = a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    if entry == "pub":
        bv = getattr(desc, "boundary_desc", None)
        rc = lib.sp_air_prove_pub(ctx._h, ctypes.byref(desc), ctypes.byref(ext), None if bv is None else ctypes.byref(bv), ptr, ctypes.c_uint64(a.shape[0]),
                                  ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    else:
        rc = lib.sp_air_prove_ext(ctx._h, ctypes.byref(desc), ctypes.byref(ext), ptr, ctypes.c_uint64(a.shape[0]), ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
    _lib.check(rc)
    return ctx._take_proof(out, ln)


def device_table(ctx, b, rows, suffix=None):
    """The main segment the device builds from `rows`, as integers; suffix: the entry points the descriptor must route to."""
    desc, keep = b.build()
    assert suffix is None or air.main_suffix(desc) == suffix
    got = ctx.air_main_trace(desc, to_bytes(rows))
    assert got.shape == (len(rows), b.main_cols, 32)
    return table_ints(got)


def same_table(ctx, b, rows, suffix=None, model=False):
    """The device's table equals the plain reference's cell for cell (and, with `model`, so does the Python model's); returns it."""
    got, want = device_table(ctx, b, rows, suffix), program_ref.main_table(b.main, rows)
    for i in range(len(rows)):
        assert got[i] == want[i], i
    assert not model or want == model_ints(b, rows)
    return want


def three_calls(ctx, desc, rows, options):
    """The three calls that build the main segment from input rows."""
    data = to_bytes(rows)
    return (lambda: ctx.air_prove(desc, data, options), lambda: ctx.air_main_trace(desc, data), lambda: ctx.air_check_trace(desc, data, options))


def device_inputs_give_the_same_bytes(ctx, b, rows, options, name=""):
    """Inputs in device memory give the proof and the table of the same inputs in host memory, and the descriptor goes back to host
    inputs afterwards.  name: what a failure says of the case."""
    import torch
    desc, keep = b.build()
    host = to_bytes(rows)
    want = ctx.air_prove(desc, host, options)
    assert api.air_verify(want, desc, options), name
    dev = torch.from_numpy(host).to("cuda:0")
    assert dev.dtype == torch.uint8
    assert ctx.air_prove(desc, dev, options) == want, name
    assert desc.main_desc.input_location == air.INPUTS_DEVICE, name
    assert np.array_equal(ctx.air_main_trace(desc, dev), ctx.air_main_trace(desc, host)), name
    assert ctx.air_prove(desc, host, options) == want and desc.main_desc.input_location == air.INPUTS_HOST, name


def _rank_proof(rank, world, case, args, options):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    b, rows = case(*args)[:2]
    desc, keep = b.build()
    proof = ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    ctx.close()
    return proof


def two_ranks_give_the_one_rank_bytes(ctx, case, args, options):
    """case(*args)[:2] = (builder, input rows), a module-level function: every rank ingests the inputs and builds every derived column
    itself, and the proof of two ranks has the bytes of the proof of one."""
    b, rows = case(*args)[:2]
    desc, keep = b.build()
    want = ctx.air_prove(desc, to_bytes(rows), api.ProofOptions(*options))
    assert api.air_verify(want, desc, api.ProofOptions(*options))
    got = run_ranks(2, _rank_proof, (case, args, options), timeout=600)
    for r in range(2):
        assert got[r] == want, (r, got[r][:400])
