"""The entry points of a program AIR share one body: the worked examples that the older entry points accept, each through its own entry
point (sp_air_prove, _aux, _periodic, _ext - where api routes it) and through sp_air_prove_pub with bvals == NULL, must give the same
bytes - the recorded proof's where one exists -, and sp_air_check_trace_pub the records of the older trace check."""
import ctypes
import os

import pytest

import aux_program_airs
import check_trace_airs
import strided_airs
from lambdaworks_cairo_prover_amd import air, api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64
OPT = api.ProofOptions.default_test_options()                  # blowup 4


def fibonacci():
    return air.fibonacci_2_columns(), check_trace_airs.fibonacci_2_columns_rows(N), None


def aux_program():
    return aux_program_airs.permutation_air(N), aux_program_airs.main_rows(N), None


def mimc_periodic():
    keys = [pow(3, 100 + j, api.P) for j in range(8)]          # (tests/test_air_periodic.py golden_air)
    return air.mimc_chain(N, 8, 3, keys), air.mimc_chain_trace(N, 3, keys), "periodic_mimc_n64.proof"


def mimc_strided():
    c = strided_airs.golden_case()
    return c.builder, c.rows, "strided_n64.proof"


def _pub_args(desc):
    ext = air.ext_of(desc)
    return ext, (ctypes.byref(ext), None)


def _prove_pub(lib, ctx, desc, trace):
    out, ln, opt = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(), OPT.to_c()
    ext, args = _pub_args(desc)
    api.check(lib.sp_air_prove_pub(ctx._h, ctypes.byref(desc), *args, trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(N), ctypes.byref(opt),
                                   ctypes.byref(out), ctypes.byref(ln)))
    proof = ctypes.string_at(out, ln.value)
    lib.sp_free(out)
    return proof


def _check_pub(lib, ctx, desc, trace, cap=8):
    out, total, opt = (air.AirViolationC * cap)(), ctypes.c_uint32(0), OPT.to_c()
    ext, args = _pub_args(desc)
    api.check(lib.sp_air_check_trace_pub(ctx._h, ctypes.byref(desc), *args, trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.c_uint64(N),
                                         ctypes.byref(opt), None, out, ctypes.c_uint32(cap), ctypes.byref(total)))
    return [air.Violation(int(v.kind), int(v.index), int(v.rows), int(v.first_row), int(v.last_row), int.from_bytes(bytes(v.value), "big"))
            for v in out[:min(cap, total.value)]]


@pytest.mark.parametrize("example,prove_name,check_name", [(fibonacci, "sp_air_prove", "sp_air_check_trace"), (aux_program, "sp_air_prove_aux", "sp_air_check_trace"),
                                                          (mimc_periodic, "sp_air_prove_periodic", "sp_air_check_trace"),
                                                          (mimc_strided, "sp_air_prove_ext", "sp_air_check_trace_ext")])
def test_own_entry_point_and_pub_give_the_same_bytes_and_records(hip_lib, hip_ctx, example, prove_name, check_name):
    b, rows, golden = example()
    desc, keep = b.build()
    assert air.route(desc, "prove")[0] == prove_name and air.route(desc, "check_trace")[0] == check_name
    trace = air.ints_to_bytes(rows)
    own = hip_ctx.air_prove(desc, trace, OPT)
    assert _prove_pub(hip_lib, hip_ctx, desc, trace) == own
    if golden:
        assert own == open(os.path.join(ROOT, "tests", "golden", golden), "rb").read()
    assert api.air_verify(own, desc, OPT)
    assert hip_ctx.air_check_trace(desc, trace, OPT) == _check_pub(hip_lib, hip_ctx, desc, trace) == []
    bad = [list(r) for r in rows]
    bad[5][0] = (bad[5][0] + 1) % api.P                         # one cell: read by the rows around it (the strided example: by row 4)
    bad_trace = air.ints_to_bytes(bad)
    found = hip_ctx.air_check_trace(desc, bad_trace, OPT)
    assert found and found == _check_pub(hip_lib, hip_ctx, desc, bad_trace)
