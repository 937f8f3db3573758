"""One table of malformed statements of a program AIR against every entry point that can carry them, no GPU: the library judges a
statement - sp_air_desc and its optional parts - in one decoder, so sp_air_prove*, sp_air_check_trace* (on a block of zeroed memory
in place of a context: the statement is judged before the context is touched) and sp_air_verify* (on a recorded proof) must all
refuse the same things: SP_E_INVALID_ARG from the prover and the trace check, 0 from the verifier."""
import ctypes
import os

import numpy as np

import periodic_airs
import public_airs
from lambdaworks_cairo_prover_amd import _lib, air, api
from test_air_public import malformed_boundary_descs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROOF = os.path.join(ROOT, "tests", "golden", "periodic_mimc_n64.proof")       # any well-framed proof: its first eight bytes say n = 64


class Case:
    """A statement with one malformed part.  part: which one ("desc", "periodic", "strides", "aux", "bvals", "ext"); old_only: malformed
    only where the auxiliary program may not read periodic columns (every entry point but _pub); named: what sp_last_error must say."""
    def __init__(self, part, label, desc, aux=None, per=None, strides=None, bvals=None, ext_size=None, old_only=False, named=None, keep=None):
        self.part, self.label, self.desc, self.old_only, self.named, self.keep = part, label, desc, old_only, named, keep
        self.parts = {"aux": aux, "periodic": per, "strides": strides, "bvals": bvals}
        self.ext_size = ext_size

    def ext(self):
        x = air.AirExtC()
        x.size = ctypes.sizeof(air.AirExtC) if self.ext_size is None else self.ext_size
        for field in ("aux", "periodic", "strides"):
            if self.parts[field] is not None:
                setattr(x, field, ctypes.pointer(self.parts[field]))
        return x

    def ref(self, part):
        return None if self.parts[part] is None else ctypes.byref(self.parts[part])


def cases(n):
    """The table, for a trace of n rows."""
    keys = periodic_airs.keys(1, 8)
    out = []

    def mimc():
        desc, keep = air.mimc_chain(n, 8, 3, keys).build()
        return desc, keep

    def lookup():
        desc, keep = public_airs.table_lookup(n, 4)[0].build()
        return desc, keep

    # ---- a malformed sp_air_desc, on an AIR with periodic columns and on one with an auxiliary program too
    for base in (mimc, lookup):
        desc, keep = base()
        desc.n_offsets = 9
        out.append(Case("desc", f"n_offsets = 9 ({base.__name__})", desc, aux=getattr(desc, "aux_desc", None), per=desc.periodic_desc, named=b"descriptor", keep=keep))
    # ---- periodic columns
    for label, columns in (("no power of two", [keys[:6]]), ("longer than the trace", [periodic_airs.keys(1, 2 * n)]), ("65 columns", [[1]] * 65)):
        desc, keep = mimc()
        per, pkeep = air.periodic_desc(columns)
        out.append(Case("periodic", label, desc, per=per, named=b"periodic columns" if label == "no power of two" else None, keep=(keep, pkeep)))
    for label, patch in (("null values", lambda p: setattr(p.cols[0], "values", None)), ("period 2^31", lambda p: setattr(p.cols[0], "period", 1 << 31))):
        desc, keep = mimc()
        per, pkeep = air.periodic_desc([keys])
        patch(per)
        out.append(Case("periodic", label, desc, per=per, keep=(keep, pkeep)))
    # ---- strides
    for label, strides in (("not one per transition", [(1, 0), (1, 0)]), ("offset >= period", [(2, 2)])):
        desc, keep = mimc()
        sd, skeep = air.stride_desc(strides)
        out.append(Case("strides", label, desc, per=desc.periodic_desc, strides=sd, named=b"strides" if label == "offset >= period" else None, keep=(keep, skeep)))
    # ---- the auxiliary program
    desc, keep = lookup()
    assert air.OP_PERIODIC in [desc.aux_desc.ops[i].op for i in range(desc.aux_desc.n_ops)]
    out.append(Case("aux", "op 6 outside _pub", desc, aux=desc.aux_desc, per=desc.periodic_desc, old_only=True, named=b"auxiliary program", keep=keep))
    desc, keep = lookup()
    desc.aux_desc.n_cols = desc.aux_cols + 1
    out.append(Case("aux", "n_cols != aux_cols", desc, aux=desc.aux_desc, per=desc.periodic_desc, named=b"auxiliary program", keep=keep))
    # ---- boundary values
    for label, patch in malformed_boundary_descs():
        desc, keep = public_airs.boundary_over_difference(n, 77)[0].build()
        patch(desc.boundary_desc)
        out.append(Case("bvals", label, desc, aux=desc.aux_desc, bvals=desc.boundary_desc, named=b"boundary values" if label == "LOAD" else None, keep=keep))
    # ---- sp_air_ext.size
    desc, keep = mimc()
    out.append(Case("ext", "size 24", desc, per=desc.periodic_desc, ext_size=24, named=b"sp_air_ext", keep=keep))
    return out


# (name, the parts it has a place for, the parts it insists on, whether it is a _pub entry point, its arguments between air and the rest)
def _single(*parts):
    return lambda case: tuple(case.ref(p) for p in parts)


def _ext(case):
    case._ext = case.ext()
    return (ctypes.byref(case._ext),)


def _pub(case):
    return _ext(case) + (case.ref("bvals"),)


PROVE = [("sp_air_prove", set(), set(), False, _single()), ("sp_air_prove_aux", {"aux"}, {"aux"}, False, _single("aux")),
         ("sp_air_prove_periodic", {"aux", "periodic"}, {"periodic"}, False, _single("aux", "periodic")),
         ("sp_air_prove_ext", {"aux", "periodic", "strides", "ext"}, set(), False, _ext),
         ("sp_air_prove_pub", {"aux", "periodic", "strides", "ext", "bvals"}, set(), True, _pub)]
CHECK = [("sp_air_check_trace", {"aux", "periodic"}, set(), False, _single("aux", "periodic")),
         ("sp_air_check_trace_ext", {"aux", "periodic", "strides", "ext"}, set(), False, _ext),
         ("sp_air_check_trace_pub", {"aux", "periodic", "strides", "ext", "bvals"}, set(), True, _pub)]
# (the verifier does not look at the auxiliary program: no entry point of it carries a malformed one)
VERIFY = [("sp_air_verify", set(), set(), False, _single()), ("sp_air_verify_backend", set(), set(), False, _single()),
          ("sp_air_verify_periodic", {"periodic"}, {"periodic"}, False, _single("periodic")),
          ("sp_air_verify_ext", {"periodic", "strides", "ext"}, set(), False, _ext), ("sp_air_verify_pub", {"periodic", "strides", "ext", "bvals"}, set(), True, _pub)]


def carriers(case, entries):
    for name, places, insists, pub, args in entries:
        if (case.part == "desc" or case.part in places) and all(case.parts[p] is not None for p in insists) and not (case.old_only and pub):
            yield name, args


def test_the_table_reaches_every_entry_point():
    for entries in (PROVE, CHECK, VERIFY):
        assert {name for case in cases(16) for name, _ in carriers(case, entries)} == {e[0] for e in entries}
    assert {c.part for c in cases(16) if c.named} == {"desc", "periodic", "strides", "aux", "bvals", "ext"}


def test_prover_and_trace_check_refuse_malformed_statements(hip_lib):
    n = 16
    ctx = ctypes.create_string_buffer(1 << 16)                  # zeroed memory in place of a context: a refusal never reads it
    opt = api.ProofOptions.default_test_options().to_c()
    out, ln, total = ctypes.POINTER(ctypes.c_uint8)(), ctypes.c_uint64(), ctypes.c_uint32(0)
    for case in cases(n):
        trace = np.zeros((n, case.desc.main_cols, 32), dtype=np.uint8)
        tp = trace.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
        for name, args in carriers(case, PROVE):
            rc = getattr(hip_lib, name)(ctx, ctypes.byref(case.desc), *args(case), tp, ctypes.c_uint64(n), ctypes.byref(opt), ctypes.byref(out), ctypes.byref(ln))
            assert rc == _lib.SP_E_INVALID_ARG, (name, case.part, case.label)
            assert case.named is None or (case.named in hip_lib.sp_last_error() and b"sp_air_" in hip_lib.sp_last_error()), (name, case.label, hip_lib.sp_last_error())
        for name, args in carriers(case, CHECK):
            rc = getattr(hip_lib, name)(ctx, ctypes.byref(case.desc), *args(case), tp, ctypes.c_uint64(n), ctypes.byref(opt), None, None, ctypes.c_uint32(0),
                                        ctypes.byref(total))
            assert rc == _lib.SP_E_INVALID_ARG, (name, case.part, case.label)
            assert case.named is None or case.named in hip_lib.sp_last_error(), (name, case.label, hip_lib.sp_last_error())
    assert not out and bytes(ctx.raw) == bytes(len(ctx.raw))   # no proof came back, and the zeroed block was never written


def test_verifiers_refuse_malformed_statements(hip_lib):
    proof = open(PROOF, "rb").read()
    n = int.from_bytes(proof[:8], "big")
    assert n == 64
    opt = api.ProofOptions(4, 3, 3, 1).to_c()
    for case in cases(n):
        for name, args in carriers(case, VERIFY):
            tail = (ctypes.byref(opt),) if name == "sp_air_verify" else (ctypes.byref(opt), 0)
            rc = getattr(hip_lib, name)(proof, ctypes.c_uint64(len(proof)), ctypes.byref(case.desc), *args(case), *tail)
            assert rc == 0, (name, case.part, case.label)
            err = hip_lib.sp_last_error()
            assert err.startswith(b"malformed"), (name, case.label, err)     # refused as a statement, not as a proof that fails a step
            assert case.named is None or case.named in err, (name, case.label, err)


def test_well_formed_statements_pass_the_decoder(hip_lib):
    """The same entry points on the table's well-formed bases: the verifiers get past the statement (the recorded proof is the mimc
    chain's own, and no other statement's)."""
    proof = open(PROOF, "rb").read()
    opt = api.ProofOptions(4, 3, 3, 1)
    desc, keep = air.mimc_chain(64, 8, 3, [pow(3, 100 + j, api.P) for j in range(8)]).build()   # (tests/test_air_periodic.py golden_air)
    assert api.air_verify(proof, desc, opt)
    for b in (public_airs.table_lookup(64, 4)[0], public_airs.boundary_over_difference(64, 77)[0]):
        desc, keep = b.build()
        assert not api.air_verify(proof, desc, opt)
        assert hip_lib.sp_last_error().startswith(b"rejected")
