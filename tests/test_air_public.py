"""Public data inside a randomized argument (sp_air_prove_pub and its siblings), the parts that need no GPU: the ABI, the host resolver of
boundary values against Python integers, its refusals, the builder and its Python-integer models of both worked examples, and the CPU
verifier on two recorded proofs."""
import ctypes
import os
import random
import re

import pytest

import public_airs as X
from lambdaworks_cairo_prover_amd import _lib, air, api

P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_LOOKUP = os.path.join(ROOT, "tests", "golden", "public_lookup_n64.proof")
GOLDEN_PERMUTATION = os.path.join(ROOT, "tests", "golden", "public_permutation_n64.proof")
NEW_SYMBOLS = ("sp_air_prove_pub", "sp_air_verify_pub", "sp_air_check_trace_pub", "sp_air_boundary_desc_size", "sp_air_boundary_resolve")


def golden_lookup():
    """The AIR and trace of tests/golden/public_lookup_n64.proof: air.table_lookup on 64 rows, a table of 8 values, seed 64."""
    return X.table_lookup(64, 8, seed=64)


def golden_permutation():
    """The AIR and trace of tests/golden/public_permutation_n64.proof: air.public_permutation on 64 rows, 5 public values, seed 64."""
    return X.public_permutation(64, 5, seed=64)


def test_struct_mirrors_and_abi(hip_lib):
    hip_lib.sp_air_boundary_desc_size.restype = ctypes.c_uint64
    assert ctypes.sizeof(air.AirBoundaryValueC) == 16
    assert ctypes.sizeof(air.AirBoundaryDescC) == hip_lib.sp_air_boundary_desc_size() == 48
    assert ctypes.sizeof(air.AirExtC) == hip_lib.sp_air_ext_size() == 32        # sp_air_ext and sp_air_desc keep their layouts
    assert ctypes.sizeof(air.AirDescC) == hip_lib.sp_air_desc_size()
    assert hip_lib.sp_abi_version() == _lib.SP_ABI_VERSION == 7
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name) and name in rust, name


# ---- the resolver ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_resolver_equals_the_python_model(hip_lib, seed):
    rng = random.Random(seed)
    b = X.random_values_builder(seed)
    assert {d == air.AUX_NO_DEN for _, _, d in b.bvalues} == {True, False}        # an N / D entry and one without a denominator
    desc, keep = b.build_boundary_desc()
    for _ in range(4):
        rap = [rng.randrange(P) for _ in range(b.n_rap)]
        assert api.air_boundary_resolve(desc, rap) == b.resolve_boundary(rap)


def test_resolver_of_the_worked_example(hip_lib):
    public = X.keys(7, 5)
    b = air.public_permutation(16, public)
    desc, keep = b.build_boundary_desc()
    gamma = 123456789
    want = 1
    for v in public:
        want = want * (gamma - v) % P
    want = want * pow(pow(gamma, 5, P), P - 2, P) % P
    assert api.air_boundary_resolve(desc, [gamma]) == b.resolve_boundary([gamma]) == [want]


def test_zero_denominator(hip_lib):
    b, rows = X.boundary_over_difference(16, 77)
    desc, keep = b.build_boundary_desc()
    assert api.air_boundary_resolve(desc, [78]) == [1]
    with pytest.raises(api.SpError) as e:
        api.air_boundary_resolve(desc, [77])
    assert e.value.code == _lib.SP_E_ZERO_INVERSE
    with pytest.raises(ValueError, match="denominator is zero"):
        b.resolve_boundary([77])
    with pytest.raises(ValueError, match="denominator is zero"):
        b.check_trace(rows, [77])


def _resolve_code(hip_lib, desc, n_rap=1):
    out = ctypes.create_string_buffer(32 * 8)
    return hip_lib.sp_air_boundary_resolve(ctypes.byref(desc), b"\0" * 32 * n_rap, ctypes.c_uint32(n_rap), out)


def malformed_boundary_descs():
    """[(label, patch(desc))]: every malformed sp_air_boundary_desc that needs no AIR to be seen, on the descriptor of
    boundary_over_difference (ops: RAP 0, CONST, SUB; one value with N = D = op 2)."""
    def field(name, value):
        return lambda d: setattr(d, name, value)

    def op(i, **kw):
        def patch(d):
            for k, v in kw.items():
                setattr(d.ops[i], k, v)
        return patch

    def value(**kw):
        def patch(d):
            for k, v in kw.items():
                setattr(d.values[0], k, v)
        return patch
    return [("null ops", field("ops", None)), ("null consts", field("consts", None)), ("null values", field("values", None)),
            ("no ops", field("n_ops", 0)), ("LOAD", op(0, op=0)), ("OUT", op(2, op=5)), ("PERIODIC", op(0, op=6)), ("op 7", op(2, op=7)),
            ("operand is itself", op(2, a=2)), ("operand is later", op(2, b=3)), ("constant beyond consts + rap", op(1, a=2)),
            ("num_op beyond the program", value(num_op=3)), ("den_op beyond the program", value(den_op=3))]


def test_resolver_refuses_malformed_descriptors(hip_lib):
    b, rows = X.boundary_over_difference(16, 77)
    assert [o for o, _, _ in b.public.ops] == [air.OP_CONST, air.OP_CONST, air.OP_SUB]
    good, keep = b.build_boundary_desc()
    assert _resolve_code(hip_lib, good) == _lib.SP_OK
    for label, patch in malformed_boundary_descs():
        desc, keep = b.build_boundary_desc()
        patch(desc)
        assert _resolve_code(hip_lib, desc) == _lib.SP_E_INVALID_ARG, label
    twice, keep = air.boundary_desc(b.public.resolved_ops(), b.public.consts, [(3, 2, 2), (1, 0, air.AUX_NO_DEN), (3, 0, 2)])
    assert _resolve_code(hip_lib, twice) == _lib.SP_E_INVALID_ARG               # the same boundary named twice
    once, keep = air.boundary_desc(b.public.resolved_ops(), b.public.consts, [(3, 2, 2), (1, 0, air.AUX_NO_DEN)])
    assert _resolve_code(hip_lib, once) == _lib.SP_OK
    assert hip_lib.sp_air_boundary_resolve(None, b"\0" * 32, 1, ctypes.create_string_buffer(32)) == _lib.SP_E_INVALID_ARG


# ---- the builder and its models -----------------------------------------------------------------------------------------------------
def test_builder_refusals_and_descriptors(hip_lib):
    b = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM, periodic=[[1, 2]])
    for shift, k, match in ((8, 0, "row shift 8"), (-1, 0, "row shift -1"), (0, 1, "column 1 is not one of the AIR's 1 periodic"), (0, -1, "column -1")):
        with pytest.raises(ValueError, match=match):
            b.aux.table(shift, k)
    with pytest.raises(ValueError, match="cannot read periodic columns"):      # the old name keeps refusing
        b.aux.periodic(0, 0)
    none = air.AirBuilder(2, [0, 1], 1, aux_cols=1, n_rap=1, aux_kind=air.AUX_PROGRAM)
    with pytest.raises(ValueError, match="not one of the AIR's 0 periodic"):
        none.aux.table(0, 0)
    with pytest.raises(ValueError, match="RAP challenge 1 of 1"):
        none.public.rap(1)
    with pytest.raises(ValueError, match="values of b.public"):
        none.boundary_from(0, 0, none.rap(0))                                   # a value of the constraint program
    assert none.bcs == [] and none.bvalues == []
    # descriptors: what is attached, and where api routes
    look, rows = X.table_lookup(16, 4)
    desc, keep = look.build()
    assert not hasattr(desc, "boundary_desc") and air.needs_pub(desc)
    assert [desc.aux_desc.ops[i].op for i in range(desc.aux_desc.n_ops)].count(air.OP_PERIODIC) == 1
    perm, rows = X.public_permutation(16, 5)
    desc, keep = perm.build()
    assert air.needs_pub(desc) and desc.boundary_desc.n_values == 1 and desc.boundary_desc.values[0].boundary == 3
    assert bytes(desc.boundary[3].value) == b"\0" * 32 and (desc.boundary[3].col, desc.boundary[3].step) == (2, 15)
    for name in ("fibonacci_rap_program",):
        desc, keep = getattr(air, name)(16, 12).build()
        assert not air.needs_pub(desc)
    # the limits cover the new program
    big = air.AirBuilder(1, [0, 1], 1, n_rap=1)
    v = big.public.rap(0)
    for _ in range(api.air_limits()["ops"]):
        v = v + v
    big.constraint(big.load(1, 0) - big.load(0, 0), 1, 1)
    big.boundary_from(0, 0, v)
    with pytest.raises(ValueError, match="boundary values exceed the ops limit"):
        big.build()


def test_models_of_the_worked_examples(hip_lib):
    n, gamma = 16, 0x1234567
    look, rows = X.table_lookup(n, 4)                          # period 4 on 16 rows: (i + shift) mod period wraps more than once
    assert len(look.periodic_cols[0]) == 4 and (look.degrees, look.exemptions, look.degree_bound_factor) == ([3], [0], 2)
    assert look.check_trace(rows, [gamma]) == []
    found = look.check_trace(X.changed(rows, (5, 0)), [gamma])                  # one `a` cell: no longer a table entry
    assert [(v.kind, v.index) for v in found] == [(air.TRANSITION, 0)]
    perm, rows = X.public_permutation(n, 5)
    assert len(perm.bvalues) == 1 and perm.exemptions == [1]
    assert perm.check_trace(rows, [gamma]) == []
    public = X.keys(2 + 2000, 5)
    public[2] = (public[2] + 1) % P
    other, rows = X.public_permutation(n, 5, public=public)                     # one public value changed: the same trace
    found = other.check_trace(rows, [gamma])
    assert [(v.kind, v.index, v.first_row) for v in found] == [(air.BOUNDARY, 3, n - 1)]
    assert found[0].value == perm.resolve_boundary([gamma])[0] != other.resolve_boundary([gamma])[0]


@pytest.mark.parametrize("n,period,shift", [(16, 4, 7), (16, 16, 7), (16, 16, 0)])
def test_aux_model_reads_the_table(hip_lib, n, period, shift):
    table = X.keys(period, period)
    p = air.AuxProgram(1, 0, [table])
    p.running_sum(p.table(shift, 0) * p.load(0, 0))
    rows = [[i + 1] for i in range(n)]
    got = p.evaluate(rows, [])
    acc = 0
    for i in range(n):
        assert got[i, 0] == acc
        acc = (acc + table[(i + shift) % period] * (i + 1)) % P
    other = [list(reversed(table))]
    assert p.evaluate(rows, [], periodic=other)[1, 0] == other[0][shift % period]


# ---- the CPU verifier on recorded proofs -----------------------------------------------------------------------------------------
def _verify_pub(lib, proof, desc, bvals="own"):
    opt = api.ProofOptions(*X.OPTIONS).to_c()
    ext = air.ext_of(desc)
    bvals = getattr(desc, "boundary_desc", None) if bvals == "own" else bvals
    return lib.sp_air_verify_pub(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(ext), None if bvals is None else ctypes.byref(bvals),
                                 ctypes.byref(opt), 0)


def test_cpu_verifier_on_the_recorded_lookup(hip_lib):
    """tests/golden/public_lookup_n64.proof was written once by this library's device prover (sp_air_prove_pub): a regression pin of
    prover and verifier together.  The independent checks are in tests/test_gpu_air_public.py (the host model's and the oracle's bytes)."""
    proof = open(GOLDEN_LOOKUP, "rb").read()
    b, rows = golden_lookup()
    desc, keep = b.build()
    opt = api.ProofOptions(*X.OPTIONS)
    assert api.air_verify(proof, desc, opt) and _verify_pub(hip_lib, proof, desc) == 1
    desc.periodic_desc, other_keep = air.periodic_desc(periodic_changed(b))     # one table value changed
    assert not api.air_verify(proof, desc, opt)
    desc, keep = b.build()
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    assert not api.air_verify(bytes(bad), desc, opt)


def periodic_changed(b):
    cols = [list(v) for v in b.periodic_cols]
    cols[0][3] = (cols[0][3] + 1) % P
    return cols


def test_cpu_verifier_on_the_recorded_permutation(hip_lib):
    """tests/golden/public_permutation_n64.proof, written once by sp_air_prove_pub: z_(n-1) = prod (gamma - v_j) / gamma^5 is computed by
    the verifier from the challenge it replays."""
    proof = open(GOLDEN_PERMUTATION, "rb").read()
    b, rows = golden_permutation()
    desc, keep = b.build()
    opt = api.ProofOptions(*X.OPTIONS)
    assert api.air_verify(proof, desc, opt) and _verify_pub(hip_lib, proof, desc) == 1
    assert _verify_pub(hip_lib, proof, desc, bvals=None) == 0                   # bvals dropped: the placeholder 0 is not z_(n-1)
    public = X.keys(64 + 2000, 5)
    public[4] = (public[4] + 1) % P
    other, okeep = X.public_permutation(64, 5, seed=64, public=public)[0].build()   # one public value changed
    assert not api.air_verify(proof, other, opt)
    # malformed boundary values: 0, whatever the proof
    for label, patch in malformed_boundary_descs()[:3]:
        desc, keep = b.build()
        patch(desc.boundary_desc)
        assert _verify_pub(hip_lib, proof, desc) == 0, label
    desc, keep = b.build()
    desc.boundary_desc.values[0].boundary = 4                                    # boundary >= air->n_boundary
    assert _verify_pub(hip_lib, proof, desc) == 0
    desc, keep = b.build()
    assert _verify_pub(hip_lib, proof, desc) == 1


def test_lookup_proof_through_the_older_verifiers(hip_lib):
    """The verifier never runs the auxiliary program: the lookup's proof is also accepted by sp_air_verify_ext, and with bvals == NULL
    sp_air_verify_pub is that call."""
    proof = open(GOLDEN_LOOKUP, "rb").read()
    desc, keep = golden_lookup()[0].build()
    opt = api.ProofOptions(*X.OPTIONS).to_c()
    ext = air.ext_of(desc)
    assert hip_lib.sp_air_verify_ext(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(opt), 0) == 1
    assert _verify_pub(hip_lib, proof, desc, bvals=None) == 1
    assert hip_lib.sp_air_verify_pub(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(ext), None, ctypes.byref(opt), 7) == _lib.SP_E_INVALID_ARG
