"""Strided transition constraints of program AIRs, the parts that need no GPU: the ABI, the verifier's zerofier and exemption product
against Python integers, the builder and its Python-integer trace model, the refusals of builder and verifier, and the CPU verifier on a
recorded proof."""
import ctypes
import os
import random
import re

import pytest

import check_trace_airs as E
import strided_airs as X
from lambdaworks_cairo_prover_amd import _lib, air, api

P = api.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "strided_n64.proof")
GOLDEN_OPTIONS = (4, 3, 3, 1)
NEW_SYMBOLS = ("sp_air_prove_ext", "sp_air_verify_ext", "sp_air_check_trace_ext", "sp_air_stride_size", "sp_air_stride_desc_size",
               "sp_air_ext_size", "sp_air_stride_limits", "sp_air_stride_eval", "sp_air_stride_table")


def test_struct_mirrors_and_abi(hip_lib):
    assert ctypes.sizeof(air.AirStrideC) == hip_lib.sp_air_stride_size() == 8
    assert ctypes.sizeof(air.AirStrideDescC) == hip_lib.sp_air_stride_desc_size() == 16
    assert ctypes.sizeof(air.AirExtC) == hip_lib.sp_air_ext_size() == 32
    assert ctypes.sizeof(air.AirDescC) == hip_lib.sp_air_desc_size()            # sp_air_desc keeps its layout
    assert hip_lib.sp_abi_version() == _lib.SP_ABI_VERSION == 7
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = integ.index("```rust")
    rust = set(re.findall(r"pub fn (sp_[a-z0-9_]+)\s*\(", integ[start:integ.index("```\n", start + 10)]))
    for name in NEW_SYMBOLS:
        assert name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name) and name in rust, name
    assert api.air_stride_limits() == {"stride_classes": 4, "stride_exemption_products": 4}


@pytest.mark.parametrize("n", [16, 256])
def test_stride_eval_against_python_integers(hip_lib, n):
    rng = random.Random(n)
    g = X.root(n.bit_length() - 1)
    for period in (1, 2, 8, n):
        m = n // period
        for offset in sorted({0, period // 2, period - 1}):
            progression = list(range(offset, n, period))
            for e in sorted({0, min(1, m), m - 1} - {-1}):
                points = [rng.randrange(P), rng.randrange(P)]
                for x in points:
                    assert api.air_stride_eval(period, offset, e, n, x) == (X.zerofier(period, offset, n, x), X.exemption_product(period, offset, e, n, x))
                # on the trace domain: Z vanishes exactly on the progression, E exactly on its last e rows
                rows = range(n) if n == 16 else sorted(set(progression[:3] + progression[-3:] + [rng.randrange(n) for _ in range(8)]))
                for i in rows:
                    z, ex = api.air_stride_eval(period, offset, e, n, pow(g, i, P))
                    assert (z == 0) == (i in progression), (period, offset, i)
                    assert (ex == 0) == (e > 0 and i in progression[len(progression) - e:]), (period, offset, e, i)


def test_stride_eval_refuses_bad_shapes(hip_lib):
    for period, offset, e, n in ((3, 0, 0, 16), (0, 0, 0, 16), (32, 0, 0, 16), (4, 4, 0, 16), (4, 0, 5, 16), (4, 0, 0, 24)):
        with pytest.raises(api.SpError) as err:
            api.air_stride_eval(period, offset, e, n, 5)
        assert err.value.code == _lib.SP_E_INVALID_ARG


def test_builder_refusals_and_descriptors(hip_lib):
    b = air.AirBuilder(1, [0, 1], 1)
    v = b.load(1, 0) - b.load(0, 0)
    for period, offset, match in ((3, 0, "not a power of two"), (0, 0, "not a power of two"), (4, 4, "offset 4"), (4, -1, "offset -1")):
        with pytest.raises(ValueError, match=match):
            b.constraint(v, 1, 0, period=period, offset=offset)
    assert b.degrees == [] and b.strides == []
    # more classes, and more exemption products, than sp_air_stride_limits
    many = air.AirBuilder(1, [0, 1], 1)
    for o in range(5):
        many.constraint(many.load(1, 0) - many.load(0, 0), 1, 0, period=8, offset=o)
    with pytest.raises(ValueError, match="stride_classes limit.*5 > 4"):
        many.build()
    cube = air.AirBuilder(1, [0, 1], 2)                                          # degree f + 1 on a stride: the quotient does not fit
    x = cube.load(0, 0)
    cube.constraint(cube.load(1, 0) - x * x * x, 3, 1, period=4, offset=0)
    with pytest.raises(ValueError, match="degree 3 on a stride needs degree_bound_factor >= 3"):
        cube.build()
    kinds = air.AirBuilder(1, [0, 1], 1)
    for e in range(1, 6):
        kinds.constraint(kinds.load(1, 0) - kinds.load(0, 0), 1, e, period=2, offset=0)
    with pytest.raises(ValueError, match="stride_exemption_products limit.*5 > 4"):
        kinds.build()
    # builders that never pass `period` produce the descriptors they always produced
    for name in E.EXAMPLES:
        desc, keep = E.EXAMPLES[name](16)[0].build()
        assert not hasattr(desc, "stride_desc"), name
    plain = air.AirBuilder(1, [0, 1], 1)
    plain.constraint(plain.load(1, 0) - plain.load(0, 0), 1, 1, period=1, offset=0)
    assert not hasattr(plain.build()[0], "stride_desc")
    c = X.two_class(16)
    desc, keep = c.builder.build()
    assert desc.stride_desc.n == 3
    assert [(desc.stride_desc.strides[k].period, desc.stride_desc.strides[k].offset) for k in range(3)] == [(1, 0), (4, 1), (16, 15)]
    ext = air.ext_of(desc)
    assert ext.size == 32 and not ext.aux and not ext.periodic and ext.strides.contents.n == 3
    # the num_transition_exemptions == 1 rule stays with the (1, 0) constraints
    r = air.AirBuilder(1, [0, 1], 1)
    for e, period in ((2, 1), (3, 4), (5, 1), (0, 1)):
        r.constraint(r.load(1, 0) - r.load(0, 0), 1, e, period=period)
    assert r.enforced_exemptions() == [2, 3, 2, 0]
    assert r.enforced_rows(1, 32) == [0, 4, 8, 12, 16] and r.enforced_rows(2, 8) == [0, 1, 2, 3, 4, 5]


@pytest.mark.parametrize("n", [16, 64])
@pytest.mark.parametrize("name", ["mimc", "two_class"])
def test_check_trace_model_follows_the_enforced_rows(hip_lib, name, n):
    c = {"mimc": X.mimc, "two_class": X.two_class}[name](n)
    b = c.builder
    assert b.check_trace(c.rows) == []
    assert b.check_trace(X.changed(c.rows, c.free_cell)) == []                 # wrong on non-enforced rows only
    assert b.check_trace(X.changed(c.rows, c.tail_cell)) == []                 # wrong on the exempted tail row of the progression
    found = b.check_trace(X.changed(c.rows, c.enforced_cell))                  # wrong on one enforced row
    assert len(found) == 1
    v = found[0]
    assert (v.kind, v.rows, v.first_row, v.last_row) == (air.TRANSITION, 1, c.enforced_row, c.enforced_row) and v.value != 0
    assert b.strides[v.index][0] > 1
    # the same trace under the every-row reading of the constraints breaks them on the free rows
    every = air.AirBuilder(b.main_cols, b.offsets, b.degree_bound_factor, periodic=b.periodic_cols)
    every.ops, every.consts, every.degrees, every.exemptions, every.bcs = b.ops, b.consts, b.degrees, b.exemptions, b.bcs
    assert any(v.rows > 1 for v in every.check_trace(c.rows))


def test_worked_example_states_one_thing_twice(hip_lib):
    n = 64
    c = X.mimc(n)
    sel, rows = X.mimc_selector(n)
    assert (c.builder.degrees, c.builder.degree_bound_factor, c.builder.strides) == ([2], 2, [(4, 0)])
    assert (sel.degrees, sel.degree_bound_factor, sel.strides) == ([3], 2, [(1, 0)])
    for cell in (c.enforced_cell, c.free_cell, c.tail_cell, None):
        t = rows if cell is None else X.changed(rows, cell)
        assert [(v.rows, v.first_row) for v in c.builder.check_trace(t)] == [(v.rows, v.first_row) for v in sel.check_trace(t)]


def _verify_ext(lib, proof, desc, options=GOLDEN_OPTIONS, backend=0):
    opt = api.ProofOptions(*options).to_c()
    ext = air.ext_of(desc)
    return lib.sp_air_verify_ext(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(opt), backend)


def test_cpu_verifier_on_the_recorded_proof(hip_lib):
    """tests/golden/strided_n64.proof was written once by this library's own device prover: the worked example
    (air.strided_mimc_chain; strided_airs.golden_case) at n = 64, stride (4, 0), options (4, 3, 3, 1).  A regression pin of prover and
    verifier together, NOT an oracle: the independent checks are test_stride_eval_against_python_integers (the verifier's Z and E) and
    tests/test_gpu_air_stride.py (the oracle's bytes for degenerate strides, the table, completeness, soundness)."""
    proof = open(GOLDEN, "rb").read()
    c = X.golden_case()
    desc, keep = c.builder.build()
    opt = api.ProofOptions(*GOLDEN_OPTIONS)
    assert api.air_verify(proof, desc, opt)
    assert _verify_ext(hip_lib, proof, desc) == 1
    for strides in ([(2, 0)], [(4, 1)], [(8, 0)], [(1, 0)]):                   # another period, another offset, no stride
        skeep = X.with_strides(desc, strides)
        assert not api.air_verify(proof, desc, opt), strides
    X.with_strides(desc, None)                                                  # strides omitted: sp_air_verify_periodic
    assert not api.air_verify(proof, desc, opt)
    for e in (0, 2):                                                            # e changed
        desc, keep = c.builder.build()
        desc.exemptions[0] = e
        assert not api.air_verify(proof, desc, opt), e
    desc, keep = c.builder.build()
    assert not api.air_verify(proof, desc, opt, api.SP_MERKLE_POSEIDON)
    rng = random.Random(64)
    for at in rng.sample(range(len(proof)), 64):
        bad = bytearray(proof)
        bad[at] ^= 1 << rng.randrange(8)
        assert not api.air_verify(bytes(bad), desc, opt), at
    assert api.air_verify(proof, desc, opt)


def test_verifier_refuses_malformed_stride_descriptors(hip_lib):
    proof = open(GOLDEN, "rb").read()
    c = X.golden_case()
    opt = api.ProofOptions(*GOLDEN_OPTIONS)
    for label, strides in X.malformed_stride_descs(c.builder, 64):
        desc, keep = c.builder.build()
        skeep = X.with_strides(desc, strides)
        assert _verify_ext(hip_lib, proof, desc) == 0, label
    desc, keep = c.builder.build()
    desc.exemptions[0] = 16                                                      # e >= n / s
    assert _verify_ext(hip_lib, proof, desc) == 0
    desc, keep = c.builder.build()
    desc.degrees[0] = 3                                                          # degree f + 1 on a stride
    assert _verify_ext(hip_lib, proof, desc) == 0
    desc, keep = c.builder.build()
    desc.stride_desc.strides = None
    assert _verify_ext(hip_lib, proof, desc) == 0
    desc, keep = c.builder.build()
    ext = air.ext_of(desc)
    ext.size = 24
    o = opt.to_c()
    assert hip_lib.sp_air_verify_ext(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(ext), ctypes.byref(o), 0) == 0
    assert hip_lib.sp_air_verify_ext(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(air.ext_of(desc)), ctypes.byref(o), 7) == _lib.SP_E_INVALID_ARG
    assert _verify_ext(hip_lib, proof, desc) == 1


@pytest.mark.parametrize("name", ["simple_fibonacci", "fibonacci_rap"])
def test_degenerate_strides_verify_the_oracles_proofs(oracle, hip_lib, name):
    """Every stride (1, 0) through sp_air_verify_ext is sp_air_verify: the oracle's proofs of two example AIRs are accepted, a flipped
    byte and a real stride are not."""
    n, options = 16, (4, 3, 3, 1)
    steps = n - 4 if name == "fibonacci_rap" else 0
    trace = oracle.example_trace(name, steps or n)
    proof = oracle.example_prove(name, trace, options, (1, 1), steps)
    b = air.fibonacci_rap(trace.shape[0], steps) if name == "fibonacci_rap" else air.simple_fibonacci(1, 1)
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    assert api.air_verify(proof, desc, opt)
    skeep = X.degenerate(desc)
    assert _verify_ext(hip_lib, proof, desc, options) == 1
    assert hip_lib.sp_air_verify_ext(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), None, ctypes.byref(opt.to_c()), 0) == 1   # no extensions at all
    bad = bytearray(proof)
    bad[len(bad) // 2] ^= 1
    assert _verify_ext(hip_lib, bytes(bad), desc, options) == 0
    skeep = X.with_strides(desc, [(2, 0)] + [(1, 0)] * (desc.n_transitions - 1))
    assert _verify_ext(hip_lib, proof, desc, options) == 0
