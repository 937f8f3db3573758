"""Periodic columns of program AIRs, the parts that need no GPU: the ABI, the host evaluation of a periodic column's polynomial against
a Lagrange interpolation in Python integers, the refusals of the builder and of the verifiers, and the CPU verifier on a recorded proof."""
import ctypes
import os
import random

import pytest

from lambdaworks_cairo_prover_amd import _lib, air, api

P = api.P
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "periodic_mimc_n64.proof")
GOLDEN_OPTIONS = (4, 3, 3, 1)


def golden_air():
    """The AIR of tests/golden/periodic_mimc_n64.proof: mimc_chain on 64 rows, period 8, x0 = 3, keys 3^(100 + j)."""
    keys = [pow(3, 100 + j, P) for j in range(8)]
    return air.mimc_chain(64, 8, 3, keys), keys


def test_struct_mirrors_and_abi(hip_lib):
    assert ctypes.sizeof(air.AirPeriodicDescC) == hip_lib.sp_air_periodic_desc_size() == 16
    assert ctypes.sizeof(air.AirPeriodicColumnC) == 16
    assert ctypes.sizeof(air.AirDescC) == hip_lib.sp_air_desc_size()            # sp_air_desc keeps its layout
    assert hip_lib.sp_abi_version() == _lib.SP_ABI_VERSION == 7
    for name in ("sp_air_prove_periodic", "sp_air_verify_periodic", "sp_air_periodic_desc_size", "sp_air_periodic_limits",
                 "sp_air_periodic_eval", "sp_air_periodic_lde"):
        assert name in _lib.NEWEST_SYMBOLS and hasattr(hip_lib, name), name
    assert api.air_periodic_limits() == {"periodic_columns": 64}
    assert air.OP_PERIODIC == 6


def lagrange_eval(values, w_p, y):
    """q(y) for the q of degree < p with q(w_p^j) = values[j], by the Lagrange formula in Python integers."""
    p = len(values)
    nodes = [pow(w_p, j, P) for j in range(p)]
    total = 0
    for j in range(p):
        num = den = 1
        for m in range(p):
            if m != j:
                num = num * (y - nodes[m]) % P
                den = den * (nodes[j] - nodes[m]) % P
        total = (total + values[j] * num * pow(den, P - 2, P)) % P
    return total


@pytest.mark.parametrize("n", [16, 64])
def test_periodic_eval_against_lagrange(oracle, n):
    rng = random.Random(n)
    g = oracle.primitive_root(n.bit_length() - 1)
    for period in (1, 2, 8, n):
        values = [rng.randrange(P) for _ in range(period)]
        w_p = pow(g, n // period, P)
        for i in range(n):                                             # P(g^i) = v[i mod p] on the whole trace domain
            assert api.air_periodic_eval(values, n, pow(g, i, P)) == values[i % period], (period, i)
        z = rng.randrange(P)
        points = [rng.randrange(P) for _ in range(20)] + [z * pow(g, k, P) % P for k in (0, 1, 2, 5)] + [0, 1, P - 1]
        for x in points:
            assert api.air_periodic_eval(values, n, x) == lagrange_eval(values, w_p, pow(x, n // period, P)), (period, x)


def test_periodic_eval_refuses_bad_shapes(hip_lib):
    for values, n in (([1, 2, 3], 16), ([1] * 32, 16), ([1, 2], 24)):
        with pytest.raises(api.SpError) as e:
            api.air_periodic_eval(values, n, 5)
        assert e.value.code == _lib.SP_E_INVALID_ARG


def test_builder_refusals(hip_lib):
    with pytest.raises(ValueError, match="not a power of two"):
        air.AirBuilder(1, [0, 1], 2, periodic=[[1, 2, 3]])
    with pytest.raises(ValueError, match="not a power of two"):
        air.AirBuilder(1, [0, 1], 2, periodic=[[]])
    with pytest.raises(ValueError, match="at most n"):
        air.mimc_chain(16, 32, 3, list(range(32)))
    b = air.AirBuilder(1, [0, 1], 2, periodic=[[1, 2]])
    with pytest.raises(ValueError, match="column 1"):
        b.periodic(0, 1)
    with pytest.raises(ValueError, match="frame row"):
        b.periodic(2, 0)
    many = air.AirBuilder(1, [0, 1], 2, periodic=[[k] for k in range(65)])
    many.constraint(many.load(1, 0) - many.load(0, 0) - many.periodic(0, 64), 1, 1)
    with pytest.raises(ValueError, match="periodic_columns limit.*65 > 64"):
        many.build()
    rap = air.fibonacci_rap_program(16, 16)
    with pytest.raises(ValueError, match="cannot read periodic columns"):
        rap.aux.periodic(0, 0)


def test_builder_carries_the_descriptor(hip_lib):
    b, keys = golden_air()
    desc, keep = b.build()
    assert desc.periodic_desc.n_cols == 1 and desc.periodic_desc.cols[0].period == 8
    raw = ctypes.string_at(desc.periodic_desc.cols[0].values, 32 * 8)
    assert [int.from_bytes(raw[32 * j:32 * j + 32], "big") for j in range(8)] == keys
    assert [op for op, _, _ in b.ops].count(air.OP_PERIODIC) == 1
    plain, plain_keep = air.quadratic().build()
    assert not hasattr(plain, "periodic_desc")
    rows = air.mimc_chain_trace(64, 3, keys)
    assert all(rows[i + 1][0] == pow(rows[i][0] + keys[i % 8], 3, P) for i in range(63)) and rows[0] == [3]


def test_periodic_verifier_on_the_oracles_proof_of_a_degenerate_column(oracle, hip_lib):
    """Independent of the device: the CPU oracle proves mimc_chain with its periodic read replaced by the constant the column holds
    everywhere; the library's verifier, evaluating the period-8 column at the out-of-domain points, accepts exactly that statement."""
    import periodic_airs as X
    for n, period, options in ((64, 8, (4, 3, 3, 1)), (16, 16, (8, 3, 3, 1)), (64, 1, (4, 4, 3, 2))):
        b, rows = X.mimc(n, period, seed=71, same=True)
        cdesc, ckeep = X.with_constants(b).build()
        proof = oracle.program_air_prove(cdesc, X.to_bytes(rows), options)
        desc, keep = b.build()
        opt = api.ProofOptions(*options)
        assert api.air_verify(proof, desc, opt), (n, period)
        desc.periodic_desc, other_keep = air.periodic_desc(X.changed(b, 0, period - 1))
        assert not api.air_verify(proof, desc, opt), (n, period)


def _verify_periodic(lib, proof, desc, per, options=GOLDEN_OPTIONS, backend=0):
    opt = api.ProofOptions(*options).to_c()
    return lib.sp_air_verify_periodic(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(per), ctypes.byref(opt), backend)


def test_cpu_verifier_on_the_recorded_proof(hip_lib):
    """tests/golden/periodic_mimc_n64.proof was written by this library's own device prover (n = 64, period 8, options (4, 3, 3, 1)): a
    regression pin of prover and verifier together, NOT an oracle.  The independent checks are test_periodic_eval_against_lagrange
    (the verifier's periodic values) and tests/test_gpu_air_periodic.py (the oracle's bytes and LDE, completeness, soundness)."""
    proof = open(GOLDEN, "rb").read()
    b, keys = golden_air()
    desc, keep = b.build()
    opt = api.ProofOptions(*GOLDEN_OPTIONS)
    assert api.air_verify(proof, desc, opt)
    for at in (9, len(proof) // 2, len(proof) - 9):
        bad = bytearray(proof)
        bad[at] ^= 1
        assert not api.air_verify(bytes(bad), desc, opt), at
    # another statement: one key changed
    other = list(keys)
    other[5] = (other[5] + 1) % P
    desc.periodic_desc, other_keep = air.periodic_desc([other])
    assert not api.air_verify(proof, desc, opt)
    assert not api.air_verify(proof, desc, opt, api.SP_MERKLE_POSEIDON)


def test_verifiers_refuse_what_they_must(hip_lib):
    proof = open(GOLDEN, "rb").read()
    b, keys = golden_air()
    desc, keep = b.build()
    per = desc.periodic_desc
    assert _verify_periodic(hip_lib, proof, desc, per) == 1
    # sp_air_verify / sp_air_verify_backend know no op 6
    opt = api.ProofOptions(*GOLDEN_OPTIONS).to_c()
    assert hip_lib.sp_air_verify(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(opt)) == 0
    assert b"constraint program" in hip_lib.sp_last_error()
    assert hip_lib.sp_air_verify_backend(proof, ctypes.c_uint64(len(proof)), ctypes.byref(desc), ctypes.byref(opt), 0) == 0
    # malformed descriptors: no power of two, longer than the trace, null values, 65 columns, an op 6 beyond the columns
    for columns in ([keys[:6]], [keys * 16], [keys] * 65):
        bad, bad_keep = air.periodic_desc(columns)
        assert _verify_periodic(hip_lib, proof, desc, bad) == 0, (len(columns), len(columns[0]))
    null, null_keep = air.periodic_desc([keys])
    null.cols[0].values = None
    assert _verify_periodic(hip_lib, proof, desc, null) == 0
    huge, huge_keep = air.periodic_desc([keys])
    huge.cols[0].period = 1 << 31                                       # refused before anything of that size is allocated or read
    assert _verify_periodic(hip_lib, proof, desc, huge) == 0
    none, none_keep = air.periodic_desc([])
    assert _verify_periodic(hip_lib, proof, desc, none) == 0
    beyond, beyond_keep = b.build()
    assert beyond.ops[1].op == air.OP_PERIODIC
    beyond.ops[1].b = 1
    assert _verify_periodic(hip_lib, proof, beyond, per) == 0
    two, two_keep = air.periodic_desc([keys, keys])                     # ... which a second column makes well-formed (and true here)
    assert _verify_periodic(hip_lib, proof, beyond, two) == 1
    assert _verify_periodic(hip_lib, proof, desc, per) == 1
