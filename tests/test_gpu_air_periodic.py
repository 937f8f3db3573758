"""Periodic columns of program AIRs on the device (sp_air_prove_periodic).  The CPU oracle has no periodic columns, so the checks are:
the oracle's bytes where the columns are degenerate (one value: a constant), the oracle's LDE for the table the kernel reads, and
completeness plus soundness around real periods through the library's verifier, whose periodic values the CPU tests pin
(tests/test_air_periodic.py)."""
import numpy as np
import pytest

import oracle_lib as O
import periodic_airs as X
from lambdaworks_cairo_prover_amd import _lib, air, api

pytestmark = pytest.mark.gpu

OPTIONS = [(4, 3, 3, 1), (8, 3, 3, 1), (4, 4, 3, 2)]
P = api.P


def _flipped(trace):
    t = trace.copy()
    t[t.shape[0] // 2, 0, 31] ^= 1
    return t


# ---- 1. the oracle's bytes for columns that hold one value ---------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
@pytest.mark.parametrize("name,n", [("mimc1", 64), ("mimc8", 64), ("mimc8", 16), ("linear", 64), ("linear", 256)])
def test_degenerate_columns_give_the_oracle_bytes(hip_ctx, oracle, name, n, options):
    """Op 6 on an all-equal column is CONST: byte for byte the oracle's proof of the AIR with the constant, for a valid trace (2n-point
    path) and a one-cell-flipped one (whole-domain path, deg H >= 2n)."""
    if name.startswith("mimc"):
        b, rows = X.mimc(n, int(name[4:]), seed=11, same=True)
    else:
        b, rows = X.linear(n, X.keys(12, 1), X.keys(13, 1) * 8)
    desc, keep = b.build()
    cdesc, ckeep = X.with_constants(b).build()
    assert not hasattr(cdesc, "periodic_desc")
    trace = X.to_bytes(rows)
    for t, path in ((trace, 1), (_flipped(trace), 3)):
        want = O.program_air_prove(cdesc, t, options)
        got = hip_ctx.air_prove(desc, t, api.ProofOptions(*options))
        assert got == want, (name, n, path)
        assert hip_ctx.last_proof_info()["composition_path"] == path


# ---- 2. the table against the oracle's LDE of the column a committed column would be ------------------------------------------
@pytest.mark.parametrize("n", [16, 64, 256])
def test_table_equals_the_oracle_lde_of_the_repeated_column(hip_ctx, oracle, n):
    """P is the interpolant of [v[i mod p]] over the trace domain, so its LDE is the oracle's LDE of that column; the table holds one
    period (p x blowup points) of it.  Periods 1 .. 16 take the direct kernels, longer ones the transform plans."""
    for period in (1, 2, 8, n):
        values = X.keys(100 + period, period)
        col = api.felts_to_bytes([values[i % period] for i in range(n)])
        coeffs = O.ntt(col, inverse=True)
        for blowup in (2, 4, 8):
            got = hip_ctx.air_periodic_lde(values, n, blowup, 3)
            assert got.shape == (period * blowup, 32)
            want = O.lde(coeffs, blowup, 3)
            assert np.array_equal(np.tile(got, (n // period, 1)), want), (n, period, blowup)


# ---- 3. completeness and soundness around real periods ------------------------------------------------------------------------
def _case(name, n):
    if name == "wrap":
        return X.wrap(n, X.keys(21, 8))
    return X.mimc(n, n if name == "mimc_n" else int(name[4:]), seed=22)


@pytest.mark.parametrize("name,n,options", [(name, 64, o) for name in ("mimc2", "mimc8", "mimc_n", "wrap") for o in OPTIONS]
                         + [(name, n, OPTIONS[0]) for name in ("mimc8", "mimc_n", "wrap") for n in (16, 256)])
def test_real_periods_prove_verify_and_reject(hip_ctx, name, n, options):
    b, rows = _case(name, n)
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    trace = X.to_bytes(rows)
    proof = hip_ctx.air_prove(desc, trace, opt)
    path = hip_ctx.last_proof_info()["composition_path"]
    print(name, n, options, "composition path", path)
    assert path in (1, 2)                      # 3: the exact trace check read a wrong periodic value
    assert api.air_verify(proof, desc, opt)
    # the statement includes the periodic values: one changed value, and the same proof is refused
    for column in range(len(b.periodic_cols)):
        other, other_keep = air.periodic_desc(X.changed(b, column, len(b.periodic_cols[column]) - 1))
        desc.periodic_desc = other
        assert not api.air_verify(proof, desc, opt), column
    desc, keep = b.build()
    # a trace wrong on one row still yields a proof (as the reference does), which the verifier refuses
    bad = hip_ctx.air_prove(desc, _flipped(trace), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 3
    assert not api.air_verify(bad, desc, opt)
    assert hip_ctx.air_prove(desc, trace, opt) == proof          # the kept buffers, a second time


# ---- 4. both degree bounds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS)
def test_degree_one_constraints_with_degree_bound_factor_one(hip_ctx, options):
    """(The cubic with factor 2 is mimc_chain above.)  Periods 2 and 32 at once: a direct-kernel table and a transform-plan table."""
    n = 64
    b, rows = X.linear(n, X.keys(31, 2), X.keys(32, 32))
    assert b.degree_bound_factor == 1 and b.degrees == [1, 1]
    desc, keep = b.build()
    opt = api.ProofOptions(*options)
    proof = hip_ctx.air_prove(desc, X.to_bytes(rows), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(proof, desc, opt)
    desc.periodic_desc, other_keep = air.periodic_desc(X.changed(b, 1, 17))
    assert not api.air_verify(proof, desc, opt)


def test_valid_trace_on_the_whole_domain_gives_the_oracle_bytes(hip_ctx, oracle):
    """composition_path 2, without periodic columns: x' = x^2 + k DECLARED cubic under the degree bound 2n, the last three rows exempt.
    By the declared degree deg H may reach 3 (n - 1) + 3 - n = 2n, so 2n points do not fix it and the 2n-point path is refused before
    the trace is looked at; the trace satisfies the constraint and its H, of degree 2 (n - 1) + 3 - n = n + 1, passes the
    high-coefficient check.  16 rows, blowup 4."""
    n, k = 16, X.keys(61, 1)[0]
    b = air.AirBuilder(1, [0, 1], 2)
    x = b.load(0, 0)
    b.constraint(b.load(1, 0) - x * x - b.const(k), degree=3, exemptions=3)
    b.boundary(0, 0, 3)
    rows = [[3]]
    while len(rows) < n:
        rows.append([(rows[-1][0] ** 2 + k) % P])
    assert b.check_trace(rows) == []
    desc, keep = b.build()
    trace, options = X.to_bytes(rows), (4, 3, 3, 1)
    want = O.program_air_prove(desc, trace, options)
    assert O.program_air_verify(desc, want, options)
    assert hip_ctx.air_prove(desc, trace, api.ProofOptions(*options)) == want
    assert hip_ctx.last_proof_info()["composition_path"] == 2


# ---- 5. Poseidon trees -----------------------------------------------------------------------------------------------------------
def test_poseidon_backend(hip_ctx):
    b, rows = X.mimc(64, 8, seed=41)
    desc, keep = b.build()
    opt = api.ProofOptions(4, 3, 3, 1)
    hip_ctx.set_option(api.SP_OPT_MERKLE_BACKEND, api.SP_MERKLE_POSEIDON)
    try:
        proof = hip_ctx.air_prove(desc, X.to_bytes(rows), opt)
    finally:
        hip_ctx.set_option(api.SP_OPT_MERKLE_BACKEND, api.SP_MERKLE_KECCAK256)
    assert api.air_verify(proof, desc, opt, api.SP_MERKLE_POSEIDON)
    assert not api.air_verify(proof, desc, opt)
    assert proof != hip_ctx.air_prove(desc, X.to_bytes(rows), opt)


# ---- 6. an auxiliary program beside periodic columns -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,options", [(64, (4, 3, 3, 1)), (16, (8, 3, 3, 1))])
def test_aux_program_with_a_periodic_selector(hip_ctx, n, options):
    b, rows = X.rap_with_selector(n)
    desc, keep = b.build()
    assert desc.aux_desc.n_cols == 1 and desc.periodic_desc.n_cols == 1
    opt = api.ProofOptions(*options)
    proof = hip_ctx.air_prove(desc, X.to_bytes(rows), opt)
    assert hip_ctx.last_proof_info()["composition_path"] == 1
    assert api.air_verify(proof, desc, opt)
    desc.periodic_desc, other_keep = air.periodic_desc([[1, 1, 0, 0]])
    assert not api.air_verify(proof, desc, opt)


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_prover_refuses_malformed_periodic_descriptors(hip_ctx):
    n, opt = 16, api.ProofOptions(4, 3, 3, 1)
    b, rows = X.mimc(n, 8, seed=51)
    trace = X.to_bytes(rows)
    good, keep = b.build()

    def code(desc):
        with pytest.raises(api.SpError) as e:
            hip_ctx.air_prove(desc, trace, opt)
        return e.value.code

    for columns in ([X.keys(1, 8)[:6]], [X.keys(1, 32)], [X.keys(1, 1)] * 65):       # no power of two, longer than the trace, 65 columns
        desc, k = b.build()
        desc.periodic_desc, k2 = air.periodic_desc(columns)
        assert code(desc) == _lib.SP_E_INVALID_ARG, len(columns[0])
    desc, k = b.build()
    desc.periodic_desc.cols[0].period = 1 << 31                                        # refused before anything of that size is allocated
    assert code(desc) == _lib.SP_E_INVALID_ARG
    desc, k = b.build()
    desc.periodic_desc.cols[0].values = None
    assert code(desc) == _lib.SP_E_INVALID_ARG
    desc, k = b.build()
    desc.ops[1].b = 1                                                                  # op 1: PERIODIC(0, 0) -> a column that is not there
    assert desc.ops[1].op == air.OP_PERIODIC
    assert code(desc) == _lib.SP_E_INVALID_ARG
    # sp_air_prove and sp_air_prove_aux know no op 6
    desc, k = b.build()
    del desc.periodic_desc
    assert code(desc) == _lib.SP_E_INVALID_ARG
    assert api.air_verify(hip_ctx.air_prove(good, trace, opt), good, opt)              # and the context still proves
