"""sp_air_prove's bounds beyond the Cairo kernels' constant blocks, on the CPU: sp_air_limits reports them, AirBuilder refuses a
descriptor beyond them, and the library's host verifier accepts the oracle's proof of a 200-column AIR with boundary
constraints on 64 rows (and rejects it after one byte of an opening is flipped)."""
import pytest

import many_column_air as M
import oracle_lib as O
from lambdaworks_cairo_prover_amd import api


def test_air_limits_are_the_documented_ones(hip_lib):
    assert api.air_limits() == {"columns": 1024, "transitions": 64, "frame_rows": 8, "boundary_constraints": 4096,
                                "constants": 4096, "ops": 65535, "live_values": 64}


def test_builder_refuses_1025_columns(hip_lib):
    b = M.build(8, 1025, n_transitions=1, per_constraint=1, boundary_row_count=2)
    with pytest.raises(ValueError, match="columns"):
        b.build()
    M.build(8, 1024, n_transitions=1, per_constraint=1, boundary_row_count=2).build()   # (the bound itself is accepted)


def test_builder_refuses_too_many_boundary_constraints(hip_lib):
    b = M.build(8, 4, n_transitions=1, boundary_row_count=2, boundary_total=4097)
    with pytest.raises(ValueError, match="boundary_constraints"):
        b.build()


def test_oracle_proof_of_200_columns_on_64_boundary_rows(oracle, hip_lib):
    n, options = 256, (4, 3, 3, 1)
    b = M.build(n, 200, boundary_row_count=64, boundary_total=300)
    assert len({step for _, step, _ in b.bcs}) == 64 and len(b.bcs) == 300 and len(b.consts) > 200
    desc, keep = b.build()
    proof = O.program_air_prove(desc, M.main_trace(n, 200), options)
    opt = api.ProofOptions(*options)
    assert api.air_verify(proof, desc, opt)
    # the last opening's trace values sit right in front of the nonce (8 bytes): flip one byte of one of them
    bad = bytearray(proof)
    bad[len(bad) - 8 - 32 * 5 - 1] ^= 1
    assert not api.air_verify(bytes(bad), desc, opt)
