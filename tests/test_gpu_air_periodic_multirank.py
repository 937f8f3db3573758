"""Periodic columns on sharded contexts: every rank builds the whole table and indexes it by the global LDE index, so every rank
returns the one-GPU proof's bytes (ranks share the one GPU over the staged all-gather, as in test_sharded_program_air).  The one-GPU
proofs come from a child process that has ended before the ranks start, so the test starts at most `world` <= 4 processes on the GPU
at a time (the pytest process itself may hold the session's context from earlier tests, as in the other sharded tests)."""
import pytest

import periodic_airs as X
from lambdaworks_cairo_prover_amd import api
from rank_procs import run_child, run_ranks

pytestmark = pytest.mark.gpu


def _cases(n):
    """mimc_chain with period n (at n >= 32 a transform-plan table) and the wrapping AIR (direct-kernel tables, three frame rows)."""
    return [X.mimc(n, n, seed=61), X.wrap(n, X.keys(62, 8))]


def _body(rank, world, n, options):
    ctx = api.Context(device=0)
    ctx.set_collective(world, rank, api.StagedAllGather())
    ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
    proofs = []
    for b, rows in _cases(n):
        desc, keep = b.build()
        proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
    ctx.close()
    return proofs


def _single_body(n, options):
    proofs = []
    with api.Context(device=0) as ctx:
        for b, rows in _cases(n):
            desc, keep = b.build()
            proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
            assert ctx.last_proof_info()["composition_path"] == 1
    return proofs


@pytest.mark.parametrize("world,n,options", [(2, 64, (4, 3, 3, 1)), (4, 256, (4, 4, 3, 2))])
def test_sharded_contexts_give_the_one_gpu_bytes(world, n, options):
    want = run_child(_single_body, (n, options), timeout=600)
    for (b, rows), proof in zip(_cases(n), want):
        desc, keep = b.build()
        assert api.air_verify(proof, desc, api.ProofOptions(*options))
    got = run_ranks(world, _body, (n, options), timeout=600)
    for r in range(world):
        assert got[r] == want, (r, "proof bytes differ")
