"""Periodic columns on sharded contexts: every rank builds the whole table and indexes it by the global LDE index, so every rank
returns the one-GPU proof's bytes (ranks share the one GPU over the staged all-gather, as in test_sharded_program_air).  The one-GPU
proofs come from a child process that has ended before the ranks start, so the test starts at most `world` <= 4 processes on the GPU
at a time (the pytest process itself may hold the session's context from earlier tests, as in the other sharded tests)."""
import os
import socket

import pytest
import torch.multiprocessing as mp

import periodic_airs as X
from lambdaworks_cairo_prover_amd import api

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _cases(n):
    """mimc_chain with period n (at n >= 32 a transform-plan table) and the wrapping AIR (direct-kernel tables, three frame rows)."""
    return [X.mimc(n, n, seed=61), X.wrap(n, X.keys(62, 8))]


def _worker(rank, world, port, n, options, q):
    import sys
    import torch.distributed as dist
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import periodic_airs as X
    from lambdaworks_cairo_prover_amd import api
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = api.Context(device=0)
        ctx.set_collective(world, rank, api.StagedAllGather())
        ctx.set_option(api.SP_OPT_FRI_SHARD_MIN_LOG, 5)
        proofs = []
        for b, rows in _cases(n):
            desc, keep = b.build()
            proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
        q.put((rank, proofs))
        ctx.close()
    except Exception:
        import traceback
        q.put((rank, ("fail: " + traceback.format_exc()).encode()))
    finally:
        dist.destroy_process_group()


def _single_worker(n, options, q):
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, here)
    import periodic_airs as X
    from lambdaworks_cairo_prover_amd import api
    try:
        proofs = []
        with api.Context(device=0) as ctx:
            for b, rows in _cases(n):
                desc, keep = b.build()
                proofs.append(ctx.air_prove(desc, X.to_bytes(rows), api.ProofOptions(*options)))
                assert ctx.last_proof_info()["composition_path"] == 1
        q.put(proofs)
    except Exception:
        import traceback
        q.put(("fail: " + traceback.format_exc()).encode())


@pytest.mark.parametrize("world,n,options", [(2, 64, (4, 3, 3, 1)), (4, 256, (4, 4, 3, 2))])
def test_sharded_contexts_give_the_one_gpu_bytes(world, n, options):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    one = ctx.Process(target=_single_worker, args=(n, options, q))
    one.start()
    want = q.get(timeout=600)
    one.join(timeout=60)
    assert isinstance(want, list), want[:2000]
    for (b, rows), proof in zip(_cases(n), want):
        desc, keep = b.build()
        assert api.air_verify(proof, desc, api.ProofOptions(*options))
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, n, options, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=600) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    for r in range(world):
        assert got[r] == want, (r, got[r][:400] if isinstance(got[r], bytes) else "proof bytes differ")
