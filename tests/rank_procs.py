"""The one launcher for the tests' rank processes: `run_ranks` starts a world of fresh processes that share a process group,
`run_child` one process without a group.  Either returns what the bodies returned, or raises `RankFailure` as soon as one rank raises
or ends without a result - and on every way out ends the processes it started, so that no rank outlives its test with the GPU open.

Every rank reports over a pipe of its own whose write end only that process holds: a rank that dies, even half-way through a
multi-megabyte result, shows as end-of-file on its pipe instead of leaving the parent inside a read that never completes."""
import os
import socket
import sys
import time
import traceback
import warnings
from multiprocessing.connection import wait

import torch.multiprocessing as mp

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
TEARDOWN_S = 120         # what a rank that has delivered its result may take to close its context and leave
TERMINATE_S = 30


class RankFailure(AssertionError):
    """Per rank: the traceback of one that raised, the exit code of one that ended without a result; on a time limit, who was heard from."""


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _child(rank, world, port, backend, device, body, args, conn):
    sys.path[:0] = [ROOT, TESTS]
    dist = None
    try:
        if backend is None:
            value = body(*args)
        else:
            import torch.distributed as dist
            os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
            group = {}
            if device is not None:
                import torch
                torch.cuda.set_device(device)
                group["device_id"] = torch.device(f"cuda:{device}")
            dist.init_process_group(backend, rank=rank, world_size=world, **group)
            value = body(rank, world, *args)
        conn.send((True, value))
    except Exception:
        conn.send((False, traceback.format_exc()))
    finally:
        if dist is not None and dist.is_initialized():
            dist.destroy_process_group()


def _launch(world, body, args, backend, timeout, devices):
    ctx = mp.get_context("spawn")
    port = free_port() if backend is not None else None
    deadline = time.monotonic() + timeout
    procs, conns, results = [], [], {}
    try:
        for r in range(world):
            reader, writer = ctx.Pipe(duplex=False)
            p = ctx.Process(target=_child, args=(r, world, port, backend, None if devices is None else devices[r], body, tuple(args), writer))
            p.start()
            writer.close()               # the rank holds the only write end now: its death is end-of-file on `reader`
            procs.append(p)
            conns.append(reader)
        while len(results) < world:
            pending = [r for r in range(world) if r not in results]
            ready = wait([conns[r] for r in pending] + [procs[r].sentinel for r in pending], max(0.0, deadline - time.monotonic()))
            if not ready:
                heard = ", ".join(map(str, sorted(results)))
                raise RankFailure(f"time limit of {timeout} s: " + (f"heard from ranks {heard} only" if results else "no rank was heard from"))
            failures = []
            for r in pending:
                if conns[r] not in ready and procs[r].sentinel not in ready:
                    continue
                try:                     # (a rank that posted and then exited: its result is still in the pipe, and is read here first)
                    ok, value = conns[r].recv()
                except (EOFError, OSError):
                    procs[r].join(TERMINATE_S)
                    failures.append(f"rank {r} ended with exit code {procs[r].exitcode} and without a result")
                    continue
                if ok:
                    results[r] = value
                else:
                    failures.append(f"rank {r} raised:\n{value}")
            if failures:
                raise RankFailure("\n".join(failures))
        for r, p in enumerate(procs):
            p.join(TEARDOWN_S)
            if p.exitcode != 0:
                warnings.warn(f"rank {r} delivered its result and then " + ("did not end: terminated" if p.exitcode is None else f"ended with exit code {p.exitcode}"))
        return results
    finally:
        for p in procs:                  # exactly the processes started above
            if p.is_alive():
                p.terminate()
                p.join(TERMINATE_S)
                if p.is_alive():
                    p.kill()
                    p.join(TERMINATE_S)
        for c in conns:
            c.close()


def run_ranks(world, body, args=(), *, backend="gloo", timeout, devices=None):
    """{rank: body(rank, world, *args)} from `world` spawned processes inside one `backend` process group; `devices[rank]` is the
    GPU a rank binds itself and the group to (RCCL).  `body` is a module-level function: it is pickled by name."""
    return _launch(world, body, args, backend, timeout, devices)


def run_child(body, args=(), *, timeout):
    """body(*args) from one spawned process without a process group, which has ended when this returns."""
    return _launch(1, body, args, None, timeout, None)[0]
