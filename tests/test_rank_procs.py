"""The rank launcher's own paths (tests/rank_procs.py), on the CPU over gloo: results come back whole, a rank that raises or ends
without a word fails the call at once and by name, the time limit ends a silent world, and no process is left behind."""
import multiprocessing
import os
import time

import pytest

from rank_procs import RankFailure, run_child, run_ranks

MB = 1 << 20


def _payload(rank, world):
    return bytes([rank + 1]) * (4 * MB)


def _zero_raises_one_sleeps(rank, world):
    if rank == 0:
        raise ValueError("boom")
    time.sleep(30)


def _one_exits_zero_reduces(rank, world):
    import torch
    import torch.distributed as dist
    if rank == 1:
        os._exit(3)
    dist.all_reduce(torch.ones(4))


def _sleeps(rank, world):
    time.sleep(60)


def _square(x):
    return x * x


def _raises(word):
    raise KeyError(word)


def _returns_then_exits_with_5():
    import threading
    threading.Thread(target=lambda: (time.sleep(0.2), os._exit(5))).start()      # (a child joins its threads before it leaves)
    return "delivered"


def _fails_within(limit, *call, **kw):
    t0 = time.monotonic()
    with pytest.raises(RankFailure) as e:
        run_ranks(*call, **kw)
    assert time.monotonic() - t0 < limit
    assert multiprocessing.active_children() == []
    return str(e.value)


def test_results_come_back_whole():
    for _ in range(3):              # (a rank exits while the tail of its 4 MB is still in the pipe: posted, then gone)
        got = run_ranks(4, _payload, timeout=120)
        assert sorted(got) == [0, 1, 2, 3]
        assert all(got[r] == bytes([r + 1]) * (4 * MB) for r in range(4))
    assert multiprocessing.active_children() == []


def test_a_rank_that_raises_ends_the_world():
    message = _fails_within(30, 2, _zero_raises_one_sleeps, timeout=60)
    assert "rank 0 raised" in message and "boom" in message and "ValueError" in message


def test_a_rank_that_ends_without_a_word_is_named_with_its_exit_code():
    message = _fails_within(30, 2, _one_exits_zero_reduces, timeout=60)
    assert "rank 1 ended with exit code 3" in message


def test_time_limit_ends_a_silent_world():
    message = _fails_within(15, 2, _sleeps, timeout=5)
    assert "time limit" in message and "no rank was heard from" in message


def test_run_child():
    assert run_child(_square, (7,), timeout=60) == 49
    with pytest.raises(RankFailure) as e:
        run_child(_raises, ("nothing here",), timeout=60)
    assert "KeyError" in str(e.value) and "nothing here" in str(e.value)
    assert multiprocessing.active_children() == []


def test_a_bad_exit_code_after_a_good_result_is_a_warning():
    with pytest.warns(UserWarning, match="rank 0 delivered its result and then ended with exit code 5"):
        assert run_child(_returns_then_exits_with_5, timeout=60) == "delivered"
