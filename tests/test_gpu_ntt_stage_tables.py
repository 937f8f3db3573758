"""Whole transforms through sp_ntt_dev at the sizes whose plans have two strided passes (2^17 ... 2^22, both stage-count splits), in
both directions and batched: every element equals the CPU oracle's.  The strided passes read each stage's twiddles from that stage's own
table inside one "pyramid" per engine (csrc/ntt.h, NttEngine::stage_tables); fresh contexts that meet a small size after a large one and a
large one after a small one cover the reuse and the growth of that allocation.  The same file passes when the library is built with
-DSP_NTT_STAGE_TW=0 (single-table addressing)."""
import numpy as np
import pytest

from hip_buffers import HipBuffer
from lambdaworks_cairo_prover_amd import api

pytestmark = pytest.mark.gpu

def _residues(k, batch, seed):
    """batch columns of 2^k uniform residues below 2^251 (< p), canonical big-endian bytes; p - 1, p - 2, 0 and 1 among them."""
    raw = np.random.default_rng(seed).integers(0, 256, size=(batch, 1 << k, 32), dtype=np.uint8)
    raw[:, :, 0] &= 0x07
    for i, v in enumerate((api.P - 1, api.P - 2, 0, 1)):
        raw[:, 5 + 3 * i] = np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8)
    return raw


def _ntt_dev(ctx, cols, inverse):
    """sp_ntt_dev on device-layout columns (batch, n, 32) -> the result as canonical big-endian bytes."""
    batch, n = cols.shape[0], cols.shape[1]
    host = np.ascontiguousarray(np.concatenate([api.fe_to_device(c) for c in cols]))
    with HipBuffer(host) as d:
        ctx.ntt_dev(d.address, n, batch, inverse=inverse)
        ctx.sync()
        out = d.to_host()
    return api.fe_from_device(out.reshape(-1, 32)).reshape(batch, n, 32)


def _check(ctx, oracle, k, batch, seed, directions=(False, True)):
    cols = _residues(k, batch, seed)
    for inverse in directions:
        got = _ntt_dev(ctx, cols, inverse)
        for v in range(batch):
            want = oracle.ntt(cols[v], inverse)
            assert np.array_equal(got[v], want), (k, batch, v, "inverse" if inverse else "forward", int((got[v] != want).any(axis=1).sum()))


@pytest.mark.parametrize("k", [17, 18, 19, 20, 21, 22])
def test_forward_and_inverse_at_every_size_with_two_strided_passes(hip_ctx, oracle, k):
    _check(hip_ctx, oracle, k, 1, 1700 + k)


def test_batch_of_three_at_2_19(hip_ctx, oracle):
    _check(hip_ctx, oracle, 19, 3, 1903)


def test_inverse_at_2_22_in_a_context_that_has_run_nothing_else(hip_lib, oracle):
    with api.Context(device=0) as ctx:
        _check(ctx, oracle, 22, 1, 2201, directions=(True,))


def test_small_size_after_a_large_one_reuses_the_tables(hip_lib, oracle):
    with api.Context(device=0) as ctx:
        _check(ctx, oracle, 22, 1, 2214, directions=(False,))
        _check(ctx, oracle, 14, 1, 1422)
        _check(ctx, oracle, 22, 1, 2215, directions=(True,))


def test_large_size_after_a_small_one_grows_the_tables(hip_lib, oracle):
    with api.Context(device=0) as ctx:
        _check(ctx, oracle, 12, 1, 1220)
        _check(ctx, oracle, 20, 1, 2012)
        _check(ctx, oracle, 12, 1, 1221)    # the first, smaller tables are still there and still right
