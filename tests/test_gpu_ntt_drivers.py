"""The three transform drivers the prover runs - NttEngine::lde_coset_major, lde_from_bitrev (sharded) and
dif_natural_to_bitrev_inverse (post_table, src) - through sp_lde_dev and sp_intt_bitrev_dev, element by element against
tests/ntt_driver_ref.py (oracle.ntt / oracle.lde and index maps), bit for bit in the device layout: a value that is right modulo p but
not canonical differs.  The shapes are tests/ntt_driver_shapes.py's table: tests/test_ntt_plan_cover.py shows that they reach every
class of launch the drivers make for k <= 20 up to 128 MiB.  A mismatch names the first differing (column, coset, index)."""
import ctypes
import functools

import numpy as np
import pytest

import ntt_driver_ref as ref
import ntt_driver_shapes as shapes
from hip_buffers import HipBuffer
from lambdaworks_cairo_prover_amd import _lib, api

pytestmark = pytest.mark.gpu

P = api.P
H = 3
GUARD = 0xA5
DISTINCT = 8                 # a wide batch repeats this many different columns in a random order: the reference stays cheap
REFERENCE_BUDGET = 1 << 20   # elements of oracle output one case asks for (about a second)
SMALL = 4 << 20              # below this footprint a shape runs with padded strides and on every rank


def _fe(v):
    return np.frombuffer(int(v).to_bytes(32, "big"), dtype=np.uint8)


def _residues(count, n, seed):
    """count columns of n uniform residues below 2^251 (< p), canonical big-endian bytes; p - 1, p - 2, 0 and 1 among them"""
    raw = np.random.default_rng(seed).integers(0, 256, size=(count, n, 32), dtype=np.uint8)
    raw[:, :, 0] &= 0x07
    for i, v in enumerate((P - 1, P - 2, 0, 1)):
        raw[:, (5 + 3 * i) % n] = _fe(v)
    return raw


def _columns(batch, seed, log_size=0):
    """which of the d different columns each vector of the batch holds: every one at least once, then at random.  d = the batch up to
    DISTINCT, fewer where d columns would ask the oracle for more than REFERENCE_BUDGET = 2^log_size-element values: the reference,
    not the GPU, is what a case's time goes to, and no case may outweigh the 2^22 transform of test_gpu_fine_grained.py"""
    d = min(batch, DISTINCT, max(1, REFERENCE_BUDGET >> log_size))
    return d, np.concatenate([np.arange(d), np.random.default_rng(seed).integers(0, d, size=batch - d)])


def _dev(canonical):
    return api.fe_to_device(canonical).reshape(canonical.shape)


def _padded(arr, stride):
    out = np.full((arr.shape[0], stride, 32), GUARD, dtype=np.uint8)
    out[:, :arr.shape[1]] = arr
    return out


# ---------------------------------------------------------------------------------------------- running the drivers
def _run_lde(ctx, dev_in, blowup, order, shard_log=0, rank=0, padded=False):
    """sp_lde_dev on device-layout input (cols, n, 32) -> device-layout output (cols, n * b_loc, 32); with padded strides the gaps
    between the columns must come back untouched, and the input always does"""
    cols, n = dev_in.shape[0], dev_in.shape[1]
    out_len = n * (blowup >> shard_log)
    ss, ds = (n + 3, out_len + 5) if padded else (n, out_len)
    host_in = _padded(dev_in, ss) if padded else np.ascontiguousarray(dev_in)
    with HipBuffer(host_in) as src, HipBuffer(nbytes=cols * ds * 32, fill=GUARD) as dst:
        ctx.lde_dev(src.address, dst.address, n, blowup, cols, ss, ds, order, shard_log, rank)
        ctx.sync()
        out = dst.to_host().reshape(cols, ds, 32)
        assert np.array_equal(src.to_host(), host_in.reshape(-1)), "the LDE wrote to its input"
    assert (out[:, out_len:] == GUARD).all(), "the LDE wrote between the columns of its output"
    return out[:, :out_len]


def _run_intt(ctx, dev_x, dev_post=None, use_src=False, padded=False):
    """sp_intt_bitrev_dev on device-layout evaluations (batch, n, 32) -> device-layout (batch, n, 32); with src the source array
    must come back unchanged"""
    batch, n = dev_x.shape[0], dev_x.shape[1]
    stride = n + 3 if padded else n
    host_x = _padded(dev_x, stride) if padded else np.ascontiguousarray(dev_x)
    post = HipBuffer(np.ascontiguousarray(dev_post)) if dev_post is not None else None
    src = HipBuffer(host_x) if use_src else None
    data = HipBuffer(nbytes=host_x.nbytes, fill=GUARD) if use_src else HipBuffer(host_x)
    try:
        ctx.intt_bitrev_dev(data.address, n, batch, stride, post.address if post else None, src.address if src else None)
        ctx.sync()
        out = data.to_host().reshape(batch, stride, 32)
        if src:
            assert np.array_equal(src.to_host(), host_x.reshape(-1)), "the inverse driver wrote to src"
        if post:
            assert np.array_equal(post.to_host(), np.ascontiguousarray(dev_post).reshape(-1)), "the inverse driver wrote to post_table"
    finally:
        for b in (post, src, data):
            if b:
                b.free()
    assert (out[:, n:] == GUARD).all(), "the inverse driver wrote between its vectors"
    return out[:, :n]


# ---------------------------------------------------------------------------------------------- references, computed once
@functools.lru_cache(maxsize=4)
def _lde_case(k, blowup, distinct, seed):
    """random coefficients -> (natural-order evaluations (distinct, N, 32), device-layout driver input (distinct, n, 32))"""
    coeffs = _residues(distinct, 1 << k, seed)
    return ref.natural_evaluations(coeffs, blowup, H), _dev(ref.lde_input(coeffs, H))


def _check_lde(ctx, shape, ranks, seed):
    order = api.LDE_COSET_MAJOR if shape.driver == "lde_coset_major" else api.LDE_NATURAL
    name = "coset_major" if order == api.LDE_COSET_MAJOR else "natural"
    blowup = 1 << shape.logb
    distinct, which = _columns(shape.batch, seed, shape.k + shape.logb)
    nat, dev_in = _lde_case(shape.k, blowup, distinct, seed)
    padded = shapes.footprint(shape) <= SMALL
    for rank in ranks:
        want = (ref.lde_coset_major if order == api.LDE_COSET_MAJOR else ref.lde_natural)(nat, blowup, shape.shard_log, rank)
        got = _run_lde(ctx, dev_in[which], blowup, order, shape.shard_log, rank, padded)
        ref.assert_same(got.reshape((shape.batch,) + want.shape[1:]), _dev(want)[which], name, f"{tuple(shape)} rank {rank}")


def _ranks(shape):
    """every rank of a small shape, the last one of a large one (the launches do not depend on the rank)"""
    world = 1 << shape.shard_log
    return range(world) if shapes.footprint(shape) <= SMALL else (world - 1,)


def _id(shape):
    return f"k{shape.k}-b{1 << shape.logb}-s{shape.shard_log}-x{shape.batch}"


_COSET_MAJOR = [s for s in shapes.table() if s.driver == "lde_coset_major"]
_NATURAL = [s for s in shapes.table() if s.driver == "lde_natural"]
_INVERSE = [s for s in shapes.table() if s.driver == "intt_bitrev"]


@pytest.mark.parametrize("shape", _COSET_MAJOR, ids=_id)
def test_coset_major_lde_matches_the_reference(hip_ctx, oracle, shape):
    _check_lde(hip_ctx, shape, _ranks(shape), 7000 + shape.k)


# one case per (k, blowup, batch): every shard_log of the table and every rank against its own slice of ONE reference
_NATURAL_GROUPS = sorted({(s.k, s.logb, s.batch) for s in _NATURAL})


@pytest.mark.parametrize("k,logb,batch", _NATURAL_GROUPS, ids=lambda v: str(v))
def test_natural_lde_matches_the_reference_on_every_rank(hip_ctx, oracle, k, logb, batch):
    for shape in _NATURAL:
        if (shape.k, shape.logb, shape.batch) == (k, logb, batch):
            _check_lde(hip_ctx, shape, _ranks(shape), 8000 + k)


@pytest.mark.parametrize("shape", _INVERSE, ids=_id)
def test_inverse_driver_matches_the_reference(hip_ctx, oracle, shape):
    n = 1 << shape.k
    distinct, which = _columns(shape.batch, 9000 + shape.k, shape.k + 1)      # two references: with and without post_table
    x = _residues(distinct, n, 9000 + shape.k)
    post = _residues(1, n, 9100 + shape.k)[0]
    small = shapes.footprint(shape) <= SMALL
    for with_post in (False, True):
        want = _dev(ref.inverse_driver(x, post if with_post else None))[which]
        for use_src in (False, True):
            got = _run_intt(hip_ctx, _dev(x)[which], _dev(post) if with_post else None, use_src, padded=small)
            ref.assert_same(got, want, "coset_major", f"{tuple(shape)} post_table={with_post} src={use_src}")


# ---------------------------------------------------------------------------------------------- sp_ntt_dev where the old lists miss
@pytest.mark.parametrize("shape", shapes.NTT_DEV_EXTRA, ids=lambda s: f"{s.driver}-k{s.k}-x{s.batch}")
def test_ntt_dev_at_a_small_size_above_the_footprint_threshold(hip_ctx, oracle, shape):
    """forward_natural / inverse_natural with 1024-element strided tiles at sizes the existing cases only run with 512-element ones"""
    inverse = shape.driver == "inverse_natural"
    distinct, which = _columns(shape.batch, 9500 + shape.k, shape.k)
    x = _residues(distinct, 1 << shape.k, 9500 + shape.k)
    want = _dev(np.stack([oracle.ntt(c, inverse) for c in x]))[which]
    with HipBuffer(np.ascontiguousarray(_dev(x)[which])) as d:
        hip_ctx.ntt_dev(d.address, 1 << shape.k, shape.batch, inverse=inverse)
        hip_ctx.sync()
        got = d.to_host().reshape(want.shape)
    ref.assert_same(got, want, "coset_major", str(tuple(shape)))


# ---------------------------------------------------------------------------------------------- extreme inputs
def _extreme_patterns(n):
    """all p - 1; alternating 0 and p - 1; one nonzero entry - as (3, n) integers"""
    out = np.zeros((3, n), dtype=object)
    out[0, :] = P - 1
    out[1, 1::2] = P - 1
    out[2, n // 3] = P - 1
    return out


def _extreme_lde(ctx, shape):
    """the DRIVER'S input - c_rev(pos) h^rev(pos) - holds the patterns: the coefficients are solved for"""
    n, blowup = 1 << shape.k, 1 << shape.logb
    pat = _extreme_patterns(n)                                    # entry pos of the driver's input
    rev = ref.bitrev(shape.k)
    hinv = ref.powers(pow(H, -1, P), n)
    coeffs = np.empty_like(pat)
    coeffs[:, rev] = pat * hinv[rev][None, :] % P                 # c[rev(pos)] = input[pos] h^-rev(pos)
    coeffs = ref.to_bytes(coeffs)
    dev_in = _dev(ref.lde_input(coeffs, H))
    assert np.array_equal(dev_in, _dev(ref.to_bytes(pat)))
    nat = ref.natural_evaluations(coeffs, blowup, H)
    which = np.arange(shape.batch) % 3
    coset_major = shape.driver == "lde_coset_major"
    rank = (1 << shape.shard_log) - 1
    want = (ref.lde_coset_major if coset_major else ref.lde_natural)(nat, blowup, shape.shard_log, rank)
    got = _run_lde(ctx, dev_in[which], blowup, api.LDE_COSET_MAJOR if coset_major else api.LDE_NATURAL, shape.shard_log, rank)
    ref.assert_same(got.reshape((shape.batch,) + want.shape[1:]), _dev(want)[which], "coset_major" if coset_major else "natural", f"extreme {tuple(shape)}")


# one strided pass (k = 12) and two (k = 17), each below and above 64 MiB
@pytest.mark.parametrize("shape", [shapes.Shape("lde_coset_major", 12, 3, 0, 3), shapes.Shape("lde_coset_major", 12, 3, 0, 65),
                                   shapes.Shape("lde_coset_major", 17, 2, 0, 3), shapes.Shape("lde_coset_major", 17, 3, 0, 3)], ids=_id)
def test_coset_major_lde_on_extreme_inputs(hip_ctx, oracle, shape):
    strided = [p for p in api.ntt_plan(*shape) if not p["contig"]]
    assert len(strided) == (1 if shape.k == 12 else 2)
    assert (shapes.footprint(shape) > shapes.FOOTPRINT_THRESHOLD) == (shape.batch == 65 or shape.logb == 3 and shape.k == 17)
    _extreme_lde(hip_ctx, shape)


# one strided pass (2^8 x 2) and two (2^12 x 2, sharded and not)
@pytest.mark.parametrize("shape", [shapes.Shape("lde_natural", 8, 1, 0, 3), shapes.Shape("lde_natural", 12, 1, 0, 3),
                                   shapes.Shape("lde_natural", 12, 2, 1, 3)], ids=_id)
def test_natural_lde_on_extreme_inputs(hip_ctx, oracle, shape):
    assert len(api.ntt_plan(*shape)) == (1 if shape.k == 8 else 2)
    _extreme_lde(hip_ctx, shape)


@pytest.mark.parametrize("k", [12, 16])
def test_inverse_driver_on_extreme_inputs(hip_ctx, oracle, k):
    """one strided pass (2^12) and two (2^16); the patterns as evaluations, with no post_table and with one of all p - 1"""
    assert len([p for p in api.ntt_plan("intt_bitrev", k, 0, 0, 3) if not p["contig"]]) == (1 if k == 12 else 2)
    n = 1 << k
    x = ref.to_bytes(_extreme_patterns(n))
    post = np.tile(_fe(P - 1), (n, 1))
    for table in (None, post):
        want = _dev(ref.inverse_driver(x, table))
        got = _run_intt(hip_ctx, _dev(x), None if table is None else _dev(table), use_src=table is not None)
        ref.assert_same(got, want, "coset_major", f"extreme inverse k={k} post_table={table is not None}")


# ---------------------------------------------------------------------------------------------- ranks, round trip
@pytest.mark.parametrize("driver", ["lde_natural", "lde_coset_major"])
@pytest.mark.parametrize("k,logb", [(9, 2), (12, 3)])
def test_union_of_the_ranks_is_the_unsharded_result(hip_ctx, oracle, driver, k, logb):
    """what the ranks of a sharded call write, put back together by global coset index, is what one unsharded call writes"""
    n, blowup, cols = 1 << k, 1 << logb, 2
    order = api.LDE_COSET_MAJOR if driver == "lde_coset_major" else api.LDE_NATURAL
    nat, dev_in = _lde_case(k, blowup, cols, 8800 + k)
    whole = _run_lde(hip_ctx, dev_in, blowup, order)
    whole = whole.reshape(cols, blowup, n, 32) if order == api.LDE_COSET_MAJOR else whole.reshape(cols, n, blowup, 32)
    ref.assert_same(whole, _dev((ref.lde_coset_major if order == api.LDE_COSET_MAJOR else ref.lde_natural)(nat, blowup)), driver[4:], "unsharded")
    for shard_log in range(1, logb + 1):
        union = np.zeros_like(whole)
        for rank in range(1 << shard_log):
            part = _run_lde(hip_ctx, dev_in, blowup, order, shard_log, rank, padded=True)
            if order == api.LDE_COSET_MAJOR:
                union[:, rank::1 << shard_log] = part.reshape(cols, blowup >> shard_log, n, 32)
            else:
                union[:, :, rank::1 << shard_log] = part.reshape(cols, n, blowup >> shard_log, 32)
        ref.assert_same(union, whole, driver[4:], f"union over 2^{shard_log} ranks")


@pytest.mark.parametrize("k,logb,cols", [(5, 1, 1), (12, 2, 3), (16, 3, 2)])
def test_round_one_chain_interpolate_then_extend(hip_ctx, oracle, k, logb, cols):
    """the prover's round 1: the inverse driver reads the trace columns from another array (src) with post = h^j / n at bit-reversed
    positions, the coset-major LDE extends what it leaves: p(h w_N^i) of the interpolating polynomial, as oracle.lde gives it"""
    n, blowup = 1 << k, 1 << logb
    trace = _residues(cols, n, 9900 + k)
    coeffs = np.stack([oracle.ntt(c, inverse=True) for c in trace])
    want = _dev(ref.lde_coset_major(ref.natural_evaluations(coeffs, blowup, H), blowup))
    post = _dev(ref.post_h_over_n(k, H))
    with HipBuffer(np.ascontiguousarray(_dev(trace))) as src, HipBuffer(nbytes=cols * n * 32, fill=GUARD) as mid, \
            HipBuffer(post) as table, HipBuffer(nbytes=cols * n * blowup * 32, fill=GUARD) as out:
        hip_ctx.intt_bitrev_dev(mid.address, n, cols, n, table.address, src.address)
        hip_ctx.lde_dev(mid.address, out.address, n, blowup, cols, n, n * blowup, api.LDE_COSET_MAJOR)      # same stream: no sync between
        hip_ctx.sync()
        got = out.to_host().reshape(want.shape)
        assert np.array_equal(mid.to_host().reshape(cols, n, 32), _dev(ref.lde_input(coeffs, H)))
    ref.assert_same(got, want, "coset_major", f"round-1 chain k={k} blowup={blowup}")


# ---------------------------------------------------------------------------------------------- argument checks
def test_invalid_arguments_are_refused_before_any_launch(hip_ctx, hip_lib):
    n, blowup, cols = 64, 4, 2
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    with HipBuffer(nbytes=cols * n * 32, fill=0) as src, HipBuffer(nbytes=cols * n * blowup * 32, fill=GUARD) as dst:
        h = hip_ctx._h

        def lde(coeffs=src.address, out=dst.address, n_=n, b=blowup, c=cols, ss=n, ds=n * blowup, order=1, sl=0, rank=0, ctx=h):
            return hip_lib.sp_lde_dev(ctx, vp(coeffs), vp(out), u64(n_), u32(b), u32(c), u64(ss), u64(ds), order, u32(sl), u32(rank))

        def intt(data=dst.address, n_=n, batch=cols, stride=n, post=None, src_=None, ctx=h):
            return hip_lib.sp_intt_bitrev_dev(ctx, vp(data), u64(n_), u32(batch), u64(stride), vp(post), vp(src_))

        bad_lde = dict(size=lde(n_=48), size_zero=lde(n_=0), blowup=lde(b=3), blowup_zero=lde(b=0), too_large=lde(n_=1 << 29, ss=1 << 29, ds=1 << 31),
                       shard_log=lde(sl=3), shard_rank=lde(sl=1, rank=2, ds=n * 2), shard_rank_unsharded=lde(rank=1),
                       src_stride=lde(ss=n - 1), dst_stride=lde(ds=n * blowup - 1), dst_stride_sharded=lde(sl=1, ds=n * 2 - 1),
                       null_coeffs=lde(coeffs=None), null_out=lde(out=None), null_ctx=lde(ctx=None), no_columns=lde(c=0), order=lde(order=2),
                       overlap=lde(coeffs=dst.address), overlap_inside=lde(coeffs=dst.address + 32 * n, c=1),
                       too_many_columns=lde(c=1 << 30))
        bad_intt = dict(size=intt(n_=48), size_zero=intt(n_=0), too_large=intt(n_=1 << 31, stride=1 << 31), stride=intt(stride=n - 1),
                        null_data=intt(data=None), null_ctx=intt(ctx=None), no_vectors=intt(batch=0),
                        src_is_data=intt(src_=dst.address), src_overlaps=intt(src_=dst.address + 32 * (n - 1)), post_overlaps=intt(post=dst.address),
                        too_many_vectors=intt(batch=1 << 30))
        hip_ctx.sync()
        assert (dst.to_host() == GUARD).all(), "a refused call wrote to its output"
        for name, code in list(bad_lde.items()) + list(bad_intt.items()):
            assert code == _lib.SP_E_INVALID_ARG, (name, code)
        # the same calls with valid arguments go through
        assert lde() == 0 and lde(sl=2, rank=3, ds=n) == 0 and intt(src_=src.address) == 0 and intt(batch=1, stride=n) == 0
        hip_ctx.sync()
