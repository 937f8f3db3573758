"""Plain references for the three transform drivers the prover runs (csrc/ntt.h: dif_natural_to_bitrev_inverse, lde_from_bitrev,
lde_coset_major), built only from oracle.ntt, oracle.lde, Python integers and numpy index maps - nothing of the product library.
tests/test_ntt_driver_ref.py anchors every map here on direct sums in Python integers at small sizes.

Arrays of field elements are numpy uint8 arrays whose last axis holds the 32 canonical big-endian bytes."""
import functools

import numpy as np

import oracle_lib as oracle

P = oracle.P
_R = 1 << 256                      # the device layout is Montgomery form with R = 2^256 ...
# generator of the 2-adic subgroup of order 2^192 (lambdaworks' Stark252PrimeField::TWO_ADIC_PRIMITVE_ROOT_OF_UNITY)
TWO_ADIC_ROOT = 0x5282DB87529CFA3F0464519C8B0FA5AD187148E11A61616070024F42F8EF94


def root_of_unity(log_order):
    """w of order 2^log_order, in Python integers."""
    return pow(TWO_ADIC_ROOT, 1 << (192 - log_order), P)


def bitrev(k):
    """rev_k as an index array of 2^k entries."""
    idx = np.arange(1 << k, dtype=np.int64)
    out = np.zeros_like(idx)
    for bit in range(k):
        out |= ((idx >> bit) & 1) << (k - 1 - bit)
    return out


def to_ints(arr):
    """(..., 32) canonical big-endian bytes -> object array of Python integers."""
    a = np.ascontiguousarray(arr, dtype=np.uint8)
    raw = a.tobytes()
    out = np.empty(a.size // 32, dtype=object)
    out[:] = [int.from_bytes(raw[i:i + 32], "big") for i in range(0, len(raw), 32)]
    return out.reshape(a.shape[:-1])


def to_bytes(ints):
    """object array of integers below 2^256 -> (..., 32) big-endian bytes."""
    v = np.asarray(ints, dtype=object)
    raw = b"".join([int(x).to_bytes(32, "big") for x in v.ravel().tolist()])
    return np.frombuffer(raw, dtype=np.uint8).reshape(v.shape + (32,)).copy()


def to_device(arr):
    """canonical big-endian bytes -> the device layout: 8 x u32 little-endian limbs of x * 2^256 mod p (one little-endian integer)."""
    return np.ascontiguousarray(to_bytes((to_ints(arr) * _R) % P)[..., ::-1])


def from_device(dev):
    """the device layout -> canonical big-endian bytes; any representative below 2^256 is reduced, so a non-canonical store shows
    up as a difference only through canonical_violations below."""
    return to_bytes((to_ints(np.ascontiguousarray(np.asarray(dev, dtype=np.uint8)[..., ::-1])) * pow(_R, -1, P)) % P)


def canonical_violations(dev):
    """how many device-layout elements are not below p (a last pass must store canonical values)"""
    return int((to_ints(np.ascontiguousarray(np.asarray(dev, dtype=np.uint8)[..., ::-1])) >= P).sum())


@functools.lru_cache(maxsize=4)
def _power_list(h, n):
    out, acc = [], 1
    for _ in range(n):
        out.append(acc)
        acc = acc * h % P
    return out


def powers(h, n):
    """h^j, j < n, as an object array"""
    out = np.empty(n, dtype=object)
    out[:] = _power_list(h, n)
    return out


def _scaled(arr, factors):
    """(n, 32) bytes times a list of n integers, element by element mod p -> (n, 32) bytes (one pass over Python integers)"""
    raw = np.ascontiguousarray(arr, dtype=np.uint8).tobytes()
    prod = b"".join([(int.from_bytes(raw[32 * i:32 * i + 32], "big") * f % P).to_bytes(32, "big") for i, f in enumerate(factors)])
    return np.frombuffer(prod, dtype=np.uint8).reshape(-1, 32)


# ---------------------------------------------------------------------------------------------- the inverse driver
def inverse_driver(x, post=None):
    """dif_natural_to_bitrev_inverse on (batch, n, 32) natural-order evaluations: out[pos] = post[pos] * n * c[rev_k(pos)] with
    c = oracle.ntt(x, inverse=True); post (n, 32) is all ones when absent.  Canonical bytes."""
    x = np.asarray(x, dtype=np.uint8)
    batch, n = x.shape[0], x.shape[1]
    k = n.bit_length() - 1
    rev = bitrev(k)
    factor = [n % P] * n if post is None else [f * n % P for f in to_ints(post).tolist()]
    inv = np.empty(n, dtype=np.int64)
    inv[rev] = np.arange(n)                      # factor[pos] meets c[rev(pos)]: scale in natural order, then permute the bytes
    by_natural = [factor[p] for p in inv.tolist()]
    out = np.empty_like(x)
    for v in range(batch):
        out[v] = _scaled(oracle.ntt(x[v], inverse=True), by_natural)[rev]
    return out


def post_h_over_n(k, h):
    """The prover's round-1 post table: h^rev(pos) / n at bit-reversed position pos, so that the inverse driver leaves the h-scaled,
    bit-reversed coefficients the LDE drivers read."""
    n = 1 << k
    return to_bytes((powers(h, n)[bitrev(k)] * pow(n, -1, P)) % P)


# ---------------------------------------------------------------------------------------------- the LDE drivers
def lde_input(coeffs, h):
    """natural-order coefficients (cols, n, 32) -> what the engine reads: entry pos = c[rev(pos)] * h^rev(pos), canonical bytes
    (to_device() of it is the device buffer)."""
    coeffs = np.asarray(coeffs, dtype=np.uint8)
    n = coeffs.shape[1]
    rev = bitrev(n.bit_length() - 1)
    hp = _power_list(h, n)
    return np.stack([_scaled(c, hp)[rev] for c in coeffs])


def natural_evaluations(coeffs, blowup, h):
    """nat[v, i] = p_v(h w_N^i), N = n * blowup: oracle.lde per column, (cols, N, 32)."""
    return np.stack([oracle.lde(c, blowup, h) for c in np.asarray(coeffs, dtype=np.uint8)])


def lde_natural(nat, blowup, shard_log=0, rank=0):
    """lde_from_bitrev on rank `rank` of 2^shard_log: out[q * b_loc + c_loc] = nat[q * b + c_loc * 2^shard_log + rank];
    returned as (cols, n, b_loc, 32) - the flat device order is (q, c_loc)."""
    cols, N = nat.shape[0], nat.shape[1]
    return np.ascontiguousarray(nat.reshape(cols, N // blowup, blowup, 32)[:, :, rank::1 << shard_log])


def lde_coset_major(nat, blowup, shard_log=0, rank=0):
    """lde_coset_major: column v, local coset c_loc, element m = nat_v[m * b + c_loc * 2^shard_log + rank]; (cols, b_loc, n, 32)."""
    return np.ascontiguousarray(lde_natural(nat, blowup, shard_log, rank).transpose(0, 2, 1, 3))


# ---------------------------------------------------------------------------------------------- comparison
def first_difference(got, want, order):
    """None when equal; else (column, coset, index) of the first differing element in the flat device order.  Arrays as
    lde_natural / lde_coset_major return them: order "natural" -> (cols, n, b_loc, 32), "coset_major" -> (cols, b_loc, n, 32); the
    inverse driver's (batch, n, 32) compares as coset_major with one coset."""
    got, want = np.asarray(got), np.asarray(want)
    if got.ndim == 3:
        got, want = got[:, None], want[:, None]
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got != want).any(axis=-1)
    if not bad.any():
        return None
    col, a, b = (int(t) for t in np.argwhere(bad)[0])
    return (col, b, a) if order == "natural" else (col, a, b)


def assert_same(got, want, order, what=""):
    d = first_difference(got, want, order)
    if d is not None:
        bad = int((np.asarray(got) != np.asarray(want)).any(axis=-1).sum())
        raise AssertionError(f"{what}: first difference at (column, coset, index) = {d}; {bad} elements differ")
