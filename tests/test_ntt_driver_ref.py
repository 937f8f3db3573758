"""Anchors tests/ntt_driver_ref.py - the reference the GPU driver tests compare with - on direct sums in Python integers: Horner
evaluation of p(h w_N^i) and the inverse DFT sum, at every k <= 4, blowup <= 4, shard and rank; and shows that the comparison helper
names the first differing (column, coset, index) and rejects the outputs a wrong tile map would produce."""
import random

import numpy as np
import pytest

import ntt_driver_ref as ref

P = ref.P
H = 3


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def _felts(rng, *shape):
    vals = np.empty(shape, dtype=object)
    for idx in np.ndindex(*shape):
        vals[idx] = rng.choice((0, 1, P - 1, P - 2, rng.randrange(P), rng.randrange(P)))
    return vals


def _rev(x, k):
    return int(format(x, f"0{k}b")[::-1], 2) if k else 0


def _horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def test_roots_and_codec_against_python_integers(oracle):
    for log_order in (0, 1, 2, 5, 22):
        w = ref.root_of_unity(log_order)
        assert w == oracle.primitive_root(log_order)
        assert pow(w, 1 << log_order, P) == 1 and (log_order == 0 or pow(w, 1 << (log_order - 1), P) == P - 1)
    rng = random.Random(5)
    vals = [0, 1, P - 1, P - 2, 2**251, 2**192] + [rng.randrange(P) for _ in range(50)]
    be = np.stack([np.frombuffer(v.to_bytes(32, "big"), dtype=np.uint8) for v in vals])
    assert list(ref.to_ints(be)) == vals and np.array_equal(ref.to_bytes(ref.to_ints(be)), be)
    dev = ref.to_device(be)
    for v, rec in zip(vals, dev):
        limbs = [int.from_bytes(bytes(rec[4 * i:4 * i + 4]), "little") for i in range(8)]
        assert sum(l << (32 * i) for i, l in enumerate(limbs)) == v * 2**256 % P
    assert np.array_equal(ref.from_device(dev), be) and ref.canonical_violations(dev) == 0
    assert ref.canonical_violations(np.full((1, 32), 0xFF, dtype=np.uint8)) == 1
    for k in range(6):
        assert list(ref.bitrev(k)) == [_rev(i, k) for i in range(1 << k)]


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_inverse_driver_against_the_direct_inverse_dft_sum(k):
    rng = random.Random(40 + k)
    n, batch = 1 << k, 2
    x = _felts(rng, batch, n)
    post = _felts(rng, n)
    winv = pow(ref.root_of_unity(k), -1, P)
    # n c_j = sum_i x_i w^(-i j): the transform the driver leaves unscaled, at position pos = rev(j)
    unscaled = [[sum(int(x[v, i]) * pow(winv, i * j, P) for i in range(n)) % P for j in range(n)] for v in range(batch)]
    for table in (None, post):
        want = np.empty((batch, n), dtype=object)
        for v in range(batch):
            for pos in range(n):
                want[v, pos] = unscaled[v][_rev(pos, k)] * (1 if table is None else int(table[pos])) % P
        got = ref.inverse_driver(ref.to_bytes(x), None if table is None else ref.to_bytes(table))
        assert np.array_equal(got, ref.to_bytes(want)), (k, table is not None)


@pytest.mark.parametrize("blowup", [1, 2, 4])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_lde_maps_against_horner_for_every_shard_and_rank(k, blowup):
    rng = random.Random(100 * k + blowup)
    n, cols, N = 1 << k, 2, (1 << k) * blowup
    logb = blowup.bit_length() - 1
    coeffs = _felts(rng, cols, n)
    w = ref.root_of_unity(k + logb)
    direct = [[_horner([int(c) for c in coeffs[v]], H * pow(w, i, P) % P) for i in range(N)] for v in range(cols)]
    nat = ref.natural_evaluations(ref.to_bytes(coeffs), blowup, H)
    assert [list(ref.to_ints(nat[v])) for v in range(cols)] == direct
    # the input helper: entry pos = c[rev(pos)] h^rev(pos)
    inp = ref.to_ints(ref.lde_input(ref.to_bytes(coeffs), H))
    for v in range(cols):
        assert list(inp[v]) == [int(coeffs[v, _rev(pos, k)]) * pow(H, _rev(pos, k), P) % P for pos in range(n)]
    for shard_log in range(logb + 1):
        b_loc = blowup >> shard_log
        for rank in range(1 << shard_log):
            natural = ref.to_ints(ref.lde_natural(nat, blowup, shard_log, rank)).reshape(cols, n * b_loc)
            major = ref.to_ints(ref.lde_coset_major(nat, blowup, shard_log, rank)).reshape(cols, b_loc * n)
            for v in range(cols):
                for q in range(n):
                    for c_loc in range(b_loc):
                        want = direct[v][q * blowup + (c_loc << shard_log) + rank]
                        assert natural[v, q * b_loc + c_loc] == want, (shard_log, rank, v, q, c_loc)
                        assert major[v, c_loc * n + q] == want, (shard_log, rank, v, q, c_loc)


def test_post_table_of_round_one_turns_evaluations_into_lde_input():
    """interpolate, scale by h^j, bit-reverse: the inverse driver with post = h^rev(pos) / n leaves what lde_input builds from the
    coefficients (the prover's round-1 chain)."""
    rng = random.Random(77)
    for k in (0, 1, 3, 4):
        coeffs = ref.to_bytes(_felts(rng, 2, 1 << k))
        evals = np.stack([ref.oracle.ntt(c) for c in coeffs])
        assert np.array_equal(ref.inverse_driver(evals, ref.post_h_over_n(k, H)), ref.lde_input(coeffs, H))


def _example():
    rng = random.Random(9)
    nat = ref.natural_evaluations(ref.to_bytes(_felts(rng, 3, 8)), 4, H)      # 3 columns, n = 8, blowup 4
    return nat


def test_helper_names_the_first_differing_column_coset_index():
    nat = _example()
    want = ref.lde_coset_major(nat, 4)
    assert ref.first_difference(want.copy(), want, "coset_major") is None
    got = want.copy()
    got[1, 2, 5, 31] ^= 1
    got[2, 0, 0, 0] ^= 1
    assert ref.first_difference(got, want, "coset_major") == (1, 2, 5)
    with pytest.raises(AssertionError, match=r"\(column, coset, index\) = \(1, 2, 5\); 2 elements differ"):
        ref.assert_same(got, want, "coset_major", "example")
    want = ref.lde_natural(nat, 4, 1, 1)               # (cols, n, b_loc): flat order (q, c_loc)
    got = want.copy()
    got[0, 6, 1, 0] ^= 0x80
    assert ref.first_difference(got, want, "natural") == (0, 1, 6)
    inv = ref.inverse_driver(nat[:, :8])
    got = inv.copy()
    got[2, 7, 3] ^= 4
    assert ref.first_difference(got, inv, "coset_major") == (2, 0, 7)


def test_helper_rejects_swapped_cosets_a_wrong_rank_and_natural_order():
    nat = _example()
    want = ref.lde_coset_major(nat, 4)
    swapped = want.copy()
    swapped[:, [1, 2]] = want[:, [2, 1]]
    assert ref.first_difference(swapped, want, "coset_major") == (0, 1, 0)
    # rank off by one: rank 1's cosets where rank 0's belong
    want0 = ref.lde_coset_major(nat, 4, 1, 0)
    assert ref.first_difference(ref.lde_coset_major(nat, 4, 1, 1), want0, "coset_major") == (0, 0, 0)
    assert ref.first_difference(ref.lde_natural(nat, 4, 2, 3), ref.lde_natural(nat, 4, 2, 2), "natural") == (0, 0, 0)
    # left in natural order (q, c) instead of coset-major (c, m): same bytes, other places
    natural_flat = ref.lde_natural(nat, 4).reshape(want.shape)
    d = ref.first_difference(natural_flat, want, "coset_major")
    assert d is not None and d[0] == 0 and d[1] == 0 and d[2] == 1
    with pytest.raises(AssertionError):
        ref.assert_same(natural_flat, want, "coset_major", "natural order")
