"""All-pairs Jaccard on the host (no GPU): lsh_bulk.jaccard_matrix / similar_pairs and their b-bit twins in
b_bit_minhash, numpy paths, against the per-object MinHash.jaccard / bBitMinHash.jaccard of the reference's API
(ref: datasketch/minhash.py:299-324, b_bit_minhash.py:53-72)."""
import numpy as np
import pytest

from datasketch_amd import LeanMinHash, MinHash, _native, b_bit_minhash, lsh_bulk
from datasketch_amd.b_bit_minhash import bBitMinHash


def _sketches(n, k, seed=1, rng_seed=0):
    """n MinHash objects of small sets drawn around a few shared cores, so that the overlaps are planted."""
    rng = np.random.RandomState(rng_seed)
    cores = [rng.randint(0, 400, size=30) for _ in range(3)]
    out = []
    for i in range(n):
        own = rng.randint(0, 400, size=rng.randint(5, 40))
        keep = cores[i % 3][rng.random_sample(30) < rng.uniform(0.2, 1.0)]
        m = MinHash(num_perm=k, seed=seed, gpu_mode="disable")
        for t in np.concatenate([own, keep]):
            m.update(b"tok%d" % t)
        out.append(m)
    return out


def test_jaccard_matrix_equals_minhash_jaccard_for_every_pair():
    ms = _sketches(23, 64)
    others = _sketches(9, 64, rng_seed=3)
    got = lsh_bulk.jaccard_matrix(ms, others, gpu_mode="disable")
    want = np.array([[x.jaccard(y) for y in others] for x in ms])
    assert got.dtype == np.float64 and got.shape == (23, 9)
    assert np.array_equal(got, want)
    assert 0.0 < want.max() and want.min() < 1.0
    # A against itself, from a uint32 matrix and from LeanMinHash objects
    sig32 = np.stack([m.hashvalues for m in ms]).astype(np.uint32)
    self_m = lsh_bulk.jaccard_matrix(sig32, gpu_mode="disable")
    assert np.array_equal(self_m, np.array([[x.jaccard(y) for y in ms] for x in ms]))
    lean = [LeanMinHash(m) for m in ms]
    assert np.array_equal(lsh_bulk.jaccard_matrix(lean, gpu_mode="disable"), self_m)


def test_jaccard_matrix_is_exact_on_the_high_word():
    a = np.array([[1, 2, 3, 4]], dtype=np.uint64)
    b = a.copy()
    b[0, 1] |= np.uint64(1) << np.uint64(40)
    assert lsh_bulk.jaccard_matrix(a, b, gpu_mode="disable")[0, 0] == 0.75


def test_similar_pairs_thresholds_on_the_grid_and_outside_it():
    k = 128
    rng = np.random.RandomState(5)
    base = rng.randint(0, 1 << 32, size=(1, k), dtype=np.uint64)
    sig = np.repeat(base, 40, axis=0)
    for i in range(40):  # row i has its first 3*i positions replaced
        sig[i, : 3 * i] = rng.randint(0, 1 << 32, size=3 * i, dtype=np.uint64) | np.uint64(1 << 33)
    objs = [MinHash(num_perm=k, seed=1, hashvalues=row, gpu_mode="disable") for row in sig]
    full = np.array([[x.jaccard(y) for y in objs] for x in objs])
    for t in (0.5, 64 / 128, 0.0, 0.3, 1.0, 1.5, -0.2, 0.7421875, 0.74219):
        pairs, jac = lsh_bulk.similar_pairs(sig, threshold=t, gpu_mode="disable")
        want = np.argwhere(np.triu(full >= t, k=1))
        assert np.array_equal(pairs, want), t
        assert np.array_equal(jac, full[want[:, 0], want[:, 1]]), t
    assert lsh_bulk.similar_pairs(sig, threshold=1.5, gpu_mode="disable")[0].shape == (0, 2)
    assert len(lsh_bulk.similar_pairs(sig, threshold=0.0, gpu_mode="disable")[0]) == 40 * 39 // 2
    # A against B: every (i, j), not only i < j
    pairs, jac = lsh_bulk.similar_pairs(sig[:7], sig[5:], threshold=0.5, gpu_mode="disable")
    sub = full[:7, 5:]
    want = np.argwhere(sub >= 0.5)
    assert np.array_equal(pairs, want) and np.array_equal(jac, sub[sub >= 0.5])


def test_the_fallback_in_blocks_agrees_with_one_block(monkeypatch):
    ms = _sketches(30, 32)
    sig = np.stack([m.hashvalues for m in ms])
    one = lsh_bulk.similar_pairs(sig, threshold=0.2, gpu_mode="disable")
    monkeypatch.setattr(lsh_bulk, "_FALLBACK_ELEMS", 64)  # one row of A per block
    many = lsh_bulk.similar_pairs(sig, threshold=0.2, gpu_mode="disable")
    assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1])
    assert np.array_equal(lsh_bulk.jaccard_matrix(sig, gpu_mode="disable"),
                          np.array([[x.jaccard(y) for y in ms] for x in ms]))


def test_mismatched_sketches_raise_the_reference_errors():
    a = _sketches(3, 64, seed=1)
    with pytest.raises(ValueError, match="different seeds"):
        lsh_bulk.jaccard_matrix(a, _sketches(2, 64, seed=2), gpu_mode="disable")
    with pytest.raises(ValueError, match="different numbers of permutation functions"):
        lsh_bulk.similar_pairs(a, _sketches(2, 32, seed=1), gpu_mode="disable")
    with pytest.raises(ValueError, match="different seeds"):
        lsh_bulk.jaccard_matrix(a + _sketches(1, 64, seed=9), gpu_mode="disable")
    with pytest.raises(ValueError, match="different numbers of permutation functions"):
        lsh_bulk.jaccard_matrix(np.zeros((2, 8), np.uint64), np.zeros((2, 9), np.uint64), gpu_mode="disable")
    with pytest.raises(ValueError):
        lsh_bulk.jaccard_matrix(np.zeros((2, 4, 2), np.int64), gpu_mode="disable")


@pytest.mark.parametrize("b", [1, 2, 3, 8, 32])
def test_bbit_estimates_equal_bbitminhash_jaccard(b):
    k = 100  # not a multiple of the values per block for any b
    ms = _sketches(12, k, rng_seed=b)
    sig = np.stack([m.hashvalues for m in ms])
    blocks = b_bit_minhash.pack_matrix(sig, b, gpu_mode="disable")
    for r_a, r_b in ((0.0, None), (0.3, 0.3), (0.2, 0.6)):
        rb = r_a if r_b is None else r_b
        full = np.array([[bBitMinHash(x, b, r_a).jaccard(bBitMinHash(y, b, rb)) for y in ms] for x in ms])
        got = b_bit_minhash.jaccard_matrix(blocks[:7], blocks, k, b, r=r_a, r_b=r_b, gpu_mode="disable")
        assert np.array_equal(got, full[:7]), (r_a, r_b)
        for t in (0.5, 0.25, float(full[0, 1]), 2.0):
            pairs, est = b_bit_minhash.similar_pairs(blocks, None, k, b, threshold=t, r=r_a, r_b=r_b, gpu_mode="disable")
            keep = np.argwhere(np.triu(full >= t, k=1))
            assert np.array_equal(pairs, keep), (r_a, r_b, t)
            assert np.array_equal(est, full[keep[:, 0], keep[:, 1]])


def test_bbit_argument_checks():
    blocks = np.zeros((3, 2), dtype=np.uint64)
    assert b_bit_minhash.jaccard_matrix(blocks, None, 100, 1, gpu_mode="disable").shape == (3, 3)  # 100 one-bit values: 2 blocks
    with pytest.raises(ValueError):
        b_bit_minhash.jaccard_matrix(blocks, None, 128, 33, gpu_mode="disable")
    with pytest.raises(ValueError):
        b_bit_minhash.similar_pairs(blocks, None, 300, 1, gpu_mode="disable")
    with pytest.raises(ValueError):
        b_bit_minhash.jaccard_matrix(blocks, None, 128, 1, r=1.5, gpu_mode="disable")


@pytest.mark.skipif(_native.gpu_node_present(), reason="host has a GPU")
def test_gpu_mode_always_raises_without_a_gpu():
    sig = np.zeros((4, 8), dtype=np.uint64)
    with pytest.raises(RuntimeError):
        lsh_bulk.jaccard_matrix(sig, gpu_mode="always")
    with pytest.raises(RuntimeError):
        lsh_bulk.similar_pairs(sig, threshold=0.5, gpu_mode="always")
    blocks = np.zeros((4, 2), dtype=np.uint64)
    with pytest.raises(RuntimeError):
        b_bit_minhash.jaccard_matrix(blocks, None, 128, 1, gpu_mode="always")
    with pytest.raises(RuntimeError):
        b_bit_minhash.similar_pairs(blocks, None, 128, 1, gpu_mode="always")
