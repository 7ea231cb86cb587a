"""Weighted Jaccard of every pair, the numpy path (gpu_mode="disable"): lsh_bulk.weighted_jaccard_pairs / _matrix,
weighted_similar_pairs, weighted_nearest_neighbors, weighted_duplicate_clusters and the weighted MinHashLSH methods against a
brute-force loop over WeightedMinHash.jaccard (ref: datasketch/weighted_minhash.py:45-60) on real signatures, and on a hand-made
matrix of near misses whose counts are known: count(x, y) is the number of samples at which BOTH int64 values agree."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import MinHash, MinHashLSH, WeightedMinHash, WeightedMinHashGenerator, _native, lsh_bulk
from tests.weighted_jaccard_guard_cases import NEAR_MISS_EQUAL, NEAR_MISS_ROWS, near_miss_matrix, planted_weighted

S = 16


def test_header_declares_the_bound_weighted_jaccard_symbols_and_the_library_exports_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mhx_weighted_jaccard.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_WJ\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_WJ == sorted(_native._PROTOTYPES_WJ) and len(declared) == 8
    assert sum(name.endswith("_dev") for name in declared) == 4
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    for other in ("", "_EXT", "_BLOOM", "_TOPK", "_CC", "_SHINGLE", "_WORDS", "_OVERLAP", "_XXH"):
        assert not set(declared) & set(getattr(_native, "EXPORTED_SYMBOLS" + other))
    main = open(os.path.join(root, "include", "mhx.h")).read()
    assert '#include "mhx_weighted_jaccard.h"' in main


@pytest.fixture(scope="module")
def corpus():
    """40 real signatures: 8 base vectors, each with four perturbed copies (a few coordinates rescaled)."""
    rng = np.random.RandomState(5)
    gen = WeightedMinHashGenerator(dim=32, sample_size=S, seed=3, gpu_mode="disable")
    base = rng.uniform(0.1, 5.0, size=(8, 32))
    vecs = []
    for v in base:
        vecs.append(v)
        for copies in range(4):
            w = v.copy()
            touched = rng.choice(32, size=1 + 2 * copies, replace=False)
            w[touched] *= rng.uniform(0.5, 2.0, size=touched.size)
            vecs.append(w)
    objs = [gen.minhash(v) for v in vecs]
    sig = np.stack([o.hashvalues for o in objs]).astype(np.int64)
    brute = np.array([[x.jaccard(y) for y in objs] for x in objs])
    return objs, sig, brute


def _brute_topk(jac, k, self_join=False, threshold=None, live=None):
    rows, vals = np.full((jac.shape[0], k), -1, dtype=np.int64), np.full((jac.shape[0], k), np.nan)
    for i in range(jac.shape[0]):
        cand = [(-jac[i, j], j) for j in range(jac.shape[1])
                if not (self_join and i == j) and (threshold is None or jac[i, j] >= threshold) and (live is None or live[j])]
        for e, (neg, j) in enumerate(sorted(cand)[:k]):
            rows[i, e], vals[i, e] = j, -neg
    return rows, vals


def test_every_function_equals_the_loop_over_weighted_minhash_jaccard(corpus):
    objs, sig, brute = corpus
    assert 0 < np.count_nonzero((brute > 0) & (brute < 1)), "the corpus has partial agreement"
    # matrix: from the array and from the objects, A with B and A with itself
    assert np.array_equal(lsh_bulk.weighted_jaccard_matrix(sig, gpu_mode="disable"), brute)
    assert np.array_equal(lsh_bulk.weighted_jaccard_matrix(objs[:7], objs[5:], gpu_mode="disable"), brute[:7, 5:])
    assert np.array_equal(lsh_bulk.weighted_jaccard_matrix(sig[:7], objs[5:], gpu_mode="disable"), brute[:7, 5:])
    # listed pairs: the new keyword changes nothing
    pairs = np.array([(i, j) for i in range(0, 40, 3) for j in range(40)], dtype=np.int64)
    want = brute[pairs[:, 0], pairs[:, 1]]
    assert np.array_equal(lsh_bulk.weighted_jaccard_pairs(sig, pairs, gpu_mode="disable"), want)
    assert np.array_equal(lsh_bulk.weighted_jaccard_pairs(sig, pairs), want)
    # thresholded pairs
    for threshold in (0.25, 0.5):
        got_pairs, got_jac = lsh_bulk.weighted_similar_pairs(sig, threshold=threshold, gpu_mode="disable")
        want_pairs = [(i, j) for i in range(40) for j in range(i + 1, 40) if brute[i, j] >= threshold]
        assert got_pairs.dtype == np.int64 and got_pairs.tolist() == [list(p) for p in want_pairs] and len(want_pairs) > 0
        assert got_jac.tolist() == [brute[i, j] for i, j in want_pairs]
        got_pairs, got_jac = lsh_bulk.weighted_similar_pairs(objs[:9], sig[4:], threshold=threshold, gpu_mode="disable")
        want_pairs = [(i, j) for i in range(9) for j in range(36) if brute[i, 4 + j] >= threshold]
        assert got_pairs.tolist() == [list(p) for p in want_pairs] and got_jac.tolist() == [brute[i, 4 + j] for i, j in want_pairs]
    # nearest neighbours
    rows, jac = lsh_bulk.weighted_nearest_neighbors(sig[:6], sig, k=7, gpu_mode="disable")
    brows, bjac = _brute_topk(brute[:6], 7)
    assert np.array_equal(rows, brows) and np.array_equal(jac, bjac)
    rows, jac = lsh_bulk.weighted_nearest_neighbors(objs, k=5, threshold=0.75, gpu_mode="disable")
    brows, bjac = _brute_topk(brute, 5, self_join=True, threshold=0.75)
    assert np.array_equal(rows, brows) and np.array_equal(jac, bjac, equal_nan=True)
    assert np.any(rows == -1) and np.any(rows >= 0) and np.all(rows != np.arange(40)[:, None])


def test_near_misses_count_exactly_the_samples_the_definition_counts():
    rows = near_miss_matrix()
    s = rows.shape[1]
    objs = [WeightedMinHash(1, r) for r in rows]
    for j, name in enumerate(NEAR_MISS_ROWS):
        want = s if j == 0 else NEAR_MISS_EQUAL
        assert objs[0].jaccard(objs[j]) == want / s, name
        # what a compare of the [N, 2 S] words would count: more than the definition for the rows that share one word of a sample
        words = np.count_nonzero(rows[0].reshape(-1) == rows[j].reshape(-1))
        assert words == 2 * want + (s - 2 if name in ("k only", "t only", "bit 40 of k", "sign of t") else 0), name
    full = lsh_bulk.weighted_jaccard_matrix(rows, gpu_mode="disable")
    assert full[0].tolist() == [1.0] + [NEAR_MISS_EQUAL / s] * 6
    assert np.array_equal(full, np.array([[x.jaccard(y) for y in objs] for x in objs]))
    pairs = np.stack([np.zeros(7, dtype=np.int64), np.arange(7)], axis=1)
    assert lsh_bulk.weighted_jaccard_pairs(rows, pairs, gpu_mode="disable").tolist() == full[0].tolist()
    got_pairs, got_jac = lsh_bulk.weighted_similar_pairs(rows[:1], rows, threshold=(NEAR_MISS_EQUAL + 1) / s, gpu_mode="disable")
    assert got_pairs.tolist() == [[0, 0]] and got_jac.tolist() == [1.0]
    near, jac = lsh_bulk.weighted_nearest_neighbors(rows[:1], rows[1:], k=6, gpu_mode="disable")
    assert near.tolist() == [[0, 1, 2, 3, 4, 5]] and jac.tolist() == [[NEAR_MISS_EQUAL / s] * 6]  # all tied: by the smaller row


def test_threshold_edges():
    rng = np.random.RandomState(2)
    a, b = planted_weighted(rng, 6, 30, 12)
    counts = lsh_bulk._equal_samples(a[:, None], b[None])
    assert 0 < counts.max() < 12 or counts.max() == 12
    c = int(np.sort(counts.reshape(-1))[-5])
    assert c > 0
    for threshold, floor in ((c / 12.0, c), (0.0, 0), (1.0, 12), (1.0 + 1e-9, 13), (2.0, 13), (np.nextafter(c / 12.0, 1.0), c + 1)):
        pairs, jac = lsh_bulk.weighted_similar_pairs(a, b, threshold=threshold, gpu_mode="disable")
        want = np.argwhere(counts >= floor)
        assert pairs.tolist() == want.tolist(), threshold
        assert jac.tolist() == (counts[want[:, 0], want[:, 1]] / 12.0).tolist()
        rows, near = lsh_bulk.weighted_nearest_neighbors(a, b, k=30, threshold=threshold, gpu_mode="disable")
        assert [int(np.count_nonzero(r >= 0)) for r in rows] == np.count_nonzero(counts >= floor, axis=1).tolist()
    assert lsh_bulk.weighted_similar_pairs(a, b, threshold=0.0, gpu_mode="disable")[0].shape == (180, 2)


def test_topk_ties_self_join_and_padding():
    rng = np.random.RandomState(4)
    a = planted_weighted(rng, 3, 9, 4)[1]
    a[5] = a[2]
    a[7] = a[2]
    rows, jac = lsh_bulk.weighted_nearest_neighbors(a, k=3, gpu_mode="disable")
    assert rows[2, :2].tolist() == [5, 7] and rows[5, :2].tolist() == [2, 7] and rows[7, :2].tolist() == [2, 5]
    assert jac[2, :2].tolist() == [1.0, 1.0]
    assert np.all(rows != np.arange(9)[:, None])
    rows, jac = lsh_bulk.weighted_nearest_neighbors(a[:2], a[:2], k=5, gpu_mode="disable")
    assert rows.shape == (2, 5) and np.all(rows[:, 2:] == -1) and np.all(np.isnan(jac[:, 2:])) and np.all(rows[:, :2] >= 0)
    rows, jac = lsh_bulk.weighted_nearest_neighbors(a[:1], k=2, gpu_mode="disable")  # alone: nothing but padding
    assert rows.tolist() == [[-1, -1]] and np.all(np.isnan(jac))


def _planted_clusters(rng, groups=12, copies=4, s=12):
    base = planted_weighted(rng, 2, groups, s)[1]
    sig = np.repeat(base, copies, axis=0)
    other = planted_weighted(rng, 2, groups * copies, s)[1]
    redraw = rng.random_sample((groups * copies, s)) < 0.2
    redraw[::copies] = False
    sig[redraw] = other[redraw]
    return sig[rng.permutation(groups * copies)]


def test_clusters_are_the_components_of_the_filtered_candidate_pairs():
    sig = _planted_clusters(np.random.RandomState(8))
    n = sig.shape[0]
    for threshold in (0.5, 0.8, None):
        labels = lsh_bulk.weighted_duplicate_clusters(sig, 6, 2, threshold, gpu_mode="disable")
        pairs = lsh_bulk.candidate_pairs(sig, 6, 2, gpu_mode="disable")
        keep = None if threshold is None else lsh_bulk.weighted_jaccard_pairs(sig, pairs, gpu_mode="disable") >= threshold
        want = lsh_bulk.connected_components(pairs, n, keep=keep, gpu_mode="disable")
        assert labels.dtype == np.int64 and np.array_equal(labels, want), threshold
        assert 1 < np.unique(labels).size < n, threshold
    tight, loose = (lsh_bulk.weighted_duplicate_clusters(sig, 6, 2, t, gpu_mode="disable") for t in (0.95, 0.5))
    assert np.unique(tight).size > np.unique(loose).size  # the threshold decides
    objs = [WeightedMinHash(1, row) for row in sig]
    assert np.array_equal(lsh_bulk.weighted_duplicate_clusters(objs, 6, 2, 0.5, gpu_mode="disable"), loose)
    assert lsh_bulk.weighted_duplicate_clusters(sig[:0], 6, 2, 0.5, gpu_mode="disable").shape == (0,)


def _weighted_index(prepickle=False):
    rng = np.random.RandomState(9)
    sig = planted_weighted(rng, 2, 30, 32)[1]
    sig[12] = sig[3]
    sig[12, :4, 1] += 1  # row 12: 28 of 32 samples of row 3 -- the other four keep k and miss t
    lsh = MinHashLSH(threshold=0.5, num_perm=32, gpu_mode="disable", prepickle=prepickle)
    lsh.insert_bulk(["k%d" % i for i in range(30)], sig)
    return lsh, sig


@pytest.mark.parametrize("prepickle", [False, True])
def test_weighted_minhash_lsh_nearest_after_a_removal_and_a_key_inserted_twice(prepickle):
    lsh, sig = _weighted_index(prepickle)
    lsh.remove("k3")  # would be the best match of the probe below
    again = sig[20].copy()
    again[:16] = sig[3, :16]
    lsh.insert_bulk(["k7"], again[None], check_duplication=False)  # k7 owns two rows now; pending until the query flushes
    probe = sig[3:4]
    keys = ["k%d" % i for i in range(30)] + ["k7"]
    rows = np.concatenate([sig, again[None]])
    live = np.array([k != "k3" for k in keys])
    jac = np.array([[WeightedMinHash(1, probe[0]).jaccard(WeightedMinHash(1, r)) for r in rows]])
    brows, bjac = _brute_topk(jac, 31, live=live)
    want, seen = [], set()
    for r, c in zip(brows[0].tolist(), bjac[0].tolist()):
        if r >= 0 and keys[r] not in seen:
            seen.add(keys[r])
            want.append((keys[r], c))
    got = lsh.nearest_bulk(probe, 5)[0]
    assert got == want[:5]
    assert got[0] == ("k12", 28 / 32.0) and got[1] == ("k7", 0.5) and "k3" not in [k for k, _ in got]
    assert lsh.nearest(WeightedMinHash(1, probe[0]), 5) == got
    assert lsh.nearest_bulk(probe, 5, threshold=0.6)[0] == [("k12", 28 / 32.0)]
    assert [len(x) for x in lsh.nearest_bulk(sig[:4], 64 - 1)] == [29] * 4  # every live key, each once
    with pytest.raises(ValueError, match="must not exceed 64"):
        lsh.nearest_bulk(probe, 64)
    with pytest.raises(ValueError, match="Expecting minhash with length 32"):
        lsh.nearest_bulk(np.zeros((1, 8, 2), dtype=np.int64), 3)


def test_mixed_kinds_raise_either_way():
    lsh, sig = _weighted_index()
    with pytest.raises(ValueError, match="WeightedMinHash"):
        lsh.nearest_bulk(np.zeros((1, 32), dtype=np.uint64), 3)
    with pytest.raises(ValueError, match="WeightedMinHash"):
        lsh.nearest(MinHash(num_perm=32, gpu_mode="disable"), 3)
    plain = MinHashLSH(threshold=0.5, num_perm=32, gpu_mode="disable")
    plain.insert_bulk(["a", "b"], np.arange(64, dtype=np.uint64).reshape(2, 32))
    with pytest.raises(ValueError, match="WeightedMinHash"):
        plain.nearest_bulk(sig[:1], 3)
    with pytest.raises(ValueError, match="WeightedMinHash"):
        plain.nearest(WeightedMinHash(1, sig[0]), 3)
    empty = MinHashLSH(threshold=0.5, num_perm=32, gpu_mode="disable")
    assert empty.nearest_bulk(sig[:2], 3) == [[], []]


def test_weighted_minhash_lsh_duplicate_clusters_with_a_threshold():
    sig = _planted_clusters(np.random.RandomState(10), groups=8, copies=3, s=12)
    n = sig.shape[0]
    lsh = MinHashLSH(num_perm=12, params=(6, 2), gpu_mode="disable")
    lsh.insert_bulk(list(range(n)), sig)
    for threshold in (0.6, None):
        labels = lsh_bulk.weighted_duplicate_clusters(sig, 6, 2, threshold, gpu_mode="disable")
        want = sorted(sorted(np.flatnonzero(labels == root).tolist()) for root in np.unique(labels))
        got = lsh.duplicate_clusters(threshold=threshold, min_size=1)
        assert sorted(sorted(c) for c in got) == want, threshold
        assert 1 < len(got) < n
    lsh.remove(0)
    rest = lsh_bulk.weighted_duplicate_clusters(sig[1:], 6, 2, 0.6, gpu_mode="disable")
    want = sorted(sorted((1 + np.flatnonzero(rest == root)).tolist()) for root in np.unique(rest))
    assert sorted(sorted(c) for c in lsh.duplicate_clusters(threshold=0.6, min_size=1)) == want


def test_argument_errors(corpus):
    objs, sig, _ = corpus
    flat = np.zeros((3, 8), dtype=np.uint64)
    for call in (lambda x: lsh_bulk.weighted_jaccard_matrix(x, gpu_mode="disable"),
                 lambda x: lsh_bulk.weighted_similar_pairs(x, gpu_mode="disable"),
                 lambda x: lsh_bulk.weighted_nearest_neighbors(x, gpu_mode="disable"),
                 lambda x: lsh_bulk.weighted_duplicate_clusters(x, 2, 2, 0.5, gpu_mode="disable"),
                 lambda x: lsh_bulk.weighted_jaccard_matrix(sig, x, gpu_mode="disable")):
        with pytest.raises(ValueError, match=r"\[N, S, 2\]"):
            call(flat)
        with pytest.raises(ValueError, match=r"\[N, S, 2\]"):
            call(np.zeros((3, 8, 3), dtype=np.int64))
        with pytest.raises(ValueError, match=r"\[N, S, 2\]"):
            call([MinHash(num_perm=16, gpu_mode="disable")])
    with pytest.raises(ValueError, match=r"\[N, S, 2\]"):
        lsh_bulk.weighted_jaccard_pairs(flat, [(0, 1)], gpu_mode="disable")
    with pytest.raises(ValueError, match="pair index out of range"):
        lsh_bulk.weighted_jaccard_pairs(sig, [(0, 40)], gpu_mode="disable")
    with pytest.raises(ValueError, match="different numbers of hash values"):
        lsh_bulk.weighted_jaccard_matrix(sig, np.zeros((3, S + 1, 2), dtype=np.int64), gpu_mode="disable")
    other_seed = WeightedMinHash(objs[0].seed + 1, objs[0].hashvalues)
    short = WeightedMinHash(objs[0].seed, objs[0].hashvalues[:4])
    with pytest.raises(ValueError, match="WeightedMinHash objects with different seeds"):
        lsh_bulk.weighted_jaccard_matrix(objs[:3], [other_seed], gpu_mode="disable")
    with pytest.raises(ValueError, match="WeightedMinHash objects with different seeds"):
        lsh_bulk.weighted_nearest_neighbors([objs[0], other_seed], gpu_mode="disable")
    with pytest.raises(ValueError, match="WeightedMinHash objects with different numbers of hash values"):
        lsh_bulk.weighted_similar_pairs([objs[0], short], gpu_mode="disable")
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            lsh_bulk.weighted_nearest_neighbors(sig, k=k, gpu_mode="disable")
    with pytest.raises(ValueError, match=r"b\*r must be in"):
        lsh_bulk.weighted_duplicate_clusters(sig, 9, 2, 0.5, gpu_mode="disable")
    for call in (lambda: lsh_bulk.weighted_jaccard_pairs(sig, [(0, 1)], gpu_mode="never"),
                 lambda: lsh_bulk.weighted_jaccard_matrix(sig, gpu_mode="never"),
                 lambda: lsh_bulk.weighted_similar_pairs(sig, gpu_mode="never"),
                 lambda: lsh_bulk.weighted_nearest_neighbors(sig, gpu_mode="never"),
                 lambda: lsh_bulk.weighted_duplicate_clusters(sig, 4, 2, 0.5, gpu_mode="never")):
        with pytest.raises(ValueError, match="gpu_mode"):
            call()
    # empty inputs, as the unweighted functions answer them
    none = sig[:0]
    assert lsh_bulk.weighted_jaccard_matrix(none, sig, gpu_mode="disable").shape == (0, 40)
    assert lsh_bulk.weighted_jaccard_matrix(sig, none, gpu_mode="disable").shape == (40, 0)
    assert lsh_bulk.weighted_similar_pairs(none, sig, gpu_mode="disable")[0].shape == (0, 2)
    assert lsh_bulk.weighted_jaccard_pairs(sig, np.empty((0, 2), dtype=np.int64), gpu_mode="disable").shape == (0,)
    empty = lsh_bulk.weighted_nearest_neighbors(none, sig, k=4, gpu_mode="disable")
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4)
    nothing = lsh_bulk.weighted_nearest_neighbors(sig, none, k=4, gpu_mode="disable")
    assert np.all(nothing[0] == -1) and np.all(np.isnan(nothing[1]))
