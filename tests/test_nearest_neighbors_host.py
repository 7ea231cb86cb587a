"""Exact top-k Jaccard neighbours, the numpy path (gpu_mode="disable"): lsh_bulk.nearest_neighbors, its b-bit twin and
MinHashLSH.nearest / nearest_bulk against a brute-force sort of the packed keys (count << 32 | 0xFFFFFFFF - row), i.e. the best
k by (count descending, row ascending), padded with -1 / nan (ref for the measure: datasketch/minhash.py:299-324)."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import MinHash, MinHashLSH, _native, b_bit_minhash, lsh_bulk


def test_header_declares_the_bound_topk_symbols_and_the_library_exports_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_TOPK\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_TOPK == sorted(_native._PROTOTYPES_TOPK) and len(declared) == 4
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    assert int(re.search(r"#define MHX_TOPK_MAX (\d+)", text).group(1)) == _native.MHX_TOPK_MAX


def _planted(rng, m, n, k):
    """A [m, k] random; B [n, k] whose rows copy a row of A with a random number of positions replaced (many tied counts)."""
    a = rng.randint(0, 1 << 32, size=(m, k), dtype=np.uint64)
    b = rng.randint(0, 1 << 32, size=(n, k), dtype=np.uint64)
    src = rng.randint(0, m, size=n)
    for j in range(n):
        keep = rng.random_sample(k) < rng.random_sample()
        b[j, keep] = a[src[j], keep]
    return a, b


def _brute(a, b, k, min_count=0, self_join=False, live=None):
    counts = np.count_nonzero(a[:, None, :] == b[None, :, :], axis=2).astype(np.int64)
    n = b.shape[0]
    key = (counts.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(n, dtype=np.uint64))[None, :]
    ok = counts >= min_count
    if self_join:
        ok &= ~np.eye(n, dtype=bool)
    if live is not None:
        ok &= live[None, :]
    key[~ok] = 0
    top = np.sort(key, axis=1)[:, ::-1][:, :k]
    rows = np.full((a.shape[0], k), -1, dtype=np.int64)
    cnt = np.full((a.shape[0], k), -1, dtype=np.int64)
    have = top != 0
    rows[:, : top.shape[1]] = np.where(have, (np.uint64(0xFFFFFFFF) - (top & np.uint64(0xFFFFFFFF))).astype(np.int64), -1)
    cnt[:, : top.shape[1]] = np.where(have, (top >> np.uint64(32)).astype(np.int64), -1)
    return rows, cnt


def _same(got, rows, cnt, k_perm):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert np.array_equal(got[0], rows)
    assert np.array_equal(got[1], np.where(rows >= 0, cnt / float(k_perm), np.nan), equal_nan=True)


@pytest.mark.parametrize("m,n,k_perm,k", [(1, 1, 1, 1), (7, 63, 3, 10), (33, 200, 64, 10), (5, 300, 128, 64), (40, 9, 16, 10)])
def test_numpy_path_equals_a_sort_of_packed_keys(m, n, k_perm, k):
    rng = np.random.RandomState(m + n + k_perm)
    a, b = _planted(rng, m, n, k_perm)
    rows, cnt = _brute(a, b, k)
    if n > k and k_perm <= 16:
        assert np.any(cnt[:, k - 1] == _brute(a, b, k + 1)[1][:, k]), "the input has no tie at the k-th place"
    _same(lsh_bulk.nearest_neighbors(a, b, k=k, gpu_mode="disable"), rows, cnt, k_perm)
    if n < k:
        assert np.all(rows[:, n:] == -1) and np.all(rows[:, :n] >= 0)


def test_self_mode_never_reports_the_row_itself():
    rng = np.random.RandomState(2)
    a, _ = _planted(rng, 50, 1, 32)
    a[10] = a[40]  # a duplicate row j != i with count K
    rows, cnt = _brute(a, a, 5, self_join=True)
    got = lsh_bulk.nearest_neighbors(a, k=5, gpu_mode="disable")
    _same(got, rows, cnt, 32)
    assert not np.any(got[0] == np.arange(50)[:, None])
    assert got[0][10, 0] == 40 and got[0][40, 0] == 10 and got[1][10, 0] == 1.0


def test_threshold_cuts_the_lists_and_leaves_the_padding():
    rng = np.random.RandomState(3)
    a, b = _planted(rng, 20, 400, 64)
    rows, cnt = _brute(a, b, 10, min_count=32)
    got = lsh_bulk.nearest_neighbors(a, b, k=10, threshold=0.5, gpu_mode="disable")
    _same(got, rows, cnt, 64)
    assert np.any(rows == -1) and np.any(rows >= 0)
    assert np.all(got[1][rows >= 0] >= 0.5)
    none = lsh_bulk.nearest_neighbors(a, b, k=3, threshold=1.5, gpu_mode="disable")
    assert np.all(none[0] == -1) and np.all(np.isnan(none[1]))


def test_equals_minhash_jaccard_on_objects():
    sets = [[b"tok%d" % t for t in range(s, s + 40)] for s in (0, 5, 10, 20, 35, 200)]
    hashes = []
    for tokens in sets:
        mh = MinHash(num_perm=64, seed=3, gpu_mode="disable")
        mh.update_batch(tokens)
        hashes.append(mh)
    rows, jac = lsh_bulk.nearest_neighbors(hashes[:2], hashes, k=6, gpu_mode="disable")
    for i in range(2):
        want = sorted(((-hashes[i].jaccard(h), j) for j, h in enumerate(hashes)))
        assert rows[i].tolist() == [j for _, j in want]
        assert jac[i].tolist() == [-s for s, _ in want]


def test_errors_are_those_of_jaccard_matrix():
    a = np.zeros((3, 8), dtype=np.uint64)
    for k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            lsh_bulk.nearest_neighbors(a, k=k, gpu_mode="disable")
    with pytest.raises(ValueError, match="different numbers of permutation functions"):
        lsh_bulk.nearest_neighbors(a, np.zeros((3, 9), dtype=np.uint64), gpu_mode="disable")
    with pytest.raises(ValueError, match="WeightedMinHash"):
        lsh_bulk.nearest_neighbors(np.zeros((3, 8, 2), dtype=np.int64), gpu_mode="disable")
    m1, m2 = MinHash(num_perm=16, seed=1, gpu_mode="disable"), MinHash(num_perm=16, seed=2, gpu_mode="disable")
    with pytest.raises(ValueError, match="different seeds"):
        lsh_bulk.nearest_neighbors([m1], [m2], gpu_mode="disable")
    empty = lsh_bulk.nearest_neighbors(np.zeros((0, 8), np.uint64), a, k=4, gpu_mode="disable")
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4)
    nothing = lsh_bulk.nearest_neighbors(a, np.zeros((0, 8), np.uint64), k=4, gpu_mode="disable")
    assert np.all(nothing[0] == -1) and np.all(np.isnan(nothing[1]))


@pytest.mark.parametrize("bits", [1, 4])
def test_bbit_twin_ranks_by_agreeing_positions(bits):
    rng = np.random.RandomState(bits)
    a, b = _planted(rng, 9, 120, 100)
    mask = np.uint64((1 << bits) - 1)
    rows, cnt = _brute(a & mask, b & mask, 10)
    pa, pb = (b_bit_minhash.pack_matrix(x, bits, gpu_mode="disable") for x in (a, b))
    got = b_bit_minhash.nearest_neighbors(pa, pb, 100, bits, k=10, r=0.1, r_b=0.2, gpu_mode="disable")
    assert np.array_equal(got[0], rows)
    full = b_bit_minhash.jaccard_matrix(pa, pb, 100, bits, r=0.1, r_b=0.2, gpu_mode="disable")
    assert np.array_equal(got[1], np.take_along_axis(full, rows, axis=1))


def _index(prepickle=False):
    rng = np.random.RandomState(9)
    sig, _ = _planted(rng, 30, 1, 32)
    sig[12] = sig[3]
    sig[12, :4] += 1  # row 12: 28 of 32 positions of row 3
    lsh = MinHashLSH(threshold=0.5, num_perm=32, gpu_mode="disable", prepickle=prepickle)
    lsh.insert_bulk(["k%d" % i for i in range(30)], sig)
    return lsh, sig


@pytest.mark.parametrize("prepickle", [False, True])
def test_minhash_lsh_nearest_after_a_removal_and_a_key_inserted_twice(prepickle):
    lsh, sig = _index(prepickle)
    lsh.remove("k3")  # would be the best match of the probe below
    again = sig[20].copy()
    again[:16] = sig[3, :16]
    lsh.insert_bulk(["k7"], again[None, :], check_duplication=False)  # k7 owns two rows now; pending until the query flushes
    probe = sig[3:4]
    keys = ["k%d" % i for i in range(30)] + ["k7"]
    rows = np.concatenate([sig, again[None, :]])
    live = np.array([k != "k3" for k in keys])
    brows, bcnt = _brute(probe, rows, 31, live=live)
    want, seen = [], set()
    for r, c in zip(brows[0].tolist(), bcnt[0].tolist()):
        if r >= 0 and keys[r] not in seen:
            seen.add(keys[r])
            want.append((keys[r], c / 32.0))
    got = lsh.nearest_bulk(probe, 5)[0]
    assert got == want[:5]
    assert got[0] == ("k12", 28 / 32.0) and got[1] == ("k7", 0.5) and "k3" not in [k for k, _ in got]
    mh = MinHash(num_perm=32, hashvalues=probe[0], gpu_mode="disable")
    assert lsh.nearest(mh, 5) == got
    assert lsh.nearest_bulk(probe, 5, threshold=0.6)[0] == [("k12", 28 / 32.0)]
    assert [len(x) for x in lsh.nearest_bulk(sig[:4], 64 - 1)] == [29] * 4  # every live key, each once
    with pytest.raises(ValueError, match="must not exceed 64"):
        lsh.nearest_bulk(probe, 64)
    with pytest.raises(ValueError, match="Expecting minhash with length 32"):
        lsh.nearest_bulk(np.zeros((1, 8), dtype=np.uint64), 3)
    with pytest.raises(ValueError, match="WeightedMinHash"):
        lsh.nearest_bulk(np.zeros((1, 32, 2), dtype=np.int64), 3)


def test_minhash_lsh_nearest_on_an_empty_index():
    lsh = MinHashLSH(threshold=0.5, num_perm=32, gpu_mode="disable")
    assert lsh.nearest_bulk(np.zeros((2, 32), dtype=np.uint64), 3) == [[], []]
