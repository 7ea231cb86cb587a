"""Near-duplicate clusters, the numpy path (gpu_mode="disable"): lsh_bulk.connected_components against a union-find written
here, lsh_bulk.duplicate_clusters against connected_components of the candidate pairs on a corpus whose figures are pinned,
and MinHashLSH.duplicate_clusters on the host back end.  labels[i] is the smallest row of i's component: a unique answer, so
everything is compared for exact equality."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import MinHash, MinHashLSH, _native, lsh_bulk


def union_find(pairs, n):
    """labels[i] = the smallest row of i's component, by the textbook algorithm."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in np.asarray(pairs, dtype=np.int64).reshape(-1, 2).tolist():
        ru, rv = find(u), find(v)
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def random_graph(seed, n, m):
    return np.random.RandomState(seed).randint(0, n, size=(m, 2)).astype(np.int64)


def checked_corpus(dtype=np.uint64):
    """3000 rows of 16 values drawn from 300 base rows with 35 % of the positions redrawn; bands 8 x 2."""
    rng = np.random.RandomState(0)
    n, k = 3000, 16
    base = rng.randint(0, 1 << 32, (300, k), dtype=np.uint64)
    sig = base[rng.randint(0, 300, n)]
    redraw = rng.random_sample((n, k)) < 0.35
    sig[redraw] = rng.randint(0, 1 << 32, int(redraw.sum()), dtype=np.uint64)
    return sig.astype(dtype), 8, 2


def test_header_declares_the_bound_cc_symbols_and_the_library_exports_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_CC\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_CC == sorted(_native._PROTOTYPES_CC) and len(declared) == 5
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)


@pytest.mark.parametrize("n", [1, 5])
def test_no_pairs_leaves_every_row_alone(n):
    labels = lsh_bulk.connected_components(np.empty((0, 2), dtype=np.int64), n, gpu_mode="disable")
    assert labels.dtype == np.int64 and np.array_equal(labels, np.arange(n))


@pytest.mark.parametrize("n,m", [(300, 200), (1000, 700), (64, 2016)])
def test_random_graphs_match_the_union_find(n, m):
    pairs = random_graph(n + m, n, m)
    labels = lsh_bulk.connected_components(pairs, n, gpu_mode="disable")
    assert labels.dtype == np.int64 and labels.shape == (n,)
    assert np.array_equal(labels, union_find(pairs, n))
    assert np.all(labels <= np.arange(n)) and np.array_equal(labels[labels], labels)


def test_order_loops_and_duplicates_do_not_matter():
    pairs = random_graph(5, 400, 250)
    want = union_find(pairs, 400)
    messy = np.concatenate([pairs[::-1, ::-1], pairs[::3], np.stack([np.arange(0, 400, 7)] * 2, axis=1), [[399, 0], [0, 399]]])
    assert np.any(messy[:, 0] > messy[:, 1]) and np.any(messy[:, 0] == messy[:, 1])
    assert np.array_equal(lsh_bulk.connected_components(messy, 400, gpu_mode="disable"), union_find(messy, 400))
    assert np.array_equal(lsh_bulk.connected_components(pairs[::-1, ::-1], 400, gpu_mode="disable"), want)


def test_keep_mask_selects_the_edges():
    pairs = random_graph(6, 500, 600)
    keep = np.random.RandomState(7).random_sample(600) < 0.4
    labels = lsh_bulk.connected_components(pairs, 500, keep=keep, gpu_mode="disable")
    assert np.array_equal(labels, union_find(pairs[keep], 500))
    assert not np.array_equal(labels, union_find(pairs, 500))
    with pytest.raises(ValueError):
        lsh_bulk.connected_components(pairs, 500, keep=keep[:-1], gpu_mode="disable")


@pytest.mark.parametrize("bad", [[3, 10], [-1, 2], [10, 10]])
def test_out_of_range_pair_raises(bad):
    with pytest.raises(ValueError):
        lsh_bulk.connected_components(np.array([[0, 1], bad]), 10, gpu_mode="disable")
    with pytest.raises(ValueError):
        lsh_bulk.connected_components(np.empty((0, 2), dtype=np.int64), -1, gpu_mode="disable")


def test_duplicate_clusters_on_the_checked_corpus():
    sig, b, r = checked_corpus()
    n = sig.shape[0]
    pairs = lsh_bulk.candidate_pairs(sig, b, r, gpu_mode="disable")
    dig, rows = lsh_bulk.sorted_bands(sig, b, r, gpu_mode="disable")
    same = dig[:, 1:] == dig[:, :-1]
    run_edges = np.stack([rows[:, :-1][same], rows[:, 1:][same]], axis=1).astype(np.int64)
    assert pairs.shape[0] == 11912 and run_edges.shape[0] == 7732

    by_pairs = union_find(pairs, n)
    assert np.array_equal(lsh_bulk.connected_components(pairs, n, gpu_mode="disable"), by_pairs)
    # linking predecessors inside the runs of the sorted bands gives the components of all the pairs of the runs
    assert np.array_equal(union_find(run_edges, n), by_pairs)
    got = lsh_bulk.duplicate_clusters(sig, b, r, gpu_mode="disable")
    assert got.dtype == np.int64 and np.array_equal(got, by_pairs)
    sizes = np.bincount(by_pairs)
    assert np.count_nonzero(sizes) == 335 and sizes.max() == 20

    jac = lsh_bulk.jaccard_pairs(sig, pairs, gpu_mode="disable")
    seen = [by_pairs]
    for threshold, components in ((0.5, 933), (0.75, 2896)):
        want = lsh_bulk.connected_components(pairs[jac >= threshold], n, gpu_mode="disable")
        assert np.array_equal(want, union_find(pairs[jac >= threshold], n))
        assert np.array_equal(lsh_bulk.connected_components(pairs, n, keep=jac >= threshold, gpu_mode="disable"), want)
        assert np.array_equal(lsh_bulk.duplicate_clusters(sig, b, r, threshold=threshold, gpu_mode="disable"), want)
        assert np.count_nonzero(want == np.arange(n)) == components
        assert all(not np.array_equal(want, other) for other in seen)
        seen.append(want)
    # uint32 rows are the same rows
    assert np.array_equal(lsh_bulk.duplicate_clusters(sig.astype(np.uint32), b, r, threshold=0.5, gpu_mode="disable"), seen[1])


def test_duplicate_clusters_weighted_and_arguments():
    rng = np.random.RandomState(3)
    base = rng.randint(0, 1 << 20, (40, 8, 2)).astype(np.int64)
    sig = base[rng.randint(0, 40, 200)]
    redraw = rng.random_sample((200, 8)) < 0.3
    sig[redraw] = rng.randint(0, 1 << 20, (int(redraw.sum()), 2))
    labels = lsh_bulk.duplicate_clusters(sig, 4, 2, gpu_mode="disable")
    want = union_find(lsh_bulk.candidate_pairs(sig, 4, 2, gpu_mode="disable"), 200)
    assert np.array_equal(labels, want) and 1 < np.count_nonzero(want == np.arange(200)) < 200
    with pytest.raises(ValueError):
        lsh_bulk.duplicate_clusters(sig, 4, 2, threshold=0.5, gpu_mode="disable")
    with pytest.raises(ValueError):
        lsh_bulk.duplicate_clusters(sig[:, :, 0], 5, 2, gpu_mode="disable")
    assert lsh_bulk.duplicate_clusters(np.empty((0, 8), dtype=np.uint64), 4, 2, gpu_mode="disable").shape == (0,)


# ---- MinHashLSH.duplicate_clusters: num_perm = 8, 4 bands of 2 ------------------------------------------------------------
def _mh(values):
    return MinHash(num_perm=8, hashvalues=np.asarray(values, dtype=np.uint64), gpu_mode="disable")


# A shares only band 0 with B, B only band 1 with C, A nothing with C
ROW_A = [1, 2, 10, 11, 12, 13, 14, 15]
ROW_B = [1, 2, 3, 4, 22, 23, 24, 25]
ROW_C = [30, 31, 3, 4, 32, 33, 34, 35]


def chain_index(gpu_mode, prepickle=False):
    lsh = MinHashLSH(num_perm=8, params=(4, 2), gpu_mode=gpu_mode, prepickle=prepickle)
    for key, row in (("A", ROW_A), ("B", ROW_B), ("C", ROW_C)):
        lsh.insert(key, _mh(row))
    return lsh


def two_row_key_index(gpu_mode):
    """Groups {P, Q} and {R, S} share nothing; key X is inserted twice, one row matching P and one matching R."""
    lsh = MinHashLSH(num_perm=8, params=(4, 2), gpu_mode=gpu_mode)
    rows = {"P": [100, 101, 1, 2, 3, 4, 5, 6], "Q": [100, 101, 7, 8, 9, 10, 11, 12], "lone": [90, 91, 92, 93, 94, 95, 96, 97],
            "R": [200, 201, 21, 22, 23, 24, 25, 26], "S": [200, 201, 27, 28, 29, 30, 31, 32]}
    for key, row in rows.items():
        lsh.insert(key, _mh(row))
    lsh.insert("X", _mh([40, 41, 1, 2, 42, 43, 44, 45]))
    lsh.insert("X", _mh([50, 51, 52, 53, 23, 24, 54, 55]), check_duplication=False)
    return lsh


def test_lsh_chain_is_one_cluster_until_the_middle_is_removed():
    lsh = chain_index("disable")
    assert lsh.duplicate_clusters() == [["A", "B", "C"]]
    # 2 of 8 positions agree along each link: not enough at 0.5
    assert lsh.duplicate_clusters(threshold=0.5) == []
    assert lsh.duplicate_clusters(threshold=0.25) == [["A", "B", "C"]]
    lsh.remove("B")
    assert lsh.duplicate_clusters() == []
    assert lsh.duplicate_clusters(min_size=1) == [["A"], ["C"]]


def test_lsh_key_with_two_rows_joins_both_groups():
    lsh = two_row_key_index("disable")
    assert lsh.duplicate_clusters() == [["P", "Q", "R", "S", "X"]]
    assert lsh.duplicate_clusters(min_size=1) == [["P", "Q", "R", "S", "X"], ["lone"]]
    lsh.remove("X")
    assert lsh.duplicate_clusters() == [["P", "Q"], ["R", "S"]]


def test_lsh_order_min_size_and_prepickle():
    lsh = MinHashLSH(num_perm=8, params=(4, 2), gpu_mode="disable", prepickle=True)
    rows = [((2, "late"), [9, 9, 1, 1, 2, 2, 3, 3]), (("solo",), [70, 71, 72, 73, 74, 75, 76, 77]), ((1, "first"), [5, 5, 6, 6, 7, 7, 8, 8]),
            ((2, "later"), [9, 9, 4, 4, 5, 6, 7, 8]), ((1, "second"), [5, 5, 16, 16, 17, 17, 18, 18])]
    for key, row in rows:
        lsh.insert(key, _mh(row))
    # clusters by their smallest slot, keys by slot, keys unpickled
    assert lsh.duplicate_clusters() == [[(2, "late"), (2, "later")], [(1, "first"), (1, "second")]]
    assert lsh.duplicate_clusters(min_size=1) == [[(2, "late"), (2, "later")], [("solo",)], [(1, "first"), (1, "second")]]
    assert lsh.duplicate_clusters(min_size=3) == []
    with pytest.raises(ValueError):
        lsh.duplicate_clusters(min_size=0)
    assert MinHashLSH(num_perm=8, params=(4, 2), gpu_mode="disable").duplicate_clusters() == []
