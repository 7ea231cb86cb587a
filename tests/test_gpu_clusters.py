"""Near-duplicate clusters on the device (run on an MI355X: python -m pytest tests -m gpu): the union-find kernels of
datasketch_amd/csrc/cc_kernels.hip through the mhx_cc_*_dev entries, and what is built on them -- lsh_bulk.connected_components,
lsh_bulk.duplicate_clusters, SortedBandsIndex.clusters, MinHashLSH.duplicate_clusters.

labels[i] is the smallest row of i's component: one answer whatever order the lanes ran in, so every result is compared for
exact equality with the host twin (scipy's connected_components relabelled to the smallest member).  Each case runs once.  Device
outputs are filled with 0xA5 bytes first and carry SPARE elements behind the end, which must still hold the fill afterwards.
The module has a Context of its own, so that a failing test cannot leave "debug.cus" set for the others."""
import ctypes

import numpy as np
import pytest

from datasketch_amd import MinHashLSH, _native, lsh_bulk
from tests.test_clusters_host import chain_index, checked_corpus, two_row_key_index

pytestmark = pytest.mark.gpu

SPARE = 37
FILL = 0xA5
_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


@pytest.fixture(params=[1, 3], ids=["debug_cus_1", "debug_cus_3"])
def cus(ctx, request):
    ctx.set_option("debug.cus", request.param)
    yield request.param
    ctx.set_option("debug.cus", 0)


def _filled(ctx, count, dtype):
    nbytes = (count + SPARE) * np.dtype(dtype).itemsize
    buf = ctx.alloc(nbytes)
    buf.upload(np.full(nbytes, FILL, dtype=np.uint8))
    return buf


def _taken(buf, count, dtype):
    size = np.dtype(dtype).itemsize
    raw = buf.download((count + SPARE) * size, np.uint8)
    assert np.all(raw[count * size:] == FILL), "written past the end of the output"
    return raw[: count * size].view(dtype).copy()


def _twin(pairs, n):
    """The host twin over the edges that lie inside [0, n)."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    inside = ((pairs >= 0) & (pairs < n)).all(axis=1)
    return lsh_bulk.connected_components(pairs[inside], n, gpu_mode="disable"), int(np.count_nonzero(~inside))


def _link(ctx, n, pairs=None, counts=None, min_count=0, bands=None, count_invalid=True):
    """init, one link call per given kind, finish through the _dev entries: (labels int64 [n], invalid)."""
    d_labels = _filled(ctx, n, np.uint32)
    d_bad = ctx.to_device(np.zeros(1 + SPARE, dtype=np.int64))
    bad = d_bad.ptr if count_invalid else None
    ctx.cc_init_dev(d_labels.ptr, n)
    if pairs is not None:
        pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
        d_pairs = ctx.to_device(pairs)
        d_counts = None if counts is None else ctx.to_device(np.ascontiguousarray(counts, dtype=np.int32))
        ctx.cc_link_pairs_dev(d_labels.ptr, n, d_pairs.ptr if pairs.shape[0] else None, pairs.shape[0],
                              None if d_counts is None else d_counts.ptr, min_count, bad)
    if bands is not None:
        dig, rows = bands
        d_dig, d_rows = ctx.to_device(np.ascontiguousarray(dig, dtype=np.uint64)), ctx.to_device(np.ascontiguousarray(rows, dtype=np.uint32))
        ctx.cc_link_bands_dev(d_labels.ptr, n, d_dig.ptr, d_rows.ptr, dig.shape[1], dig.shape[0], bad)
    ctx.cc_finish_dev(d_labels.ptr, n)
    ctx.synchronize()
    counter = d_bad.download(1 + SPARE, np.int64)
    assert np.all(counter[1:] == 0), "written past the invalid counter"
    return _taken(d_labels, n, np.uint32).astype(np.int64), int(counter[0])


def _check_pairs(ctx, n, pairs):
    got, invalid = _link(ctx, n, pairs=pairs)
    want, want_invalid = _twin(pairs, n)
    assert np.array_equal(got, want) and invalid == want_invalid


# ------------------------------------------------------------------------------------------------------- link pairs + finish
def test_one_row(ctx):
    got, invalid = _link(ctx, 1, pairs=np.array([[0, 0]]))
    assert got.tolist() == [0] and invalid == 0


def test_no_pairs_gives_arange(ctx):
    got, invalid = _link(ctx, 1000, pairs=np.empty((0, 2), dtype=np.int64))
    assert np.array_equal(got, np.arange(1000)) and invalid == 0


def _path(n=4096):
    i = np.arange(n - 1, 0, -1, dtype=np.int64)
    return np.stack([i, i - 1], axis=1)


def test_path_from_the_far_end_gives_deep_chains(ctx):
    got, invalid = _link(ctx, 4096, pairs=_path())
    assert np.array_equal(got, np.zeros(4096, dtype=np.int64)) and invalid == 0


def test_path_with_shuffled_edges(ctx):
    pairs = _path()[np.random.RandomState(1).permutation(4095)]
    _check_pairs(ctx, 4096, pairs)
    assert _twin(pairs, 4096)[0].max() == 0


def test_star_whose_centre_is_the_largest_row(ctx):
    i = np.arange(4096, dtype=np.int64)
    got, invalid = _link(ctx, 4097, pairs=np.stack([i, np.full(4096, 4096)], axis=1))
    assert np.array_equal(got, np.zeros(4097, dtype=np.int64)) and invalid == 0


def test_complete_graph_on_one_wave(ctx):
    i, j = np.triu_indices(64, k=1)
    pairs = np.stack([i, j], axis=1) + 3  # rows 3 .. 66 of 70: the rows around them stay alone
    got, invalid = _link(ctx, 70, pairs=pairs)
    assert np.array_equal(got, np.array([0, 1, 2] + [3] * 64 + [67, 68, 69])) and invalid == 0


def _random_graph():
    rng = np.random.RandomState(2)
    pairs = rng.randint(0, 3000, size=(2000, 2)).astype(np.int64)
    again = pairs[rng.choice(2000, 2000 // 3, replace=False)][:, ::-1]
    return np.concatenate([pairs, again])[rng.permutation(2000 + 2000 // 3)]


def test_random_graph_with_duplicated_and_reversed_edges(ctx):
    _check_pairs(ctx, 3000, _random_graph())


def test_counts_below_min_count_are_no_edges(ctx):
    rng = np.random.RandomState(3)
    pairs = rng.randint(0, 3000, size=(2000, 2)).astype(np.int64)
    counts = rng.permutation(np.arange(2000) % 2 * 5 + 3).astype(np.int32)  # half 3, half 8
    got, invalid = _link(ctx, 3000, pairs=pairs, counts=counts, min_count=8)
    want = lsh_bulk.connected_components(pairs, 3000, keep=counts >= 8, gpu_mode="disable")
    assert np.array_equal(got, want) and invalid == 0
    assert not np.array_equal(want, lsh_bulk.connected_components(pairs, 3000, gpu_mode="disable"))
    # an edge the counts leave out is not looked at: its rows may be anything
    pairs[counts < 8] = -7
    got, invalid = _link(ctx, 3000, pairs=pairs, counts=counts, min_count=8)
    assert np.array_equal(got, want) and invalid == 0


def test_edges_outside_the_rows_are_skipped_and_counted(ctx):
    n = 3000
    good = _random_graph()
    bad = np.array([[-1, 5], [5, -1], [n, 7], [7, n], [-1, n], [n, n], [1 << 40, 0], [0, -(1 << 40)]], dtype=np.int64)
    pairs = np.concatenate([good[:1000], bad, good[1000:]])
    got, invalid = _link(ctx, n, pairs=pairs)
    want, _ = _twin(good, n)
    assert np.array_equal(got, want) and invalid == len(bad)
    got, invalid = _link(ctx, n, pairs=pairs, count_invalid=False)  # d_invalid NULL: skipped all the same
    assert np.array_equal(got, want) and invalid == 0


def test_host_form_and_connected_components(ctx):
    pairs = _random_graph()
    want, _ = _twin(pairs, 3000)
    labels, invalid = ctx.cc_pairs(pairs, 3000)
    assert labels.dtype == np.uint32 and np.array_equal(labels, want) and invalid == 0
    labels, invalid = ctx.cc_pairs(np.concatenate([pairs, [[3000, 0]]]), 3000)
    assert np.array_equal(labels, want) and invalid == 1
    assert ctx.cc_pairs(np.empty((0, 2), dtype=np.int64), 0)[0].shape == (0,)
    assert ctx.cc_pairs(np.array([[0, 0]]), 0)[1] == 1
    got = lsh_bulk.connected_components(pairs, 3000, gpu_mode="always")
    assert got.dtype == np.int64 and np.array_equal(got, want)
    keep = np.random.RandomState(4).random_sample(len(pairs)) < 0.5
    assert np.array_equal(lsh_bulk.connected_components(pairs, 3000, keep=keep, gpu_mode="always"),
                          lsh_bulk.connected_components(pairs, 3000, keep=keep, gpu_mode="disable"))
    with pytest.raises(ValueError):
        lsh_bulk.connected_components(np.array([[0, 1], [2, 3000]]), 3000, gpu_mode="always")


# ------------------------------------------------------------------------------------------------------------------ link bands
def test_hand_made_bands(ctx):
    """bands = 3, n_sigs = 5.  Band 0 ends with digest 9 and band 1 begins with 9, rows 4 and 6: never compared.  Band 0 begins
    with a run (rows 0, 2); band 1 holds a run of three (5, 1, 3); band 2 ends with a run (7, 8)."""
    dig = np.array([[4, 4, 6, 7, 9],
                    [9, 11, 11, 11, 12],
                    [1, 2, 3, 5, 5]], dtype=np.uint64)
    rows = np.array([[0, 2, 1, 3, 4],
                     [6, 5, 1, 3, 9],
                     [0, 9, 4, 7, 8]], dtype=np.uint32)
    got, invalid = _link(ctx, 10, bands=(dig, rows))
    assert got.tolist() == [0, 1, 0, 1, 4, 1, 6, 7, 7, 9] and invalid == 0
    assert np.array_equal(got, lsh_bulk._components_host(*lsh_bulk._run_edges(dig, rows), 10))
    # rows >= n inside a run are invalid edges: n = 8 cuts (7, 8) off
    got, invalid = _link(ctx, 8, bands=(dig, rows))
    assert got.tolist() == [0, 1, 0, 1, 4, 1, 6, 7] and invalid == 1


def test_identical_rows_cost_links_not_pairs(ctx):
    """20 000 identical rows, b = 2: the pair form would need 2 x 10^8 pairs; the run form links 2 x 19 999 neighbours."""
    sig = np.tile(np.arange(1, 9, dtype=np.uint64), (20000, 1))
    labels = lsh_bulk.duplicate_clusters(sig, 2, 4, gpu_mode="always")
    assert labels.dtype == np.int64 and labels.shape == (20000,) and not labels.any()


# ------------------------------------------------------------------------------------------------------------------ end to end
_WANT = {}


def _want_labels(threshold):
    if threshold not in _WANT:
        sig, b, r = checked_corpus()
        _WANT[threshold] = lsh_bulk.duplicate_clusters(sig, b, r, threshold=threshold, gpu_mode="disable")
    return _WANT[threshold]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("threshold", [None, 0.5, 0.75])
def test_corpus_clusters_match_the_host(threshold, dtype):
    sig, b, r = checked_corpus(dtype)
    want = _want_labels(threshold)
    assert np.array_equal(lsh_bulk.duplicate_clusters(sig, b, r, threshold=threshold, gpu_mode="always"), want)
    assert np.array_equal(lsh_bulk.SortedBandsIndex(sig, b, r).clusters(threshold), want)
    lsh = MinHashLSH(num_perm=16, params=(b, r), gpu_mode="always")
    lsh.insert_bulk(list(range(len(sig))), sig)
    order = np.argsort(want, kind="stable")
    cuts = np.flatnonzero(np.diff(want[order])) + 1
    assert lsh.duplicate_clusters(threshold, min_size=1) == [part.tolist() for part in np.split(order, cuts)]


def test_weighted_matrix_without_threshold():
    rng = np.random.RandomState(5)
    base = rng.randint(0, 1 << 20, (40, 8, 2)).astype(np.int64)
    sig = base[rng.randint(0, 40, 200)]
    redraw = rng.random_sample((200, 8)) < 0.3
    sig[redraw] = rng.randint(0, 1 << 20, (int(redraw.sum()), 2))
    want = lsh_bulk.duplicate_clusters(sig, 4, 2, gpu_mode="disable")
    assert 1 < np.count_nonzero(want == np.arange(200)) < 200
    assert np.array_equal(lsh_bulk.duplicate_clusters(sig, 4, 2, gpu_mode="always"), want)
    with pytest.raises(ValueError):
        lsh_bulk.duplicate_clusters(sig, 4, 2, threshold=0.5, gpu_mode="always")


def test_lsh_chain_and_two_row_key_on_the_device():
    lsh = chain_index("always")
    assert lsh.duplicate_clusters() == [["A", "B", "C"]]
    assert lsh.duplicate_clusters(threshold=0.5) == []
    lsh.remove("B")
    assert lsh.duplicate_clusters() == []
    assert lsh.duplicate_clusters(min_size=1) == [["A"], ["C"]]
    lsh = two_row_key_index("always")
    assert lsh.duplicate_clusters() == [["P", "Q", "R", "S", "X"]]
    assert lsh.duplicate_clusters(min_size=1) == [["P", "Q", "R", "S", "X"], ["lone"]]
    lsh.remove("X")
    assert lsh.duplicate_clusters() == [["P", "Q"], ["R", "S"]]


# ------------------------------------------------------------------------------------------------------------------ later trips
def _per_trip(cus):
    return cus * 16 * 256  # grid_for(ctx, items): min(ceil(items / 256), CUs * 16) workgroups of 256 threads, one item each


def test_link_pairs_beyond_the_first_trip(ctx, cus):
    """cc_link_pairs_kernel (launch_cc_link_pairs): grid = grid_for(n_pairs) = min(ceil(n_pairs / 256), CUs * 16) workgroups of
    256 threads, one pair per thread and trip: 4 096 pairs per trip at one CU, 12 288 at three.  2 x that + 1 pairs: three
    trips, the last with one pair."""
    m = 2 * _per_trip(cus) + 1
    rng = np.random.RandomState(10 + cus)
    pairs = rng.randint(0, 20000, size=(m, 2)).astype(np.int64)
    pairs[-1] = (19999, 0)  # the one pair of the last trip decides a label
    _check_pairs(ctx, 20000, pairs)
    assert _twin(pairs, 20000)[0][19999] == 0


def test_link_bands_beyond_the_first_trip(ctx, cus):
    """cc_link_bands_kernel (launch_cc_link_bands): grid = grid_for(bands * n_sigs), one position per thread and trip: 4 096
    positions per trip at one CU, 12 288 at three.  3 x 2 731 = 8 193 positions (one CU) and 7 x 3 511 = 24 577 (three) are
    2 x that + 1: three trips, the last with the last position of the last band, which closes a run."""
    bands, n = {1: (3, 2731), 3: (7, 3511)}[cus]
    assert bands * n == 2 * _per_trip(cus) + 1
    sig = np.random.RandomState(20 + cus).randint(0, 40, size=(n, bands), dtype=np.uint64)  # runs of about n / 40 rows
    dig, rows = lsh_bulk.sorted_bands(sig, bands, 1, gpu_mode="disable")
    assert dig[-1, -1] == dig[-1, -2]
    got, invalid = _link(ctx, n, bands=(dig, rows))
    assert np.array_equal(got, lsh_bulk._components_host(*lsh_bulk._run_edges(dig, rows), n)) and invalid == 0


def test_init_and_finish_beyond_the_first_trip(ctx, cus):
    """cc_init_kernel and cc_finish_kernel (launch_cc_init, launch_cc_finish): grid = grid_for(n), one label per thread and trip:
    4 096 labels per trip at one CU, 12 288 at three; n = 2 x that + 1.  The edges tie the one label of the last trip to one of
    the first trip through one of the second."""
    per = _per_trip(cus)
    n = 2 * per + 1
    pairs = np.array([[n - 1, per + 5], [per + 5, 7], [per - 1, per], [2 * per - 1, 2 * per - 2]], dtype=np.int64)
    got, invalid = _link(ctx, n, pairs=pairs)
    want = np.arange(n)
    want[[n - 1, per + 5]] = 7
    want[per] = per - 1
    want[2 * per - 1] = 2 * per - 2
    assert np.array_equal(got, want) and invalid == 0


# -------------------------------------------------------------------------------------------------------------------- arguments
def _invalid(rc):
    assert rc == _native.MHX_ERR_INVALID and _native.last_error(), (rc, _native.last_error())


def test_arguments(ctx):
    lib, h = ctx.lib, ctx.handle
    d = ctx.to_device(np.zeros(64, dtype=np.int64))
    p, null = _vp(d.ptr), None
    for n in (-1, 1 << 32):
        _invalid(lib.mhx_cc_init_dev(h, p, n))
        _invalid(lib.mhx_cc_finish_dev(h, p, n))
        _invalid(lib.mhx_cc_link_pairs_dev(h, p, n, p, 1, null, 0, null))
        _invalid(lib.mhx_cc_link_bands_dev(h, p, n, p, p, 1, 1, null))
        _invalid(lib.mhx_cc_pairs(h, p, 0, null, 0, n, p, None))
    _invalid(lib.mhx_cc_link_pairs_dev(h, p, 4, p, -1, null, 0, null))
    _invalid(lib.mhx_cc_link_bands_dev(h, p, 4, p, p, 4, -1, null))
    _invalid(lib.mhx_cc_link_bands_dev(h, p, 4, p, p, -1, 1, null))
    _invalid(lib.mhx_cc_pairs(h, null, -1, null, 0, 4, p, None))
    # NULL with a non-zero size
    _invalid(lib.mhx_cc_init_dev(h, null, 4))
    _invalid(lib.mhx_cc_finish_dev(h, null, 4))
    _invalid(lib.mhx_cc_link_pairs_dev(h, null, 4, p, 1, null, 0, null))
    _invalid(lib.mhx_cc_link_pairs_dev(h, p, 4, null, 1, null, 0, null))
    _invalid(lib.mhx_cc_link_bands_dev(h, null, 4, p, p, 4, 1, null))
    _invalid(lib.mhx_cc_link_bands_dev(h, p, 4, null, p, 4, 1, null))
    _invalid(lib.mhx_cc_link_bands_dev(h, p, 4, p, null, 4, 1, null))
    host = np.zeros(8, dtype=np.int64)
    _invalid(lib.mhx_cc_pairs(h, null, 1, null, 0, 4, _vp(host.ctypes.data), None))
    _invalid(lib.mhx_cc_pairs(h, _vp(host.ctypes.data), 1, null, 0, 4, null, None))
    _invalid(lib.mhx_cc_init_dev(None, p, 4))
    # NULL with size 0 is accepted
    for rc in (lib.mhx_cc_init_dev(h, null, 0), lib.mhx_cc_finish_dev(h, null, 0), lib.mhx_cc_link_pairs_dev(h, p, 4, null, 0, null, 0, null),
               lib.mhx_cc_link_pairs_dev(h, null, 0, null, 0, null, 0, null), lib.mhx_cc_link_bands_dev(h, p, 4, null, null, 0, 3, null),
               lib.mhx_cc_link_bands_dev(h, p, 4, null, null, 4, 0, null), lib.mhx_cc_pairs(h, null, 0, null, 0, 0, null, None)):
        assert rc == _native.MHX_OK
    ctx.synchronize()
