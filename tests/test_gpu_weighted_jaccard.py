"""Weighted Jaccard on the MI355X through the C ABI (mhx_weighted_jaccard_*) and the Python layer above it: gpu_mode="always"
against the numpy definition in datasketch_amd/lsh_bulk.py (count(x, y) = the samples at which both int64 values of the (k, t)
pair agree, ref: datasketch/weighted_minhash.py:45-60), exact equality everywhere.  Shapes at the edges of the 128 x 128 tile
and of its 16-word LDS chunk (4 samples), both top-k kernels, the pair kernel below, at and above 64 samples."""
import ctypes

import numpy as np
import pytest

from datasketch_amd import MinHashLSH, _native, lsh_bulk
from tests.weighted_jaccard_guard_cases import (NEAR_MISS_EQUAL, near_miss_matrix, planted_weighted, want_matrix, want_pairs,
                                                want_threshold, want_topk)

pytestmark = pytest.mark.gpu

KMAX = _native.MHX_TOPK_MAX
EDGES = (1, 127, 128, 129, 257)
SAMPLES = (1, 3, 4, 5, 33, 128)


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    return _native.context()


@pytest.fixture
def options(ctx):
    def set_(path=0, segments=0, chunk=0):
        ctx.set_option("jaccard.topk_path", path)
        ctx.set_option("jaccard.topk_segments", segments)
        ctx.set_option("host.chunk_bytes", chunk)
    yield set_
    set_()


_CORPUS = {}


def _case(m, n, s):
    """The planted input of a shape and its counts, computed once for the module and never written to."""
    if (m, n, s) not in _CORPUS:
        a, b = planted_weighted(np.random.RandomState(1000 * s + 7 * m + n), m, n, s)
        counts = want_matrix(a, b)
        for x in (a, b, counts):
            x.setflags(write=False)
        _CORPUS[(m, n, s)] = (a, b, counts)
    return _CORPUS[(m, n, s)]


def _p(buf):
    return None if buf is None else buf.ptr


def _dev_matrix(ctx, a, b, ldc=None):
    m, n_b = a.shape[0], a.shape[0] if b is None else b.shape[0]
    ldc = n_b if ldc is None else ldc
    d_a, d_b = ctx.to_device(a), None if b is None else ctx.to_device(b)
    d_c = ctx.to_device(np.full(m * ldc + 5, -7, dtype=np.int32))
    ctx.weighted_jaccard_matrix_dev(d_a.ptr, m, _p(d_b), 0 if b is None else n_b, a.shape[1], d_c.ptr, ldc)
    out = d_c.download(m * ldc + 5, np.int32)
    assert np.all(out[m * ldc:] == -7), "written past the matrix"
    out = out[: m * ldc].reshape(m, ldc)
    assert np.all(out[:, n_b:] == -7), "written between the rows"
    return out[:, :n_b]


def _dev_topk(ctx, a, b, k, live=None, min_count=0, extra=37):
    m, n_b = a.shape[0], 0 if b is None else b.shape[0]
    d_a, d_b = ctx.to_device(a), None if b is None else ctx.to_device(b)
    d_live = None if live is None else ctx.to_device(lsh_bulk.live_bits(live))
    d_r, d_c = ctx.to_device(np.full(m * k + extra, -5, dtype=np.int64)), ctx.to_device(np.full(m * k + extra, -5, dtype=np.int32))
    ctx.weighted_jaccard_topk_dev(d_a.ptr, m, _p(d_b), n_b, a.shape[1], _p(d_live), min_count, k, d_r.ptr, d_c.ptr)
    rows, cnt = d_r.download(m * k + extra, np.int64), d_c.download(m * k + extra, np.int32)
    assert np.all(rows[m * k:] == -5) and np.all(cnt[m * k:] == -5), "written past n_a * k entries"
    return rows[: m * k].reshape(m, k), cnt[: m * k].reshape(m, k)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


@pytest.mark.parametrize("s", SAMPLES)
def test_matrix_at_the_edges_of_the_tile_and_of_the_chunk(ctx, s):
    for m in EDGES:
        for n in EDGES:
            if (m in (127, 129)) != (n in (127, 129)) and s not in (5, 128):
                continue  # (the mixed edges once per kind of last chunk: a one-sample one and a full one)
            a, b, counts = _case(m, n, s)
            assert np.array_equal(_dev_matrix(ctx, a, b), counts), (m, n)
    a, b, counts = _case(129, 257, s)
    assert 0 < counts.max() <= s and (s == 1 or np.any((counts > 0) & (counts < s)))
    assert np.array_equal(ctx.weighted_jaccard_matrix(a, b), counts), "host form"
    assert np.array_equal(_dev_matrix(ctx, a, b, ldc=259), counts), "ldc > n_b (scalar stores)"
    assert np.array_equal(_dev_matrix(ctx, a, b, ldc=260), counts), "ldc > n_b (16-byte stores)"
    assert np.array_equal(_dev_matrix(ctx, b, None), want_matrix(b, None)), "A with itself"
    assert np.array_equal(lsh_bulk.weighted_jaccard_matrix(a, b, gpu_mode="always"), lsh_bulk.weighted_jaccard_matrix(a, b, gpu_mode="disable"))


def test_near_misses_on_every_entry(ctx, options):
    rows = near_miss_matrix()
    s = rows.shape[1]
    want = np.array([s] + [NEAR_MISS_EQUAL] * 6, dtype=np.int32)
    assert np.array_equal(want_matrix(rows[:1], rows)[0], want)
    assert np.array_equal(_dev_matrix(ctx, rows, None), want_matrix(rows, None))
    assert np.array_equal(_dev_matrix(ctx, rows[:1], rows)[0], want)
    pairs = np.stack([np.zeros(7, dtype=np.int64), np.arange(7)], axis=1)
    assert np.array_equal(ctx.weighted_jaccard_pairs(rows, pairs), want)
    got_pairs, got_counts = ctx.weighted_jaccard_threshold_pairs(rows[:1], rows, NEAR_MISS_EQUAL + 1)
    assert got_pairs.tolist() == [[0, 0]] and got_counts.tolist() == [s]
    for path in (1, 2):
        options(path=path)
        got = _dev_topk(ctx, rows[:1], rows[1:], 6)
        assert got[0].tolist() == [[0, 1, 2, 3, 4, 5]] and got[1].tolist() == [[NEAR_MISS_EQUAL] * 6], path  # all tied: by the row


def test_negative_and_large_t_and_k(ctx):
    """Samples that differ in one bit only, of either value, anywhere in the 64: sign bits, bit 31 / 32, the lowest."""
    s = 64
    base = np.empty((s, 2), dtype=np.int64)
    base[:, 0] = np.arange(s) * 0x0101010101010101 % (1 << 62)
    base[:, 1] = -(np.arange(s, dtype=np.int64) << 40) - 1
    rows = np.repeat(base[None], 129, axis=0)
    for j in range(1, 129):  # row j: bit (j - 1) % 64 of k (j <= 64) or of t flipped in sample (j - 1) % 64
        rows[j, (j - 1) % 64, 0 if j <= 64 else 1] ^= np.int64(1) << np.int64((j - 1) % 64) if (j - 1) % 64 < 63 else np.int64(-2**63)
    want = want_matrix(rows, None)
    assert want[0].tolist() == [s] + [s - 1] * 128
    assert np.array_equal(_dev_matrix(ctx, rows, None), want)
    pairs = np.stack([np.zeros(129, dtype=np.int64), np.arange(129)], axis=1)
    assert np.array_equal(ctx.weighted_jaccard_pairs(rows, pairs), want[0])
    extremes = np.array([[[np.iinfo(np.int64).min, np.iinfo(np.int64).max]], [[np.iinfo(np.int64).max, np.iinfo(np.int64).min]],
                         [[-1, -1]], [[0, 0]], [[-1, 0]], [[0xFFFFFFFF, -0x100000000]]], dtype=np.int64)
    assert np.array_equal(_dev_matrix(ctx, extremes, None), np.eye(6, dtype=np.int32))


@pytest.mark.parametrize("s", (1, 3, 32, 63, 64, 65, 128, 200))
def test_listed_pairs_below_at_and_above_64_samples(ctx, s):
    rng = np.random.RandomState(s)
    a, b = planted_weighted(rng, 50, 70, s)
    pairs = np.stack([rng.randint(0, 50, size=1003), rng.randint(0, 70, size=1003)], axis=1).astype(np.int64)
    want = want_pairs(a, b, pairs)
    assert s == 1 or np.any((want > 0) & (want < s))
    d_a, d_b, d_p = ctx.to_device(a), ctx.to_device(b), ctx.to_device(pairs)
    d_c = ctx.to_device(np.full(1003 + 3, -9, dtype=np.int32))
    ctx.weighted_jaccard_pairs_dev(d_a.ptr, d_b.ptr, s, d_p.ptr, 1003, d_c.ptr)
    got = d_c.download(1006, np.int32)
    assert np.array_equal(got[:1003], want) and np.all(got[1003:] == -9)
    # rows at 8-byte, not 16-byte aligned addresses: the two-load path of the kernel
    shifted = ctx.alloc(a.nbytes + 8)
    ctx.copy_dev(shifted.ptr + 8, d_a.ptr, a.nbytes)
    ctx.weighted_jaccard_pairs_dev(shifted.ptr + 8, d_b.ptr, s, d_p.ptr, 1003, d_c.ptr)
    assert np.array_equal(d_c.download(1006, np.int32)[:1003], want), "8-byte aligned rows"
    both = np.concatenate([a, b])
    both_pairs = pairs + np.array([0, 50])
    assert np.array_equal(ctx.weighted_jaccard_pairs(both, both_pairs), want), "host form"
    assert np.array_equal(lsh_bulk.weighted_jaccard_pairs(both, both_pairs, gpu_mode="always"), want / float(s))
    ctx.weighted_jaccard_pairs_dev(d_a.ptr, d_b.ptr, s, d_p.ptr, 0, d_c.ptr)  # no pairs: nothing is launched


@pytest.mark.parametrize("s", (3, 33, 128))
def test_threshold_pairs_capacity_and_the_retry(ctx, s):
    a, b, counts = _case(129, 257, s)
    floor = max(1, s // 3)
    pairs, cnt = want_threshold(a, b, floor)
    assert 10 < len(pairs) < counts.size
    got = ctx.weighted_jaccard_threshold_pairs(a, b, floor, capacity=len(pairs))
    assert np.array_equal(got[0], pairs) and np.array_equal(got[1], cnt)
    got = ctx.weighted_jaccard_threshold_pairs(a, b, floor, capacity=3)  # too small, then the retry with the exact total
    assert np.array_equal(got[0], pairs) and np.array_equal(got[1], cnt)
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    cap = 7
    d_p, d_c = ctx.to_device(np.full(2 * cap + 2, -3, dtype=np.int64)), ctx.to_device(np.full(cap + 1, -3, dtype=np.int32))
    assert ctx.weighted_jaccard_threshold_pairs_dev(d_a.ptr, 129, d_b.ptr, 257, s, floor, d_p.ptr, d_c.ptr, cap) == len(pairs)
    assert np.all(d_p.download(2 * cap + 2, np.int64)[2 * cap:] == -3) and d_c.download(cap + 1, np.int32)[cap] == -3, "written past capacity"
    assert ctx.weighted_jaccard_threshold_pairs_dev(d_a.ptr, 129, d_b.ptr, 257, s, floor, None, None, 0) == len(pairs)
    # the self-join: pairs i < j only; min_count edges
    self_pairs, self_cnt = want_threshold(b, None, floor)
    got = ctx.weighted_jaccard_threshold_pairs(b, None, floor)
    assert np.array_equal(got[0], self_pairs) and np.array_equal(got[1], self_cnt) and np.all(got[0][:, 0] < got[0][:, 1])
    assert len(ctx.weighted_jaccard_threshold_pairs(a[:5], b[:9], 0)[0]) == 45 and len(ctx.weighted_jaccard_threshold_pairs(a[:5], b[:9], -4)[0]) == 45
    assert len(ctx.weighted_jaccard_threshold_pairs(a, b, s + 1)[0]) == 0
    top = ctx.weighted_jaccard_threshold_pairs(a, b, s)
    assert np.array_equal(top[0], np.argwhere(counts >= s)) and np.all(top[1] == s)
    for threshold in (floor / float(s), 0.0, 1.0, 1.5):
        g = lsh_bulk.weighted_similar_pairs(a, b, threshold=threshold, gpu_mode="always")
        h = lsh_bulk.weighted_similar_pairs(a, b, threshold=threshold, gpu_mode="disable")
        assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1]), threshold


@pytest.mark.parametrize("s", SAMPLES)
@pytest.mark.parametrize("path", (1, 2), ids=("strip", "stream"))
def test_topk_both_kernels_one_and_several_segments_with_and_without_live_bits(ctx, options, path, s):
    rng = np.random.RandomState(s)
    for m, n in ((1, 1), (3, 127), (9, 1000), (129, 257)):
        a, b, counts = _case(m, n, s) if (m, n) == (129, 257) else planted_weighted(np.random.RandomState(m * n + s), m, n, s) + (None,)
        live = rng.random_sample(n) < 0.7
        for segments in (0, 1, 3):
            options(path=path, segments=segments)
            what = f"{m}x{n} segments={segments}"
            _same(_dev_topk(ctx, a, b, 10), want_topk(a, b, 10, 0), what)
            _same(_dev_topk(ctx, a, b, KMAX, live=live, min_count=s // 3), want_topk(a, b, KMAX, s // 3, live), what + " live floor")
            _same(_dev_topk(ctx, b, None, 7, live=live), want_topk(b, None, 7, 0, live), what + " self")
    options(path=path)
    a, b, _ = _case(129, 257, s)
    dead = _dev_topk(ctx, a, b, 5, live=np.zeros(257, dtype=bool))
    assert np.all(dead[0] == -1) and np.all(dead[1] == -1)
    none = _dev_topk(ctx, a, b, 5, min_count=s + 1)  # > S: nothing is compared
    assert np.all(none[0] == -1) and np.all(none[1] == -1)
    options(path=path, chunk=100 * s * 16)
    _same(ctx.weighted_jaccard_topk(a, b, 10), want_topk(a, b, 10, 0), "host form, 3 blocks of B")
    _same(ctx.weighted_jaccard_topk(b, None, 10), want_topk(b, None, 10, 0), "host form, self")


def test_python_layer_and_the_indexes_equal_their_numpy_twins(ctx):
    rng = np.random.RandomState(12)
    a, b = planted_weighted(rng, 40, 300, 32)
    for kwargs in ({"k": 10}, {"k": 10, "threshold": 0.4}, {"k": KMAX}):
        g = lsh_bulk.weighted_nearest_neighbors(a, b, gpu_mode="always", **kwargs)
        h = lsh_bulk.weighted_nearest_neighbors(a, b, gpu_mode="disable", **kwargs)
        assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True), kwargs
    g, h = (lsh_bulk.weighted_nearest_neighbors(b, k=5, gpu_mode=mode) for mode in ("always", "disable"))
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True)
    for threshold in (0.5, 0.9, None):
        g, h = (lsh_bulk.weighted_duplicate_clusters(b, 8, 2, threshold, gpu_mode=mode) for mode in ("always", "disable"))
        assert np.array_equal(g, h) and (threshold != 0.5 or 1 < np.unique(g).size < 300), threshold
    index = lsh_bulk.SortedBandsIndex(b, 8, 2)
    assert index.words == 2 and index.n == 300
    got = index.nearest(a[:9], 10, threshold=0.2)
    want = lsh_bulk.weighted_nearest_neighbors(a[:9], b, k=10, threshold=0.2, gpu_mode="disable")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)
    assert np.array_equal(index.clusters(0.5), lsh_bulk.weighted_duplicate_clusters(b, 8, 2, 0.5, gpu_mode="disable"))
    assert np.array_equal(index.clusters(), lsh_bulk.duplicate_clusters(b, 8, 2, gpu_mode="disable"))
    offsets, rows = index.query(a[:9])
    assert offsets.shape == (10,) and np.all(rows < 300)
    with pytest.raises(ValueError, match="WeightedMinHash"):
        index.nearest(np.zeros((2, 64), dtype=np.uint64), 3)
    with pytest.raises(ValueError, match="Expecting minhash with length 32"):
        index.nearest(np.zeros((2, 8, 2), dtype=np.int64), 3)
    plain = lsh_bulk.SortedBandsIndex(np.arange(640, dtype=np.uint64).reshape(10, 64), 8, 2)
    with pytest.raises(ValueError, match="WeightedMinHash"):
        plain.nearest(a[:2], 3)


def test_weighted_minhash_lsh_on_the_device_equals_the_host_index(ctx):
    rng = np.random.RandomState(13)
    probes, sig = planted_weighted(rng, 12, 200, 32)
    built = []
    for mode in ("always", "disable"):
        lsh = MinHashLSH(num_perm=32, params=(8, 2), gpu_mode=mode)
        lsh.insert_bulk(list(range(150)), sig[:150])
        best = int(np.argmax(want_matrix(probes[:1], sig[:150])[0]))  # the best match of probe 0
        lsh.remove(best)
        lsh.remove(7 if best != 7 else 8)
        lsh.insert_bulk(list(range(150, 200)) + [17, 18], np.concatenate([sig[150:], sig[[3, 4]]]), check_duplication=False)
        built.append(lsh)
    dev, host = built
    for kwargs in ({"k": 5}, {"k": 10, "threshold": 0.3}):
        assert dev.nearest_bulk(probes, **kwargs) == host.nearest_bulk(probes, **kwargs), kwargs
    assert any(dev.nearest_bulk(probes, 5))
    for threshold in (0.5, None):
        got, want = (x.duplicate_clusters(threshold=threshold) for x in (dev, host))
        assert got == want and len(got) > 0, threshold
    with pytest.raises(ValueError, match="WeightedMinHash"):
        dev.nearest_bulk(np.zeros((1, 32), dtype=np.uint64), 3)


def test_argument_checks_of_the_eight_entry_points(ctx):
    lib, h = ctx.lib, ctx.handle
    found = ctypes.c_int64(-1)
    f = ctypes.byref(found)
    calls = {  # pointers are never followed: every call below fails its checks first
        "mhx_weighted_jaccard_pairs_dev": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_pairs_dev(c, a, 1, s, 1, n, 1),
        "mhx_weighted_jaccard_pairs": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_pairs(c, a, 4, s, 1, n, 1),
        "mhx_weighted_jaccard_matrix_dev": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_matrix_dev(c, a, n, 1, 4, s, 1, 4),
        "mhx_weighted_jaccard_matrix": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_matrix(c, a, n, 1, 4, s, 1),
        "mhx_weighted_jaccard_threshold_pairs_dev": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_threshold_pairs_dev(c, a, n, 1, 4, s, 2, 1, 1, 8, f),
        "mhx_weighted_jaccard_threshold_pairs": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_threshold_pairs(c, a, n, 1, 4, s, 2, 1, 1, 8, f),
        "mhx_weighted_jaccard_topk_dev": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_topk_dev(c, a, n, 1, 4, s, None, 0, k, 1, 1),
        "mhx_weighted_jaccard_topk": lambda c=h, a=1, n=4, s=16, k=3: lib.mhx_weighted_jaccard_topk(c, a, n, 1, 4, s, 0, k, 1, 1),
    }
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_WJ
    for name, call in calls.items():
        listed, topk = "_pairs" in name and "threshold" not in name, "topk" in name
        checks = [({"c": None}, "ctx is NULL"), ({"s": 0}, "bad shape" if listed else "samples must be positive"), ({"n": -1}, "bad shape"),
                  ({"a": None}, "NULL (host|device) pointer")]
        if not listed:
            checks.append(({"n": 1 << 32}, "2\\^32-1 rows"))
        if topk:
            checks += [({"k": 0}, "k must be in"), ({"k": KMAX + 1}, "k must be in")]
        for kwargs, message in checks:
            with pytest.raises(ValueError, match=message):
                _native.check(call(**kwargs))
    with pytest.raises(ValueError, match="ldc must be >= n_b"):
        _native.check(lib.mhx_weighted_jaccard_matrix_dev(h, 1, 4, 1, 4, 16, 1, 3))
    with pytest.raises(ValueError, match="n_pairs is NULL"):
        _native.check(lib.mhx_weighted_jaccard_threshold_pairs_dev(h, 1, 4, 1, 4, 16, 2, 1, 1, 8, None))
    with pytest.raises(ValueError, match="bad capacity"):
        _native.check(lib.mhx_weighted_jaccard_threshold_pairs_dev(h, 1, 4, 1, 4, 16, 2, 1, 1, -1, f))
    with pytest.raises(ValueError, match="pair index 4 out of range"):
        pairs = np.array([[0, 4]], dtype=np.int64)
        _native.check(lib.mhx_weighted_jaccard_pairs(h, 1, 4, 16, pairs.ctypes.data, 1, 1))
    # the quiet cases: empty sides and a floor above S launch nothing and need no pointers
    _native.check(lib.mhx_weighted_jaccard_matrix_dev(h, None, 0, None, 4, 16, None, 4))
    _native.check(lib.mhx_weighted_jaccard_threshold_pairs_dev(h, None, 4, None, 4, 16, 17, None, None, 0, f))
    assert found.value == 0
    _native.check(lib.mhx_weighted_jaccard_topk_dev(h, None, 0, None, 4, 16, None, 0, 3, None, None))
    d_r, d_c = ctx.to_device(np.full(20, -5, dtype=np.int64)), ctx.to_device(np.full(20, -5, dtype=np.int32))
    d_a = ctx.to_device(np.zeros((5, 16, 2), dtype=np.int64))
    ctx.weighted_jaccard_topk_dev(d_a.ptr, 5, d_a.ptr, 0, 16, None, 0, 3, d_r.ptr, d_c.ptr)  # n_b == 0: the padding
    got_r, got_c = d_r.download(20, np.int64), d_c.download(20, np.int32)
    assert np.all(got_r[:15] == -1) and np.all(got_c[:15] == -1) and np.all(got_r[15:] == -5) and np.all(got_c[15:] == -5)
