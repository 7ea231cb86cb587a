"""Exact top-k Jaccard neighbours on the MI355X through the C ABI (mhx_jaccard_topk*, mhx_bbit_jaccard_topk*) and the Python
layer above it: every list equal to numpy's sort of the packed keys (count << 32 | 0xFFFFFFFF - row) -- the best k by (count
descending, row ascending), padded with -1 -- on both kernels (strip, stream), however B is cut into segments
(ref for the counts: datasketch/minhash.py:299-324, b_bit_minhash.py:53-72)."""
import numpy as np
import pytest

from datasketch_amd import MinHashLSH, _native, b_bit_minhash, lsh_bulk
from tests.test_gpu_jaccard_matrix import _counts, _planted

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
KMAX = _native.MHX_TOPK_MAX
LOW = np.uint64(0xFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    return _native.context()


@pytest.fixture
def options(ctx):
    """set(path, segments) for the test; back to auto afterwards."""
    def set_(path=0, segments=0, chunk=0):
        ctx.set_option("jaccard.topk_path", path)
        ctx.set_option("jaccard.topk_segments", segments)
        ctx.set_option("host.chunk_bytes", chunk)
    yield set_
    set_()


def _want(counts, k, min_count=0, self_join=False, live=None):
    """(rows int64 [m, k], counts int32 [m, k]) of a counts matrix: the sort of the packed keys."""
    m, n = counts.shape
    key = (counts.astype(np.uint64) << np.uint64(32)) | (LOW - np.arange(n, dtype=np.uint64))[None, :]
    ok = counts >= min_count
    if self_join:
        ok &= ~np.eye(m, n, dtype=bool)
    if live is not None:
        ok &= live[None, :]
    key[~ok] = 0
    top = np.sort(key, axis=1)[:, ::-1][:, :k]
    rows, cnt = np.full((m, k), -1, dtype=np.int64), np.full((m, k), -1, dtype=np.int32)
    have = top != 0
    rows[:, : top.shape[1]] = np.where(have, (LOW - (top & LOW)).astype(np.int64), -1)
    cnt[:, : top.shape[1]] = np.where(have, (top >> np.uint64(32)).astype(np.int32), -1)
    return rows, cnt


def _tie_at_k(counts, k):
    """Whether some row's k-th and (k+1)-th best counts are equal: the row order decides who is in the list."""
    if counts.shape[1] <= k:
        return False
    s = np.sort(counts, axis=1)[:, ::-1]
    return bool(np.any(s[:, k - 1] == s[:, k]))


def _bits(live):
    return lsh_bulk.live_bits(np.asarray(live, dtype=bool))


def _dev_topk(ctx, a, b, num_perm, k, code=U32, live=None, min_count=0, bbit=None, extra=37):
    """The _dev entry on poisoned buffers with `extra` entries behind the n_a * k the call may write."""
    m = a.shape[0]
    d_a = ctx.to_device(a)
    d_b = None if b is None else ctx.to_device(b)
    n_b = 0 if b is None else b.shape[0]
    d_live = None if live is None else ctx.to_device(_bits(live))
    d_r, d_c = ctx.alloc(8 * (m * k + extra)), ctx.alloc(4 * (m * k + extra))
    d_r.upload(np.full(m * k + extra, -5, dtype=np.int64))
    d_c.upload(np.full(m * k + extra, -5, dtype=np.int32))
    p = lambda buf: None if buf is None else buf.ptr  # noqa: E731
    if bbit is None:
        ctx.jaccard_topk_dev(d_a.ptr, m, p(d_b), n_b, code, num_perm, p(d_live), min_count, k, d_r.ptr, d_c.ptr)
    else:
        ctx.bbit_jaccard_topk_dev(d_a.ptr, m, p(d_b), n_b, num_perm, bbit, p(d_live), min_count, k, d_r.ptr, d_c.ptr)
    rows, cnt = d_r.download(m * k + extra, np.int64), d_c.download(m * k + extra, np.int32)
    assert np.all(rows[m * k:] == -5) and np.all(cnt[m * k:] == -5), "written past n_a * k entries"
    return rows[: m * k].reshape(m, k), cnt[: m * k].reshape(m, k)


def _check(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what


SHAPES = [(1, 1, 1), (2, 63, 3), (64, 65, 100), (129, 127, 128), (130, 257, 320), (1, 1000, 128), (3, 4097, 64), (129, 4097, 3)]
_REFERENCE = {}


def _case(m, n, k_perm):
    """The planted input of a shape and its counts, computed once for the module."""
    if (m, n, k_perm) not in _REFERENCE:
        rng = np.random.RandomState(m * 7 + n + k_perm)
        a, b = _planted(rng, m, n, k_perm)
        _REFERENCE[(m, n, k_perm)] = (a, b, _counts(a, b))
    return _REFERENCE[(m, n, k_perm)]


@pytest.mark.parametrize("k", [1, 10, KMAX])
@pytest.mark.parametrize("m,n,k_perm", SHAPES)
def test_dense_lists_equal_numpy_both_dtypes_both_kernels(ctx, options, m, n, k_perm, k):
    a, b, counts = _case(m, n, k_perm)
    want = _want(counts, k)
    if n > k and m > 1:
        assert _tie_at_k(counts, k), "the input has no tie at the k-th place"
    if n < k:
        assert np.all(want[0][:, n:] == -1) and np.all(want[0][:, :n] >= 0)
    a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
    for path in (0, 1, 2):
        options(path=path)
        _check(_dev_topk(ctx, a, b, k_perm, k, code=U32), want, f"uint32 path {path}")
        _check(_dev_topk(ctx, a64, b64, k_perm, k, code=U64), want, f"uint64 path {path}")
    options()
    _check(ctx.jaccard_topk(a64, b64, k), want, "host form")


def test_uint64_values_that_differ_only_in_the_high_word_are_not_equal(ctx, options):
    rng = np.random.RandomState(5)
    a, b = _planted(rng, 130, 300, 100, dtype=np.uint64, high=True)
    counts = _counts(a, b)
    assert not np.array_equal(counts, _counts(a & LOW, b & LOW)) and _tie_at_k(counts, 10)
    for path in (1, 2):
        options(path=path)
        _check(_dev_topk(ctx, a, b, 100, 10, code=U64), _want(counts, 10), f"path {path}")
        _check(_dev_topk(ctx, a[:3], b, 100, 10, code=U64), _want(counts[:3], 10), f"path {path}, 3 probes")


@pytest.mark.parametrize("m", [3, 130])
def test_forced_paths_and_segments_agree_with_numpy(ctx, options, m):
    k_perm, k = 64, 10
    n = 128 * 5 + 7  # 6 tiles; the last segment holds 7 rows < k however B is cut
    rng = np.random.RandomState(m)
    a, b = _planted(rng, m, n, k_perm)
    counts = _counts(a, b)
    assert _tie_at_k(counts, k)
    want = _want(counts, k)
    for path in (1, 2):
        for segments in (1, 2, 3, 6, 1000):  # 6 and beyond: one segment per tile
            options(path=path, segments=segments)
            _check(_dev_topk(ctx, a, b, k_perm, k), want, f"path {path}, {segments} segments")
            _check(_dev_topk(ctx, a, b, k_perm, KMAX), _want(counts, KMAX), f"path {path}, {segments} segments, k = {KMAX}")


def test_self_mode_never_reports_the_row_itself(ctx, options):
    rng = np.random.RandomState(6)
    a, _ = _planted(rng, 300, 1, 128)
    a[150:] = a[:150]
    a[150:, :40] ^= 1
    a[7] = a[200]  # a duplicate row j != i: count K
    counts = _counts(a, a)
    assert _tie_at_k(counts, 10)
    want = _want(counts, 10, self_join=True)
    assert want[0][7, 0] == 200 and want[1][7, 0] == 128
    for path in (1, 2):
        options(path=path)
        got = _dev_topk(ctx, a, None, 128, 10)
        _check(got, want, f"path {path}")
        assert not np.any(got[0] == np.arange(300)[:, None])
    options()
    _check(_dev_topk(ctx, a[:5], None, 128, 10), _want(counts[:5, :5], 10, self_join=True), "5 rows, auto")
    _check(ctx.jaccard_topk(a.astype(np.uint64), None, 10), want, "host form")


def test_dead_rows_are_no_candidates(ctx, options):
    rng = np.random.RandomState(7)
    n = 32 * 9 + 5  # the last word of the map is partial
    a, b = _planted(rng, 70, n, 64)
    counts = _counts(a, b)
    live = rng.random_sample(n) < 0.7
    live[np.argmax(counts[0])] = False  # the row that would be rank 1 of probe 0
    live[n - 1] = False
    assert _tie_at_k(counts[:, live], 10)
    want = _want(counts, 10, live=live)
    assert want[0][0, 0] != np.argmax(counts[0])
    for path in (1, 2):
        options(path=path)
        _check(_dev_topk(ctx, a, b, 64, 10, live=live), want, f"path {path}")
        _check(_dev_topk(ctx, a[:2], b, 64, 10, live=live), _want(counts[:2], 10, live=live), f"path {path}, 2 probes")
        dead = _dev_topk(ctx, a, b, 64, 10, live=np.zeros(n, dtype=bool))
        assert np.all(dead[0] == -1) and np.all(dead[1] == -1)


def test_min_count_cuts_the_lists_at_the_floor(ctx, options):
    rng = np.random.RandomState(8)
    a, b = _planted(rng, 70, 600, 64)
    counts = _counts(a, b)
    assert _tie_at_k(counts, 10)
    want = _want(counts, 10, min_count=40)
    assert np.any(want[0] == -1) and np.any(want[0] >= 0) and np.all(want[1][want[0] >= 0] >= 40)
    for path in (1, 2):
        options(path=path)
        _check(_dev_topk(ctx, a, b, 64, 10, min_count=40), want, f"path {path}")
        none = _dev_topk(ctx, a, b, 64, 10, min_count=65)  # > K: nothing is compared
        assert np.all(none[0] == -1) and np.all(none[1] == -1)
    options()
    _check(ctx.jaccard_topk(a.astype(np.uint64), b.astype(np.uint64), 10, min_count=40), want, "host form")


def test_bad_k_and_empty_sides(ctx):
    a = np.zeros((5, 16), dtype=np.uint32)
    for k in (0, -1, KMAX + 1):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            ctx.jaccard_topk_dev(1, 5, 1, 5, U32, 16, None, 0, k, 1, 1)
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            ctx.bbit_jaccard_topk_dev(1, 5, 1, 5, 16, 1, None, 0, k, 1, 1)
    with pytest.raises(ValueError):
        ctx.bbit_jaccard_topk_dev(1, 5, 1, 5, 16, 33, None, 0, 3, 1, 1)
    d_a = ctx.to_device(a)
    d_r, d_c = ctx.alloc(8 * 20), ctx.alloc(4 * 20)
    d_r.upload(np.full(20, -5, dtype=np.int64))
    d_c.upload(np.full(20, -5, dtype=np.int32))
    ctx.jaccard_topk_dev(d_a.ptr, 0, d_a.ptr, 5, U32, 16, None, 0, 3, d_r.ptr, d_c.ptr)  # n_a == 0: nothing is written
    assert np.all(d_r.download(20, np.int64) == -5)
    ctx.jaccard_topk_dev(d_a.ptr, 5, d_a.ptr, 0, U32, 16, None, 0, 3, d_r.ptr, d_c.ptr)  # n_b == 0: the padding
    got_r, got_c = d_r.download(20, np.int64), d_c.download(20, np.int32)
    assert np.all(got_r[:15] == -1) and np.all(got_c[:15] == -1) and np.all(got_r[15:] == -5) and np.all(got_c[15:] == -5)
    rows, cnt = ctx.jaccard_topk(np.zeros((2, 8), np.uint64), np.zeros((0, 8), np.uint64), 4)
    assert np.all(rows == -1) and np.all(cnt == -1)


def test_argument_checks_of_the_four_entry_points(ctx):
    lib, h = ctx.lib, ctx.handle
    calls = {  # pointers are never followed: every call below fails its checks first
        "mhx_jaccard_topk_dev": lambda c=h, a=1, n_a=4, np_=16, k=3: lib.mhx_jaccard_topk_dev(c, a, n_a, 1, 4, U32, np_, None, 0, k, 1, 1),
        "mhx_jaccard_topk": lambda c=h, a=1, n_a=4, np_=16, k=3: lib.mhx_jaccard_topk(c, a, n_a, 1, 4, np_, 0, k, 1, 1),
        "mhx_bbit_jaccard_topk_dev": lambda c=h, a=1, n_a=4, np_=16, k=3: lib.mhx_bbit_jaccard_topk_dev(c, a, n_a, 1, 4, np_, 2, None, 0, k, 1, 1),
        "mhx_bbit_jaccard_topk": lambda c=h, a=1, n_a=4, np_=16, k=3: lib.mhx_bbit_jaccard_topk(c, a, n_a, 1, 4, np_, 2, 0, k, 1, 1),
    }
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_TOPK
    for name, call in calls.items():
        for kwargs, message in (({"c": None}, "ctx is NULL"), ({"np_": 0}, "num_perm must be positive"), ({"n_a": -1}, "bad shape"),
                                ({"n_a": 1 << 32}, "2\\^32-1 rows"), ({"k": 0}, "k must be in"), ({"k": KMAX + 1}, "k must be in"),
                                ({"a": None}, "NULL (host|device) pointer")):
            with pytest.raises(ValueError, match=message):
                _native.check(call(**kwargs))
    with pytest.raises(ValueError, match="bad sig_dtype"):
        _native.check(lib.mhx_jaccard_topk_dev(h, 1, 4, 1, 4, 7, 16, None, 0, 3, 1, 1))
    for option, bad in (("jaccard.topk_path", 3), ("jaccard.topk_path", -1), ("jaccard.topk_segments", -1)):
        with pytest.raises(ValueError, match=option):
            ctx.set_option(option, bad)


@pytest.mark.parametrize("k_perm", [64, 100, 128])
@pytest.mark.parametrize("bits", [1, 2, 4, 8])
def test_bbit_lists_equal_numpy_on_unpacked_values(ctx, options, bits, k_perm):
    rng = np.random.RandomState(bits * 1000 + k_perm)
    a, b = _planted(rng, 130, 257, k_perm, dtype=np.uint64)
    mask = np.uint64((1 << bits) - 1)
    counts = _counts(a & mask, b & mask)
    assert _tie_at_k(counts, 10)
    pa, pb = ctx.bbit_pack(a, bits), ctx.bbit_pack(b, bits)
    _check(_dev_topk(ctx, pa, pb, k_perm, 10, bbit=bits), _want(counts, 10), "dev")
    options(path=2, segments=2)  # b-bit rows always take the strip kernel
    _check(_dev_topk(ctx, pa, pb, k_perm, KMAX, bbit=bits), _want(counts, KMAX), "dev, two segments")
    live = rng.random_sample(257) < 0.5
    _check(_dev_topk(ctx, pa, pb, k_perm, 10, bbit=bits, live=live, min_count=k_perm // 2), _want(counts, 10, k_perm // 2, live=live), "live + floor")
    self_counts = _counts(a & mask, a & mask)
    _check(_dev_topk(ctx, pa, None, k_perm, 10, bbit=bits), _want(self_counts, 10, self_join=True), "self")
    options(chunk=100 * pb.shape[1] * 8)
    _check(ctx.bbit_jaccard_topk(pa, pb, k_perm, bits, 10), _want(counts, 10), "host form, 3 blocks of B")


def test_host_forms_stream_b_in_blocks(ctx, options):
    rng = np.random.RandomState(9)
    a, b = _planted(rng, 140, 1000, 64, dtype=np.uint64)
    counts = _counts(a, b)
    assert _tie_at_k(counts, 10)
    dev = _dev_topk(ctx, a, b, 64, 10, code=U64)
    _check(dev, _want(counts, 10))
    for rows_per_block in (1000, 333, 128, 7):  # 1, 4, 8 and 143 blocks; the last one short of k rows
        options(chunk=rows_per_block * 64 * 8)
        _check(ctx.jaccard_topk(a, b, 10), dev, f"{rows_per_block} rows per block")
    options(chunk=64 * 8 * 100, path=2)
    _check(ctx.jaccard_topk(a[:4], b, KMAX), _want(counts[:4], KMAX), "stream kernel, blocks of 100 rows")


def test_python_layer_on_the_gpu_equals_the_numpy_path(ctx):
    rng = np.random.RandomState(10)
    a, b = _planted(rng, 150, 400, 128, dtype=np.uint64)
    for kwargs in ({"k": 10}, {"k": 10, "threshold": 0.4}, {"k": KMAX}):
        g = lsh_bulk.nearest_neighbors(a, b, gpu_mode="always", **kwargs)
        h = lsh_bulk.nearest_neighbors(a, b, gpu_mode="disable", **kwargs)
        assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True)
    g = lsh_bulk.nearest_neighbors(b, k=5, gpu_mode="always")
    h = lsh_bulk.nearest_neighbors(b, k=5, gpu_mode="disable")
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True)
    blocks_a, blocks_b = b_bit_minhash.pack_matrix(a, 2), b_bit_minhash.pack_matrix(b, 2)
    g = b_bit_minhash.nearest_neighbors(blocks_a, blocks_b, 128, 2, k=10, threshold=0.3, r=0.1, r_b=0.3)
    h = b_bit_minhash.nearest_neighbors(blocks_a, blocks_b, 128, 2, k=10, threshold=0.3, r=0.1, r_b=0.3, gpu_mode="disable")
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True)
    index = lsh_bulk.SortedBandsIndex(b.astype(np.uint32), 32, 4)
    g = index.nearest(a[:9].astype(np.uint32), 10, threshold=0.2)
    h = lsh_bulk.nearest_neighbors(a[:9], b, k=10, threshold=0.2, gpu_mode="disable")
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1], equal_nan=True)
    with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
        index.nearest(a[:9].astype(np.uint32), 65)


def test_minhash_lsh_nearest_bulk_after_inserts_a_removal_and_a_duplicate_key(ctx):
    rng = np.random.RandomState(11)
    probes, sig = _planted(rng, 20, 500, 64)
    best = int(np.argmax(_counts(probes[:1], sig[:400])[0]))
    # slots: 0..399 the first batch (key = slot, `best` removed), 400..499 the second, 500 / 501 further rows of keys 17 and 18
    rows = np.concatenate([sig, sig[[best, 3]]])
    keys = list(range(500)) + [17, 18]
    live = np.arange(502) != best
    by_slot = _want(_counts(probes, rows), 12, live=live)
    want = []
    for slots, cnt in zip(by_slot[0].tolist(), by_slot[1].tolist()):
        seen, top = set(), []
        for slot, c in zip(slots, cnt):
            if keys[slot] not in seen:
                seen.add(keys[slot])
                top.append((keys[slot], c / 64.0))
        want.append(top[:10])
    assert best not in [key for key, _ in want[0]] and 17 in [key for key, _ in want[0]]
    for mode in ("always", "disable"):
        lsh = MinHashLSH(threshold=0.5, num_perm=64, gpu_mode=mode)
        lsh.insert_bulk(range(400), sig[:400])
        lsh.flush()
        lsh.remove(best)
        lsh.insert_bulk(range(400, 500), sig[400:])
        lsh.insert_bulk([17, 18], sig[[best, 3]], check_duplication=False)  # 17 gets the removed key's row as a second row
        assert lsh.nearest_bulk(probes, 10) == want, mode
        assert lsh.nearest_bulk(probes, 10, threshold=0.9) == [[kv for kv in x if kv[1] >= 0.9] for x in want], mode
        assert [len(x) for x in lsh.nearest_bulk(probes[:2], 62)] == [62, 62]
        with pytest.raises(ValueError, match="must not exceed 64"):
            lsh.nearest_bulk(probes, 63)


def test_100k_rows_against_the_matrix_kernel_and_one_probe_on_the_stream_kernel(ctx):
    rng = np.random.RandomState(12)
    m, n, k_perm, k = 64, 100_000, 128, 10
    a = rng.randint(0, 2**32, size=(m, k_perm), dtype=np.uint64).astype(np.uint32)
    b = rng.randint(0, 2**32, size=(n, k_perm), dtype=np.uint64).astype(np.uint32)
    src = rng.randint(0, m, size=n)
    keep = rng.random_sample((n, k_perm)) < rng.random_sample((n, 1))
    b[keep] = a[src][keep]
    d_a, d_b, d_m = ctx.to_device(a), ctx.to_device(b), ctx.alloc(4 * m * n)
    ctx.jaccard_matrix_dev(d_a.ptr, m, d_b.ptr, n, U32, k_perm, d_m.ptr, n)
    counts = d_m.download((m, n), np.int32)
    assert _tie_at_k(counts, k)
    want = _want(counts, k)
    d_r, d_c = ctx.alloc(8 * m * k), ctx.alloc(4 * m * k)
    ctx.jaccard_topk_dev(d_a.ptr, m, d_b.ptr, n, U32, k_perm, None, 0, k, d_r.ptr, d_c.ptr)
    _check((d_r.download((m, k), np.int64), d_c.download((m, k), np.int32)), want, "64 probes")
    ctx.jaccard_topk_dev(d_a.ptr, 1, d_b.ptr, n, U32, k_perm, None, 0, k, d_r.ptr, d_c.ptr)  # auto: the stream kernel
    _check((d_r.download((1, k), np.int64), d_c.download((1, k), np.int32)), (want[0][:1], want[1][:1]), "one probe")
