"""The device side of datasketch_amd.MinHashLSHForest: the build entry point against np.lexsort, the query entry point against the
numpy back end (slots, counts and the cells past the counts), refused arguments, the golden answers and the order of the
device index against the numpy back end's, and one run at a million rows."""
import ctypes

import numpy as np
import pytest

from datasketch_amd import MinHashLSHForest, _native
from datasketch_amd import lshforest as F
from tests.test_lshforest_host import CASES, clustered, golden_case, golden_inputs, lexsort_order

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes past the output that must keep their fill byte
FILL32 = 0xA5A5A5A5
SIZES = (0, 1, 2, 255, 256, 257, 5000, 100_003)
L = 3  # trees of the entry point tests; one more word per row belongs to no tree


@pytest.fixture(scope="module")
def ctx():
    return _native.context()


def _guarded(ctx, nbytes):
    buf = ctx.alloc(nbytes + GUARD)
    buf.upload(np.full(nbytes + GUARD, 0xA5, dtype=np.uint8))
    return buf


def _guard_intact(buf, nbytes):
    return bool(np.all(buf.download(GUARD, np.uint8, offset=nbytes) == 0xA5))


def _code(dtype):
    return _native.MHX_U32 if np.dtype(dtype) == np.uint32 else _native.MHX_U64


def _corpus(rng, n, width, alpha, dtype, bases=None):
    """Clustered rows over an alphabet of `alpha` values (0: the full range of dtype, spread over the high bits too)."""
    full = alpha == 0
    rows, bases = clustered(rng, n, width, 2**31 if full else alpha, bases=bases)
    rows = rows.astype(np.uint64)
    if full:
        rows = rows * np.uint64(0x9E3779B97F4A7C15 if np.dtype(dtype) == np.uint64 else 3)
    return rows.astype(dtype), bases


def _build(ctx, sig, l, tree_words):
    n = sig.shape[0]
    d_sig = ctx.to_device(sig) if n else None
    out = _guarded(ctx, 4 * l * n)
    ctx.lsh_forest_build_dev(d_sig.ptr if n else None, _code(sig.dtype), n, sig.shape[1], l, tree_words, out.ptr)
    ctx.synchronize()
    assert _guard_intact(out, 4 * l * n)
    return d_sig, out, out.download((l, n), np.uint32) if n else np.empty((l, 0), dtype=np.uint32)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("tree_words", [1, 2, 16, 32])
@pytest.mark.parametrize("alpha", [1, 2, 0])
def test_build_equals_lexsort_with_the_slot_as_the_last_key(ctx, dtype, tree_words, alpha):
    rng = np.random.RandomState(tree_words + alpha)
    for n in SIZES:
        sig, _ = _corpus(rng, n, L * tree_words + 1, alpha, dtype)
        _, _, got = _build(ctx, sig, L, tree_words)
        assert np.array_equal(got, lexsort_order(sig, L, tree_words) if n else got), n
        if alpha == 1 and n:
            assert np.array_equal(got, np.tile(np.arange(n, dtype=np.uint32), (L, 1))), n  # all rows identical: slot order


def _query_case(ctx, sig, d_sig, d_order, order, probes, l, tree_words, w, k):
    """The entry point on exact-size outputs with a filled trailer against the numpy back end's walk."""
    m, n = probes.shape[0], sig.shape[0]
    d_q = ctx.to_device(probes) if m else None
    slots, counts = _guarded(ctx, 4 * m * k), _guarded(ctx, 4 * m)
    ctx.lsh_forest_query_dev(d_sig.ptr if n else None, _code(sig.dtype), n, sig.shape[1], l, tree_words, w, d_order.ptr if n else None,
                             d_q.ptr if m else None, m, k, slots.ptr, counts.ptr)
    ctx.synchronize()
    assert _guard_intact(slots, 4 * m * k) and _guard_intact(counts, 4 * m)
    if m == 0:
        return
    got_slots, got_counts = slots.download((m, k), np.uint32), counts.download((m,), np.int32)
    want_slots, want_counts = F.host_query(sig, order, probes, l, tree_words // w, w, k)
    assert np.array_equal(got_counts, want_counts), (n, m, k)
    past = np.arange(k)[None, :] >= want_counts[:, None]
    assert np.array_equal(np.where(past, 0, got_slots), want_slots), (n, m, k)
    assert np.all(got_slots[past] == FILL32), (n, m, k)  # the cells past the count are not written


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("w,tree_words", [(1, 1), (1, 2), (1, 16), (1, 32), (2, 2), (2, 16), (2, 32)])
@pytest.mark.parametrize("alpha", [1, 2, 0])
def test_query_equals_the_numpy_back_end(ctx, dtype, w, tree_words, alpha):
    rng = np.random.RandomState(7 * tree_words + alpha + w)
    width = L * tree_words + 1
    for n in SIZES:
        sig, bases = _corpus(rng, n, width, alpha, dtype)
        d_sig, d_order, order = _build(ctx, sig, L, tree_words)
        many = 1000 if n in (257, 100_003) else 48
        probes, _ = _corpus(rng, many, width, alpha, dtype, bases=bases)
        if n:
            probes[: many // 3] = sig[rng.randint(n, size=many // 3)]
            cut = rng.randint(0, width, size=many // 3)  # rows of the index, redrawn from a random column on
            tail = np.arange(width)[None, :] >= cut[:, None]
            probes[: many // 3][tail] = probes[many // 3 : 2 * (many // 3)][tail]
        for k in (1, 2, 10, 64, 1024):
            for m in (0, 1, many) if k in (2, 64) else (many,):
                _query_case(ctx, sig, d_sig, d_order, order, probes[:m], L, tree_words, w, k)


def test_k_1024_at_eight_trees_is_within_the_bound(ctx):
    rng = np.random.RandomState(21)
    sig, bases = _corpus(rng, 20_000, 128, 3, np.uint32)
    d_sig, d_order, order = _build(ctx, sig, 8, 16)
    probes, _ = _corpus(rng, 64, 128, 3, np.uint32, bases=bases)
    assert 8 * (2 * 1024 - 1) <= F.MAX_CANDIDATES
    _query_case(ctx, sig, d_sig, d_order, order, probes, 8, 16, 1, 1024)


def test_entry_points_refuse_bad_arguments(ctx):
    lib, h = ctx.lib, ctx.handle
    sig = np.arange(40, dtype=np.uint32).reshape(5, 8)
    d_sig, d_order, _ = _build(ctx, sig, 2, 4)
    out = _guarded(ctx, 0)
    u32 = _native.MHX_U32
    bad = _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_forest_build_dev_typed(None, d_sig.ptr, u32, 5, 8, 2, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, u32, 5, 8, 0, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, u32, 5, 8, 3, 4, out.ptr) == bad  # l * tree_words > row_words
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, u32, 1 << 32, 8, 2, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, u32, -1, 8, 2, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, 7, 5, 8, 2, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, None, u32, 5, 8, 2, 4, out.ptr) == bad
    assert lib.mhx_lsh_forest_build_dev_typed(h, d_sig.ptr, u32, 5, 8, 2, 4, None) == bad
    assert _native.last_error()
    q = lib.mhx_lsh_forest_query_dev_typed
    assert q(None, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 0, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 3, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 0, out.ptr, out.ptr) == bad  # k <= 0
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 3, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad  # w
    assert q(h, d_sig.ptr, u32, 5, 9, 3, 3, 2, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad  # w does not divide
    assert q(h, d_sig.ptr, u32, 1 << 32, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, -1, 3, out.ptr, out.ptr) == bad
    assert q(h, None, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, None, d_sig.ptr, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, None, 5, 3, out.ptr, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, None, out.ptr) == bad
    assert q(h, d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 3, out.ptr, None) == bad
    assert _native.last_error()
    # more candidates per probe than the kernel stages: l * min(2k - 1, n) > MAX_CANDIDATES
    n = F.MAX_CANDIDATES // 2 + 1
    big = np.zeros((n, 2), dtype=np.uint32)
    d_big, d_big_order, _ = _build(ctx, big, 2, 1)
    assert q(h, d_big.ptr, u32, n, 2, 2, 1, 1, d_big_order.ptr, d_big.ptr, 1, n, out.ptr, out.ptr) == bad
    assert "MHX_LSH_FOREST_MAX_CANDIDATES" in _native.last_error()
    ctx.synchronize()
    assert _guard_intact(out, 0)
    with pytest.raises(ValueError):
        ctx.lsh_forest_query_dev(d_sig.ptr, u32, 5, 8, 2, 4, 1, d_order.ptr, d_sig.ptr, 5, 0, out.ptr, out.ptr)
    index = MinHashLSHForest(num_perm=2, l=2, gpu_mode="always")  # the class answers such a k by the host walk
    index.add_bulk(list(range(n)), big)
    index.index()
    assert index.query_bulk(big[:1], n) == [list(range(n))]


@pytest.mark.parametrize("case", list(CASES))
def test_golden_answers_on_the_device(case):
    one = golden_case(case, "always")
    assert type(one._backend).__name__ == "_DeviceForest"


@pytest.mark.parametrize("case", list(CASES))
def test_device_order_equals_the_numpy_back_end_after_every_index(case):
    spec, keys, rows, probes = golden_inputs(case)
    dev = MinHashLSHForest(num_perm=spec["num_perm"], l=spec["l"], gpu_mode="always")
    host = MinHashLSHForest(num_perm=spec["num_perm"], l=spec["l"], gpu_mode="disable")

    def same(step):
        assert np.array_equal(dev._backend.order(), host._backend.order()), step
        assert np.array_equal(dev._backend.matrix(), host._backend.matrix()) and dev._backend.dtype == host._backend.dtype, step
        for k in (1, 10, 250):
            assert dev.query_bulk(probes, k) == host.query_bulk(probes, k), (step, k)

    from tests.test_lshforest_host import signature

    for one in (dev, host):
        for key, row in zip(keys[:60], rows[:60]):
            one.add(key, signature(row))
        one.index()
    same("add")
    for one in (dev, host):
        one.add_bulk(keys[60:], rows[60:])
        assert one.query_bulk(probes, 250) == host.query_bulk(probes, 250)  # added, not indexed: not searchable yet
        one.index()
    same("add_bulk")
    for one in (dev, host):
        assert np.array_equal(one.get_minhash_hashvalues(keys[5]), host.get_minhash_hashvalues(keys[5]))


def test_a_million_rows():
    rng = np.random.RandomState(9)
    n, num_perm, l = 1_000_000, 128, 8
    bases = rng.randint(0, 2**32, (2000, num_perm), dtype=np.int64)
    sig = np.empty((n, num_perm), dtype=np.uint32)
    for at in range(0, n, 100_000):
        sig[at : at + 100_000] = clustered(rng, 100_000, num_perm, 2**32, shares=(0.0, 0.01, 0.05, 0.2, 0.6), bases=bases)[0]
    probes = sig[rng.randint(n, size=10_000)].copy()
    redraw = rng.rand(5000, num_perm) < rng.choice([0.02, 0.1, 0.4], size=5000)[:, None]
    probes[5000:][redraw] = rng.randint(0, 2**32, int(redraw.sum()), dtype=np.int64)
    keys = range(n)
    dev = MinHashLSHForest(num_perm=num_perm, l=l, gpu_mode="always")
    host = MinHashLSHForest(num_perm=num_perm, l=l, gpu_mode="disable")
    for one in (dev, host):
        one.add_bulk(keys, sig)
        one.index()
    assert np.array_equal(dev._backend.order(), host._backend.order())
    for k in (1, 10, 100):
        got, want = dev.query_bulk(probes, k), host.query_bulk(probes, k)
        assert got == want, k
        assert sum(len(a) == k for a in got) > 5000
