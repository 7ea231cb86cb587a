"""The device update path of datasketch_amd.MinHashLSH: the merge and compaction entry points against numpy, and the index with
gpu_mode='always' against the numpy back end, a dict model, the golden answers and SortedBandsIndex at 2M rows."""
import numpy as np
import pytest

from datasketch_amd import MinHashLSH, _native
from datasketch_amd import lsh_bulk as LB
from datasketch_amd import lsh as L
from tests.test_minhash_lsh_host import GOLDEN_CASES, caller_buffer_reuse, golden_case, run_differential

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes past the output that must keep their fill byte


@pytest.fixture(scope="module")
def ctx():
    return _native.context()


def _sorted_run(rng, n, bands, spread, first_row=0):
    """Per band: digests drawn from `spread` values (ties, long runs) with rows first_row.., sorted by (digest, row)."""
    dig = rng.randint(0, spread, (bands, n)).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    rows = np.broadcast_to(np.arange(first_row, first_row + n, dtype=np.uint32), (bands, n)).copy()
    for j in range(bands):
        rng.shuffle(rows[j])
        order = np.lexsort((rows[j], dig[j]))
        dig[j], rows[j] = dig[j][order], rows[j][order]
    return dig, rows


def _guarded(ctx, nbytes):
    buf = ctx.alloc(nbytes + GUARD)
    buf.upload(np.full(nbytes + GUARD, 0xA5, dtype=np.uint8))
    return buf


def _guard_intact(buf, nbytes):
    return bool(np.all(buf.download(GUARD, np.uint8, offset=nbytes) == 0xA5))


@pytest.mark.parametrize("n_a,n_b,bands,spread", [(0, 1, 3, 5), (1, 0, 3, 5), (1, 1, 2, 1), (0, 0, 2, 1), (2047, 1, 4, 50),
                                                  (2048, 1, 4, 50), (2049, 2047, 3, 7), (4095, 4097, 2, 3), (1, 6000, 5, 100),
                                                  (20000, 333, 8, 1 << 30), (2_000_000, 10_000, 32, 1 << 20)])
@pytest.mark.parametrize("items", [8, 16])
def test_bands_merge_equals_a_sort_of_the_union(ctx, n_a, n_b, bands, spread, items):
    ctx.set_option("lsh.merge_items", items)
    try:
        _merge_case(ctx, n_a, n_b, bands, spread)
    finally:
        ctx.set_option("lsh.merge_items", 0)


def _merge_case(ctx, n_a, n_b, bands, spread):
    rng = np.random.RandomState(n_a + 7 * n_b)
    dig_a, rows_a = _sorted_run(rng, n_a, bands, spread)
    dig_b, rows_b = _sorted_run(rng, n_b, bands, spread)
    n = n_a + n_b
    d_da, d_ra, d_db, d_rb = (ctx.to_device(x) for x in (dig_a, rows_a, dig_b, rows_b))
    out_d, out_r = _guarded(ctx, 8 * bands * n), _guarded(ctx, 4 * bands * n)
    ctx.lsh_bands_merge_dev(d_da.ptr, d_ra.ptr, n_a, d_db.ptr, d_rb.ptr, n_b, n_a, bands, out_d.ptr, out_r.ptr)
    ctx.synchronize()
    assert _guard_intact(out_d, 8 * bands * n) and _guard_intact(out_r, 4 * bands * n)
    if n == 0:
        return
    got_d, got_r = out_d.download((bands, n), np.uint64), out_r.download((bands, n), np.uint32)
    dig = np.concatenate([dig_a, dig_b], axis=1)
    rows = np.concatenate([rows_a, rows_b + np.uint32(n_a)], axis=1)
    for j in range(bands):
        order = np.lexsort((rows[j], dig[j]))
        assert np.array_equal(got_d[j], dig[j][order]) and np.array_equal(got_r[j], rows[j][order]), j


def _bits(live):
    words = np.zeros((live.size + 31) // 32 * 4, dtype=np.uint8)
    packed = np.packbits(live, bitorder="little")
    words[: packed.size] = packed
    return words.view(np.uint32)


def _dead_patterns(n, rng):
    yield "none", np.ones(n, dtype=bool)
    yield "1%", rng.rand(n) >= 0.01
    yield "50%", rng.rand(n) >= 0.5
    yield "all", np.zeros(n, dtype=bool)
    run = np.ones(n, dtype=bool)
    run[29:29 + min(n, 100)] = False  # a dead run across bitmap words
    yield "run", run


@pytest.mark.parametrize("n,bands", [(1, 2), (33, 3), (5000, 4), (100_003, 8)])
def test_bands_and_rows_compaction_equal_mask_and_remap(ctx, n, bands):
    rng = np.random.RandomState(n)
    dig, rows = _sorted_run(rng, n, bands, max(2, n // 3))
    d_dig, d_rows = ctx.to_device(dig), ctx.to_device(rows)
    for row_bytes, dtype in ((1024, np.uint32), (24, np.uint64), (12, np.uint32), (5, np.uint8)):
        sig = rng.randint(0, 255, (n, row_bytes // np.dtype(dtype).itemsize)).astype(dtype)
        d_sig = ctx.to_device(sig)
        for name, live in _dead_patterns(n, rng):
            n_live = int(live.sum())
            d_bits = ctx.to_device(_bits(live))
            out = _guarded(ctx, n_live * row_bytes)
            assert ctx.rows_compact_dev(d_sig.ptr, row_bytes, n, d_bits.ptr, out.ptr) == n_live
            assert _guard_intact(out, n_live * row_bytes), name
            assert np.array_equal(out.download(sig[live].shape, dtype), sig[live]), name
            if row_bytes != 1024:
                continue
            out_d, out_r = _guarded(ctx, 8 * bands * n_live), _guarded(ctx, 4 * bands * n_live)
            ctx.lsh_bands_compact_dev(d_dig.ptr, d_rows.ptr, n, bands, d_bits.ptr, n_live, out_d.ptr, out_r.ptr)
            assert _guard_intact(out_d, 8 * bands * n_live) and _guard_intact(out_r, 4 * bands * n_live), name
            remap = (np.cumsum(live) - 1).astype(np.uint32)
            keep = live[rows]
            assert np.array_equal(out_d.download((bands, n_live), np.uint64), dig[keep].reshape(bands, n_live)), name
            assert np.array_equal(out_r.download((bands, n_live), np.uint32), remap[rows[keep]].reshape(bands, n_live)), name
            if 0 < n_live < n:  # a wrong n_live is an error, and nothing is written
                small = _guarded(ctx, 0)
                with pytest.raises(ValueError):
                    ctx.lsh_bands_compact_dev(d_dig.ptr, d_rows.ptr, n, bands, d_bits.ptr, n_live + 1, small.ptr, small.ptr)
                with pytest.raises(ValueError):
                    ctx.lsh_bands_compact_dev(d_dig.ptr, d_rows.ptr, n, bands, d_bits.ptr, n_live - 1, small.ptr, small.ptr)
                assert _guard_intact(small, 0)


def test_entry_points_reject_bad_arguments(ctx):
    lib, h = ctx.lib, ctx.handle
    assert lib.mhx_lsh_bands_merge_dev(None, None, None, 1, None, None, 1, 0, 1, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_merge_dev(h, None, None, 1, None, None, 1, 0, 1, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_merge_dev(h, None, None, -1, None, None, 1, 0, 1, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_merge_dev(h, None, None, 1 << 31, None, None, 1 << 31, 0, 1, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_compact_dev(h, None, None, 10, 2, None, 3, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_compact_dev(h, None, None, 10, 2, None, 11, None, None) == _native.MHX_ERR_INVALID
    assert lib.mhx_lsh_bands_compact_dev(h, None, None, 1 << 32, 2, None, 0, None, None) == _native.MHX_ERR_INVALID
    import ctypes

    kept = ctypes.c_int64(7)
    assert lib.mhx_rows_compact_dev(h, None, 8, 10, None, None, ctypes.byref(kept)) == _native.MHX_ERR_INVALID and kept.value == 0
    assert lib.mhx_rows_compact_dev(h, None, 0, 10, None, None, ctypes.byref(kept)) == _native.MHX_ERR_INVALID
    assert lib.mhx_rows_compact_dev(h, None, 8, 10, None, None, None) == _native.MHX_ERR_INVALID
    assert _native.last_error()
    with pytest.raises(ValueError):
        ctx.set_option("lsh.merge_items", 12)


def _stable_bands(index):
    """A stable sort by digest of the band digests of the slots the device bands hold, numbered by slot."""
    mat = index._backend.matrix()
    dig = LB.band_digests(mat, index.b, index._backend.r, gpu_mode="disable").T
    order = np.argsort(dig, axis=1, kind="stable")
    return np.take_along_axis(dig, order, axis=1), order.astype(np.uint32)


@pytest.mark.parametrize("variant,prepickle", [("u32", False), ("u64", True), ("weighted", False)])
def test_incremental_index_equals_from_scratch_and_the_numpy_back_end(variant, prepickle, monkeypatch):
    checked = {"flush": 0, "compact": 0}

    def from_scratch(index, what):
        """After every flush and every compaction of the device index: its bands are the stable sort by digest of the band
        digests of the slots it holds, numbered by slot; after a compaction those slots are exactly the live ones."""
        if not isinstance(index._backend, L._DeviceBands):
            return
        d_dig, d_rows = index._backend.bands()
        s_dig, s_rows = _stable_bands(index)
        assert np.array_equal(d_dig, s_dig) and np.array_equal(d_rows, s_rows), what
        if what == "compact":
            assert index._n_dead == 0 and np.all(index._slot_kid[: index._n_flushed] >= 0)
        checked[what] += 1

    upload, compact = MinHashLSH._upload_pending, MinHashLSH._compact

    def upload_and_check(self):
        had = bool(self._pending)
        upload(self)
        if had:
            from_scratch(self, "flush")

    def compact_and_check(self):
        had = self._n_dead
        compact(self)
        if had:
            from_scratch(self, "compact")

    monkeypatch.setattr(MinHashLSH, "_upload_pending", upload_and_check)
    monkeypatch.setattr(MinHashLSH, "_compact", compact_and_check)

    def same_as_numpy(lshs, step):
        """After every operation: the same slots, the same bands and the same matrix as the numpy back end."""
        dev, host = lshs
        if dev._backend is None:
            return
        assert dev._n_flushed == host._n_flushed and dev._n_slots == host._n_slots, step
        d_dig, d_rows = dev._backend.bands()
        h_dig, h_rows = host._backend.bands()
        assert np.array_equal(d_dig, h_dig) and np.array_equal(d_rows, h_rows), step
        assert np.array_equal(dev._backend.matrix(), host._backend.matrix().astype(dev._backend.dtype)), step

    run_differential(["always", "disable"], variant, prepickle, seed=1 + ["u32", "u64", "weighted"].index(variant), after_op=same_as_numpy)
    assert checked["flush"] > 100 and checked["compact"] >= 3, checked


@pytest.mark.parametrize("kind", ["u32", "u64", "weighted"])
def test_insert_bulk_takes_the_values_at_call_time_on_the_device(kind):
    caller_buffer_reuse("always", kind)


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_golden_answers_on_the_device(case):
    one = golden_case(case, "always")
    assert type(one._backend).__name__ == "_DeviceBands"


def test_two_million_rows_in_batches_removals_and_queries():
    rng = np.random.RandomState(5)
    n, k = 2_000_000, 256
    sig = rng.randint(0, 2**32, (n, k), dtype=np.uint32)
    sig[1::1000, :8] = sig[0, :8]  # a bucket shared in band 0
    keys = [f"doc-{i}" for i in range(n)]
    index = MinHashLSH(num_perm=k, params=(32, 8), gpu_mode="always")
    for part in np.array_split(np.arange(n), 8):
        index.insert_bulk([keys[i] for i in part], sig[part])
    gone = rng.rand(n) < 0.3
    for i in np.flatnonzero(gone):
        index.remove(keys[i])
    more = rng.randint(0, 2**32, (10_000, k), dtype=np.uint32)
    more_keys = [f"new-{i}" for i in range(more.shape[0])]
    index.insert_bulk(more_keys, more)
    probes = np.concatenate([sig[rng.randint(0, n, 5000)], more[:2500], rng.randint(0, 2**32, (2500, k), dtype=np.uint64).astype(np.uint32)])
    probes[::4, 100:] = 1
    got = index.query_bulk(probes)
    assert index._n_dead == 0  # 30 % dead: the query compacted first
    live_mat = np.concatenate([sig[~gone], more])
    live_keys = [keys[i] for i in np.flatnonzero(~gone)] + more_keys
    ctx = _native.context()
    want_d, want_r = ctx.lsh_sort_bands(live_mat, 32, 8)
    got_d, got_r = index._backend.bands()
    assert np.array_equal(got_d, want_d) and np.array_equal(got_r, want_r)
    offsets, rows = LB.SortedBandsIndex(live_mat, 32, 8).query(probes)
    for i in range(probes.shape[0]):
        assert sorted(got[i]) == sorted(live_keys[j] for j in rows[offsets[i] : offsets[i + 1]]), i
    assert sum(map(len, got)) > probes.shape[0]


def test_bulk_query_with_more_band_searches_than_threads():
    """40 000 probes x 32 bands = 1.28M (probe, band) searches: more than the 256 CUs x 16 workgroups x 256 threads the ranges and
    emit kernels are launched with, so their grid-stride loops go round.  Against the numpy back end."""
    rng = np.random.RandomState(11)
    n, m, bands, r = 2000, 40_000, 32, 2
    sig = rng.randint(0, 64, (n, bands * r)).astype(np.uint32)  # 4096 keys per band: about half the probes' bands meet a row
    probes = rng.randint(0, 64, (m, bands * r)).astype(np.uint32)
    host, device = L._HostBands(bands * r, bands, r, np.uint32), L._DeviceBands(_native.context(), bands * r, bands, r, np.uint32)
    host.append(sig)
    device.append(sig)
    want, got = host.query(probes), device.query(probes)
    print(f"{m * bands} searches, {want[1].size} (probe, row) pairs")
    assert want[1].size > m
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
