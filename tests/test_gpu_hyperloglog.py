"""HyperLogLog on the device (run on an MI355X: python -m pytest tests -m gpu).

Expected values are the numpy twin of datasketch_amd.hyperloglog -- pinned to the reference by tests/test_hyperloglog_host.py --
and the fixture tests/golden/hyperloglog.json.  Shapes are the smallest at which each path of hll_kernels.hip is taken: every
LDS layout and both sides of every switch between them (read from mhx_hll_layout, not guessed), sets around the wave size, more
workgroups than one, and the split path forced by a low "hll.split_tokens".
"""
import ctypes
import json

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, _native, prehashed, sha1_hash32, sha1_hash64
from datasketch_amd import hyperloglog as H
from tests.test_hyperloglog_host import GOLDEN, KINDS, edge_hashes

pytestmark = pytest.mark.gpu

RAGGED = (0, 1, 63, 64, 65, 257, 5000)
COMBOS = ((np.uint32, 32), (np.uint32, 64), (np.uint64, 32), (np.uint64, 64))


def p_values():
    """4, 8, 16 and the p on either side of every layout switch of the dispatch."""
    ps = {4, 8, 16}
    for p in range(4, 16):
        if _native.hll_layout(p) != _native.hll_layout(p + 1):
            ps |= {p, p + 1}
    return sorted(ps)


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    return _native.context()


def hashes(rng, n, dtype, bits):
    """n random hashes of `dtype` that fit `bits`, with long runs of leading zeros among them (high ranks)."""
    wide = dtype == np.uint64 and bits == 64
    hv = rng.randint(0, 2**32, size=n, dtype=np.uint64)
    if wide:
        hv = (hv << np.uint64(32)) | rng.randint(0, 2**32, size=n, dtype=np.uint64)
    hv >>= rng.randint(0, 64 if wide else 32, size=n).astype(np.uint64)
    return hv.astype(dtype)


def csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def check(ctx, hv, offsets, fixed_len, n, p, bits, init=None):
    got, overflow = ctx.hll_bulk(hv, offsets, fixed_len, n, p, bits, init)
    want = H._registers_host(hv, offsets, fixed_len, n, p, bits, init)
    assert overflow == 0
    assert got.shape == want.shape and np.array_equal(got, want), (p, bits, hv.dtype, np.argwhere(got != want)[:5].tolist())
    return got


def test_ragged_sets_every_layout_dtype_and_hash_width(ctx):
    assert len({_native.hll_layout(p) for p in p_values()}) == 3  # every layout of the dispatch is reached
    rng = np.random.RandomState(4)
    lengths = list(RAGGED) + list(RAGGED[::-1])
    for p in p_values():
        for dtype, bits in COMBOS:
            check(ctx, hashes(rng, sum(lengths), dtype, bits), csr(lengths), 0, len(lengths), p, bits)


@pytest.mark.parametrize("n", [1, 3, 1000])
def test_call_shapes(ctx, n):
    rng = np.random.RandomState(n)
    for p in (5, 10) if n == 1000 else p_values():
        for dtype, bits in COMBOS[::3]:
            check(ctx, hashes(rng, n * 37, dtype, bits), None, 37, n, p, bits)  # fixed_len, NULL offsets
            lengths = rng.randint(0, 90, size=n)
            check(ctx, hashes(rng, int(lengths.sum()), dtype, bits), csr(lengths), 0, n, p, bits)


def test_collisions_one_register_and_every_register(ctx):
    rng = np.random.RandomState(5)
    for p in p_values():
        m = 1 << p
        one = (hashes(rng, 5000, np.uint64, 64) << np.uint64(p)) | np.uint64(m - 3)  # every lane contends for one word
        every = (rng.randint(0, 2**16, size=m, dtype=np.uint64) << np.uint64(p)) | rng.permutation(m).astype(np.uint64)
        hv = np.concatenate([one, every])
        got = check(ctx, hv, csr([one.size, every.size]), 0, 2, p, 64)
        assert np.count_nonzero(got[0]) == 1 and np.count_nonzero(got[1]) == m
        check(ctx, (hv & np.uint64(0xFFFFFFFF)).astype(np.uint32), csr([one.size, every.size]), 0, 2, p, 32)


def test_edge_hashes_of_the_golden_file(ctx):
    with open(GOLDEN) as f:
        golden = json.load(f)
    for key, rows in golden["edges"].items():
        kind, p = key.split("-")
        bits, p = KINDS[kind], int(p[1:])
        hv = np.array(edge_hashes(bits, p), dtype=np.uint64)
        for dtype in (np.uint64, np.uint32) if int(hv.max()) < 2**32 else (np.uint64,):
            got, overflow = ctx.hll_bulk(hv.astype(dtype), None, 1, hv.size, p, bits)
            assert overflow == 0
            for row, (_, idx, rank) in zip(got, rows):
                assert np.flatnonzero(row).tolist() == [idx] and row[idx] == rank, (key, dtype)


def test_overflow_is_counted_and_raised(ctx):
    hv = np.array([5, 1 << 32, 7, (1 << 64) - 1], dtype=np.uint64)
    _, overflow = ctx.hll_bulk(hv, None, 2, 2, 8, 32)
    assert overflow == 2
    assert ctx.hll_bulk(hv, None, 2, 2, 8, 64)[1] == 0
    with pytest.raises(ValueError, match="Hash value overflow"):
        HyperLogLog.bulk_registers(hv.reshape(2, 2), p=8, hashfunc=prehashed, gpu_mode="always")
    with pytest.raises(ValueError, match="Hash value overflow"):
        HyperLogLog(8, hashfunc=prehashed, gpu_mode="always").update_batch(hv)


def test_init_rows_and_update_batch(ctx):
    rng = np.random.RandomState(9)
    for p in p_values():
        m = 1 << p
        lengths = [0, 40, 0, 700]
        hv = hashes(rng, sum(lengths), np.uint32, 32)
        shared, per_row = rng.randint(0, 20, size=m).astype(np.uint8), rng.randint(0, 20, size=(4, m)).astype(np.uint8)
        got = check(ctx, hv, csr(lengths), 0, 4, p, 32, shared)
        assert np.array_equal(got[0], shared) and np.array_equal(got[2], shared)  # an empty set keeps its init row
        got = check(ctx, hv, csr(lengths), 0, 4, p, 32, per_row)
        assert np.array_equal(got[2], per_row[2])
        on, off = HyperLogLog(p, hashfunc=prehashed, gpu_mode="always"), HyperLogLog(p, hashfunc=prehashed, gpu_mode="disable")
        for part in (hv[:300], hv[300:]):
            on.update_batch(part)
            off.update_batch(part)
            assert on == off and on.reg.dtype == np.int8
    words = [b"w%d" % i for i in range(999)]
    on, off = HyperLogLog(gpu_mode="always"), HyperLogLog(gpu_mode="disable")
    on.update_batch(words)
    off.update_batch(words)
    assert on == off and on.count() == off.count()


def test_split_sets_give_the_same_bytes(ctx):
    rng = np.random.RandomState(11)
    try:
        for p in (4, 16):
            for dtype, bits in COMBOS[::3]:
                lengths = [3, 0, 20000, 70, 999, 1001, 5]  # one set far over the threshold, one at it, one just over, short ones around
                hv, offsets = hashes(rng, sum(lengths), dtype, bits), csr(lengths)
                init = rng.randint(0, 9, size=(len(lengths), 1 << p)).astype(np.uint8)
                ctx.set_option("hll.split_tokens", 0)
                whole = check(ctx, hv, offsets, 0, len(lengths), p, bits, init)
                one = check(ctx, hv[:20000], None, 20000, 1, p, bits)
                ctx.set_option("hll.split_tokens", 1000)
                assert np.array_equal(check(ctx, hv, offsets, 0, len(lengths), p, bits, init), whole)
                assert np.array_equal(check(ctx, hv[:20000], None, 20000, 1, p, bits), one)  # fixed length: every set splits
                assert np.array_equal(check(ctx, hv[:18000], None, 6000, 3, p, bits), H._registers_host(hv[:18000], None, 6000, 3, p, bits, None))
    finally:
        ctx.set_option("hll.split_tokens", 0)


def test_byte_tokens_through_the_sha1_kernel(ctx):
    rng = np.random.RandomState(13)
    sets = [[bytes(rng.randint(0, 256, size=rng.randint(0, 70), dtype=np.uint8)) for _ in range(n)] for n in (0, 1, 65, 300, 0, 2)]
    buf, byte_offsets, set_offsets = _native.Context.pack_sets(sets)
    for p in (4, 9, 14):
        for bits, f in ((32, sha1_hash32), (64, sha1_hash64)):
            hv = np.array([f(t) for s in sets for t in s], dtype=np.uint64)
            want = H._registers_host(hv, set_offsets, 0, len(sets), p, bits, None)
            assert np.array_equal(ctx.hll_bulk_bytes(buf, byte_offsets, set_offsets, p, bits), want)
            assert np.array_equal(HyperLogLog.bulk_registers(sets, p=p, hashfunc=f, hash_bits=bits, gpu_mode="always"), want.view(np.int8))
    assert [h.reg.tolist() for h in HyperLogLog.bulk(sets, p=6, gpu_mode="always")] == [h.reg.tolist() for h in HyperLogLog.bulk(sets, p=6, gpu_mode="disable")]


def test_histogram_merge_union_and_count_many(ctx):
    rng = np.random.RandomState(15)
    for p, n in ((4, 1), (8, 1001), (12, 7), (16, 3)):
        m = 1 << p
        reg = rng.randint(0, 30, size=(n, m)).astype(np.uint8)
        reg[0] = 0
        hist, invalid = ctx.hll_histogram(reg)
        assert invalid == 0 and np.array_equal(hist, np.stack([np.bincount(r, minlength=64) for r in reg]))
        assert np.array_equal(hist, H._histogram_host(reg))
        bad = reg.copy()
        bad[-1, 5], bad[-1, m - 1] = 64, 255
        hist, invalid = ctx.hll_histogram(bad)
        assert invalid == 2 and hist[-1].sum() == m - 2
        other = rng.randint(0, 30, size=(n, m)).astype(np.uint8)
        assert np.array_equal(ctx.hll_merge(reg, other), np.maximum(reg, other))
        assert np.array_equal(H.merge_many(reg.view(np.int8), other.view(np.int8), gpu_mode="always"), np.maximum(reg, other).view(np.int8))
        groups = np.array(sorted([0, 0, n] + rng.randint(0, n + 1, size=4).tolist() + [min(1, n)] * 2), dtype=np.int64)  # empty and single-row groups
        assert np.array_equal(H.union_groups(reg, groups, gpu_mode="always"), H.union_groups(reg, groups, gpu_mode="disable"))
    for p in (4, 8, 12):  # registers of real sets on both sides of the small-range threshold, the large range and a saturated row
        m = 1 << p
        sets = [rng.randint(0, 2**32, size=c, dtype=np.uint64) for c in (0, 1, m // 2, 2 * m, 3 * m, 40 * m)]
        reg = HyperLogLog.bulk_registers((np.concatenate(sets), csr([s.size for s in sets])), p=p, hashfunc=prehashed, gpu_mode="always")
        reg = np.concatenate([reg, np.full((1, m), 32 - p - 1, dtype=np.int8), np.full((1, m), 32 - p + 1, dtype=np.int8)])
        on, off = H.count_many(reg, gpu_mode="always"), H.count_many(reg, gpu_mode="disable")
        assert np.array_equal(on, off, equal_nan=True) and np.isnan(on[-1]) and np.all(on[1:-1] > 0)


def test_argument_errors_are_a_status_and_a_message(ctx):
    hv, out = np.zeros(8, dtype=np.uint32), np.zeros((2, 256), dtype=np.uint8)
    for p, bits, n, offsets, words in ((3, 32, 2, None, "range [4 : 16]"), (17, 32, 2, None, "range [4 : 16]"), (8, 48, 2, None, "hash_bits"),
                                       (8, 32, -1, None, "n_sets"), (8, 32, 2, np.array([0, 5, 3], dtype=np.int64), "non-decreasing")):
        rc = ctx.lib.mhx_hll_bulk_typed(ctx.handle, hv.ctypes.data, _native.MHX_U32, None if offsets is None else offsets.ctypes.data, 4, n, p, bits,
                                        None, 0, out.ctypes.data, None)
        assert rc == _native.MHX_ERR_INVALID and words in _native.last_error(), (p, bits, n, _native.last_error())
    rc = ctx.lib.mhx_hll_bulk_typed(ctx.handle, hv.view(np.uint64).ctypes.data, _native.MHX_U64, None, 2, 2, 8, 32, None, 0, out.ctypes.data, None)
    assert rc == _native.MHX_ERR_INVALID and "overflow counter" in _native.last_error()
    rc = ctx.lib.mhx_hll_bulk_typed(ctx.handle, hv.ctypes.data, 7, None, 4, 2, 8, 32, None, 0, out.ctypes.data, None)
    assert rc == _native.MHX_ERR_INVALID and "hv_dtype" in _native.last_error()
    with pytest.raises(ValueError, match="non-decreasing"):
        ctx.hll_union_groups(out, np.array([0, 2, 1], dtype=np.int64))
    with pytest.raises(ValueError, match="inside"):
        ctx.hll_union_groups(out, np.array([0, 3], dtype=np.int64))
    with pytest.raises(ValueError, match="unknown option"):
        ctx.set_option("hll.split", 1)
    with pytest.raises(ValueError, match="hll.split_tokens"):
        ctx.set_option("hll.split_tokens", -1)


def test_every_hyperloglog_entry_point_rejects_a_bad_argument(ctx):
    lib, h, INVALID = ctx.lib, ctx.handle, _native.MHX_ERR_INVALID
    d = ctx.alloc(4096)
    host = np.zeros(1024, dtype=np.uint8)
    off = np.array([0, 1], dtype=np.int64)
    layout = ctypes.c_int(0)
    count = ctypes.c_int64(0)
    calls = {
        "mhx_hll_layout": lambda: lib.mhx_hll_layout(3, ctypes.byref(layout)),
        "mhx_hll_bulk_dev": lambda: lib.mhx_hll_bulk_dev(h, d.ptr, _native.MHX_U32, None, 4, 1, 4, 17, 32, None, 0, d.ptr + 1024, None),
        "mhx_hll_bulk_typed": lambda: lib.mhx_hll_bulk_typed(h, host.ctypes.data, _native.MHX_U32, None, -1, 1, 8, 32, None, 0, host.ctypes.data, None),
        "mhx_hll_bulk_bytes": lambda: lib.mhx_hll_bulk_bytes(h, host.ctypes.data, off.ctypes.data, 1, 16, off.ctypes.data, 1, 8, None, 0, host.ctypes.data),
        "mhx_hll_histogram_dev": lambda: lib.mhx_hll_histogram_dev(h, d.ptr, -1, 8, d.ptr + 1024, d.ptr + 2048),
        "mhx_hll_histogram": lambda: lib.mhx_hll_histogram(h, host.ctypes.data, 1, 2, host.ctypes.data, ctypes.byref(count)),
        "mhx_hll_merge_dev": lambda: lib.mhx_hll_merge_dev(h, d.ptr, d.ptr + 1024, -1),
        "mhx_hll_union_groups_dev": lambda: lib.mhx_hll_union_groups_dev(h, d.ptr + 1, 1, 8, d.ptr + 2048, 1, d.ptr + 1024),
        "mhx_hll_union_groups": lambda: lib.mhx_hll_union_groups(h, host.ctypes.data, 1, 20, off.ctypes.data, 1, host.ctypes.data),
    }
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_EXT
    for name, call in calls.items():
        assert call() == INVALID and _native.last_error(), name
    assert lib.mhx_hll_bulk_dev(None, d.ptr, _native.MHX_U32, None, 4, 1, 4, 8, 32, None, 0, d.ptr + 1024, None) == INVALID
