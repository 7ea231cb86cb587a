"""The update path of the sorted-band index and the digest layouts of include/mhx.h on buffers that abut an unmapped page (test
infrastructure, run as a script in a process of its own by tests/test_gpu_index_guard.py -- a kernel that over-reads kills the
process).

    python tests/index_guard_cases.py <align>       all cases; prints "INDEX GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: every input and every output of a call is a separate exact-size
allocation from mhx_debug_guard_alloc, outputs pre-filled with a pattern, and the results are checked against numpy or the
gpu_mode="disable" host twins.  mhx_lsh_bands_merge_dev (both merge tiles; odd counts, so that bands 1 and 2 of every array
start on an address that is no multiple of 16), mhx_lsh_bands_compact_dev and mhx_rows_compact_dev (a bitmap of exactly
ceil(n / 32) words, the four access units of a row), mhx_band_digests_layout_dev, mhx_lsh_sort_digests_layout_dev and
mhx_bbit_pack_band_digests_dev (both layouts, both element types, a shape that can fuse and one that cannot).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, b_bit_minhash, lsh_bulk  # noqa: E402
from datasketch_amd._native import BAND_MAJOR, MHX_U32, MHX_U64, ROW_MAJOR, check  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _begin, _dev, _done, _expect  # noqa: E402
from tests.test_gpu_minhash_lsh import _dead_patterns, _sorted_run  # noqa: E402

PATTERN = 0xA5


def _untouched(buf, what):
    """An output of zero bytes is a pointer to one byte the call must leave alone."""
    _expect(buf.download((1,), np.uint8), np.full(1, PATTERN, dtype=np.uint8), what + ": an output of zero bytes was written")


def merge_cases(ctx):
    for items in (8, 16):
        ctx.set_option("lsh.merge_items", items)
        for n_a, n_b, bands in ((0, 1, 3), (1, 0, 3), (1, 1, 1), (2047, 2, 3), (2049, 2047, 3)):
            what = f"bands merge items={items} {n_a}+{n_b} rows, {bands} bands"
            rng = np.random.RandomState(n_a + 7 * n_b)
            dig_a, rows_a = _sorted_run(rng, n_a, bands, 7)  # digests from 7 values: ties, long runs
            dig_b, rows_b = _sorted_run(rng, n_b, bands, 7)
            n = n_a + n_b
            _begin(what)
            d_da, d_ra, d_db, d_rb = (_dev(ctx, x) for x in (dig_a, rows_a, dig_b, rows_b))
            out_d, out_r = _alloc(ctx, 8 * bands * n), _alloc(ctx, 4 * bands * n)
            ctx.lsh_bands_merge_dev(d_da.ptr, d_ra.ptr, n_a, d_db.ptr, d_rb.ptr, n_b, n_a, bands, out_d.ptr, out_r.ptr)
            dig = np.concatenate([dig_a, dig_b], axis=1)
            rows = np.concatenate([rows_a, rows_b + np.uint32(n_a)], axis=1)
            order = np.stack([np.lexsort((rows[j], dig[j])) for j in range(bands)])
            _expect(out_d.download((bands, n), np.uint64), np.take_along_axis(dig, order, axis=1), what + " digests")
            _expect(out_r.download((bands, n), np.uint32), np.take_along_axis(rows, order, axis=1), what + " rows")
            _done(what)
    ctx.set_option("lsh.merge_items", 0)


def compact_cases(ctx):
    bands = 3
    for n in (1, 33, 5001):
        rng = np.random.RandomState(n)
        dig, rows = _sorted_run(rng, n, bands, max(2, n // 3))
        d_dig, d_rows = _dev(ctx, dig), _dev(ctx, rows)
        matrices = []
        for row_bytes, dtype in ((1024, np.uint32), (24, np.uint64), (12, np.uint32), (5, np.uint8)):  # the four access units
            sig = rng.randint(0, 255, (n, row_bytes // np.dtype(dtype).itemsize)).astype(dtype)
            matrices.append((row_bytes, sig, _dev(ctx, sig)))
        for name, live in _dead_patterns(n, rng):
            if name == "1%":
                continue
            n_live = int(live.sum())
            d_bits = _dev(ctx, lsh_bulk.live_bits(live))  # exactly ceil(n / 32) words
            for row_bytes, sig, d_sig in matrices:
                what = f"rows compact n={n} row_bytes={row_bytes} dead: {name}"
                _begin(what)
                out = _alloc(ctx, max(1, n_live * row_bytes))
                kept = ctx.rows_compact_dev(d_sig.ptr, row_bytes, n, d_bits.ptr, out.ptr)
                assert kept == n_live, (what, kept, n_live)
                if n_live:
                    _expect(out.download(sig[live].shape, sig.dtype), sig[live], what)
                else:
                    _untouched(out, what)
                _done(what)
            what = f"bands compact n={n} dead: {name}"
            _begin(what)
            out_d, out_r = _alloc(ctx, max(1, 8 * bands * n_live)), _alloc(ctx, max(1, 4 * bands * n_live))
            ctx.lsh_bands_compact_dev(d_dig.ptr, d_rows.ptr, n, bands, d_bits.ptr, n_live, out_d.ptr, out_r.ptr)
            if n_live:
                remap = (np.cumsum(live) - 1).astype(np.uint32)
                keep = live[rows]
                _expect(out_d.download((bands, n_live), np.uint64), dig[keep].reshape(bands, n_live), what + " digests")
                _expect(out_r.download((bands, n_live), np.uint32), remap[rows[keep]].reshape(bands, n_live), what + " rows")
            else:
                _untouched(out_d, what + " digests")
                _untouched(out_r, what + " rows")
            _done(what)


def digest_cases(ctx):
    rng = np.random.RandomState(51)
    for n in (1, 67, 128):
        # bands * r < num_perm: the two kernels one after the other; (8, 4, 32): the shape that can fuse
        for bands, r, num_perm, bits in ((3, 5, 17, 3), (8, 4, 32, 4)):
            values = rng.randint(0, 2**32, size=(n, num_perm), dtype=np.uint64)
            values[n // 2:] = values[: n - n // 2]  # equal digests: runs in the sort
            dig = lsh_bulk.band_digests(values, bands, r, gpu_mode="disable")
            blocks = b_bit_minhash.pack_matrix(values, bits, gpu_mode="disable")
            order = np.argsort(dig.T, axis=1, kind="stable")
            want_rows, want_sorted = order.astype(np.uint32), np.take_along_axis(dig.T, order, axis=1)
            for dtype, code in ((np.uint32, MHX_U32), (np.uint64, MHX_U64)):
                d_sig = _dev(ctx, values.astype(dtype))
                for layout, ref in ((ROW_MAJOR, dig), (BAND_MAJOR, np.ascontiguousarray(dig.T))):
                    shape = f"n={n} bands={bands} r={r} K={num_perm} {np.dtype(dtype).name} layout={layout}"
                    what = "band digests " + shape
                    _begin(what)
                    d_dig = _alloc(ctx, 8 * n * bands)
                    check(ctx.lib.mhx_band_digests_layout_dev(ctx.handle, d_sig.ptr, code, n, num_perm, bands, r, layout, d_dig.ptr))
                    _expect(d_dig.download(ref.shape, np.uint64), ref, what)
                    _done(what)
                    what = "sort digests " + shape
                    _begin(what)
                    d_in, d_sd, d_sr = _dev(ctx, ref), _alloc(ctx, 8 * n * bands), _alloc(ctx, 4 * n * bands)
                    check(ctx.lib.mhx_lsh_sort_digests_layout_dev(ctx.handle, d_in.ptr, n, bands, layout, d_sd.ptr, d_sr.ptr))
                    _expect(d_sr.download((bands, n), np.uint32), want_rows, what + " rows")
                    _expect(d_sd.download((bands, n), np.uint64), want_sorted, what + " digests")
                    _done(what)
                    what = f"pack and digests b={bits} " + shape  # (whether it fused is the base address's to decide: not asserted)
                    _begin(what)
                    d_blk, d_dig = _alloc(ctx, blocks.nbytes), _alloc(ctx, 8 * n * bands)
                    ctx.bbit_pack_band_digests_dev(d_sig.ptr, code, n, num_perm, bits, bands, r, d_blk.ptr, d_dig.ptr, layout)
                    _expect(d_blk.download(blocks.shape, np.uint64), blocks, what + " blocks")
                    _expect(d_dig.download(ref.shape, np.uint64), ref, what + " digests")
                    _done(what)


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    merge_cases(ctx)
    compact_cases(ctx)
    digest_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"INDEX GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"INDEX GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
