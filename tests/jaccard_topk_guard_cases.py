"""The top-k Jaccard device entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a
script in a process of its own by tests/test_gpu_jaccard_topk_guard.py -- a kernel that over-reads kills the process).

    python tests/jaccard_topk_guard_cases.py <align>        all cases; prints "TOPK GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: A, B, the live-bit map, rows and counts of every call are separate
exact-size allocations from mhx_debug_guard_alloc (the library's scratch for the partial lists is one too), outputs pre-filled
with a pattern, and the results are checked against numpy.  Both kernels (strip, stream), B cut into one and into several
segments, dense uint32 / uint64 rows and b-bit blocks, with and without the map, A against itself.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, b_bit_minhash, lsh_bulk  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64, check  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect, _p  # noqa: E402


def _want(a, b, k, min_count, self_join, live):
    rows, counts = lsh_bulk._topk_from_blocks(lsh_bulk._equal_counts_blocks(a, None if self_join else b), a.shape[0], k, min_count,
                                              self_join, live)
    return rows, counts.astype(np.int32)


def one_call(ctx, a, b, num_perm, k, what, bits=None, live=None, min_count=0):
    """a / b: the rows as the entry takes them (dense, or values to pack); b None: A against itself."""
    values_a, values_b = a, b
    if bits is not None:
        mask = np.uint64((1 << bits) - 1)
        values_a, values_b = a & mask, None if b is None else b & mask
        a = b_bit_minhash.pack_matrix(a, bits, gpu_mode="disable")
        b = None if b is None else b_bit_minhash.pack_matrix(b, bits, gpu_mode="disable")
    m, n_b = a.shape[0], 0 if b is None else b.shape[0]
    d_a, d_b = _dev(ctx, a), None if b is None else _dev(ctx, b)
    d_live = None if live is None else _dev(ctx, lsh_bulk.live_bits(live))
    d_rows, d_counts = _alloc(ctx, 8 * m * k), _alloc(ctx, 4 * m * k)
    if bits is None:
        check(ctx.lib.mhx_jaccard_topk_dev(ctx.handle, _p(d_a), m, _p(d_b), n_b, MHX_U32 if a.dtype == np.uint32 else MHX_U64, num_perm,
                                           _p(d_live), min_count, k, _p(d_rows), _p(d_counts)))
    else:
        check(ctx.lib.mhx_bbit_jaccard_topk_dev(ctx.handle, _p(d_a), m, _p(d_b), n_b, num_perm, bits, _p(d_live), min_count, k, _p(d_rows),
                                                _p(d_counts)))
    rows, counts = _want(values_a, values_a if values_b is None else values_b, k, min_count, b is None, live)
    _expect(d_rows.download((m, k), np.int64), rows, what + " rows")
    _expect(d_counts.download((m, k), np.int32), counts, what + " counts")
    _done(what)


def planted(rng, m, n, k, dtype):
    a = rng.randint(0, 1 << 32, size=(m, k), dtype=np.uint64)
    b = rng.randint(0, 1 << 32, size=(n, k), dtype=np.uint64)
    src = rng.randint(0, m, size=n)
    keep = rng.random_sample((n, k)) < rng.random_sample((n, 1))
    b[keep] = a[src][keep]
    return a.astype(dtype), b.astype(dtype)


def dense_cases(ctx):
    rng = np.random.RandomState(31)
    for path in (1, 2):  # strip, stream
        ctx.set_option("jaccard.topk_path", path)
        for segments in (0, 3):
            ctx.set_option("jaccard.topk_segments", segments)
            for dtype in (np.uint32, np.uint64):
                for m, n, k_perm in ((1, 1, 1), (2, 63, 3), (3, 385, 100), (129, 257, 128), (5, 300, 321)):
                    a, b = planted(rng, m, n, k_perm, dtype)
                    name = f"topk path={path} segments={segments} {np.dtype(dtype).name} {m}x{n}x{k_perm}"
                    live = rng.random_sample(n) < 0.8
                    one_call(ctx, a, b, k_perm, 10, name)
                    one_call(ctx, a, b, k_perm, 64, name + " k=64 live floor", live=live, min_count=k_perm // 3)
                    one_call(ctx, b, None, k_perm, 7, name + " self", live=live)
    ctx.set_option("jaccard.topk_path", 0)
    ctx.set_option("jaccard.topk_segments", 0)


def bbit_cases(ctx):
    rng = np.random.RandomState(32)
    for segments in (0, 2):
        ctx.set_option("jaccard.topk_segments", segments)
        for bits in (1, 2, 4, 8, 16, 32):
            for m, n, k_perm in ((1, 1, 1), (3, 200, 100), (130, 257, 128)):
                a, b = planted(rng, m, n, k_perm, np.uint64)
                name = f"bbit topk b={bits} segments={segments} {m}x{n}x{k_perm}"
                live = rng.random_sample(n) < 0.8
                one_call(ctx, a, b, k_perm, 10, name, bits=bits)
                one_call(ctx, a, b, k_perm, 64, name + " k=64 live floor", bits=bits, live=live, min_count=k_perm // 2)
                one_call(ctx, b, None, k_perm, 7, name + " self", bits=bits, live=live)
    ctx.set_option("jaccard.topk_segments", 0)


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    dense_cases(ctx)
    bbit_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"TOPK GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"TOPK GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
