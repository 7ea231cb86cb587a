"""The Bloom-filter device entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a
script in a process of its own by tests/test_gpu_bloom_guard.py -- a kernel that over-reads kills the process).

    python tests/bloom_guard_cases.py <align>        all cases; prints "BLOOM GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: signatures, filter and answers of every call are separate exact-size
allocations from mhx_debug_guard_alloc, the answers pre-filled with a pattern, and the results are checked against the numpy
twin.  Row counts that are no multiple of the rows a workgroup takes, band counts that leave lanes idle and filters of one,
three or 1001 blocks are the point; both lane mappings and the default mix of them run.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native  # noqa: E402
from datasketch_amd import lsh_bloom as B  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64, check  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect, _p  # noqa: E402


def filter_cases(ctx):
    rng = np.random.RandomState(31)
    lib = ctx.lib
    for num_perm, b, r in ((16, 2, 1), (16, 3, 5), (128, 9, 13), (128, 32, 4), (128, 128, 1), (5, 5, 1), (37, 2, 17)):
        for n, nb, k in ((1, 1, 1), (63, 3, 7), (65, 1001, 8), (129, 2, 15), (1000, 3, 32)):
            for dtype, code in ((np.uint32, MHX_U32), (np.uint64, MHX_U64)):
                what = f"bloom n={n} K={num_perm} b={b} r={r} blocks={nb} k={k} {np.dtype(dtype).name}"
                sig = rng.randint(0, 2**32 if dtype == np.uint32 else 2**64, size=(n, num_perm), dtype=np.uint64).astype(dtype)
                old = rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x10001)
                want = old.copy()
                B.insert_host(want, sig[: n // 2 + 1], r, k)
                d_sig, d_half, d_filter, d_hit = _dev(ctx, sig), _dev(ctx, sig[: n // 2 + 1]), _dev(ctx, old), _alloc(ctx, n)
                check(lib.mhx_bloom_insert_dev(ctx.handle, _p(d_half), code, n // 2 + 1, num_perm, b, r, k, nb, _p(d_filter)))
                _expect(d_filter.download((b, nb, 16), np.uint32), want, what + " insert")
                check(lib.mhx_bloom_query_dev(ctx.handle, _p(d_sig), code, n, num_perm, b, r, k, nb, _p(d_filter), _p(d_hit), 0))
                _expect(d_hit.download((n,), np.uint8), B.query_host(want, sig, r, k).view(np.uint8), what + " query")
                _expect(d_filter.download((b, nb, 16), np.uint32), want, what + " query leaves the filter alone")
                d_hit2 = _alloc(ctx, n)
                check(lib.mhx_bloom_query_dev(ctx.handle, _p(d_sig), code, n, num_perm, b, r, k, nb, _p(d_filter), _p(d_hit2), 1))
                _expect(d_hit2.download((n,), np.uint8), B.query_host(want, sig, r, k).view(np.uint8), what + " query then insert")
                B.insert_host(want, sig, r, k)
                _expect(d_filter.download((b, nb, 16), np.uint32), want, what + " the insert after the query")
                d_other = _dev(ctx, old)
                check(lib.mhx_bloom_union_dev(ctx.handle, _p(d_other), _p(d_filter), b, nb))
                _expect(d_other.download((b, nb, 16), np.uint32), want | old, what + " union")
                _expect(d_filter.download((b, nb, 16), np.uint32), want, what + " union: the second operand")
                _done(what)
                for buf in (d_sig, d_half, d_filter, d_hit, d_hit2, d_other):
                    if not os.environ.get("GUARD_KEEP"):
                        buf.free()


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    for lanes in (16, 1, 0):
        ctx.set_option("bloom.lanes", lanes)
        filter_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"BLOOM GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"BLOOM GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
