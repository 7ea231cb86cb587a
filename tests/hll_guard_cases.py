"""The HyperLogLog device entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a
script in a process of its own by tests/test_gpu_hll_guard.py -- a kernel that over-reads kills the process).

    python tests/hll_guard_cases.py <align>        all cases; prints "HLL GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: inputs and outputs of every call are separate exact-size
allocations from mhx_debug_guard_alloc, outputs pre-filled with a pattern, and the results are checked against the numpy twin.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native  # noqa: E402
from datasketch_amd import hyperloglog as H  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64, check  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect, _p  # noqa: E402


def p_values():
    ps = {4, 8, 16}
    for p in range(4, 16):
        if _native.hll_layout(p) != _native.hll_layout(p + 1):
            ps |= {p, p + 1}
    return sorted(ps)


def bulk_dev(ctx, hv, offsets, fixed_len, n, p, bits, init, what):
    m = 1 << p
    d_hv = _dev(ctx, hv) if hv.size else ctx.alloc(8)
    d_off = _dev(ctx, offsets) if offsets is not None else None
    d_init = _dev(ctx, init) if init is not None else None
    d_out, d_ovf = _alloc(ctx, n * m), _alloc(ctx, 8)
    stride = 0 if init is None or init.ndim == 1 else m
    check(ctx.lib.mhx_hll_bulk_dev(ctx.handle, _p(d_hv), MHX_U32 if hv.dtype == np.uint32 else MHX_U64, _p(d_off), fixed_len, n, hv.size, p, bits,
                                   _p(d_init), stride, _p(d_out), _p(d_ovf)))
    _expect(d_out.download((n, m), np.uint8), H._registers_host(hv, offsets, fixed_len, n, p, bits, init), what)
    _expect(d_ovf.download((1,), np.int64), np.zeros(1, dtype=np.int64), what + " overflow count")
    _done(what)


def bulk_cases(ctx):
    rng = np.random.RandomState(21)
    lengths = [0, 1, 63, 64, 65, 257, 5000, 0, 3]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    for p in p_values():
        m = 1 << p
        for dtype, bits in ((np.uint32, 32), (np.uint64, 64)):
            hv = (rng.randint(0, 2**32, size=int(offsets[-1]), dtype=np.uint64) >> rng.randint(0, 32, size=int(offsets[-1])).astype(np.uint64)).astype(dtype)
            per_row = rng.randint(0, 9, size=(len(lengths), m)).astype(np.uint8)
            bulk_dev(ctx, hv, offsets, 0, len(lengths), p, bits, None, f"hll bulk csr p={p} {np.dtype(dtype).name}")
            bulk_dev(ctx, hv, offsets, 0, len(lengths), p, bits, per_row, f"hll bulk csr init rows p={p} {np.dtype(dtype).name}")
            bulk_dev(ctx, hv[:111], None, 37, 3, p, bits, per_row[0], f"hll bulk fixed shared init p={p} {np.dtype(dtype).name}")
            bulk_dev(ctx, hv[:1], None, 1, 1, p, bits, None, f"hll bulk one token p={p} {np.dtype(dtype).name}")
        ctx.set_option("hll.split_tokens", 1000)  # the split path: its last workgroup ends at the end of the token array
        bulk_dev(ctx, hv, offsets, 0, len(lengths), p, 64, per_row, f"hll bulk split csr p={p}")
        bulk_dev(ctx, hv[:5001], None, 5001, 1, p, 64, None, f"hll bulk split one set p={p}")
        ctx.set_option("hll.split_tokens", 0)


def matrix_cases(ctx):
    rng = np.random.RandomState(22)
    for p, n in ((4, 1), (4, 3), (8, 1001), (13, 5), (16, 2)):
        m = 1 << p
        reg = rng.randint(0, 64, size=(n, m)).astype(np.uint8)
        reg[0] = 0
        reg[-1, m - 1] = 200
        d_reg, d_hist, d_bad = _dev(ctx, reg), _alloc(ctx, n * 256), _alloc(ctx, 8)
        check(ctx.lib.mhx_hll_histogram_dev(ctx.handle, _p(d_reg), n, p, _p(d_hist), _p(d_bad)))
        _expect(d_hist.download((n, 64), np.uint32), np.stack([np.bincount(r[r < 64], minlength=64) for r in reg]), f"hll histogram p={p} n={n}")
        _expect(d_bad.download((1,), np.int64), np.ones(1, dtype=np.int64), "hll histogram invalid count")
        _done(f"hll histogram p={p} n={n}")
        groups = np.array([0, 0, 1, n, n], dtype=np.int64)
        d_groups, d_out = _dev(ctx, groups), _alloc(ctx, 4 * m)
        check(ctx.lib.mhx_hll_union_groups_dev(ctx.handle, _p(d_reg), n, p, _p(d_groups), 4, _p(d_out)))
        _expect(d_out.download((4, m), np.uint8), H.union_groups(reg, groups, gpu_mode="disable").view(np.uint8), f"hll union p={p} n={n}")
        _done(f"hll union p={p} n={n}")
    for count in (1, 3, 16, 17, 100, 4099, 16 * 1000 + 5):
        a, b = rng.randint(0, 64, size=count).astype(np.uint8), rng.randint(0, 64, size=count).astype(np.uint8)
        d_a, d_b = _dev(ctx, a), _dev(ctx, b)
        check(ctx.lib.mhx_hll_merge_dev(ctx.handle, _p(d_a), _p(d_b), count))
        _expect(d_a.download((count,), np.uint8), np.maximum(a, b), f"hll merge {count} bytes")
        _expect(d_b.download((count,), np.uint8), b, f"hll merge {count} bytes: the second operand")
        _done(f"hll merge {count}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    bulk_cases(ctx)
    matrix_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"HLL GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"HLL GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
