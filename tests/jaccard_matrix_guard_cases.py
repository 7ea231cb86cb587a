"""The all-pairs Jaccard device entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a
script in a process of its own by tests/test_gpu_jaccard_matrix_guard.py -- a kernel that over-reads kills the process).

    python tests/jaccard_matrix_guard_cases.py <align>      all cases; prints "MATRIX GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: A, B, the counts and the pair list of every call are separate
exact-size allocations from mhx_debug_guard_alloc, outputs pre-filled with a pattern, and the results are checked against numpy:
the counts against (a[:, None, :] == b[None, :, :]).sum(-1), the pair lists against np.argwhere of it.  mhx_jaccard_matrix_dev,
mhx_jaccard_threshold_pairs_dev and their b-bit twins at the smallest shapes that take every addressing decision: one row and one
word, 12-byte rows, one row past a 128-row tile on both sides and one word past a 16-word chunk, the triangle of A against itself,
ldc == n_b and ldc == n_b + 3 (the cells j >= n_b keep the pattern), a pair list of exactly the total and one below it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, b_bit_minhash  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _begin, _dev, _done, _expect  # noqa: E402
from tests.jaccard_topk_guard_cases import planted  # noqa: E402

PATTERN32 = np.uint32(0xA5A5A5A5).view(np.int32)
# (n_a, n_b, num_perm); n_b None: d_b = NULL, the triangle of A against itself
SHAPES = ((1, 1, 1), (3, 5, 3), (129, 130, 17), (5, 257, 100), (131, None, 17))


def _counts(a, b):
    return (a[:, None, :] == b[None, :, :]).sum(-1).astype(np.int32)


class Operands:
    """A and B of one shape on the device (packed for the b-bit twins), and numpy's counts of them."""

    def __init__(self, ctx, a, b, num_perm, bits=None):
        self.ctx, self.num_perm, self.bits, self.self_join = ctx, num_perm, bits, b is None
        values_a, values_b = a, a if b is None else b
        if bits is not None:
            mask = np.uint64((1 << bits) - 1)
            values_a, values_b = values_a & mask, values_b & mask
            a = b_bit_minhash.pack_matrix(a, bits, gpu_mode="disable")
            b = None if b is None else b_bit_minhash.pack_matrix(b, bits, gpu_mode="disable")
        self.code = MHX_U32 if a.dtype == np.uint32 else MHX_U64
        self.n_a, self.n_b = a.shape[0], a.shape[0] if b is None else b.shape[0]
        self.d_a, self.d_b = _dev(ctx, a), None if b is None else _dev(ctx, b)
        self.b_ptr = None if b is None else self.d_b.ptr
        self.want = _counts(values_a, values_b)

    def matrix(self, ldc, what):
        ctx, n_a, n_b = self.ctx, self.n_a, self.n_b
        _begin(what)
        d_counts = _alloc(ctx, 4 * n_a * ldc)
        if self.bits is None:
            ctx.jaccard_matrix_dev(self.d_a.ptr, n_a, self.b_ptr, n_b, self.code, self.num_perm, d_counts.ptr, ldc)
        else:
            ctx.bbit_jaccard_matrix_dev(self.d_a.ptr, n_a, self.b_ptr, n_b, self.num_perm, self.bits, d_counts.ptr, ldc)
        want = np.full((n_a, ldc), PATTERN32, dtype=np.int32)  # the cells j >= n_b of every row are not written
        want[:, :n_b] = self.want
        _expect(d_counts.download((n_a, ldc), np.int32), want, what)
        _done(what)

    def threshold(self, what):
        """A min_count that some but not all pairs reach (where the shape has two different counts); the list with room for
        exactly the total, then with room for half of it: the total comes back and nothing is written past the room."""
        ctx = self.ctx
        keep_from = np.triu(np.ones_like(self.want, dtype=bool), k=1) if self.self_join else np.ones_like(self.want, dtype=bool)
        levels = np.unique(self.want[keep_from])
        min_count = int(levels[len(levels) // 2])
        ij = np.argwhere((self.want >= min_count) & keep_from)
        total = len(ij)
        assert total > 0 and (len(levels) == 1 or total < int(keep_from.sum())), (what, total)
        for capacity in (total, total // 2):
            name = f"{what} min_count={min_count} capacity {capacity} of {total}"
            _begin(name)
            d_pairs, d_counts = _alloc(ctx, 16 * capacity), _alloc(ctx, 4 * capacity)
            if self.bits is None:
                found = ctx.jaccard_threshold_pairs_dev(self.d_a.ptr, self.n_a, self.b_ptr, 0 if self.self_join else self.n_b, self.code,
                                                        self.num_perm, min_count, d_pairs.ptr, d_counts.ptr, capacity)
            else:
                found = ctx.bbit_jaccard_threshold_pairs_dev(self.d_a.ptr, self.n_a, self.b_ptr, 0 if self.self_join else self.n_b, self.num_perm,
                                                             self.bits, min_count, d_pairs.ptr, d_counts.ptr, capacity)
            assert found == total, (name, found)
            if capacity == total:
                _expect(d_pairs.download((total, 2), np.int64), ij, name + " pairs")
                _expect(d_counts.download((total,), np.int32), self.want[ij[:, 0], ij[:, 1]], name + " counts")
            _done(name)


def _rows(rng, n_a, n_b, num_perm, dtype):
    a, b = planted(rng, n_a, 7 if n_b is None else n_b, num_perm, dtype)
    if n_b is None:  # the triangle: rows that agree with earlier rows of the same matrix
        a[n_a // 2:] = np.where(rng.random_sample((n_a - n_a // 2, num_perm)) < 0.5, a[: n_a - n_a // 2], a[n_a // 2:])
    return a, None if n_b is None else b


def dense_cases(ctx):
    rng = np.random.RandomState(41)
    for dtype in (np.uint32, np.uint64):
        for n_a, n_b, num_perm in SHAPES:
            a, b = _rows(rng, n_a, n_b, num_perm, dtype)
            one = Operands(ctx, a, b, num_perm)
            name = f"matrix {np.dtype(dtype).name} {n_a}x{n_b}x{num_perm}"
            for extra in (0, 3):
                one.matrix(one.n_b + extra, f"{name} ldc=n_b+{extra}")
            one.threshold(f"threshold {np.dtype(dtype).name} {n_a}x{n_b}x{num_perm}")
    # uint64 values that differ only in bits 32..63: the wide compare
    a, b = planted(rng, 129, 130, 17, np.uint64)
    a |= rng.randint(0, 2, size=a.shape).astype(np.uint64) << np.uint64(40)
    b |= rng.randint(0, 2, size=b.shape).astype(np.uint64) << np.uint64(40)
    assert not np.array_equal(_counts(a, b), _counts(a & np.uint64(0xFFFFFFFF), b & np.uint64(0xFFFFFFFF)))
    one = Operands(ctx, a, b, 17)
    one.matrix(133, "matrix uint64 high words 129x130x17 ldc=n_b+3")
    one.threshold("threshold uint64 high words 129x130x17")


def bbit_cases(ctx):
    rng = np.random.RandomState(42)
    at = 0
    for bits in (1, 3, 32):
        for num_perm in (1, 100, 128):
            n_a, n_b, _ = SHAPES[at % len(SHAPES)]  # every shape's rows and tiles, the words per row being those of (bits, num_perm)
            at += 1
            a, b = _rows(rng, n_a, n_b, num_perm, np.uint64)
            one = Operands(ctx, a, b, num_perm, bits=bits)
            name = f"bbit b={bits} {n_a}x{n_b}x{num_perm}"
            for extra in (0, 3):
                one.matrix(one.n_b + extra, f"matrix {name} ldc=n_b+{extra}")
            one.threshold(f"threshold {name}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    dense_cases(ctx)
    bbit_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"MATRIX GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"MATRIX GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
