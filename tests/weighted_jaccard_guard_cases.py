"""The weighted Jaccard device entry points of include/mhx_weighted_jaccard.h on buffers that abut an unmapped page (test
infrastructure, run as a script in a process of its own by tests/test_gpu_weighted_jaccard_guard.py -- a kernel that over-reads
kills the process).

    python tests/weighted_jaccard_guard_cases.py <align>      all cases; prints "WJ GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: A, B, the pairs, the live-bit map and every output of a call are
separate exact-size allocations from mhx_debug_guard_alloc (the library's scratch is one too), outputs pre-filled with a pattern,
and the results are checked against the numpy definition in datasketch_amd/lsh_bulk.py.  The four entries: listed pairs (fewer
than, exactly and more than 64 samples), the matrix (ldc > n_b, A with itself), the thresholded pairs and the top-k lists (strip
and stream kernel, B in one and in several segments, with the live-bit map, A among itself).

The corpora of the other weighted Jaccard tests come from here too: planted_weighted() and near_miss_matrix().
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, lsh_bulk  # noqa: E402
from datasketch_amd._native import check  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect, _p  # noqa: E402

_i64 = ctypes.c_int64


def random_samples(rng, shape):
    """int64 (k, t) pairs as the generator writes them: k a small index, t of either sign and well past 32 bits."""
    out = np.empty(tuple(shape) + (2,), dtype=np.int64)
    out[..., 0] = rng.randint(0, 4096, size=shape)
    out[..., 1] = rng.randint(-(1 << 62), 1 << 62, size=shape, dtype=np.int64)
    return out


def planted_weighted(rng, m, n, s):
    """A [m, s, 2], B [n, s, 2]: every row of B shares a random fraction of its samples with a row of A -- and of the rest half
    keep that row's k with another t, a quarter its t with another k: the near misses a [n, 2 s] word compare would count."""
    a, b = random_samples(rng, (m, s)), random_samples(rng, (n, s))
    src = rng.randint(0, m, size=n)
    u = rng.random_sample((n, s))
    share = rng.random_sample((n, 1))
    from_a = a[src]
    keep = u < share
    b[keep] = from_a[keep]
    k_only = ~keep & (u < share + (1 - share) / 2)
    b[..., 0][k_only] = from_a[..., 0][k_only]
    t_only = ~keep & ~k_only & (u < share + 3 * (1 - share) / 4)
    b[..., 1][t_only] = from_a[..., 1][t_only]
    return a, b


NEAR_MISS_ROWS = ("base", "k only", "t only", "bit 40 of k", "sign of t", "k and t swapped", "shifted by one word")
NEAR_MISS_EQUAL = 2  # samples 0 and 1 of every row are the base row's


def near_miss_matrix(s=8, seed=77):
    """[7, s, 2]: row 0 is the base; every other row agrees with it in samples 0 and 1 and in the rest misses it in the way
    NEAR_MISS_ROWS names, so count(base, row) is NEAR_MISS_EQUAL for each of them and no more."""
    rng = np.random.RandomState(seed)
    base = random_samples(rng, (s,))
    base[:, 0] |= 1 << 33                                  # k past 32 bits too
    base[:, 1] = -np.abs(base[:, 1]) - 1                   # t negative: its high word is no zero
    rows = np.repeat(base[None], len(NEAR_MISS_ROWS), axis=0)
    other = random_samples(rng, (s,))
    rows[1, 2:, 1] = other[2:, 1]                          # k only
    rows[2, 2:, 0] = other[2:, 0] | (1 << 34)              # t only
    rows[3, 2:, 0] ^= 1 << 40                              # everything but bit 40 of k
    rows[4, 2:, 1] = -rows[4, 2:, 1]                       # everything but the sign of t
    rows[5, 2:] = rows[5, 2:, ::-1]                        # (k, t) swapped
    words = base.reshape(-1).copy()
    words[4:-1] = base.reshape(-1)[5:]                     # from sample 2 on: k'_s = t_s, t'_s = k_{s+1}
    words[-1] = 12345
    rows[6] = words.reshape(s, 2)
    return rows


def want_pairs(a, b, pairs):
    return lsh_bulk._equal_samples(a[pairs[:, 0]], b[pairs[:, 1]]).astype(np.int32)


def want_matrix(a, b):
    other = a if b is None else b
    return lsh_bulk._matrix_from_blocks(lsh_bulk._equal_samples_blocks(a, b), a.shape[0], other.shape[0]).astype(np.int32)


def want_threshold(a, b, min_count):
    pairs, counts = lsh_bulk._pairs_from_blocks(lsh_bulk._equal_samples_blocks(a, b), min_count, b is None)
    return pairs, counts.astype(np.int32)


def want_topk(a, b, k, min_count, live=None):
    rows, counts = lsh_bulk._topk_from_blocks(lsh_bulk._equal_samples_blocks(a, b), a.shape[0], k, min_count, b is None, live)
    return rows, counts.astype(np.int32)


def pairs_call(ctx, a, b, pairs, what):
    d_a, d_b, d_pairs = _dev(ctx, a), _dev(ctx, b), _dev(ctx, pairs)
    d_counts = _alloc(ctx, 4 * len(pairs))
    check(ctx.lib.mhx_weighted_jaccard_pairs_dev(ctx.handle, _p(d_a), _p(d_b), a.shape[1], _p(d_pairs), len(pairs), _p(d_counts)))
    _expect(d_counts.download((len(pairs),), np.int32), want_pairs(a, b, pairs), what)
    _done(what)


def matrix_call(ctx, a, b, ldc, what):
    n_b = a.shape[0] if b is None else b.shape[0]
    d_a, d_b = _dev(ctx, a), None if b is None else _dev(ctx, b)
    d_counts = _alloc(ctx, 4 * ((a.shape[0] - 1) * ldc + n_b))  # exactly up to the last element of the last row
    check(ctx.lib.mhx_weighted_jaccard_matrix_dev(ctx.handle, _p(d_a), a.shape[0], _p(d_b), 0 if b is None else n_b, a.shape[1], _p(d_counts), ldc))
    flat = d_counts.download(((a.shape[0] - 1) * ldc + n_b,), np.int32)
    padded = np.full(a.shape[0] * ldc, np.int32(-1515870811))  # 0xA5A5A5A5: what the entry leaves between the rows
    padded[: flat.size] = flat
    got = padded.reshape(a.shape[0], ldc)
    _expect(got[:, :n_b], want_matrix(a, b), what)
    _expect(got[:-1, n_b:], np.full((a.shape[0] - 1, ldc - n_b), np.int32(-1515870811)), what + " (the columns past n_b)")
    _done(what)


def threshold_call(ctx, a, b, min_count, what):
    pairs, counts = want_threshold(a, b, min_count)
    cap = max(1, len(pairs))
    d_a, d_b = _dev(ctx, a), None if b is None else _dev(ctx, b)
    d_pairs, d_counts = _alloc(ctx, 16 * cap), _alloc(ctx, 4 * cap)
    found = _i64(-1)
    check(ctx.lib.mhx_weighted_jaccard_threshold_pairs_dev(ctx.handle, _p(d_a), a.shape[0], _p(d_b), 0 if b is None else b.shape[0], a.shape[1],
                                                           min_count, _p(d_pairs), _p(d_counts), cap, ctypes.byref(found)))
    assert found.value == len(pairs), (what, found.value, len(pairs))
    _expect(d_pairs.download((cap, 2), np.int64)[: len(pairs)], pairs, what + " pairs")
    _expect(d_counts.download((cap,), np.int32)[: len(pairs)], counts, what + " counts")
    _done(what)


def topk_call(ctx, a, b, k, what, live=None, min_count=0):
    m, n_b = a.shape[0], 0 if b is None else b.shape[0]
    d_a, d_b = _dev(ctx, a), None if b is None else _dev(ctx, b)
    d_live = None if live is None else _dev(ctx, lsh_bulk.live_bits(live))
    d_rows, d_counts = _alloc(ctx, 8 * m * k), _alloc(ctx, 4 * m * k)
    check(ctx.lib.mhx_weighted_jaccard_topk_dev(ctx.handle, _p(d_a), m, _p(d_b), n_b, a.shape[1], _p(d_live), min_count, k, _p(d_rows),
                                                _p(d_counts)))
    rows, counts = want_topk(a, b, k, min_count, live)
    _expect(d_rows.download((m, k), np.int64), rows, what + " rows")
    _expect(d_counts.download((m, k), np.int32), counts, what + " counts")
    _done(what)


def listed_cases(ctx):
    rng = np.random.RandomState(41)
    for m, n, s in ((1, 1, 1), (5, 9, 3), (40, 33, 63), (40, 33, 64), (17, 50, 65), (9, 12, 200)):
        a, b = planted_weighted(rng, m, n, s)
        pairs = np.stack([rng.randint(0, m, size=301), rng.randint(0, n, size=301)], axis=1).astype(np.int64)
        pairs[-1] = (m - 1, n - 1)  # the last rows: their last sample ends the mapping
        pairs_call(ctx, a, b, pairs, f"weighted pairs {m}x{n} S={s}")
    rows = near_miss_matrix()
    pairs_call(ctx, rows, rows, np.stack([np.zeros(7, np.int64), np.arange(7)], axis=1), "weighted pairs near misses")


def tile_cases(ctx):
    rng = np.random.RandomState(42)
    for m, n, s in ((1, 1, 1), (3, 129, 5), (129, 257, 33), (130, 127, 128)):
        a, b = planted_weighted(rng, m, n, s)
        matrix_call(ctx, a, b, n, f"weighted matrix {m}x{n} S={s}")
        matrix_call(ctx, a, b, n + 3, f"weighted matrix {m}x{n} S={s} ldc=n_b+3")
        matrix_call(ctx, b, None, n, f"weighted matrix {n} with itself S={s}")
        threshold_call(ctx, a, b, max(1, s // 3), f"weighted threshold {m}x{n} S={s}")
        threshold_call(ctx, b, None, max(1, s // 4), f"weighted threshold {n} with itself S={s}")


def topk_cases(ctx):
    rng = np.random.RandomState(43)
    for path in (1, 2):  # strip, stream
        ctx.set_option("jaccard.topk_path", path)
        for segments in (0, 3):
            ctx.set_option("jaccard.topk_segments", segments)
            for m, n, s in ((1, 1, 1), (2, 63, 3), (3, 385, 33), (129, 257, 128)):
                a, b = planted_weighted(rng, m, n, s)
                name = f"weighted topk path={path} segments={segments} {m}x{n} S={s}"
                live = rng.random_sample(n) < 0.8
                topk_call(ctx, a, b, 10, name)
                topk_call(ctx, a, b, 64, name + " k=64 live floor", live=live, min_count=s // 3)
                topk_call(ctx, b, None, 7, name + " self", live=live)
    ctx.set_option("jaccard.topk_path", 0)
    ctx.set_option("jaccard.topk_segments", 0)


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    listed_cases(ctx)
    tile_cases(ctx)
    topk_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"WJ GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"WJ GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
