#!/usr/bin/env python3
"""tools/bench_device_weighted_jaccard.py -- WeightedMinHash.jaccard on the device (mhx_weighted_jaccard_*), each figure next to
two yardsticks taken in the same run.  After tools/_warm.py's clock warm-up; device work timed with HIP events, five launches
each; the numpy path with a host clock.  S = 128 samples per row (2 KiB) throughout:

  pairs    10^6 listed pairs of a resident matrix of 10^5 rows          mhx_weighted_jaccard_pairs_dev
  matrix   10^4 x 10^4 counts                                           mhx_weighted_jaccard_matrix_dev
  topk     the 10 best of 10^6 rows for each of 10^3 probes             mhx_weighted_jaccard_topk_dev

  twin     the MinHash entry of the same step (mhx_jaccard_pairs_dev_typed, mhx_jaccard_matrix_dev, mhx_jaccard_topk_dev) on the
           same bytes read as MHX_U64 rows of num_perm = 2 S: the same traffic and tile, only the compare differs (it counts
           words, not samples, so its answers are other numbers)
  numpy    the gpu_mode="disable" path of the same lsh_bulk call; where that would take minutes it runs on a subsample and is
           scaled by the number of compared samples -- the record says which ("numpy_scaled_from")

Results of the device entries are compared with the numpy definition on a slice.  `python tools/bench_device_weighted_jaccard.py
[pairs] [matrix] [topk] [--out file]` (default: all three, profiles/weighted_jaccard_bench.txt).  SCALE (env, float, default 1)
scales every row count for a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
S = 128
RECORDS = []


def n_of(x):
    return max(256, int(x * SCALE))


def emit(**rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def corpus(rng, n, bases):
    """[n, S, 2] int64: copies of `bases` base rows with a row's own share of the samples redrawn, a third of those keeping k."""
    base = np.stack([rng.integers(0, 4096, size=(bases, S)), rng.integers(-(1 << 62), 1 << 62, size=(bases, S))], axis=2)
    sig = base[rng.integers(0, bases, size=n)]
    redraw = rng.random((n, S)) < rng.random((n, 1))
    sig[..., 1][redraw] = rng.integers(-(1 << 62), 1 << 62, size=int(redraw.sum()))
    other_k = redraw & (rng.random((n, S)) < 2 / 3)
    sig[..., 0][other_k] = rng.integers(0, 4096, size=int(other_k.sum()))
    return np.ascontiguousarray(sig, dtype=np.int64)


def timed(ctx, call, reps=5):
    out = []
    for _ in range(reps):
        e0 = ctx.event().record()
        call()
        e1 = ctx.event().record()
        e1.synchronize()
        out.append(round(e0.elapsed_ms(e1), 4))
    return out


def med(ms):
    return float(np.median(ms))


def host_seconds(call):
    t0 = time.perf_counter()
    out = call()
    return time.perf_counter() - t0, out


def bench_pairs(ctx, rng):
    from datasketch_amd import _native, lsh_bulk

    n, m = n_of(100_000), n_of(1_000_000)
    sig = corpus(rng, n, max(2, n // 50))
    pairs = rng.integers(0, n, size=(m, 2)).astype(np.int64)
    d_sig, d_pairs, d_counts = ctx.to_device(sig), ctx.to_device(pairs), ctx.alloc(4 * m)
    weighted = lambda: ctx.weighted_jaccard_pairs_dev(d_sig.ptr, d_sig.ptr, S, d_pairs.ptr, m, d_counts.ptr)  # noqa: E731
    twin = lambda: ctx.jaccard_pairs_dev(d_sig.ptr, d_sig.ptr, _native.MHX_U64, 2 * S, d_pairs.ptr, m, d_counts.ptr)  # noqa: E731
    warm(weighted, ctx.synchronize)
    t_w = timed(ctx, weighted)
    got = d_counts.download((m,), np.int32)
    warm(twin, ctx.synchronize)
    t_t = timed(ctx, twin)
    sub = max(1, m // 20)
    t_np, want = host_seconds(lambda: lsh_bulk.weighted_jaccard_pairs(sig, pairs[:sub], gpu_mode="disable"))
    assert np.array_equal(got[:sub] / float(S), want)
    read = 2 * m * S * 16
    emit(what="pairs", rows=n, pairs=m, samples=S, weighted_ms=t_w, weighted_ms_median=med(t_w), twin_u64_ms=t_t, twin_u64_ms_median=med(t_t),
         weighted_over_twin=med(t_w) / med(t_t), row_bytes_read=read, weighted_TBps=read / (med(t_w) * 1e-3) / 1e12,
         numpy_s=t_np * m / sub, numpy_scaled_from=f"{sub} pairs in {t_np:.3f} s", mean_count=float(got.mean()))


def bench_matrix(ctx, rng):
    from datasketch_amd import _native, lsh_bulk

    n = n_of(10_000)
    a, b = corpus(rng, n, max(2, n // 50)), corpus(rng, n, max(2, n // 50))
    d_a, d_b, d_c = ctx.to_device(a), ctx.to_device(b), ctx.alloc(4 * n * n)
    weighted = lambda: ctx.weighted_jaccard_matrix_dev(d_a.ptr, n, d_b.ptr, n, S, d_c.ptr, n)  # noqa: E731
    twin = lambda: ctx.jaccard_matrix_dev(d_a.ptr, n, d_b.ptr, n, _native.MHX_U64, 2 * S, d_c.ptr, n)  # noqa: E731
    warm(weighted, ctx.synchronize)
    t_w = timed(ctx, weighted)
    sub = max(1, n // 50)
    got = d_c.download((sub, n), np.int32)
    warm(twin, ctx.synchronize)
    t_t = timed(ctx, twin)
    t_np, want = host_seconds(lambda: lsh_bulk.weighted_jaccard_matrix(a[:sub], b, gpu_mode="disable"))
    assert np.array_equal(got / float(S), want)
    cells = n * n * S
    emit(what="matrix", n_a=n, n_b=n, samples=S, weighted_ms=t_w, weighted_ms_median=med(t_w), twin_u64_ms=t_t, twin_u64_ms_median=med(t_t),
         weighted_over_twin=med(t_w) / med(t_t), cell_samples=cells, weighted_cell_samples_per_ns=cells / (med(t_w) * 1e6),
         twin_cell_words_per_ns=2 * cells / (med(t_t) * 1e6), numpy_s=t_np * n / sub, numpy_scaled_from=f"{sub} rows of A in {t_np:.3f} s")


def bench_topk(ctx, rng):
    from datasketch_amd import _native, lsh_bulk

    m, n, k = n_of(1_000), n_of(1_000_000), 10
    block = corpus(rng, max(256, n // 10), max(2, n // 500))
    b = np.concatenate([block] * (n // block.shape[0] + 1))[:n]
    b[:, 0, 1] += np.arange(n)  # (the copies of the block differ from one another in one sample)
    a = b[rng.integers(0, n, size=m)].copy()
    redraw = rng.random((m, S)) < 0.3
    a[..., 1][redraw] = rng.integers(-(1 << 62), 1 << 62, size=int(redraw.sum()))
    d_a, d_b = ctx.to_device(a), ctx.to_device(b)
    d_rows, d_counts = ctx.alloc(8 * m * k), ctx.alloc(4 * m * k)
    weighted = lambda: ctx.weighted_jaccard_topk_dev(d_a.ptr, m, d_b.ptr, n, S, None, 0, k, d_rows.ptr, d_counts.ptr)  # noqa: E731
    twin = lambda: ctx.jaccard_topk_dev(d_a.ptr, m, d_b.ptr, n, _native.MHX_U64, 2 * S, None, 0, k, d_rows.ptr, d_counts.ptr)  # noqa: E731
    warm(weighted, ctx.synchronize, seconds=0.1)
    t_w = timed(ctx, weighted)
    got_rows, got_counts = d_rows.download((m, k), np.int64), d_counts.download((m, k), np.int32)
    warm(twin, ctx.synchronize, seconds=0.1)
    t_t = timed(ctx, twin)
    probes, rows = min(m, 4), max(256, n // 10)
    t_np, _ = host_seconds(lambda: lsh_bulk.weighted_nearest_neighbors(a[:probes], b[:rows], k=k, gpu_mode="disable"))
    counts = lsh_bulk._equal_samples(a[:probes, None], b[got_rows[:probes]])  # the reported rows hold the reported counts
    assert np.array_equal(counts, got_counts[:probes]) and np.all(np.diff(got_counts, axis=1) <= 0)
    cells = m * n * S
    emit(what="topk", probes=m, rows=n, k=k, samples=S, weighted_ms=t_w, weighted_ms_median=med(t_w), twin_u64_ms=t_t, twin_u64_ms_median=med(t_t),
         weighted_over_twin=med(t_w) / med(t_t), cell_samples=cells, weighted_cell_samples_per_ns=cells / (med(t_w) * 1e6),
         numpy_s=t_np * (m / probes) * (n / rows), numpy_scaled_from=f"{probes} probes against {rows} rows in {t_np:.3f} s")


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_weighted_jaccard.py needs an MI355X")
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "weighted_jaccard_bench.txt")
    if "--out" in args:
        at = args.index("--out")
        out = args[at + 1]
        del args[at: at + 2]
    which = args or ["pairs", "matrix", "topk"]
    ctx = _native.context()
    emit(what="device", library="libmhx.so", scale=SCALE, note="one run on one box: medians of five launches after a clock warm-up", **ctx.info())
    rng = np.random.default_rng(7)
    for name, bench in (("pairs", bench_pairs), ("matrix", bench_matrix), ("topk", bench_topk)):
        if name in which:
            bench(ctx, rng)
            ctx.release_scratch()
    with open(out, "w") as f:
        for rec in RECORDS:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
