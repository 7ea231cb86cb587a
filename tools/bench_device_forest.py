#!/usr/bin/env python3
"""tools/bench_device_forest.py -- datasketch_amd.MinHashLSHForest on the device, each figure next to what it is measured against.
One JSON line per measurement, every one repeated so that the spread shows; after tools/_warm.py's clock warm-up; device work
timed with HIP events, host-visible steps with a host clock around work that ends in a synchronise.

  build       mhx_lsh_forest_build_dev_typed on a resident clustered matrix (num_perm = 128, l = 8, uint32) of 1M and 10M rows,
              and in the same run the floor no build can beat: rocPRIM radix_sort_pairs of ONE 64-bit key per (tree, row) of the
              same n (mhx_lsh_sort_digests_dev with lsh.sort = 1, all 64 bits)
  index       add_bulk + index() end to end (host matrix in, index ready), device and -- at 1M rows -- the numpy back end
  query       mhx_lsh_forest_query_dev_typed of 100k probes (half rows of the index, half perturbed) at k = 10 and 100
  query_bulk  query_bulk end to end (host matrix in, lists of keys out), device and -- at 1M rows, 10k probes -- the numpy back end

`python tools/bench_device_forest.py [1m] [10m] [trace]` (default: 1m 10m; trace = the 1M shape without the numpy back end, for a
kernel trace).  SCALE (env, float, default 1) scales every row count for a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
K, L = 128, 8


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    print(json.dumps(rec), flush=True)


def corpus(rng, n):
    """Clustered uint32 rows: copies of n / 500 bases, 3 % of all positions redrawn, so most rows tie with their cluster on the
    leading words of every tree and nearly half of them (the untouched ones) are exact duplicates of their base."""
    bases = rng.randint(0, 2**32, (max(2, n // 500), K), dtype=np.uint32)
    sig = bases[rng.randint(len(bases), size=n)]
    flat = sig.reshape(-1)
    touched = rng.randint(0, n, n * 4 // 5).astype(np.int64)  # four fifths of the rows (with repeats) get redrawn positions
    at = np.repeat(touched, 5) * K + rng.randint(0, K, touched.size * 5)
    flat[at] = rng.randint(0, 2**32, at.size, dtype=np.uint32)
    return sig


def timed(ctx, call, reps):
    out = []
    for _ in range(reps):
        e0 = ctx.event().record()
        call()
        e1 = ctx.event().record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1))
    return out


def bench(n, with_numpy):
    from datasketch_amd import MinHashLSHForest, _native

    ctx = _native.context()
    rng = np.random.RandomState(n % 1000 + 1)
    sig = corpus(rng, n)
    m = n_of(100_000)
    probes = sig[rng.randint(n, size=m)].copy()
    half = probes[m // 2 :]
    redraw = rng.rand(*half.shape) < 0.1
    half[redraw] = rng.randint(0, 2**32, int(redraw.sum()), dtype=np.uint32)
    keys = range(n)
    # index(): end to end
    ends = []
    for _ in range(3):
        index = MinHashLSHForest(num_perm=K, l=L, gpu_mode="always")
        t0 = time.perf_counter()
        index.add_bulk(keys, sig)
        index.index()
        ends.append(time.perf_counter() - t0)
    emit(what="index", backend="device", n=n, num_perm=K, l=L, s=ends, rows_per_s_median=n / float(np.median(ends)))
    be = index._backend
    # the build alone, on the resident matrix
    d_order = ctx.alloc(4 * L * n)
    build = lambda: ctx.lsh_forest_build_dev(be.d_sig.ptr, be.code, n, K, L, K // L, d_order.ptr)
    warm(build, ctx.synchronize)
    t = timed(ctx, build, 5)
    emit(what="build", n=n, num_perm=K, l=L, passes=K // L, ms=t, ms_median=float(np.median(t)), order_bytes=4 * L * n)
    # the floor: one 64-bit key per (tree, row) through rocPRIM's radix sort
    d_dig = ctx.to_device(rng.randint(0, 2**63, (n, L), dtype=np.int64).astype(np.uint64))
    d_sd, d_sr = ctx.alloc(8 * L * n), ctx.alloc(4 * L * n)
    ctx.set_option("lsh.sort", 1)
    ctx.set_option("lsh.sort_bits", 64)
    floor = lambda: _native.check(ctx.lib.mhx_lsh_sort_digests_dev(ctx.handle, d_dig.ptr, n, L, d_sd.ptr, d_sr.ptr))
    warm(floor, ctx.synchronize)
    f = timed(ctx, floor, 5)
    ctx.set_option("lsh.sort", 0)
    ctx.set_option("lsh.sort_bits", 0)
    emit(what="single_key_sort", n=n, keys_per_row=L, ms=f, ms_median=float(np.median(f)),
         build_over_floor=float(np.median(t)) / float(np.median(f)))
    del d_dig, d_sd, d_sr
    # queries: the entry point alone, then query_bulk end to end
    d_q = ctx.to_device(probes)
    for k in (10, 100):
        d_slots, d_counts = ctx.alloc(4 * m * k), ctx.alloc(4 * m)
        query = lambda: ctx.lsh_forest_query_dev(be.d_sig.ptr, be.code, n, K, L, K // L, 1, be.d_order.ptr, d_q.ptr, m, k, d_slots.ptr,
                                                 d_counts.ptr)
        warm(query, ctx.synchronize)
        q = timed(ctx, query, 5)
        emit(what="query", n=n, n_probes=m, k=k, ms=q, ms_median=float(np.median(q)), probes_per_s=m / float(np.median(q)) * 1e3)
        ends = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = index.query_bulk(probes, k)
            ends.append(time.perf_counter() - t0)
        emit(what="query_bulk", backend="device", n=n, n_probes=m, k=k, keys_out=sum(map(len, got)), s=ends,
             probes_per_s_median=m / float(np.median(ends)))
    if not with_numpy:
        return
    host = MinHashLSHForest(num_perm=K, l=L, gpu_mode="disable")
    t0 = time.perf_counter()
    host.add_bulk(keys, sig)
    host.index()
    s = time.perf_counter() - t0
    emit(what="index", backend="numpy", n=n, num_perm=K, l=L, s=[s], rows_per_s_median=n / s)
    assert np.array_equal(host._backend.order(), be.order())
    mh = n_of(10_000)
    some = probes[(m - mh) // 2 : (m + mh) // 2]  # half rows of the index, half perturbed, like the whole set
    for k in (10, 100):
        t0 = time.perf_counter()
        want = host.query_bulk(some, k)
        s = time.perf_counter() - t0
        emit(what="query_bulk", backend="numpy", n=n, n_probes=mh, k=k, keys_out=sum(map(len, want)), s=[s], probes_per_s_median=mh / s)
        assert want == index.query_bulk(some, k)


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_forest.py needs an MI355X")
    which = sys.argv[1:] or ["1m", "10m"]
    if "1m" in which:
        bench(n_of(1_000_000), with_numpy=True)
    if "10m" in which:
        bench(n_of(10_000_000), with_numpy=False)
    if "trace" in which:  # the device side of the 1M shape alone: what a rocprofv3 --kernel-trace run wraps
        bench(n_of(1_000_000), with_numpy=False)


if __name__ == "__main__":
    main()
