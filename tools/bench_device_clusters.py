#!/usr/bin/env python3
"""tools/bench_device_clusters.py -- near-duplicate clustering on the device (cc_kernels.hip), each figure next to what a user
has today.  After tools/_warm.py's clock warm-up; device work timed with HIP events, medians of five; host steps with a host
clock.  On a resident clustered matrix (num_perm = 128, uint32, 32 bands of 4) and its resident sorted bands:

  link_bands  (a) mhx_cc_init_dev + mhx_cc_link_bands_dev + mhx_cc_finish_dev: the clusters with no pair formed
  link_pairs  (b) mhx_lsh_candidate_pairs_dev (blocking; pairs stay on the device) + init + mhx_cc_link_pairs_dev + finish
  host        (c) the same pair list downloaded and given to scipy.sparse.csgraph.connected_components: today's baseline

The corpus is tools/bench_device_forest.py's (copies of n / cluster bases, 3 % of the positions redrawn) at two cluster sizes:
500 rows, where every cluster is one bucket in most bands and the pair list is 250 times the rows (the pair form may not fit:
MHX_ERR_OOM is recorded, not hidden; it is run at 1M rows only, and (c) only up to 10^8 pairs), and 8 rows, where the pair list is a few times the rows and all three forms run.
Labels of the three forms are compared.  Algorithmic bytes (what a pass must read and write once) over time against 8 TB/s.

`python tools/bench_device_clusters.py [1m] [10m] [--out file]` (default: 1m 10m, profiles/device_clusters_bench.json).  SCALE
(env, float, default 1) scales every row count for a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
K, B, R = 128, 32, 4
HBM = 8e12
RECORDS = []


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def corpus(rng, n, cluster):
    """Clustered uint32 rows: copies of n / cluster bases; four fifths of the rows (with repeats) get five positions redrawn."""
    bases = rng.randint(0, 2**32, (max(2, n // cluster), K), dtype=np.uint32)
    sig = bases[rng.randint(len(bases), size=n)]
    flat = sig.reshape(-1)
    touched = rng.randint(0, n, n * 4 // 5).astype(np.int64)
    at = np.repeat(touched, 5) * K + rng.randint(0, K, touched.size * 5)
    flat[at] = rng.randint(0, 2**32, at.size, dtype=np.uint32)
    return sig


def timed(ctx, call, reps=5):
    out = []
    for _ in range(reps):
        e0 = ctx.event().record()
        call()
        e1 = ctx.event().record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1))
    return out


def med(ms):
    return float(np.median(ms))


HOST_PAIRS_MAX = 100_000_000  # (c) is skipped beyond this many pairs: 1.6 GB to download and several times that in scipy


def bench(n, cluster, pair_form=True):
    from datasketch_amd import _native, lsh_bulk

    ctx = _native.context()
    rng = np.random.RandomState(n % 1000 + cluster)
    index = lsh_bulk.SortedBandsIndex(corpus(rng, n, cluster), B, R)
    d_dig, d_rows, d_sig = index._d_dig.ptr, index._d_rows.ptr, index._rows.d_sig.ptr
    d_labels = ctx.alloc(4 * n)
    d_bad = ctx.to_device(np.zeros(1, dtype=np.int64))
    shape = dict(n=n, cluster=cluster, num_perm=K, bands=B, r=R)

    # (a) the run form
    init = lambda: ctx.cc_init_dev(d_labels.ptr, n)
    finish = lambda: ctx.cc_finish_dev(d_labels.ptr, n)
    link_bands = lambda: ctx.cc_link_bands_dev(d_labels.ptr, n, d_dig, d_rows, n, B, d_bad.ptr)

    def run_form():
        init()
        link_bands()
        finish()

    def fresh(link):  # a link launch timed on labels just initialised, five times: every union is still to be made
        out = []
        for _ in range(5):
            init()
            out += timed(ctx, link, 1)
        return out

    warm(run_form, ctx.synchronize)
    t_init = timed(ctx, init)
    t_link = fresh(link_bands)
    t_fin = timed(ctx, finish)
    t_all = timed(ctx, run_form)
    by_bands = d_labels.download((n,), np.uint32)
    band_bytes = B * n * 12 + 4 * n  # digests and rows read once, a label per row touched at least once
    emit(what="link_bands", **shape, init_ms=t_init, link_ms=t_link, finish_ms=t_fin, ms=t_all, ms_median=med(t_all),
         link_ms_median=med(t_link), clusters=int(np.count_nonzero(by_bands == np.arange(n, dtype=np.uint32))),
         largest=int(np.bincount(by_bands).max()), link_bytes=band_bytes, link_fraction_of_8TBps=band_bytes / (med(t_link) * 1e-3) / HBM,
         init_fraction_of_8TBps=4 * n / (med(t_init) * 1e-3) / HBM, finish_fraction_of_8TBps=8 * n / (med(t_fin) * 1e-3) / HBM)

    # (b) the pair form
    if not pair_form:
        emit(what="link_pairs", **shape, skipped="about %d pairs expected" % (n * cluster // 2))
        return
    try:
        t0 = time.perf_counter()
        d_pairs, found = ctx.lsh_candidate_pairs_dev(d_dig, d_rows, n, B)
        first_s = time.perf_counter() - t0  # (with the capacity retry)
        t_pairs = timed(ctx, lambda: ctx.lsh_candidate_pairs_dev(d_dig, d_rows, n, B, capacity=found), 3)
    except (MemoryError, _native.MhxError) as e:
        emit(what="link_pairs", **shape, failed=type(e).__name__, message=str(e)[:200])
        return
    link_pairs = lambda: ctx.cc_link_pairs_dev(d_labels.ptr, n, d_pairs.ptr, found, None, 0, d_bad.ptr)

    def pair_form():
        init()
        link_pairs()
        finish()

    warm(pair_form, ctx.synchronize)
    t_link = fresh(link_pairs)
    t_all = timed(ctx, pair_form)
    by_pairs = d_labels.download((n,), np.uint32)
    pair_bytes = 16 * found + 4 * n
    emit(what="link_pairs", **shape, pairs=found, candidate_pairs_ms=t_pairs, candidate_pairs_first_call_s=first_s, link_ms=t_link,
         ms=t_all, ms_median=med(t_pairs) + med(t_all), link_ms_median=med(t_link), link_bytes=pair_bytes,
         link_fraction_of_8TBps=pair_bytes / (med(t_link) * 1e-3) / HBM, same_labels_as_link_bands=bool(np.array_equal(by_pairs, by_bands)))

    # (c) today's baseline: the pairs come down, scipy labels them
    if found > HOST_PAIRS_MAX:
        emit(what="host", **shape, pairs=found, skipped="more than %d pairs" % HOST_PAIRS_MAX)
        return
    t0 = time.perf_counter()
    pairs = d_pairs.download((found, 2), np.int64)
    t1 = time.perf_counter()
    host = lsh_bulk.connected_components(pairs, n, gpu_mode="disable")
    t2 = time.perf_counter()
    emit(what="host", **shape, pairs=found, download_s=t1 - t0, scipy_s=t2 - t1, s=t2 - t0,
         same_labels_as_link_bands=bool(np.array_equal(host, by_bands.astype(np.int64))))
    assert int(d_bad.download((1,), np.int64)[0]) == 0


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_clusters.py needs an MI355X")
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "device_clusters_bench.json")
    if "--out" in args:
        at = args.index("--out")
        out = args[at + 1]
        del args[at : at + 2]
    which = args or ["1m", "10m"]
    for name, rows in (("1m", 1_000_000), ("10m", 10_000_000)):
        if name in which:
            bench(n_of(rows), 8)
            bench(n_of(rows), 500, pair_form=name == "1m")  # (at 10M rows the 500-row clusters hold 2.5 * 10^9 pairs)
    with open(out, "w") as f:
        json.dump({"device": _native.context().info(), "scale": SCALE, "records": RECORDS}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
