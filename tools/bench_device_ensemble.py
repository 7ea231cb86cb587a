#!/usr/bin/env python3
"""tools/bench_device_ensemble.py -- datasketch_amd.MinHashLSHEnsemble on the device, each figure next to what it is measured
against.  One JSON line per measurement, every one repeated 5 times so that the spread shows; after tools/_warm.py's clock warm-up;
device work timed with HIP events, host-visible steps with a host clock around work that ends in a synchronise.

1M clustered rows of num_perm = 128 (uint32), sizes from a bounded domain of at most 2 000 distinct values with a long tail; 100k
probes, half rows of the index and half perturbed, sizes spread over four decades.  Two indexes: the default constructor arguments,
and threshold = 0.5 (more levels).

  index         index_bulk end to end (host matrix in, index ready)
  query         mhx_lsh_ensemble_query_dev alone, probes and choice bytes resident
  query_looped  the same answers from the same resident buffers by a loop over mhx_lsh_query_dev, one call per (partition,
                selected parameter) pair on that pair's probes (gathered and uploaded beforehand, outside the timing; turning the
                calls' local pairs into global ones is outside it too).  The answers are asserted equal to the one call's.
  query_bulk    query_bulk end to end (host matrix in, lists of keys out), device
  numpy         the numpy back end at 10k probes (index_bulk and query_bulk), default arguments only; answers asserted equal

`python tools/bench_device_ensemble.py [default] [t05] [trace]` (default: default t05; trace = the device side of the default
shape alone, for a kernel trace).  SCALE (env, float, default 1) scales every row count for a dry run."""
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
K = 128
REPS = 5


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    print(json.dumps(rec), flush=True)


def corpus(rng, n):
    """Clustered uint32 rows: copies of n / 500 bases with a tenth of the positions of most rows redrawn."""
    bases = rng.randint(0, 2**32, (max(2, n // 500), K), dtype=np.uint32)
    sig = bases[rng.randint(len(bases), size=n)]
    flat = sig.reshape(-1)
    touched = rng.randint(0, n, n * 4 // 5).astype(np.int64)
    at = np.repeat(touched, 13) * K + rng.randint(0, K, touched.size * 13)
    flat[at] = rng.randint(0, 2**32, at.size, dtype=np.uint32)
    return sig


def set_sizes(rng, n):
    """A domain of at most 2 000 distinct sizes, geometric from 1 to 10^6, drawn with a long tail towards the large ones."""
    domain = np.unique(np.round(np.exp(np.linspace(0, np.log(1e6), 2000))).astype(np.int64))
    return domain[np.minimum((rng.pareto(1.2, n) * len(domain) / 25).astype(np.int64), len(domain) - 1)]


def timed(ctx, call, reps=REPS):
    out = []
    for _ in range(reps):
        e0 = ctx.event().record()
        call()
        e1 = ctx.event().record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1))
    return out


def median(xs):
    return float(np.median(xs))


def bench(label, n, with_numpy, **ctor):
    from datasketch_amd import MinHashLSHEnsemble, _native

    ctx = _native.context()
    lib = ctx.lib
    rng = np.random.RandomState(17)
    sig, sizes = corpus(rng, n), set_sizes(rng, n)
    m = n_of(100_000)
    probes = sig[rng.randint(n, size=m)].copy()
    half = probes[m // 2 :]
    redraw = rng.rand(*half.shape) < 0.1
    half[redraw] = rng.randint(0, 2**32, int(redraw.sum()), dtype=np.uint32)
    probe_sizes = np.exp(rng.uniform(0, np.log(1e4), m)).astype(np.int64)
    keys = range(n)
    shape = dict(config=label, n=n, num_perm=K, distinct_sizes=int(np.unique(sizes).size), **ctor)
    # index_bulk: end to end
    ends = []
    for _ in range(REPS):
        index = MinHashLSHEnsemble(num_perm=K, gpu_mode="always", **ctor)
        t0 = time.perf_counter()
        index.index_bulk(keys, sig, sizes)
        ends.append(time.perf_counter() - t0)
    be = index._backend
    emit(what="index", backend="device", s=ends, rows_per_s_median=n / median(ends), levels=[list(lv) for lv in be.levels],
         params=index.params.tolist(), **shape)
    # the one call: probes and choice bytes resident
    choice, table, start = index._choice(probe_sizes), index._table, index._start
    levels = be.native_levels()
    c_levels = (_native.EnsembleLevel * len(levels))(*[_native.EnsembleLevel(d, rw, r, b) for d, rw, r, b in levels])
    d_q, d_choice = ctx.to_device(probes), ctx.to_device(choice)
    found = ctypes.c_int64(0)
    p_start, p_table = start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))

    def one_call(d_pairs, cap):
        _native.check(lib.mhx_lsh_ensemble_query_dev(ctx.handle, c_levels, len(levels), p_start, start.size - 1, be.d_sig.ptr, be.code, K,
                                                     d_q.ptr, m, d_choice.ptr, p_table, table.shape[0], d_pairs, cap, ctypes.byref(found)))

    one_call(None, 0)
    n_pairs = int(found.value)
    d_pairs = ctx.alloc(max(1, n_pairs) * 16)
    query = lambda: one_call(d_pairs.ptr, n_pairs)
    warm(query, ctx.synchronize)
    q = timed(ctx, query)
    items = int(sum(int(table[c, 1]) * int(cnt) for c, cnt in zip(*np.unique(choice[choice < len(table)], return_counts=True))))
    emit(what="query", n_probes=m, pairs=n_pairs, band_searches=items, ms=q, ms_median=median(q), probes_per_s=m / median(q) * 1e3, **shape)
    ctx.synchronize()
    one = d_pairs.download((n_pairs, 2), np.int64)
    # the loop over the existing entry point: one call per (partition, selected parameter)
    calls = []
    for p in range(start.size - 1):
        s0, n_p = int(start[p]), int(start[p + 1] - start[p])
        for c in np.unique(choice[:, p]).tolist():
            if c >= len(table) or n_p == 0 or table[c, 1] == 0:
                continue
            level, b = table[c].tolist()
            d_dig, d_rows, r, bands = levels[level]
            who = np.flatnonzero(choice[:, p] == c)
            calls.append(dict(who=who, s0=s0, n_p=n_p, b=b, r=r, d_dig=d_dig + bands * s0 * 8, d_rows=d_rows + bands * s0 * 4,
                              d_sig=be.d_sig.ptr + s0 * be.row_bytes, d_q=ctx.to_device(probes[who]), found=ctypes.c_int64(0)))

    def run(call):
        _native.check(lib.mhx_lsh_query_dev(ctx.handle, call["d_dig"], call["d_rows"], call["n_p"], call["b"], call["r"], call["d_q"].ptr,
                                            call["d_sig"], be.code, K, call["who"].size, call["d_out"].ptr if call.get("d_out") else None,
                                            call["cap"], ctypes.byref(call["found"])))

    for call in calls:  # size every call's output once
        call["cap"] = 0
        run(call)
        call["cap"] = int(call["found"].value)
        call["d_out"] = ctx.alloc(max(1, call["cap"]) * 16)
    looped = lambda: [run(call) for call in calls]
    warm(looped, ctx.synchronize)
    lp = timed(ctx, looped)
    ctx.synchronize()
    parts = []
    for call in calls:
        local = call["d_out"].download((call["cap"], 2), np.int64) if call["cap"] else np.empty((0, 2), dtype=np.int64)
        parts.append(np.stack([call["who"][local[:, 0]], call["s0"] + local[:, 1]], axis=1))
    merged = np.concatenate(parts) if parts else np.empty((0, 2), dtype=np.int64)
    merged = merged[np.lexsort((merged[:, 1], merged[:, 0]))]
    assert np.array_equal(merged, one), "the loop over mhx_lsh_query_dev and the one call disagree"
    emit(what="query_looped", n_probes=m, calls=len(calls), pairs=int(merged.shape[0]), ms=lp, ms_median=median(lp),
         one_call_over_looped=median(q) / median(lp), **shape)
    del calls, parts, merged
    # query_bulk: end to end
    ends = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        got = index.query_bulk(probes, probe_sizes)
        ends.append(time.perf_counter() - t0)
    emit(what="query_bulk", backend="device", n_probes=m, keys_out=sum(map(len, got)), s=ends, probes_per_s_median=m / median(ends), **shape)
    if not with_numpy:
        return
    host = MinHashLSHEnsemble(num_perm=K, gpu_mode="disable", **ctor)
    t0 = time.perf_counter()
    host.index_bulk(keys, sig, sizes)
    s = time.perf_counter() - t0
    emit(what="index", backend="numpy", s=[s], rows_per_s_median=n / s, **shape)
    mh = n_of(10_000)
    some = slice((m - mh) // 2, (m + mh) // 2)  # half rows of the index, half perturbed, like the whole set
    ends = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        want = host.query_bulk(probes[some], probe_sizes[some])
        ends.append(time.perf_counter() - t0)
    emit(what="numpy", n_probes=mh, keys_out=sum(map(len, want)), s=ends, probes_per_s_median=mh / median(ends), **shape)
    assert want == got[some]


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_ensemble.py needs an MI355X")
    which = sys.argv[1:] or ["default", "t05"]
    n = n_of(1_000_000)
    if "default" in which:
        bench("default", n, with_numpy=True)
    if "t05" in which:
        bench("threshold=0.5", n, with_numpy=False, threshold=0.5)
    if "trace" in which:
        bench("default", n, with_numpy=False)


if __name__ == "__main__":
    main()
