#!/usr/bin/env python3
"""tools/bench_device_hll.py -- the HyperLogLog kernels on the device, each figure next to what it is measured against.

Device work is timed with HIP events behind tools/_warm.py's clock warm-up, median of 11 runs (all of them are kept).  Shapes:

  bulk        mhx_hll_bulk_dev on resident uint32 hashes: 1M x 256 at p = 8 and p = 12, 100k x 4096 at p = 14, one set of 10^8
              tokens at p = 16 (the split path).  Algorithmic bytes: hash bytes + n * m.
  histogram   mhx_hll_histogram_dev over 1M x 256 registers.  Algorithmic bytes: n * m + n * 256.
  union       mhx_hll_union_groups_dev over the same matrix in groups of 8 rows.  Algorithmic bytes: n * m + n_groups * m.
  merge       mhx_hll_merge_dev of two such matrices.  Algorithmic bytes: 3 * n * m.
  crossover   update_batch of one sketch (p = 8) end to end, host arrays in and out: the vectorised numpy twin against the
              device path (upload, kernel, download), 2^8 .. 2^22 tokens -- the two curves UPDATE_BATCH_HOST_TOKENS is read from.
  per_token   the per-token Python loop (hashfunc, bit_length, max on a numpy scalar) the reference runs, on a subsample, and
              its linear extrapolation to the headline shape.  With DATASKETCH_REFERENCE set the
              loop is the reference's own HyperLogLog.update; otherwise this package's update, which takes the same steps.

`python tools/bench_device_hll.py [--out profiles/hll_bench.json]`; SCALE (env, float, default 1) scales the set counts for
a dry run.  Fractions are of 8 TB/s."""
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
REPS = 11
PEAK = 8e12
RECORDS = []


def n_of(x):
    return max(8, int(x * SCALE))


def emit(**rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def timed(ctx, call, reps=REPS):
    out = []
    for _ in range(reps):
        e0 = ctx.event().record()
        call()
        e1 = ctx.event().record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1))
    return out


def device_rate(ctx, what, call, nbytes, **shape):
    warm(call, ctx.synchronize)
    ms = timed(ctx, call)
    med = float(np.median(ms))
    emit(what=what, ms=ms, ms_median=med, algorithmic_bytes=int(nbytes), tb_per_s=nbytes / med / 1e9, fraction_of_8tbs=nbytes / (med * 1e-3) / PEAK, **shape)


def random_u32(rng, count):
    out = np.empty(count, dtype=np.uint32)
    step = 1 << 26
    for s in range(0, count, step):
        out[s: s + step] = rng.randint(0, 2**32, size=min(step, count - s), dtype=np.uint32)
    return out


def main():
    from datasketch_amd import HyperLogLog, _native, prehashed
    from datasketch_amd import hyperloglog as H
    from datasketch_amd._native import MHX_U32, check

    if not _native.gpu_available():
        raise SystemExit("bench_device_hll.py needs an MI355X")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hll_bench.json")
    ctx = _native.context()
    lib = ctx.lib
    vp = ctypes.c_void_p
    rng = np.random.RandomState(19)
    emit(what="device", **ctx.info())
    # bulk: resident hashes
    d_keep = None
    for n, t, p in ((n_of(1_000_000), 256, 8), (n_of(1_000_000), 256, 12), (n_of(100_000), 4096, 14), (1, n_of(100_000_000), 16)):
        m = 1 << p
        hv = random_u32(rng, n * t)
        d_hv, d_out = ctx.to_device(hv), ctx.alloc(n * m)
        call = lambda: check(lib.mhx_hll_bulk_dev(ctx.handle, vp(d_hv.ptr), MHX_U32, None, t, n, n * t, p, 32, None, 0, vp(d_out.ptr), None))
        device_rate(ctx, "bulk", call, hv.nbytes + n * m, n_sets=n, tokens_per_set=t, p=p, layout=_native.hll_layout(p),
                    split=bool(t > 32768))
        if d_keep is None:
            d_keep, n_keep = d_out, n  # the 1M x 256 register matrix for the reductions below
            some = min(n, 64)
            want = H._registers_host(hv, None, t, some, p, 32, None)
            assert np.array_equal(d_out.download((some, m), np.uint8), want)
        else:
            d_out.free()
        d_hv.free()
        del hv
    n, m, p = n_keep, 256, 8
    d_hist, d_bad = ctx.alloc(n * 256), ctx.alloc(8)
    device_rate(ctx, "histogram", lambda: check(lib.mhx_hll_histogram_dev(ctx.handle, vp(d_keep.ptr), n, p, vp(d_hist.ptr), vp(d_bad.ptr))),
                n * m + n * 256, n_rows=n, p=p)
    groups = np.arange(0, n + 1, 8, dtype=np.int64)
    d_groups, d_union = ctx.to_device(groups), ctx.alloc((groups.size - 1) * m)
    device_rate(ctx, "union", lambda: check(lib.mhx_hll_union_groups_dev(ctx.handle, vp(d_keep.ptr), n, p, vp(d_groups.ptr), groups.size - 1, vp(d_union.ptr))),
                n * m + (groups.size - 1) * m, n_rows=n, n_groups=int(groups.size - 1), p=p)
    d_other = ctx.alloc(n * m)
    ctx.copy_dev(d_other.ptr, d_keep.ptr, n * m)
    device_rate(ctx, "merge", lambda: check(lib.mhx_hll_merge_dev(ctx.handle, vp(d_other.ptr), vp(d_keep.ptr), n * m)), 3 * n * m, n_rows=n, p=p)
    # crossover of update_batch: host twin against the device path, end to end
    for e in range(8, 23, 2):
        t = 1 << e
        hv = random_u32(rng, t).astype(np.uint64)
        init = np.zeros(256, dtype=np.uint8)
        host, dev = [], []
        for _ in range(7):
            t0 = time.perf_counter()
            a = H._registers_host(hv, None, t, 1, 8, 32, init)
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            b, _ = ctx.hll_bulk(hv, None, t, 1, 8, 32, init)
            dev.append(time.perf_counter() - t0)
        assert np.array_equal(a, b)
        emit(what="crossover", tokens=t, host_ms_median=float(np.median(host)) * 1e3, device_ms_median=float(np.median(dev)) * 1e3)
    # the reference's per-token loop on a subsample
    ref_dir = os.environ.get("DATASKETCH_REFERENCE")
    if ref_dir:
        sys.path.insert(0, ref_dir)
        import datasketch as ref

        make, loop = (lambda: ref.HyperLogLog(p=8, hashfunc=lambda x: x)), "reference HyperLogLog.update"
    else:
        make, loop = (lambda: HyperLogLog(p=8, hashfunc=prehashed, gpu_mode="disable")), "datasketch_amd HyperLogLog.update (the reference's steps)"
    sub = rng.randint(0, 2**32, size=200 * 256, dtype=np.uint64).reshape(200, 256).tolist()
    t0 = time.perf_counter()
    for tokens in sub:
        h = make()
        for tok in tokens:
            h.update(tok)
    s = time.perf_counter() - t0
    per_token = s / (200 * 256)
    emit(what="per_token", loop=loop, sets=200, tokens_per_set=256, s=s, ns_per_token=per_token * 1e9,
         extrapolated_s_for_1M_x_256=per_token * 1_000_000 * 256)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(RECORDS, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
