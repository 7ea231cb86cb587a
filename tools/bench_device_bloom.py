#!/usr/bin/env python3
"""tools/bench_device_bloom.py -- the Bloom-filter kernels of MinHashLSHBloom on the device.

Device work is timed with HIP events behind tools/_warm.py's clock warm-up, median of 11 runs (all of them are kept).

  insert / query / query_then_insert
              mhx_bloom_*_dev on a resident 1M x 128 uint32 signature matrix, (b, r) = (9, 13) and (32, 4), filters sized for
              n = 1M and fp = 1e-4, on a fresh corpus and on one whose second half repeats its first; both lane mappings and
              the default, which takes the faster of the two for each operation (option bloom.lanes = 16, 1, 0).  The filter is zeroed before every timed insert (outside the events).  Algorithmic bytes:
              the signature bytes the bands cover + 64 per (row, band) (x 2 for query then insert, whose second launch reads
              the signatures again).  Fractions are of 8 TB/s.
  atomics     the same insert into a filter that holds every key already (reads only) next to the fresh insert: the
              difference is what the atomics cost.  This tool is the only measurement of the integer-atomic rate of the chip
              in this repository; it is not checked against hardware counters.
  crossover   insert_bulk + query_bulk of one batch end to end, host arrays in and out: the numpy twin against the device path
              (upload, two kernels, download), 2^4 .. 2^18 rows of (b, r) = (9, 13) -- the curves DETECT_DEVICE_KEYS is read from.
  minhash_lsh the sorted-band MinHashLSH of this package at the same shape, as context: the build of the index from the resident
              matrix (mhx_lsh_sort_bands_dev, its bulk insert) and mhx_lsh_query_dev of the same 1M rows as resident probes
              (blocking: the pair count comes back to the host inside the timed span).

`python tools/bench_device_bloom.py [--out profiles/bloom_bench.json]`; SCALE (env, float, default 1) scales the row count."""
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


def emit(**rec):
    RECORDS.append(rec)
    print(json.dumps(rec), flush=True)


def timed(ctx, call, before=None, reps=REPS):
    out = []
    e0, e1 = ctx.event(), ctx.event()  # one pair for all repetitions
    for _ in range(reps):
        if before:
            before()
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_ms(e1))
    return out


def main():
    from datasketch_amd import _native
    from datasketch_amd import lsh_bloom as B
    from datasketch_amd._native import MHX_U32, check

    if not _native.gpu_available():
        raise SystemExit("bench_device_bloom.py needs an MI355X")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "bloom_bench.json")
    ctx = _native.context()
    lib, vp = ctx.lib, ctypes.c_void_p
    rng = np.random.RandomState(23)
    emit(what="device", **ctx.info())
    n, num_perm = max(64, int(1_000_000 * SCALE)), 128
    k, nb = B.bloom_size(1_000_000, 1e-4)
    fresh = rng.randint(0, 2**32, size=(n, num_perm), dtype=np.uint32)
    dup = fresh.copy()
    dup[n // 2:] = dup[: n - n // 2]
    d_hit = ctx.alloc(n)
    for b, r in ((9, 13), (32, 4)):
        nbytes = b * nb * 64
        d_filter = ctx.alloc(nbytes)
        zero = lambda: (check(lib.mhx_memset_dev(ctx.handle, vp(d_filter.ptr), 0, nbytes)), ctx.synchronize())  # noqa: E731
        algo = n * b * r * 4 + n * b * 64
        for corpus, sig in (("fresh", fresh), ("half_duplicated", dup)):
            d_sig = ctx.to_device(sig)
            args = (ctx.handle, vp(d_sig.ptr), MHX_U32, n, num_perm, b, r, k, nb, vp(d_filter.ptr))
            insert = lambda: check(lib.mhx_bloom_insert_dev(*args))  # noqa: E731
            query = lambda: check(lib.mhx_bloom_query_dev(*args, vp(d_hit.ptr), 0))  # noqa: E731
            both = lambda: check(lib.mhx_bloom_query_dev(*args, vp(d_hit.ptr), 1))  # noqa: E731
            for lanes in (16, 1, 0):
                ctx.set_option("bloom.lanes", lanes)
                shape = dict(rows=n, num_perm=num_perm, b=b, r=r, k=k, n_blocks=nb, filter_bytes=nbytes, corpus=corpus, lanes=lanes)

                def rate(what, call, nbytes_moved, before=None):
                    warm(call, ctx.synchronize)
                    ms = timed(ctx, call, before)
                    med = float(np.median(ms))
                    emit(what=what, ms=ms, ms_median=med, algorithmic_bytes=int(nbytes_moved), fraction_of_8tbs=nbytes_moved / (med * 1e-3) / PEAK,
                         keys_per_s=n * b / (med * 1e-3), **shape)
                    return med

                t_fresh = rate("insert", insert, algo, before=zero)
                t_full = rate("insert_all_present", insert, algo)  # the filter holds every key: loads, no atomics
                emit(what="atomics", ms_with=t_fresh, ms_without=t_full, keys=n * b, note="unchecked against counters", **shape)
                rate("query", query, algo)
                rate("query_then_insert", both, 2 * algo, before=zero)
            ctx.set_option("bloom.lanes", 0)
            if corpus == "fresh":  # the device's words against the twin's, on a slice
                zero()
                some = fresh[:2000]
                check(lib.mhx_bloom_insert_dev(ctx.handle, vp(d_sig.ptr), MHX_U32, 2000, num_perm, b, r, k, nb, vp(d_filter.ptr)))
                want = np.zeros((b, nb, 16), dtype=np.uint32)
                B.insert_host(want, some, r, k)
                assert np.array_equal(d_filter.download((b, nb, 16), np.uint32), want)
            d_sig.free()
        d_filter.free()
    # crossover: twin against device, end to end
    b, r = 9, 13
    for e in range(4, 19, 2):
        rows = 1 << e
        sig = rng.randint(0, 2**32, size=(rows, num_perm), dtype=np.uint32)
        host, dev = [], []
        words = np.zeros((b, nb, 16), dtype=np.uint32)
        d_filter = ctx.to_device(words)
        for _ in range(5):
            t0 = time.perf_counter()
            B.insert_host(words, sig, r, k)
            a = B.query_host(words, sig, r, k)
            host.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            ctx.bloom_insert(sig, d_filter, b, r, k, nb)
            c = ctx.bloom_query(sig, d_filter, b, r, k, nb)
            dev.append(time.perf_counter() - t0)
        assert np.array_equal(a, c)
        t0 = time.perf_counter()
        ctx.to_device(words).free()
        emit(what="crossover", rows=rows, keys=rows * b, host_ms_median=float(np.median(host)) * 1e3, device_ms_median=float(np.median(dev)) * 1e3,
             filter_upload_ms=(time.perf_counter() - t0) * 1e3, filter_bytes=int(words.nbytes))
        d_filter.free()
    # context: the sorted-band MinHashLSH at the same shape
    d_sig = ctx.to_device(fresh)
    for b, r in ((9, 13), (32, 4)):
        d_dig, d_rows = ctx.alloc(8 * n * b), ctx.alloc(4 * n * b)
        build = lambda: ctx.lsh_sort_bands_dev(d_sig.ptr, MHX_U32, n, num_perm, b, r, d_dig.ptr, d_rows.ptr)  # noqa: E731
        warm(build, ctx.synchronize)
        ms = timed(ctx, build)
        emit(what="minhash_lsh_build", rows=n, b=b, r=r, ms=ms, ms_median=float(np.median(ms)))
        capacity, found = 4 * n, ctypes.c_int64(0)
        d_pairs = ctx.alloc(capacity * 16)
        query = lambda: check(lib.mhx_lsh_query_dev(ctx.handle, vp(d_dig.ptr), vp(d_rows.ptr), n, b, r, vp(d_sig.ptr), vp(d_sig.ptr), MHX_U32,  # noqa: E731
                                                    num_perm, n, vp(d_pairs.ptr), capacity, ctypes.byref(found)))
        warm(query, ctx.synchronize)
        ms = timed(ctx, query)
        assert n <= found.value <= capacity  # every probe finds itself
        emit(what="minhash_lsh_query", rows=n, probes=n, b=b, r=r, pairs=int(found.value), ms=ms, ms_median=float(np.median(ms)))
        d_pairs.free()
        d_dig.free()
        d_rows.free()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(RECORDS, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
