#!/usr/bin/env python3
"""tools/bench_device_lsh.py -- datasketch_amd.MinHashLSH on the device: the update path (merge, flush, compaction) and the
bulk / per-key entry points.  One JSON line per measurement, every one repeated so that the spread shows; after tools/_warm.py's
clock warm-up; device work timed with HIP events, host-visible steps with a host clock around work that ends in a synchronise.

  merge       mhx_lsh_bands_merge_dev of 10k rows into a 10M x 32-band index; bytes = read + write of 12 B per entry
  flush       insert_bulk + flush of 10k rows (K = 256, uint32) into a 10M-row index, against SortedBandsIndex.extend of the
              same batch on an index of the same rows, in the same run
  compact     compact() after removing 10 % of that index; bytes = what the two passes move
  insert_bulk 1M str keys, K = 256 uint32 host matrix in, index ready (flushed)
  query_bulk  1M probes against that index, lists of keys out
  per_key     insert() of 100k keys one by one, then one query

SCALE (env, float, default 1) scales every row count for a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
HBM_PEAK = 8.0e12
K, B, R = 256, 32, 8


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    print(json.dumps(rec), flush=True)


def chunks(rng, n, k, step=1_250_000):
    for i0 in range(0, n, step):
        yield i0, rng.randint(0, 2**32, (min(step, n - i0), k), dtype=np.uint32)


def bench_merge(ctx):
    n_a, n_b = n_of(10_000_000), n_of(10_000)
    rng = np.random.RandomState(1)
    band = np.cumsum(rng.randint(1, 2**40, n_a, dtype=np.uint64))
    d_da = ctx.to_device(np.tile(band, B))
    d_ra = ctx.to_device(np.tile(np.arange(n_a, dtype=np.uint32), B))
    b_band = np.sort(rng.randint(0, int(band[-1]), n_b, dtype=np.uint64))
    d_db = ctx.to_device(np.tile(b_band, B))
    d_rb = ctx.to_device(np.tile(np.arange(n_b, dtype=np.uint32), B))
    n = n_a + n_b
    out_d, out_r = ctx.alloc(8 * B * n), ctx.alloc(4 * B * n)
    call = lambda: ctx.lsh_bands_merge_dev(d_da.ptr, d_ra.ptr, n_a, d_db.ptr, d_rb.ptr, n_b, n_a, B, out_d.ptr, out_r.ptr)
    moved = 12 * B * (n_a + n_b) * 2
    shapes = (8, 16)  # outputs per thread of the 256-thread tile (option lsh.merge_items), alternated call by call
    times = {items: [] for items in shapes}
    for items in shapes:
        ctx.set_option("lsh.merge_items", items)
        warm(call, ctx.synchronize)
    for _ in range(20):
        for items in shapes:
            ctx.set_option("lsh.merge_items", items)
            e0 = ctx.event().record()
            call()
            e1 = ctx.event().record()
            e1.synchronize()
            times[items].append(e0.elapsed_ms(e1))
    ctx.set_option("lsh.merge_items", 0)
    for items in shapes:
        t = times[items]
        ms = float(np.median(t))
        emit(what="merge", tile=f"256x{items}", n_index=n_a, n_batch=n_b, bands=B, bytes_moved=moved, ms_median=ms, ms_min=min(t),
             ms_max=max(t), tb_per_s=moved / ms / 1e9, share_of_hbm_peak=moved / ms / 1e-3 / HBM_PEAK, target_ms=1.8)


def bench_flush_and_compact():
    from datasketch_amd import MinHashLSH
    from datasketch_amd import lsh_bulk as LB

    n, m = n_of(10_000_000), n_of(10_000)
    rng = np.random.RandomState(2)
    index = MinHashLSH(num_perm=K, params=(B, R), gpu_mode="always")
    sbi = None
    for i0, part in chunks(rng, n, K):
        index.insert_bulk(range(i0, i0 + part.shape[0]), part)
        index.flush()
        if sbi is None:
            sbi = LB.SortedBandsIndex(part, B, R)
        else:
            sbi.extend(part)
    key = n
    flush_s, extend_s = [], []
    for rep in range(6):  # alternated: flush, extend
        batch = rng.randint(0, 2**32, (m, K), dtype=np.uint32)
        t0 = time.perf_counter()
        index.insert_bulk(range(key, key + m), batch)
        index.flush()
        index._backend.ctx.synchronize()
        flush_s.append(time.perf_counter() - t0)
        key += m
        if rep < 3:
            t0 = time.perf_counter()
            sbi.extend(batch)
            sbi.ctx.synchronize()
            extend_s.append(time.perf_counter() - t0)
    del sbi
    f, e = float(np.median(flush_s)), float(np.median(extend_s))
    emit(what="flush", n_index=n, n_batch=m, k=K, bands=B, flush_ms=[1e3 * x for x in flush_s], extend_ms=[1e3 * x for x in extend_s],
         flush_ms_median=1e3 * f, extend_ms_median=1e3 * e, speedup_vs_extend=e / f, target_speedup=3.0)
    gone = rng.choice(key, key // 10, replace=False)
    for g in gone.tolist():
        index.remove(g)
    n_used = index._n_flushed
    n_live = n_used - len(gone)
    row_bytes = K * 4
    moved = n_used * row_bytes + n_live * row_bytes + B * n_used * (4 + 4 + 8) + B * n_live * 12 + n_used // 8
    ctx = index._backend.ctx
    t0 = time.perf_counter()
    index.compact()
    ctx.synchronize()
    s = time.perf_counter() - t0
    # the device part alone, on the compacted index's own buffers (no host bookkeeping): bands and rows of a 10 % dead bitmap
    be = index._backend
    live = rng.rand(be.n) >= 0.1
    n_live = int(live.sum())
    words = np.zeros((be.n + 31) // 32 * 4, dtype=np.uint8)
    packed = np.packbits(live, bitorder="little")
    words[: packed.size] = packed
    d_bits = ctx.to_device(words.view(np.uint32))
    d_sig, d_dig, d_rows = ctx.alloc(n_live * be.row_bytes), ctx.alloc(n_live * B * 8), ctx.alloc(n_live * B * 4)
    dev = []
    for _ in range(4):
        e0 = ctx.event().record()
        ctx.rows_compact_dev(be.d_sig.ptr, be.row_bytes, be.n, d_bits.ptr, d_sig.ptr)
        ctx.lsh_bands_compact_dev(be.d_dig.ptr, be.d_rows.ptr, be.n, B, d_bits.ptr, n_live, d_dig.ptr, d_rows.ptr)
        e1 = ctx.event().record()
        e1.synchronize()
        dev.append(e0.elapsed_ms(e1))
    emit(what="compact", n_used=n_used, n_removed=len(gone), k=K, bands=B, ms=1e3 * s, bytes_moved=moved, tb_per_s=moved / s / 1e12,
         device_passes_ms=dev, device_passes_n=be.n)


class _Sig:
    """A signature as the index sees one: hashvalues and len() (a MinHash's permutations are not needed here)."""

    def __init__(self, hashvalues):
        self.hashvalues = hashvalues

    def __len__(self):
        return len(self.hashvalues)


def bench_bulk_and_per_key():
    from datasketch_amd import MinHashLSH

    n = n_of(1_000_000)
    rng = np.random.RandomState(3)
    sig = rng.randint(0, 2**32, (n, K), dtype=np.uint32)
    sig[1::100_000, :R] = sig[0, :R]  # a few rows share band 0
    keys = [f"doc-{i}" for i in range(n)]
    probes = sig[rng.randint(0, n, n)].copy()
    probes[::2, R:] = 7
    ins, qry = [], []
    for rep in range(3):
        index = MinHashLSH(num_perm=K, params=(B, R), gpu_mode="always")
        index.buffer_size = n
        t0 = time.perf_counter()
        index.insert_bulk(keys, sig)
        index.flush()
        index._backend.ctx.synchronize()
        ins.append(time.perf_counter() - t0)
        if rep < 2:
            t0 = time.perf_counter()
            got = index.query_bulk(probes)
            qry.append(time.perf_counter() - t0)
    found = sum(map(len, got))
    emit(what="insert_bulk", n=n, k=K, s=ins, keys_per_s_median=n / float(np.median(ins)), target_keys_per_s=1e6)
    emit(what="query_bulk", n_probes=n, n_index=n, keys_out=found, s=qry, probes_per_s_median=n / float(np.median(qry)),
         target_probes_per_s=1e6)
    m = n_of(100_000)
    objs = [_Sig(row.astype(np.uint64)) for row in sig[:m]]
    per = []
    for rep in range(2):
        index = MinHashLSH(num_perm=K, params=(B, R), gpu_mode="always")
        t0 = time.perf_counter()
        for key, mh in zip(keys, objs):
            index.insert(key, mh)
        index.query(objs[0])
        per.append(time.perf_counter() - t0)
    emit(what="per_key_insert", n=m, k=K, s=per, keys_per_s_median=m / float(np.median(per)), target_keys_per_s=1e5)


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_lsh.py needs an MI355X")
    ctx = _native.context()
    which = sys.argv[1:] or ["merge", "flush", "bulk"]
    if "merge" in which:
        bench_merge(ctx)
    if "flush" in which:
        bench_flush_and_compact()
    if "bulk" in which:
        bench_bulk_and_per_key()


if __name__ == "__main__":
    main()
