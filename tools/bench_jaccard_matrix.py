#!/usr/bin/env python3
"""tools/bench_jaccard_matrix.py -- the all-pairs Jaccard kernels (jaccard_kernels.hip) on device-resident matrices: one JSON
line per shape with the time per call (HIP events, after tools/_warm.py's clock warm-up), pairs/s, and the share of the bound
that limits the shape.

Bounds (MI355X): VALU 256 CUs x 4 SIMD x 32 lanes x 2.4 GHz = 7.86e13 lane-ops/s; HBM 8 TB/s.  Lane-ops per
pair are counted from the kernels' inner loops: 2 per 32-bit word for dense uint32 (v_cmp_eq + v_addc), 2 per packed word for
b = 1 (v_xor + v_bcnt), 4 per packed word for b = 2 (xor, shift, bitop3, bcnt).  The matrix
form also writes 4 bytes per pair.  A self-join computes the n (n - 1) / 2 pairs i < j (plus the diagonal tiles' lower halves).

SHAPES (env, comma-separated) picks a subset by name; SCALE (env, float, default 1) scales the row counts for a dry run.

`bench_jaccard_matrix.py topk [out.jsonl]` times the top-k form instead (jaccard_topk_kernels.hip, k = 10): the strip kernel next
to the matrix kernel on the same shape in the same run (`ratio_to_matrix`), the strip and the stream kernel on 1 .. 32 probes
against 10^7 rows (the crossover table; `hbm_frac` = the bytes of B read once at 8 TB/s over the time), 1000 probes against 10^7
rows, and b = 1.  The lines go to stdout and, appended, to the file (profiles/jaccard_topk_bench.jsonl)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

VALU_PEAK = 256 * 4 * 32 * 2.4e9
HBM_PEAK = 8.0e12

# name, kind ("u32" dense or b-bit width), rows of A, rows of B (0: self-join), K, threshold form?, min_count
SHAPES = [
    ("dense_k128_matrix_32k", "u32", 32768, 32768, 128, False, 0),
    ("dense_k128_selfjoin_200k_t0.5", "u32", 200_000, 0, 128, True, 64),
    ("dense_k256_matrix_16k", "u32", 16384, 16384, 256, False, 0),
    ("bbit1_k128_selfjoin_1m_t0.5", 1, 1_000_000, 0, 128, True, 96),
    ("bbit2_k128_selfjoin_1m_t0.5", 2, 1_000_000, 0, 128, True, 80),
    ("bbit1_k128_matrix_32k", 1, 32768, 32768, 128, False, 0),
]


def _words(kind, k):
    if kind == "u32":
        return k
    slot = 1 if kind == 1 else 2 if kind == 2 else 4
    return 2 * -(-k // (64 // slot))


def _ops_per_word(kind):
    return 2 if kind in ("u32", 1) else 4


def _planted(rng, n, k):
    """n random uint32 rows with 1% of them near-copies (a quarter of the positions replaced) of another row."""
    sig = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64).astype(np.uint32)
    dup = rng.choice(n, size=n // 100, replace=False)
    src = rng.randint(0, n, size=dup.size)
    sig[dup] = sig[src]
    repl = rng.random_sample((dup.size, k)) < 0.25
    sig[dup] = np.where(repl, rng.randint(0, 2**32, size=(dup.size, k), dtype=np.uint64).astype(np.uint32), sig[dup])
    return sig


def _timed(ctx, run, reps=5):
    run()
    ctx.synchronize()
    warm(run, ctx.synchronize, 0.5)  # GPU clocks (tools/_warm.py)
    ms = []
    for _ in range(reps):
        e0, e1 = ctx.event(), ctx.event()
        e0.record()
        run()
        e1.record()
        ctx.synchronize()
        ms.append(e0.elapsed_ms(e1))
    return ms


# name, kind, rows of A, rows of B, K, paths (1 strip, 2 stream, 0 auto), also time the matrix kernel?
TOPK_SHAPES = [
    ("topk_dense_k128_32k", "u32", 32768, 32768, 128, (1,), True),
    ("topk_dense_k128_4096x1m", "u32", 4096, 1_000_000, 128, (1,), True),
    ("topk_bbit1_k128_4096x1m", 1, 4096, 1_000_000, 128, (1,), True),
] + [("topk_dense_k128_%dx1m" % q, "u32", q, 1_000_000, 128, (1, 2), False) for q in (1, 2, 4, 8, 16, 32)] + [
    ("topk_dense_k128_%dx10m" % q, "u32", q, 10_000_000, 128, (1, 2), False) for q in (1, 2, 4, 8, 16, 32)] + [
    ("topk_dense_k128_1000x10m", "u32", 1000, 10_000_000, 128, (0,), False),
]


def topk_main(out_path):
    from datasketch_amd import _native

    pick = set(filter(None, os.environ.get("SHAPES", "").split(",")))
    scale = float(os.environ.get("SCALE", "1"))
    topk = 10
    ctx = _native.context()
    rng = np.random.RandomState(7)
    base = _planted(rng, max(1, int(1_000_000 * scale)) + 32768, 128)  # B is this matrix, repeated where it is longer
    out = open(out_path, "a") if out_path else None
    held = (None, None, None)  # (kind, n_b, B on the device): consecutive shapes share it
    for name, kind, n_a, n_b, k, paths, with_matrix in TOPK_SHAPES:
        if pick and name not in pick:
            continue
        n_b = max(1, int(n_b * scale))
        a_rows = base[base.shape[0] - 32768:][:n_a]
        row_bytes = 4 * k if kind == "u32" else 8 * (_words(kind, k) // 2)

        def on_device(rows):
            if kind == "u32":
                return ctx.to_device(rows)
            d_full, dst = ctx.to_device(rows), ctx.alloc(row_bytes * rows.shape[0])
            _native.check(ctx.lib.mhx_bbit_pack_dev_typed(ctx.handle, d_full.ptr, _native.MHX_U32, rows.shape[0], k, kind, dst.ptr))
            ctx.synchronize()
            return dst

        if held[:2] != (kind, n_b):
            held = (None, None, None)
            reps_b = -(-n_b // (base.shape[0] - 32768))
            held = (kind, n_b, on_device(np.tile(base[: base.shape[0] - 32768], (reps_b, 1))[:n_b]))
        d_a, d_b = on_device(a_rows), held[2]
        d_r, d_c = ctx.alloc(8 * n_a * topk), ctx.alloc(4 * n_a * topk)
        matrix_ms = None
        if with_matrix:
            d_m = ctx.alloc(4 * n_a * n_b)
            if kind == "u32":
                matrix_ms = min(_timed(ctx, lambda: ctx.jaccard_matrix_dev(d_a.ptr, n_a, d_b.ptr, n_b, _native.MHX_U32, k, d_m.ptr, n_b)))
            else:
                matrix_ms = min(_timed(ctx, lambda: ctx.bbit_jaccard_matrix_dev(d_a.ptr, n_a, d_b.ptr, n_b, k, kind, d_m.ptr, n_b)))
            del d_m
        for path in paths:
            ctx.set_option("jaccard.topk_path", path)
            if kind == "u32":
                run = lambda: ctx.jaccard_topk_dev(d_a.ptr, n_a, d_b.ptr, n_b, _native.MHX_U32, k, None, 0, topk, d_r.ptr, d_c.ptr)
            else:
                run = lambda: ctx.bbit_jaccard_topk_dev(d_a.ptr, n_a, d_b.ptr, n_b, k, kind, None, 0, topk, d_r.ptr, d_c.ptr)
            ms = _timed(ctx, run)
            t = min(ms) * 1e-3
            rec = {"shape": name, "kind": kind, "n_a": n_a, "n_b": n_b, "k": k, "topk": topk,
                   "path": {0: "auto", 1: "strip", 2: "stream"}[path], "ms_min": round(min(ms), 4), "ms": [round(x, 4) for x in ms],
                   "pairs_per_s": n_a * n_b / t, "hbm_frac": round(n_b * row_bytes / HBM_PEAK / t, 4),
                   "matrix_ms_min": None if matrix_ms is None else round(matrix_ms, 4),
                   "ratio_to_matrix": None if matrix_ms is None else round(min(ms) / matrix_ms, 4)}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        ctx.set_option("jaccard.topk_path", 0)
        del d_a, d_b, d_r, d_c
        ctx.release_scratch()
    if out:
        out.close()


def main():
    from datasketch_amd import _native

    pick = set(filter(None, os.environ.get("SHAPES", "").split(",")))
    scale = float(os.environ.get("SCALE", "1"))
    ctx = _native.context()
    rng = np.random.RandomState(7)
    for name, kind, n_a, n_b, k, thresh, min_count in SHAPES:
        if pick and name not in pick:
            continue
        n_a, n_b = max(1, int(n_a * scale)), int(n_b * scale)
        self_join = n_b == 0
        sig = _planted(rng, n_a + n_b, k)
        if kind == "u32":
            d_sig = ctx.to_device(sig)
            row_bytes = 4 * k
        else:
            d_full = ctx.to_device(sig)
            nb = _words(kind, k) // 2
            d_sig = ctx.alloc(8 * (n_a + n_b) * nb)
            _native.check(ctx.lib.mhx_bbit_pack_dev_typed(ctx.handle, d_full.ptr, _native.MHX_U32, n_a + n_b, k, kind, d_sig.ptr))
            ctx.synchronize()
            del d_full
            row_bytes = 8 * nb
        d_a = d_sig.ptr
        d_b = None if self_join else d_sig.ptr + n_a * row_bytes
        nb_rows = n_a if self_join else n_b
        pairs = n_a * (n_a - 1) // 2 if self_join else n_a * nb_rows
        if thresh:
            cap = 1 << 22
            d_p, d_c = ctx.alloc(16 * cap), ctx.alloc(4 * cap)
            if kind == "u32":
                run = lambda: ctx.jaccard_threshold_pairs_dev(d_a, n_a, d_b, nb_rows, _native.MHX_U32, k, min_count, d_p.ptr, d_c.ptr, cap)
            else:
                run = lambda: ctx.bbit_jaccard_threshold_pairs_dev(d_a, n_a, d_b, nb_rows, k, kind, min_count, d_p.ptr, d_c.ptr, cap)
        else:
            d_m = ctx.alloc(4 * n_a * nb_rows)
            if kind == "u32":
                run = lambda: ctx.jaccard_matrix_dev(d_a, n_a, d_b, nb_rows, _native.MHX_U32, k, d_m.ptr, nb_rows)
            else:
                run = lambda: ctx.bbit_jaccard_matrix_dev(d_a, n_a, d_b, nb_rows, k, kind, d_m.ptr, nb_rows)
        found = run()
        ctx.synchronize()
        warm(run, ctx.synchronize, 0.5)  # GPU clocks (tools/_warm.py)
        ms = []
        reps = 5
        for _ in range(reps):
            e0, e1 = ctx.event(), ctx.event()
            e0.record()
            run()
            e1.record()
            ctx.synchronize()
            ms.append(e0.elapsed_ms(e1))
        t = min(ms) * 1e-3
        w = _words(kind, k)
        valu_s = pairs * w * _ops_per_word(kind) / VALU_PEAK
        hbm_s = 0.0 if thresh else pairs * 4 / HBM_PEAK
        bound = "valu" if valu_s >= hbm_s else "hbm_write"
        rec = {"shape": name, "kind": kind, "n_a": n_a, "n_b": nb_rows, "self_join": self_join, "k": k, "threshold_form": thresh,
               "min_count": min_count if thresh else None, "pairs_found": found if thresh else None,
               "ms_min": round(min(ms), 4), "ms": [round(x, 4) for x in ms], "pairs_per_s": pairs / t,
               "bound": bound, "bound_ms": round(max(valu_s, hbm_s) * 1e3, 4), "share_of_bound": round(max(valu_s, hbm_s) / t, 4)}
        print(json.dumps(rec), flush=True)
        del d_sig
        if thresh:
            del d_p, d_c
        else:
            del d_m
        ctx.release_scratch()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "topk":
        topk_main(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main()
