#!/usr/bin/env python3
"""tools/bench_device_shingles.py -- shingles hashed in place (sha1_windows_kernel), each figure next to what it is measured against.

Corpus: seeded, synthetic, nothing downloaded -- 200 000 documents of about 1 KiB, words of 2 .. 9 letters drawn from a
Zipf-distributed list of 50 000 and separated by blanks, so that shingles repeat as they do in text.

  (a) kernel   mhx_sha1_windows_dev against mhx_sha1_tokens_dev on the SAME windows materialised into a packed buffer (what the
               library offered before): byte mode k = 5 and 9, token mode w = 3 (a token is a word with its blank), on the first
               50 000 documents, everything resident.  Launches are timed with the context's events behind tools/_warm.py's clock
               warm-up, the two kernels alternating, 11 runs each; all of them are printed.  The windows kernel is accepted if
               its median does not exceed the token kernel's by more than that kernel's own spread (max - min).
  (b) end to end   host arrays in, signatures out (num_perm 128, wall clock, the upload and the download included):
               MinHash.bulk_signatures(documents=, shingle=k) on the whole corpus against the two routes there were --
               Python slices into bulk_signatures(b), and a numpy-built packed= triple with the time to build it counted.  The
               two old routes run on a subsample (2 000 and 20 000 documents) and are scaled to the corpus by documents; the
               line says so.
  (c) counters     mhx_ctx_counters over the MinHash launches of (b)'s new route: how many sets left the sieve.

`python tools/bench_device_shingles.py [kernel] [end_to_end] [--out profiles/shingles_bench.txt]` (no part named: both); with
MHX_LIBRARY naming a second build of the library, part (a) is the same-box A/B of two kernel variants.  SCALE (env, float, default 1) scales the document
counts for a dry run."""
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
LINES = []


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def corpus(n_docs, seed=0, vocab_size=50_000):
    """(uint8 text, int64 doc_offsets, int64 word_offsets): word i is text[word_offsets[i]:word_offsets[i+1]], its blank included."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(2, 10, size=vocab_size)
    starts = np.concatenate([[0], np.cumsum(lens + 1)])
    vocab = rng.randint(97, 123, size=int(starts[-1]), dtype=np.uint8)
    vocab[starts[1:] - 1] = 32
    words_per_doc = rng.randint(120, 196, size=n_docs)
    parts, word_lens = [], []
    for s in range(0, n_docs, 10_000):
        n_words = int(words_per_doc[s: s + 10_000].sum())
        ranks = np.minimum(rng.zipf(1.2, size=n_words), vocab_size) - 1
        wl = lens[ranks] + 1
        out_start = np.concatenate([[0], np.cumsum(wl)])
        parts.append(vocab[np.repeat(starts[ranks] - out_start[:-1], wl) + np.arange(int(out_start[-1]))])
        word_lens.append(wl)
    word_offsets = np.concatenate([[0], np.cumsum(np.concatenate(word_lens))]).astype(np.int64)
    doc_words = np.concatenate([[0], np.cumsum(words_per_doc)]).astype(np.int64)
    return np.concatenate(parts), word_offsets[doc_words], word_offsets, doc_words


def materialised(text, item_offsets, doc_offsets, width, set_offsets):
    """The windows copied back to back: (packed bytes, int64 byte offsets) -- the input mhx_sha1_tokens_dev needs."""
    counts = np.diff(set_offsets)
    first = np.repeat(doc_offsets[:-1] - set_offsets[:-1], counts) + np.arange(int(set_offsets[-1]))  # every document has >= width items
    if item_offsets is None:
        packed = np.lib.stride_tricks.sliding_window_view(text, width)[first].reshape(-1)
        return packed, np.arange(first.size + 1, dtype=np.int64) * width
    beg, end = item_offsets[first], item_offsets[first + width]
    offs = np.concatenate([[0], np.cumsum(end - beg)]).astype(np.int64)
    parts = []
    for s in range(0, first.size, 1 << 21):
        e = min(first.size, s + (1 << 21))
        parts.append(text[np.repeat(beg[s:e] - offs[s:e], end[s:e] - beg[s:e]) + np.arange(int(offs[s]), int(offs[e]))])
    return np.concatenate(parts), offs


def timed_pair(ctx, run_a, run_b):
    """Event times (ms) of the two launches, alternating, REPS each, behind the clock warm-up."""
    warm(lambda: (run_a(), run_b()), ctx.synchronize)
    ms = ([], [])
    for _ in range(REPS):
        for which, run in enumerate((run_a, run_b)):
            e0 = ctx.event().record()
            run()
            e1 = ctx.event().record()
            e1.synchronize()
            ms[which].append(e0.elapsed_ms(e1))
    return ms


def kernel_alone(ctx, text, doc_offsets, word_offsets, doc_words):
    from datasketch_amd import shingle
    from datasketch_amd._native import MHX_U32, check

    d_text = ctx.to_device(text)
    for mode, width in (("bytes", 5), ("bytes", 9), ("tokens", 3)):
        items, docs = (None, doc_offsets) if mode == "bytes" else (word_offsets, doc_words)
        set_offsets = shingle.window_offsets(docs, width)
        n_docs, n_windows = docs.size - 1, int(set_offsets[-1])
        t0 = time.perf_counter()
        packed, offs = materialised(text, items, docs, width, set_offsets)
        build_s = time.perf_counter() - t0
        d_items = None if items is None else ctx.to_device(items)
        d_docs, d_sets = ctx.to_device(docs), ctx.to_device(set_offsets)
        d_packed, d_offs = ctx.to_device(packed), ctx.to_device(offs)
        d_win, d_tok = ctx.alloc(4 * n_windows), ctx.alloc(4 * n_windows)

        def windows():
            ctx.sha1_windows_dev(d_text.ptr, None if d_items is None else d_items.ptr, d_docs.ptr, d_sets.ptr, n_docs, n_windows, width, MHX_U32, d_win.ptr)

        def tokens():
            check(ctx.lib.mhx_sha1_tokens_dev(ctx.handle, d_packed.ptr, d_offs.ptr, n_windows, MHX_U32, d_tok.ptr))

        ms_w, ms_t = timed_pair(ctx, windows, tokens)
        same = bool(np.array_equal(d_win.download(n_windows, np.uint32), d_tok.download(n_windows, np.uint32)))
        med_w, med_t, spread_t = float(np.median(ms_w)), float(np.median(ms_t)), max(ms_t) - min(ms_t)
        emit(what="(a) kernel alone", mode=mode, width=width, documents=n_docs, windows=n_windows, text_bytes=int(text.size),
             materialised_bytes=int(packed.size + offs.nbytes), host_seconds_to_materialise=round(build_s, 3), same_hashes=same,
             windows_kernel_ms=[round(x, 4) for x in ms_w], tokens_kernel_ms=[round(x, 4) for x in ms_t],
             windows_ns_per_window=round(med_w * 1e6 / n_windows, 4), tokens_ns_per_window=round(med_t * 1e6 / n_windows, 4),
             windows_ghash_per_s=round(n_windows / med_w / 1e6, 3), tokens_kernel_spread_ms=round(spread_t, 4),
             accepted=bool(med_w <= med_t + spread_t))
        for buf in (d_items, d_docs, d_sets, d_packed, d_offs, d_win, d_tok):
            if buf is not None:
                buf.free()
    d_text.free()


def end_to_end(ctx, text, doc_offsets):
    from datasketch_amd import MinHash, shingle

    n_docs = doc_offsets.size - 1
    kw = dict(num_perm=128, seed=1, gpu_mode="always")
    for k in (5, 9):
        MinHash.bulk_signatures(documents=(text[: int(doc_offsets[64])], doc_offsets[:65]), shingle=k, **kw)  # code objects, scratch
        ctx.counters(True)
        ctx.minhash_mode(reset=True)
        new = []
        for _ in range(3):
            t0 = time.perf_counter()
            sig = MinHash.bulk_signatures(documents=(text, doc_offsets), shingle=k, out_dtype=np.uint32, **kw)
            new.append(time.perf_counter() - t0)
        counters = ctx.counters(True)
        n_windows = int(shingle.window_offsets(doc_offsets, k)[-1])
        emit(what="(c) MinHash counters over the three runs of (b)'s new route", k=k, sets=3 * n_docs, windows=3 * n_windows, minhash_mode_after=ctx.minhash_mode(),
             **counters)
        # the old routes, on subsamples
        n1 = min(n_docs, n_of(2_000))
        raw = text[: int(doc_offsets[n1])].tobytes()
        t0 = time.perf_counter()
        sets = [[raw[i: i + k] for i in range(int(doc_offsets[d]), int(doc_offsets[d + 1]) - k + 1)] for d in range(n1)]
        old1 = MinHash.bulk_signatures(sets, **kw)
        slices_s = time.perf_counter() - t0
        n2 = min(n_docs, n_of(20_000))
        t0 = time.perf_counter()
        sub_offsets = doc_offsets[: n2 + 1]
        set_offsets = shingle.window_offsets(sub_offsets, k)
        packed, offs = materialised(text, None, sub_offsets, k, set_offsets)
        build_s = time.perf_counter() - t0
        old2 = MinHash.bulk_signatures(packed=(packed, offs, set_offsets), **kw)
        packed_s = time.perf_counter() - t0
        emit(what="(b) host in, signatures out", k=k, documents=n_docs, text_bytes=int(text.size), windows=n_windows,
             documents_shingle_seconds=[round(x, 3) for x in new], documents_shingle_mb_per_s=round(text.size / min(new) / 1e6, 1),
             python_slices_documents=n1, python_slices_seconds=round(slices_s, 3), python_slices_scaled_to_corpus_seconds=round(slices_s * n_docs / n1, 1),
             numpy_packed_documents=n2, numpy_packed_seconds=round(packed_s, 3), of_which_building_the_triple=round(build_s, 3),
             numpy_packed_scaled_to_corpus_seconds=round(packed_s * n_docs / n2, 1),
             same_signatures=bool(np.array_equal(sig[:n1], old1) and np.array_equal(sig[:n2], old2)))


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_shingles.py needs an MI355X")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "shingles_bench.txt")
    ctx = _native.context()
    info = ctx.info()
    t0 = time.perf_counter()
    text, doc_offsets, word_offsets, doc_words = corpus(n_of(200_000))
    emit(what="corpus", library=os.path.basename(_native.LIB_PATH), device=info["name"], cus=info["compute_units"], documents=int(doc_offsets.size - 1), text_bytes=int(text.size), words=int(word_offsets.size - 1),
         seconds_to_draw=round(time.perf_counter() - t0, 2))
    n_a = min(doc_offsets.size - 1, n_of(50_000))
    parts = [a for a in sys.argv[1:] if a in ("kernel", "end_to_end")] or ["kernel", "end_to_end"]
    if "kernel" in parts:
        kernel_alone(ctx, text[: int(doc_offsets[n_a])], doc_offsets[: n_a + 1], word_offsets[: int(doc_words[n_a]) + 1], doc_words[: n_a + 1])
    if "end_to_end" in parts:
        end_to_end(ctx, text, doc_offsets)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
