#!/usr/bin/env python3
"""tools/bench_device_words.py -- word shingles from raw text on the device (words_kernels.hip), each figure next to what it is
measured against.

Corpus: the one of tools/bench_device_shingles.py (seeded, synthetic, nothing downloaded: 200 000 documents of about 1 KiB, Zipf
words separated by blanks) made word-like: a tenth of the words capitalised, a tenth of the blanks turned into commas and line
ends, so that normalising changes bytes.  w = 5, num_perm = 128.

  (a) the new whole call    MinHash.bulk_signatures(documents=, shingle=5, words=True): host arrays in, signatures out
  (b) the route there was   a numpy-vectorised host normaliser producing the packed= triple (its time counted and shown), then
                            bulk_signatures(packed=, shingle=5) on the device
  (c) the byte-shingle call bulk_signatures(documents=, shingle=5) on the same corpus, as context
  (d) the normalise launches alone   mhx_words_normalize_dev on resident arrays (bitmap, count, tile offsets, the read-back of the two
                            totals, emit), beside its traffic model at 8 TB/s: the input read twice, the bitmap, out_buf, 8 bytes
                            per word.  Recorded, not gated.

(a), (b) and (c) are host calls, so they are wall-clock times (best and all of three runs, after a small call that loads the code
objects and a full-size one that grows the scratch); (d) is timed with the context's events behind tools/_warm.py's clock warm-up,
11 runs, all printed.  Accepted: (a) faster than (b), identical signatures, and a subsample equal to word_shingles hashed on the host.

`python tools/bench_device_words.py [--out profiles/words_bench.txt]`; SCALE (env, float, default 1) scales the document count for
a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402
from tools.bench_device_shingles import corpus, n_of  # noqa: E402

REPS = 11
W = 5
LINES = []


def emit(**rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def word_like(text, word_offsets, seed=1):
    """The corpus with a tenth of its words capitalised and a tenth of its blanks turned into ',' or a line end (same length)."""
    rng = np.random.RandomState(seed)
    text = text.copy()
    starts = word_offsets[:-1]
    text[starts[rng.random_sample(starts.size) < 0.1]] -= 32
    blanks = word_offsets[1:] - 1
    pick = blanks[rng.random_sample(blanks.size) < 0.1]
    text[pick] = np.frombuffer(b",\n", dtype=np.uint8)[rng.randint(0, 2, size=pick.size)]
    return text


def numpy_normalize(text, doc_offsets, table):
    """normalize_words with numpy alone: the best host route to the packed= triple."""
    n = text.size
    t = table[text]
    w = t != 0
    first = np.zeros(n + 1, dtype=bool)
    first[doc_offsets] = True
    start = w & (first[:-1] | ~np.concatenate([[False], w[:-1]]))
    end = w & (first[1:] | ~np.concatenate([w[1:], [False]]))
    pos = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(w.astype(np.int64) + end, out=pos[1:])
    out = np.empty(int(pos[-1]), dtype=np.uint8)
    out[pos[:-1][w]] = t[w]
    out[pos[:-1][end] + 1] = 32
    words_before = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(start, out=words_before[1:])
    return out, np.concatenate([pos[:-1][start], pos[-1:]]), words_before[doc_offsets]


def best_of(run, n=3):
    times, result = [], None
    for _ in range(n):
        t0 = time.perf_counter()
        result = run()
        times.append(time.perf_counter() - t0)
    return times, result


def main():
    from datasketch_amd import MinHash, _native, shingle

    if not _native.gpu_available():
        raise SystemExit("bench_device_words.py needs an MI355X")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "words_bench.txt")
    ctx = _native.context()
    info = ctx.info()
    text, doc_offsets, word_offsets, _ = corpus(n_of(200_000))
    text = word_like(text, word_offsets)
    n_docs = doc_offsets.size - 1
    table = shingle.word_table()
    emit(what="corpus", library=os.path.basename(_native.LIB_PATH), device=info["name"], cus=info["compute_units"], documents=int(n_docs),
         text_bytes=int(text.size), w=W, num_perm=128)
    kw = dict(num_perm=128, seed=1, gpu_mode="always", out_dtype=np.uint32)
    small = (text[: int(doc_offsets[64])], doc_offsets[:65])
    MinHash.bulk_signatures(documents=small, shingle=W, words=True, **kw)  # code objects
    MinHash.bulk_signatures(documents=(text, doc_offsets), shingle=W, words=True, **kw)  # scratch
    new_s, sig_new = best_of(lambda: MinHash.bulk_signatures(documents=(text, doc_offsets), shingle=W, words=True, **kw))

    build_s, packed = best_of(lambda: numpy_normalize(text, doc_offsets, table), 1)
    MinHash.bulk_signatures(packed=packed, shingle=W, **kw)
    dev_s, sig_old = best_of(lambda: MinHash.bulk_signatures(packed=packed, shingle=W, **kw))
    old_s = [build_s[0] + x for x in dev_s]

    MinHash.bulk_signatures(documents=(text, doc_offsets), shingle=W, **kw)
    byte_s, _ = best_of(lambda: MinHash.bulk_signatures(documents=(text, doc_offsets), shingle=W, **kw))

    # a subsample against the definition hashed on the host, and the triple of the device against numpy's
    n_sub = min(n_docs, 500)
    sub = (text[: int(doc_offsets[n_sub])], doc_offsets[: n_sub + 1])
    want = MinHash.bulk_signatures([shingle.word_shingles(sub[0][int(sub[1][d]): int(sub[1][d + 1])].tobytes(), W) for d in range(n_sub)],
                                   num_perm=128, seed=1, gpu_mode="disable")
    same_def = bool(np.array_equal(sig_new[:n_sub], want))
    same = bool(np.array_equal(sig_new, sig_old))
    emit(what="(a) raw text in, word-shingle signatures out", seconds=[round(x, 4) for x in new_s], mb_per_s=round(text.size / min(new_s) / 1e6, 1))
    emit(what="(b) numpy normaliser, then packed= on the device", seconds=[round(x, 4) for x in old_s], of_which_numpy_normaliser=round(build_s[0], 4),
         device_call_seconds=[round(x, 4) for x in dev_s], words=int(packed[1].size - 1), normal_form_bytes=int(packed[0].size))
    emit(what="(c) byte shingles k=5 of the same corpus, as context", seconds=[round(x, 4) for x in byte_s])
    emit(what="acceptance", a_over_b_speedup=round(min(old_s) / min(new_s), 2), a_faster_than_b=bool(min(new_s) < min(old_s)),
         same_signatures_a_b=same, subsample_documents=int(n_sub), subsample_equals_word_shingles_on_the_host=same_def)

    # (d) the normalise launches alone, everything resident
    d_text, d_docs = ctx.to_device(text), ctx.to_device(doc_offsets)
    _, n_words, n_out = ctx.words_normalize_dev(d_text.ptr, text.size, d_docs.ptr, n_docs, table)
    d_out, d_items, d_wdocs = ctx.alloc(max(n_out, 1)), ctx.alloc(8 * (n_words + 1)), ctx.alloc(8 * (n_docs + 1))

    def run():
        ctx.words_normalize_dev(d_text.ptr, text.size, d_docs.ptr, n_docs, table, d_out.ptr, n_out, d_items.ptr, n_words, d_wdocs.ptr)

    warm(run, ctx.synchronize)
    ms = []
    for _ in range(REPS):
        e0 = ctx.event().record()
        run()
        e1 = ctx.event().record()
        e1.synchronize()
        ms.append(e0.elapsed_ms(e1))
    triple_same = bool(np.array_equal(d_out.download(n_out, np.uint8), packed[0]) and np.array_equal(d_items.download(n_words + 1, np.int64), packed[1])
                       and np.array_equal(d_wdocs.download(n_docs + 1, np.int64), packed[2]))
    model_bytes = 2 * text.size + text.size // 8 + n_out + 8 * n_words
    emit(what="(d) normalise launches alone (count, read-back of the totals, emit)", ms=[round(x, 4) for x in ms], median_ms=round(float(np.median(ms)), 4),
         words=int(n_words), normal_form_bytes=int(n_out), model_bytes=int(model_bytes), model_ms_at_8_tb_per_s=round(model_bytes / 8e12 * 1e3, 4),
         gb_per_s_of_the_model=round(model_bytes / float(np.median(ms)) / 1e6, 1), same_triple_as_numpy=triple_same)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)
    if not (same and same_def and triple_same and min(new_s) < min(old_s)):
        raise SystemExit("bench_device_words.py: acceptance failed")


if __name__ == "__main__":
    main()
