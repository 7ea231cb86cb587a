#!/usr/bin/env python3
"""tools/bench_device_overlaps.py -- exact overlap counts of candidate pairs (overlap_kernels.hip), each figure next to what it is
measured against.

Corpus: seeded, synthetic, nothing downloaded -- words of 2 .. 9 letters drawn from a Zipf-distributed list of 50 000 and separated
by blanks; documents come in groups of eight, a base document and seven copies with about 5 % of their words replaced, so that
candidate_pairs (32 bands x 4 rows over 128 permutations) has pairs to report.  10^6 pairs are drawn from candidate_pairs, with
replacement (so a pair list of any length gives the same number of pairs; the line says how many different ones there were).

  run 1   200 000 documents of about 1 KiB, 9-byte shingles: about 2 000 items per pair
  run 2   the same documents, shingles of 5 words of the normalised text (words=True)
  run 3   40 000 documents of about 6 KiB, 9-byte shingles: more items per pair than an LDS table takes, the global class

Per run, bits = 64:
  * seconds for overlap.text_overlap_counts, host arrays in and counts out (wall clock, three runs, all printed);
  * the pair kernels alone: mhx_overlap_pairs_dev on resident hashes (the classify pass and the launch of every class), timed with
    the context's events behind tools/_warm.py's clock warm-up, 7 runs, all printed -- with the LDS pairs binned by table size and
    one wave per pair in the smallest bin ("overlap.bins" 0, the default), as one launch sized for the largest table of the call
    ("overlap.bins" 1), and binned with a workgroup per pair in every bin ("overlap.bins" 2);
  * items/s and the fraction of 8 TB/s under the traffic model (|A| + |B|) x 8 bytes per pair.  The model counts every pair's two
    sets as read from memory once; it ignores that a document named by many pairs is re-read (mostly from L2) and that the table
    is cleared and probed, so it is a yardstick for the rate, not a roofline;
  * the split of the pairs between the classes;
  * baseline 1, the best path there was: shingle.sha1_windows on the device, the hashes down to the host, then np.unique /
    np.intersect1d per pair -- on a stated subsample of the pairs, scaled to 10^6 by pairs; the hashing is counted once, unscaled;
  * baseline 2: Python sets of slices of the text, per pair -- on a smaller stated subsample, scaled likewise;
  * the counts of the subsamples agree with the device's.

`python tools/bench_device_overlaps.py [run1] [run2] [run3] [--out profiles/overlaps_bench.txt]` (no run named: all three).
SCALE (env, float, default 1) scales the document and pair counts for a dry run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools._warm import warm  # noqa: E402

SCALE = float(os.environ.get("SCALE", "1"))
REPS = 7
LINES = []
HBM_BYTES_PER_S = 8e12


def n_of(x):
    return max(64, int(x * SCALE))


def emit(**rec):
    LINES.append(json.dumps(rec))
    print(LINES[-1], flush=True)


def corpus(n_docs, words_lo, words_hi, seed=0, vocab_size=50_000, group=8, replaced=0.05):
    """(uint8 text, int64 doc_offsets): groups of `group` documents, the first drawn and the others copies of it with `replaced` of
    their words redrawn."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(2, 10, size=vocab_size)
    starts = np.concatenate([[0], np.cumsum(lens + 1)])
    vocab = rng.randint(97, 123, size=int(starts[-1]), dtype=np.uint8)
    vocab[starts[1:] - 1] = 32
    parts, doc_bytes = [], []
    for s in range(0, n_docs, group):
        n_words = int(rng.randint(words_lo, words_hi))
        base = np.minimum(rng.zipf(1.2, size=n_words), vocab_size) - 1
        for c in range(min(group, n_docs - s)):
            ranks = base
            if c:
                ranks = base.copy()
                at = rng.randint(0, n_words, max(1, int(n_words * replaced)))
                ranks[at] = np.minimum(rng.zipf(1.2, size=at.size), vocab_size) - 1
            parts.append(ranks)
    words_per_doc = np.fromiter(map(len, parts), dtype=np.int64, count=len(parts))
    ranks = np.concatenate(parts)
    wl = lens[ranks] + 1
    out_start = np.concatenate([[0], np.cumsum(wl)])
    text = np.empty(int(out_start[-1]), dtype=np.uint8)
    for s in range(0, ranks.size, 1 << 22):  # in pieces: the gather index is 8 bytes per byte of text
        e = min(ranks.size, s + (1 << 22))
        text[out_start[s]: out_start[e]] = vocab[np.repeat(starts[ranks[s:e]] - out_start[s:e], wl[s:e]) + np.arange(int(out_start[s]), int(out_start[e]))]
    doc_words = np.concatenate([[0], np.cumsum(words_per_doc)])
    return text, out_start[doc_words].astype(np.int64)


def one_run(ctx, name, text, doc_offsets, width, words, n_pairs):
    from datasketch_amd import MinHash, _native, lsh_bulk, overlap, shingle

    how = {"words": True} if words else {}
    docs = (text, doc_offsets)
    n_docs = doc_offsets.size - 1
    t0 = time.perf_counter()
    sig = MinHash.bulk_signatures(documents=docs, shingle=width, num_perm=128, seed=1, out_dtype=np.uint32, gpu_mode="always", **how)
    candidates = lsh_bulk.candidate_pairs(sig, 32, 4, gpu_mode="always")
    del sig
    rng = np.random.RandomState(1)
    pairs = candidates[rng.randint(0, len(candidates), n_pairs)]
    emit(what=name + ": pairs", documents=n_docs, text_bytes=int(text.size), shingle=f"{width} {'words' if words else 'bytes'}",
         candidate_pairs=int(len(candidates)), pairs_drawn_with_replacement=int(n_pairs), different_pairs_drawn=int(len(np.unique(pairs, axis=0))),
         seconds_for_signatures_and_candidates=round(time.perf_counter() - t0, 3))

    # (1) host arrays in, counts out
    overlap.text_overlap_counts(pairs[:64], documents=docs, shingle=width, bits=64, gpu_mode="always", **how)  # code objects, scratch
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        counts = overlap.text_overlap_counts(pairs, documents=docs, shingle=width, bits=64, gpu_mode="always", **how)
        wall.append(time.perf_counter() - t0)

    # the hashes, for the kernels alone and for baseline 1 (this IS baseline 1's device step)
    t0 = time.perf_counter()
    if words:
        norm, item_offsets, word_docs = shingle.normalize_words(text, doc_offsets, gpu_mode="always")
        hashes, set_offsets = shingle.sha1_windows(norm, word_docs, width, item_offsets=item_offsets, bits=64, gpu_mode="always")
    else:
        hashes, set_offsets = shingle.sha1_windows(text, doc_offsets, width, bits=64, gpu_mode="always")
    hash_s = time.perf_counter() - t0
    sizes = np.diff(set_offsets)
    items = sizes[pairs].sum(axis=1)
    limit = _native.overlap_limits(64, 160 << 10)
    slots = np.maximum(64, 2 ** np.ceil(np.log2(np.maximum(2 * items, 1))).astype(np.int64))
    split = {"empty": int((items == 0).sum()), "lds_up_to_1024_slots": int(((items > 0) & (slots <= 1024)).sum()),
             "lds_up_to_4096_slots": int(((slots > 1024) & (slots <= 4096)).sum()), "lds_larger": int(((slots > 4096) & (items <= limit)).sum()),
             "global": int((items > limit).sum())}
    emit(what=name + ": (1) text_overlap_counts, host arrays in and counts out", pairs=int(n_pairs), seconds=[round(x, 3) for x in wall],
         hashes=int(hashes.size), items_per_pair_mean=round(float(items.mean()), 1), items_per_pair_max=int(items.max()), lds_max_items=limit,
         class_split=split, jaccard_at_least_0_7=int((overlap.jaccard_of(counts) >= 0.7).sum()))

    # (2) the pair kernels alone
    d_hv, d_sets, d_pairs = ctx.to_device(hashes), ctx.to_device(set_offsets), ctx.to_device(pairs)
    d_counts = ctx.alloc(12 * n_pairs)
    most = int(sizes.max())
    model_bytes = float(items.sum()) * 8

    def run():
        ctx.overlap_pairs_dev(d_hv.ptr, _native.MHX_U64, d_sets.ptr, n_docs, most, d_pairs.ptr, n_pairs, d_counts.ptr, None)

    for bins, label in ((0, "binned by table size, one wave per pair in the bin of up to 1024 slots (default)"),
                        (1, "one launch sized for the largest table"), (2, "binned, a workgroup per pair in every bin")):
        ctx.set_option("overlap.bins", bins)
        warm(run, ctx.synchronize)
        ms = []
        for _ in range(REPS):
            e0 = ctx.event().record()
            run()
            e1 = ctx.event().record()
            e1.synchronize()
            ms.append(e0.elapsed_ms(e1))
        med = float(np.median(ms))
        same = bool(np.array_equal(d_counts.download((n_pairs, 3), np.int32), counts))
        emit(what=name + ": (2) mhx_overlap_pairs_dev alone", lds_pairs=label, ms=[round(x, 3) for x in ms], median_ms=round(med, 3),
             pairs_per_s=round(n_pairs / med * 1e3), items_per_s=round(float(items.sum()) / med * 1e3), model_bytes=int(model_bytes),
             model_tb_per_s=round(model_bytes / med * 1e3 / 1e12, 4), fraction_of_8_tb_per_s=round(model_bytes / med * 1e3 / HBM_BYTES_PER_S, 4),
             same_counts_as_the_text_entry=same)
    ctx.set_option("overlap.bins", 0)
    for buf in (d_hv, d_sets, d_pairs, d_counts):
        buf.free()

    # baseline 1: hashes on the host, np.unique / np.intersect1d per pair
    n1 = min(n_pairs, n_of(20_000))
    t0 = time.perf_counter()
    got1 = np.empty((n1, 3), dtype=np.int32)
    for p in range(n1):
        i, j = pairs[p]
        a, b = np.unique(hashes[set_offsets[i]: set_offsets[i + 1]]), np.unique(hashes[set_offsets[j]: set_offsets[j + 1]])
        got1[p] = (np.intersect1d(a, b, assume_unique=True).size, a.size, b.size)
    numpy_s = time.perf_counter() - t0
    # baseline 2: Python sets of slices (byte shingles) or of word shingles
    n2 = min(n_pairs, n_of(2_000))
    raw = text.tobytes()
    t0 = time.perf_counter()
    got2 = np.empty((n2, 3), dtype=np.int32)
    for p in range(n2):
        sets = []
        for d in pairs[p]:
            doc = raw[int(doc_offsets[d]): int(doc_offsets[d + 1])]
            sets.append(set(shingle.word_shingles(doc, width)) if words else {doc[t: t + width] for t in range(max(1, len(doc) - width + 1))} if doc else set())
        got2[p] = (len(sets[0] & sets[1]), len(sets[0]), len(sets[1]))
    python_s = time.perf_counter() - t0
    emit(what=name + ": baselines, scaled to the pairs of (1) by pairs", device_seconds_best=round(min(wall), 3),
         numpy_pairs=n1, numpy_seconds=round(numpy_s, 3), sha1_windows_to_host_seconds=round(hash_s, 3),
         numpy_scaled_seconds=round(hash_s + numpy_s * n_pairs / n1, 1), python_sets_pairs=n2, python_sets_seconds=round(python_s, 3),
         python_sets_scaled_seconds=round(python_s * n_pairs / n2, 1), speedup_over_numpy=round((hash_s + numpy_s * n_pairs / n1) / min(wall), 1),
         speedup_over_python_sets=round(python_s * n_pairs / n2 / min(wall), 1),
         same_counts=bool(np.array_equal(got1, counts[:n1]) and np.array_equal(got2, counts[:n2])))


def main():
    from datasketch_amd import _native

    if not _native.gpu_available():
        raise SystemExit("bench_device_overlaps.py needs an MI355X")
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "overlaps_bench.txt")
    ctx = _native.context()
    info = ctx.info()
    runs = [a for a in sys.argv[1:] if a in ("run1", "run2", "run3")] or ["run1", "run2", "run3"]
    emit(what="device", library=os.path.basename(_native.LIB_PATH), device=info["name"], cus=info["compute_units"], scale=SCALE,
         wave_per_pair_form="the default for pairs of up to 512 items; overlap.bins = 2 is the workgroup form")
    n_pairs = n_of(1_000_000)
    if "run1" in runs or "run2" in runs:
        t0 = time.perf_counter()
        text, doc_offsets = corpus(n_of(200_000), 120, 196)
        emit(what="corpus of runs 1 and 2", documents=int(doc_offsets.size - 1), text_bytes=int(text.size), seconds_to_draw=round(time.perf_counter() - t0, 2))
        if "run1" in runs:
            one_run(ctx, "run 1", text, doc_offsets, 9, False, n_pairs)
        if "run2" in runs:
            one_run(ctx, "run 2", text, doc_offsets, 5, True, n_pairs)
    if "run3" in runs:
        t0 = time.perf_counter()
        text, doc_offsets = corpus(n_of(40_000), 850, 1000, seed=2)
        emit(what="corpus of run 3", documents=int(doc_offsets.size - 1), text_bytes=int(text.size), seconds_to_draw=round(time.perf_counter() - t0, 2))
        one_run(ctx, "run 3", text, doc_offsets, 9, False, n_pairs)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
