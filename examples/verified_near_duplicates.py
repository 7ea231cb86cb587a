#!/usr/bin/env python3
"""Near-duplicate clusters with the candidate pairs VERIFIED: the exact Jaccard of the shingle sets, not the estimate.

    python examples/verified_near_duplicates.py [--docs 20000] [--shingle 9] [--words 0] [--threshold 0.7] [--gpu-mode detect]

1. ``MinHash.bulk_signatures(documents=..., shingle=k)`` and ``lsh_bulk.candidate_pairs`` -- the chain of
   examples/near_duplicate_text.py: every step after the signatures sees only the sketch;
2. ``overlap.exact_jaccard_pairs(pairs, documents=..., shingle=k)`` -- for every candidate pair the true Jaccard of the two shingle
   sets.  On the device the corpus goes up once, the windows are hashed where they lie, one workgroup per pair builds a hash set of
   the pair in LDS (``overlap_kernels.hip``) and only three counts per pair come back;
3. ``lsh_bulk.connected_components(pairs, n, keep=exact >= threshold)`` -- the clusters of the pairs that really reach the threshold.

It prints how many candidate pairs the verification dropped, and how the clusters differ from ``duplicate_clusters`` with the same
threshold applied to the ESTIMATE: an estimate above the threshold for a pair below it is an edge that may chain two unrelated
groups into one cluster; one below the threshold for a pair above it splits a cluster.

The corpus plants both kinds on purpose: besides light edits (about 5 % of the words replaced) every twentieth document is a
heavier edit, whose true Jaccard lies around the threshold.  With ``--gpu-mode disable`` everything runs on the host paths and gives
the same answer.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datasketch_amd import MinHash  # noqa: E402
from datasketch_amd import lsh_bulk, overlap  # noqa: E402


def synthetic_text(n_docs: int, seed: int = 0, vocab_size: int = 20_000):
    """Documents of 60..180 words from a Zipf-distributed vocabulary.  Every tenth document is an earlier one with about 5 % of its
    words replaced, every twentieth one instead with 8 .. 20 % replaced: pairs on both sides of a threshold of 0.7 over 9-byte
    shingles."""
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    vocab = [bytes(letters[rng.randint(0, 26, size=rng.randint(2, 10))]) for _ in range(vocab_size)]
    docs, words_of, planted = [], [], []
    for i in range(n_docs):
        if i % 10 == 9:
            src = int(rng.randint(0, i))
            words = list(words_of[src])
            share = 0.05 if i % 20 == 9 else rng.uniform(0.08, 0.20)
            for pos in rng.randint(0, len(words), max(1, int(len(words) * share))):
                words[pos] = vocab[rng.randint(0, vocab_size)]
            planted.append((src, i))
        else:
            ranks = np.minimum(rng.zipf(1.3, size=rng.randint(60, 181)), vocab_size) - 1
            words = [vocab[j] for j in ranks]
        words_of.append(words)
        docs.append(b" ".join(words))
    return docs, planted


def verified_clusters(docs, width, how, num_perm, bands, rows, threshold, gpu_mode):
    """(candidate pairs, their exact Jaccard, the labels of the verified clusters, the signatures)"""
    sig = MinHash.bulk_signatures(documents=docs, shingle=width, num_perm=num_perm, seed=1, gpu_mode=gpu_mode, **how)
    pairs = lsh_bulk.candidate_pairs(sig, bands, rows, gpu_mode=gpu_mode)
    exact = overlap.exact_jaccard_pairs(pairs, documents=docs, shingle=width, gpu_mode=gpu_mode, **how)
    labels = lsh_bulk.connected_components(pairs, len(docs), keep=exact >= threshold, gpu_mode=gpu_mode)
    return pairs, exact, labels, sig


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=20_000)
    ap.add_argument("--shingle", type=int, default=9)
    ap.add_argument("--words", type=int, default=0, help="shingle over this many words of the normalised text, not over bytes")
    ap.add_argument("--num-perm", type=int, default=128)
    ap.add_argument("--bands", type=int, default=32)
    ap.add_argument("--rows", type=int, default=4)
    ap.add_argument("--threshold", type=float, default=0.7)
    ap.add_argument("--gpu-mode", default="detect", choices=["detect", "always", "disable"])
    args = ap.parse_args(argv)

    docs, planted = synthetic_text(args.docs)
    width, how = (args.words, {"words": True}) if args.words else (args.shingle, {})
    t0 = time.perf_counter()
    pairs, exact, labels, sig = verified_clusters(docs, width, how, args.num_perm, args.bands, args.rows, args.threshold, args.gpu_mode)
    t1 = time.perf_counter()
    keep = exact >= args.threshold
    print(f"{len(docs)} documents, {sum(map(len, docs)) / 1e6:.1f} MB of text, {width}-{'word' if args.words else 'byte'} shingles: "
          f"{len(pairs)} candidate pairs, {int(keep.sum())} with exact Jaccard >= {args.threshold}, "
          f"{int(len(pairs) - keep.sum())} dropped by the verification ({t1 - t0:.3f} s in all)")
    est = lsh_bulk.jaccard_pairs(sig, pairs, gpu_mode=args.gpu_mode)
    wrongly_kept = int(np.count_nonzero((est >= args.threshold) & ~keep))
    wrongly_dropped = int(np.count_nonzero((est < args.threshold) & keep))
    print(f"the estimate disagrees on {wrongly_kept + wrongly_dropped} pairs: {wrongly_kept} kept below the threshold, "
          f"{wrongly_dropped} dropped above it (largest error {np.abs(est - exact).max() if len(pairs) else 0.0:.3f})")
    estimated = lsh_bulk.duplicate_clusters(sig, args.bands, args.rows, threshold=args.threshold, gpu_mode=args.gpu_mode)
    moved = int(np.count_nonzero(labels != estimated))
    n = len(docs)
    clusters = lambda lab: int(np.count_nonzero(np.bincount(lab, minlength=n) > 1))  # noqa: E731
    print(f"verified: {clusters(labels)} clusters of more than one document, {int(np.count_nonzero(labels == np.arange(n)))} documents kept; "
          f"estimated: {clusters(estimated)} clusters, {int(np.count_nonzero(estimated == np.arange(n)))} kept; "
          f"{moved} documents sit in a different cluster")
    found = set(map(tuple, pairs[keep].tolist()))
    print(f"{sum((a, b) in found for a, b in planted)} of the {len(planted)} planted edits reach the threshold exactly")
    return {"pairs": pairs, "exact": exact, "labels": labels, "estimated_labels": estimated, "dropped": int(len(pairs) - keep.sum()),
            "moved": moved}


if __name__ == "__main__":
    main()
