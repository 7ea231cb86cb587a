#!/usr/bin/env python3
"""Near-duplicate detection from raw text: documents in, clusters out, no tokens built on the host.

    python examples/near_duplicate_text.py [--docs 20000] [--shingle 9] [--words 0] [--gpu-mode detect]

1. ``MinHash.bulk_signatures(documents=..., shingle=k)`` -- one signature row per document over its k-byte shingles.  On the
   device every window is hashed where it lies in the text (``sha1_windows_kernel``): nothing like
   ``for i in range(len(d) - k + 1): m.update(d[i:i+k])`` runs, and no copy of the corpus per shingle byte is made;
2. ``HyperLogLog.bulk_registers(documents=..., shingle=k)`` + ``count_many`` -- the number of distinct shingles per document;
3. ``lsh_bulk.candidate_pairs`` / ``jaccard_pairs`` / ``duplicate_clusters`` -- the chain of examples/near_duplicates.py.

``--words w`` shingles over ``w`` consecutive *words* of the normalised text instead (``words=True``: case folded, punctuation and runs
of white space ignored); the raw text is tokenised and normalised on the device too (``words_kernels.hip``).

With ``--gpu-mode disable`` everything runs on the host paths and gives the same answer.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from datasketch_amd import HyperLogLog, MinHash  # noqa: E402
from datasketch_amd import hyperloglog, lsh_bulk  # noqa: E402


def synthetic_text(n_docs: int, seed: int = 0, vocab_size: int = 20_000):
    """Documents of 60..180 words drawn from a Zipf-distributed vocabulary (words repeat as they do in text), separated by blanks;
    every tenth document is an earlier one with about 5 % of its words replaced."""
    rng = np.random.RandomState(seed)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", dtype=np.uint8)
    vocab = [bytes(letters[rng.randint(0, 26, size=rng.randint(2, 10))]) for _ in range(vocab_size)]
    docs, words_of, truth = [], [], []
    for i in range(n_docs):
        if i % 10 == 9:
            src = int(rng.randint(0, i))
            words = list(words_of[src])
            for pos in rng.randint(0, len(words), max(1, len(words) // 20)):
                words[pos] = vocab[rng.randint(0, vocab_size)]
            truth.append((src, i))
        else:
            ranks = np.minimum(rng.zipf(1.3, size=rng.randint(60, 181)), vocab_size) - 1
            words = [vocab[j] for j in ranks]
        words_of.append(words)
        docs.append(b" ".join(words))
    return docs, truth


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

    docs, truth = synthetic_text(args.docs)
    t0 = time.perf_counter()
    width, how = (args.words, {"words": True}) if args.words else (args.shingle, {})
    sig = MinHash.bulk_signatures(documents=docs, shingle=width, num_perm=args.num_perm, seed=1, gpu_mode=args.gpu_mode, **how)
    t1 = time.perf_counter()
    reg = HyperLogLog.bulk_registers(documents=docs, shingle=width, p=8, gpu_mode=args.gpu_mode, **how)
    distinct = hyperloglog.count_many(reg, gpu_mode=args.gpu_mode)
    t2 = time.perf_counter()
    n_bytes = sum(map(len, docs))
    print(f"{len(docs)} documents, {n_bytes / 1e6:.1f} MB of text, {width}-{'word' if args.words else 'byte'} shingles -> signatures {t1 - t0:.3f} s; "
          f"distinct shingles per document {t2 - t1:.3f} s (median {np.median(distinct):.0f})")
    pairs = lsh_bulk.candidate_pairs(sig, args.bands, args.rows, gpu_mode=args.gpu_mode)
    est = lsh_bulk.jaccard_pairs(sig, pairs, gpu_mode=args.gpu_mode)
    keep = pairs[est >= args.threshold]
    t3 = time.perf_counter()
    found = set(map(tuple, keep.tolist()))
    recall = sum((a, b) in found for a, b in truth) / max(1, len(truth))
    print(f"{len(pairs)} candidate pairs, {len(keep)} with estimated Jaccard >= {args.threshold} in {t3 - t2:.3f} s; "
          f"{recall:.1%} of the {len(truth)} planted near-duplicates found")
    labels = lsh_bulk.duplicate_clusters(sig, args.bands, args.rows, threshold=args.threshold, gpu_mode=args.gpu_mode)
    t4 = time.perf_counter()
    sizes = np.bincount(labels, minlength=len(docs))
    print(f"{int(np.count_nonzero(sizes > 1))} clusters of more than one document in {t4 - t3:.3f} s; "
          f"{int(np.count_nonzero(labels == np.arange(len(docs))))} of {len(docs)} documents kept (one per cluster)")
    return {"signatures": sig, "distinct": distinct, "pairs": pairs, "kept": keep, "recall": recall, "labels": labels}


if __name__ == "__main__":
    main()
