#!/usr/bin/env python3
"""tools/text_entries_once.py -- each of the six text-to-sketch entries called once on a tiny corpus, for a kernel trace:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/text_entries_once.py

Three sources (packed byte tokens, windows over bytes, words of raw text) into two sinks (MinHash signatures, HyperLogLog
registers).  The kernel names and dispatch counts of two builds of the library compare; PYTHONPATH picks the package."""
import numpy as np

from datasketch_amd import MinHash, _native, shingle


def main():
    if not _native.gpu_available():
        raise SystemExit("text_entries_once.py needs an MI355X")
    ctx = _native.context()
    docs = [b"The quick brown fox, the lazy dog.", b"", b"ab", b"Pack my box with five dozen liquor jugs " * 3]
    buf, doc_offsets = shingle.join_documents(docs)
    sets = [d.split() for d in docs]
    packed = _native.Context.pack_sets(sets)
    perms = MinHash(num_perm=64, seed=1).permutations
    table = shingle.word_table()
    out = [
        ctx.minhash_bulk_bytes(perms, *packed),
        ctx.hll_bulk_bytes(*packed, 8),
        ctx.minhash_bulk_windows(perms, buf, doc_offsets, 5),
        ctx.hll_bulk_windows(buf, doc_offsets, 5, 8),
        ctx.minhash_bulk_words(perms, buf, doc_offsets, 3, table),
        ctx.hll_bulk_words(buf, doc_offsets, 3, 8, table),
    ]
    print("six entries of", _native.LIB_PATH, [o.shape for o in out], "checksums", [int(o.astype(np.uint64).sum()) for o in out])


if __name__ == "__main__":
    main()
