"""The word entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a script in a process
of its own by tests/test_gpu_words_guard.py -- a kernel that over-reads or over-writes kills the process).

    python tests/words_guard_cases.py <align>        all cases; prints "WORDS GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: the bytes, the document offsets and the three outputs of every
mhx_words_normalize_dev call are separate exact-size allocations from mhx_debug_guard_alloc -- the text exactly n_out_bytes bytes,
the item offsets exactly n_words + 1 entries.  Input lengths take every residue mod 16 on both sides of a tile (4096 bytes); the
first and the last byte of every corpus are word bytes, so the first and the last granule are read and the last word ends on the
last byte.  The host forms follow (their staging buffers are exact-size allocations too).  Results are checked against the host
path (datasketch_amd.shingle).  tests/words_poison_cases.py runs the same cases on poisoned allocations: the bitmap and the scan
scratch are then full of the poison byte before the kernels write them.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import HyperLogLog, MinHash, _native, shingle  # noqa: E402
from datasketch_amd.hashfunc import sha1_hash64  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect  # noqa: E402

ALPHABET = np.frombuffer(b"aB ,\xc3\xa9", dtype=np.uint8)
TABLE = shingle.word_table()


def corpus(rng, n, n_docs):
    """n bytes over ALPHABET that start and end in a word byte; n_docs documents, some of them empty."""
    buf = ALPHABET[rng.randint(0, ALPHABET.size, size=n)].copy()
    if n:
        buf[0], buf[-1] = ord("a"), ord("B")
    cuts = np.sort(rng.randint(0, n + 1, size=max(n_docs - 1, 0)))
    if cuts.size > 3:
        cuts[1] = cuts[0]  # an empty document in the middle
    doc_offsets = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    return buf, doc_offsets


def dev_call(ctx, buf, doc_offsets, what):
    want = shingle.normalize_words(buf, doc_offsets, TABLE, gpu_mode="disable")
    n_docs, n_words, n_out = doc_offsets.size - 1, want[1].size - 1, want[0].size
    d_bytes = _dev(ctx, buf) if buf.size else None
    d_docs = _dev(ctx, doc_offsets)
    p_bytes = None if d_bytes is None else d_bytes.ptr
    assert ctx.words_normalize_dev(p_bytes, buf.size, d_docs.ptr, n_docs, TABLE) == (0, n_words, n_out), what
    d_text = _alloc(ctx, n_out) if n_out else None
    d_items, d_wdocs = _alloc(ctx, 8 * (n_words + 1)), _alloc(ctx, 8 * (n_docs + 1))
    got = ctx.words_normalize_dev(p_bytes, buf.size, d_docs.ptr, n_docs, TABLE, None if d_text is None else d_text.ptr, n_out, d_items.ptr, n_words,
                                  d_wdocs.ptr)
    assert got == (0, n_words, n_out), what
    ctx.synchronize()
    if n_out:
        _expect(d_text.download(n_out, np.uint8), want[0], what + ": text")
    _expect(d_items.download(n_words + 1, np.int64), want[1], what + ": item offsets")
    _expect(d_wdocs.download(n_docs + 1, np.int64), want[2], what + ": word offsets of the documents")
    _done(what)


def cases(ctx):
    rng = np.random.RandomState(91)
    for base in (0, 4096 - 8):  # every residue mod 16, inside one tile and across the first tile edge
        for r in range(1, 17):
            n = base + r
            buf, doc_offsets = corpus(rng, n, 1 + n // 9)
            dev_call(ctx, buf, doc_offsets, f"dev len={n} (mod 16 = {n % 16}) docs={doc_offsets.size - 1}")
    buf, doc_offsets = corpus(rng, 3 * 4096 + 5, 300)
    dev_call(ctx, buf, doc_offsets, "dev three tiles and five bytes")
    n = 4096 + 3
    dev_call(ctx, np.full(n, ord("a"), dtype=np.uint8), np.arange(n + 1, dtype=np.int64), "dev one-byte documents: twice the input")
    dev_call(ctx, np.full(n, ord("a"), dtype=np.uint8), np.array([0, n], dtype=np.int64), "dev one word longer than a tile")
    dev_call(ctx, np.full(50, ord(" "), dtype=np.uint8), np.array([0, 0, 20, 50, 50], dtype=np.int64), "dev separators only")
    dev_call(ctx, np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.int64), "dev no bytes, three documents")
    # the host forms: bytes, offsets, the normal form, hashes and results are pieces of exact-size scratch slots
    for n, w in ((4096 + 1, 1), (4096 + 6, 2), (2 * 4096 + 11, 3), (777, 5)):
        buf, doc_offsets = corpus(rng, n, 1 + n // 40)
        want = shingle.normalize_words(buf, doc_offsets, TABLE, gpu_mode="disable")
        for g, x, name in zip(ctx.words_normalize(buf, doc_offsets, TABLE), want, ("text", "item offsets", "word offsets")):
            _expect(g, x, f"host form normal form len={n}: {name}")
        _done(f"host form mhx_words_normalize len={n}")
        m = MinHash(num_perm=64, seed=3, gpu_mode="disable")
        want = MinHash.bulk_signatures(documents=(buf, doc_offsets), shingle=w, words=True, num_perm=64, seed=3, gpu_mode="disable")
        for out_dtype in (np.uint64, np.uint32):
            got = ctx.minhash_bulk_words(m.permutations, buf, doc_offsets, w, TABLE, None, 32, out_dtype)
            _expect(got.astype(np.uint64), want, f"host form signatures len={n} w={w} {np.dtype(out_dtype).name}")
            _done(f"host form mhx_minhash_bulk_words_typed len={n} w={w} {np.dtype(out_dtype).name}")
        init = rng.randint(0, 2**32, size=(doc_offsets.size - 1, 64)).astype(np.uint64)
        want64 = np.minimum(init, MinHash.bulk_signatures(documents=(buf, doc_offsets), shingle=w, words=True, num_perm=64, seed=3,
                                                          hashfunc=sha1_hash64, gpu_mode="disable"))
        _expect(ctx.minhash_bulk_words(m.permutations, buf, doc_offsets, w, TABLE, init, 64), want64, f"host form signatures len={n} w={w} init, 64 bits")
        _done(f"host form mhx_minhash_bulk_words_typed len={n} w={w} with init, sha1_hash64")
        for bits, f in ((32, None), (64, sha1_hash64)):
            kw = {} if f is None else {"hashfunc": f}
            want = HyperLogLog.bulk_registers(documents=(buf, doc_offsets), shingle=w, words=True, p=8, hash_bits=bits, gpu_mode="disable", **kw)
            _expect(ctx.hll_bulk_words(buf, doc_offsets, w, 8, TABLE, bits), want.view(np.uint8), f"host form registers len={n} w={w} bits={bits}")
            _done(f"host form mhx_hll_bulk_words len={n} w={w} bits={bits}")
    buf, doc_offsets = np.zeros(0, dtype=np.uint8), np.zeros(3, dtype=np.int64)
    m = MinHash(num_perm=64, seed=3, gpu_mode="disable")
    _expect(ctx.minhash_bulk_words(m.permutations, buf, doc_offsets, 2, TABLE), np.tile(m.hashvalues, (2, 1)), "host form signatures of no bytes")
    _done("host form mhx_minhash_bulk_words_typed no bytes, two documents")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"WORDS GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"WORDS GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
