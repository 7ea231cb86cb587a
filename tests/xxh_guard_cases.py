"""The xxHash entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a script in a
process of its own by tests/test_gpu_xxh_guard.py -- a kernel that over-reads kills the process).

    python tests/xxh_guard_cases.py <align>        all cases; prints "XXH GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used.  The MHX_API_XXH family has host forms only: their staging buffers
are exact-size allocations of mhx_debug_guard_alloc -- the bytes of a corpus are a scratch slot of their own, exactly as long as
the corpus (mhx_api.hip: Windows::stage, and Tokens::stage with the in_slack of 0 that every xxHash entry passes), so the first
window or token starts on the first byte of an allocation and the last one ends on its last byte.  Both kernels, both widths;
window widths 5, 33 and 70 (XXH32: no stripe, two stripes, four; XXH64: no stripe, one, two); byte buffers of every length mod 8;
byte mode and token mode; xxh_tokens_kernel through mhx_hash_tokens and through the three `bytes` chains.  Results are checked
against the Python definition.  tests/xxh_poison_cases.py runs the same cases on poisoned allocations.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import HyperLogLog, MinHash, _native, overlap, shingle  # noqa: E402
from datasketch_amd._native import MHX_HASH_XXH as XXH  # noqa: E402
from datasketch_amd.hashfunc import xxh32_hash32, xxh64_hash64  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _begin, _done, _expect  # noqa: E402

FUNC = {32: xxh32_hash32, 64: xxh64_hash64}


def byte_corpus(rng, width, total_mod8):
    """Documents whose first and last have at least `width` bytes, short and empty ones between; total length = total_mod8 mod 8."""
    lengths = [width + 2, 0, 1, width - 1, width, 3 * width + 1, 0, int(rng.randint(1, 200)), width + int(rng.randint(0, 9))]
    lengths[-1] += (total_mod8 - sum(lengths)) % 8
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8), doc_offsets


def token_corpus(rng, w, total_mod8):
    """Tokens of 0 .. 70 bytes, the first and the last one not empty; documents of 0, fewer than w, w and more tokens; the first
    and the last document have at least w tokens."""
    counts = [w + 1, 0, 1, max(w - 1, 1), w, 3 * w, 0, w + 2]
    n_items = sum(counts)
    lens = rng.randint(0, 71, size=n_items)
    lens[0], lens[1], lens[-2] = 33, 0, 0
    lens[-1] = 1 + (total_mod8 - 1 - int(lens[:-1].sum())) % 8 + 8 * int(rng.randint(0, 5))
    item_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rng.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8), item_offsets, doc_offsets


def windows_call(ctx, buf, item_offsets, doc_offsets, width, bits, what):
    _begin(what)
    want, want_offsets = shingle.hash_windows(buf, doc_offsets, width, item_offsets=item_offsets, hashfunc=FUNC[bits], gpu_mode="disable")
    got, set_offsets = ctx.hash_windows(buf, doc_offsets, width, item_offsets, bits, XXH)
    _expect(set_offsets, want_offsets, what + " (set offsets)")
    _expect(got, want, what)
    _done(what)


def tokens_call(ctx, buf, byte_offsets, bits, what):
    _begin(what)
    raw, at, f = buf.tobytes(), byte_offsets.tolist(), FUNC[bits]
    want = np.array([f(raw[at[i]: at[i + 1]]) for i in range(len(at) - 1)], dtype=np.uint32 if bits == 32 else np.uint64)
    _expect(ctx.hash_tokens(buf, byte_offsets, bits, XXH), want, what)
    _done(what)


def cases(ctx):
    rng = np.random.RandomState(74)
    for width in (5, 33, 70):
        for mod in range(8):
            buf, doc_offsets = byte_corpus(rng, width, mod)
            assert buf.size % 8 == mod and doc_offsets[1] >= width and doc_offsets[-1] - doc_offsets[-2] >= width
            for bits in (32, 64):
                windows_call(ctx, buf, None, doc_offsets, width, bits, f"bytes width={width} len={buf.size} (mod 8 = {mod}) bits={bits}")
    for w in (1, 2):  # token windows of about 35 w bytes
        for mod in range(8):
            buf, item_offsets, doc_offsets = token_corpus(rng, w, mod)
            assert buf.size % 8 == mod
            for bits in (32, 64):
                windows_call(ctx, buf, item_offsets, doc_offsets, w, bits, f"tokens w={w} len={buf.size} (mod 8 = {mod}) bits={bits}")
                if w == 1:
                    tokens_call(ctx, buf, item_offsets, bits, f"mhx_hash_tokens len={buf.size} (mod 8 = {mod}) bits={bits}")
    # one document that is one window; only short documents; empty tokens only
    for width in (5, 33, 70):
        for n in (1, width - 1, width, width + 1):
            buf = rng.randint(0, 256, size=n, dtype=np.uint8)
            windows_call(ctx, buf, None, np.array([0, n], dtype=np.int64), width, 32 if n % 2 else 64, f"one document of {n} bytes, width={width}")
    buf = rng.randint(0, 256, size=7, dtype=np.uint8)
    windows_call(ctx, buf, None, np.array([0, 3, 3, 5, 7, 7], dtype=np.int64), 70, 64, "short documents only")
    windows_call(ctx, buf[:0], np.zeros(4, dtype=np.int64), np.array([0, 1, 3], dtype=np.int64), 2, 32, "empty tokens only")
    tokens_call(ctx, buf[:0], np.zeros(4, dtype=np.int64), 64, "mhx_hash_tokens, empty tokens only")
    # the chains: bytes, offsets, hashes and results are pieces of exact-size scratch slots
    for width, mod, bits in ((5, 1, 32), (33, 6, 64), (70, 3, 32)):
        buf, doc_offsets = byte_corpus(rng, width, mod)
        f = FUNC[bits]
        corpus = dict(documents=(buf, doc_offsets), shingle=width)
        what = f"chains bytes width={width} bits={bits}"
        _begin(what)
        m = MinHash(num_perm=64, seed=3, gpu_mode="disable")
        want = MinHash.bulk_signatures(num_perm=64, seed=3, hashfunc=f, gpu_mode="disable", **corpus)
        _expect(ctx.minhash_bulk_windows(m.permutations, buf, doc_offsets, width, None, None, bits, np.uint64, XXH), want, what + " signatures")
        want = HyperLogLog.bulk_registers(p=8, hashfunc=f, hash_bits=bits, gpu_mode="disable", **corpus).view(np.uint8)
        _expect(ctx.hll_bulk_windows(buf, doc_offsets, width, 8, None, bits, None, XXH), want, what + " registers")
        pairs = np.array([[0, 5], [4, 8], [1, 2], [5, 5]], dtype=np.int64)
        want = overlap.text_overlap_counts(pairs, hashfunc=f, gpu_mode="disable", **corpus)
        _expect(ctx.overlap_pairs_windows(pairs, buf, doc_offsets, width, None, bits, XXH), want, what + " overlap counts")
        _done(what)
    # the same three sinks over packed tokens: xxh_tokens_kernel on a byte slot that ends with the last token
    for mod, bits in ((1, 32), (4, 64), (7, 32)):
        buf, byte_offsets, set_offsets = token_corpus(rng, 2, mod)
        f = FUNC[bits]
        corpus = dict(packed=(buf, byte_offsets, set_offsets))
        what = f"chains tokens len={buf.size} (mod 8 = {mod}) bits={bits}"
        _begin(what)
        m = MinHash(num_perm=64, seed=3, gpu_mode="disable")
        want = MinHash.bulk_signatures(num_perm=64, seed=3, hashfunc=f, gpu_mode="disable", **corpus)
        _expect(ctx.minhash_bulk_bytes(m.permutations, buf, byte_offsets, set_offsets, None, bits, np.uint64, XXH), want, what + " signatures")
        want = HyperLogLog.bulk_registers(p=8, hashfunc=f, hash_bits=bits, gpu_mode="disable", **corpus).view(np.uint8)
        _expect(ctx.hll_bulk_bytes(buf, byte_offsets, set_offsets, 8, bits, None, XXH), want, what + " registers")
        pairs = np.array([[0, 5], [4, 7], [1, 2], [5, 5]], dtype=np.int64)
        want = overlap.text_overlap_counts(pairs, hashfunc=f, gpu_mode="disable", **corpus)
        _expect(ctx.overlap_pairs_bytes(pairs, buf, byte_offsets, set_offsets, bits, XXH), want, what + " overlap counts")
        _done(what)


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"XXH GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"XXH GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
