"""The shingle entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a script in a
process of its own by tests/test_gpu_shingles_guard.py -- a kernel that over-reads kills the process).

    python tests/shingle_guard_cases.py <align>        all cases; prints "SHINGLE GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: the bytes, the item, document and set offsets and the hashes of every
mhx_sha1_windows_dev call are separate exact-size allocations from mhx_debug_guard_alloc.  The first window starts on the first
byte of the byte buffer and the last window ends on its last byte; buffer lengths are 0, 1, 2 and 3 mod 4; widths 5, 56 and 120 are
the one, two and three block paths; both modes.  The host forms follow (their staging buffers are exact-size allocations too).
Results are checked against the host path (hashlib over datasketch_amd.shingle).  tests/shingle_poison_cases.py runs the same
cases on poisoned allocations.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import HyperLogLog, MinHash, _native, shingle  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64  # noqa: E402
from datasketch_amd.hashfunc import sha1_hash64  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect  # noqa: E402


def dev_call(ctx, buf, item_offsets, doc_offsets, width, bits, what):
    want, set_offsets = shingle.sha1_windows(buf, doc_offsets, width, item_offsets=item_offsets, bits=bits, gpu_mode="disable")
    assert np.array_equal(set_offsets, _native.window_offsets(doc_offsets, width))
    n_docs, n_windows = doc_offsets.size - 1, int(set_offsets[-1])
    d_bytes = _dev(ctx, buf) if buf.size else None
    d_items = None if item_offsets is None else _dev(ctx, item_offsets)
    d_docs, d_sets = _dev(ctx, doc_offsets), _dev(ctx, set_offsets)
    d_out = _alloc(ctx, max(want.nbytes, 1))
    ctx.sha1_windows_dev(None if d_bytes is None else d_bytes.ptr, None if d_items is None else d_items.ptr, d_docs.ptr, d_sets.ptr, n_docs,
                         n_windows, width, MHX_U32 if bits == 32 else MHX_U64, d_out.ptr)
    ctx.synchronize()
    _expect(d_out.download(want.shape, want.dtype), want, what)
    _done(what)


def byte_corpus(rng, width, total_mod4):
    """Documents whose first and last have at least `width` bytes, short and empty ones between; total length = total_mod4 mod 4."""
    lengths = [width + 2, 0, 1, width - 1, width, 3 * width + 1, 0, int(rng.randint(1, 200)), width + int(rng.randint(0, 9))]
    lengths[-1] += (total_mod4 - sum(lengths)) % 4
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8), doc_offsets


def token_corpus(rng, w, total_mod4):
    """Tokens of 0 .. 70 bytes, the last one not empty; documents of 0, fewer than w, w and more tokens; the first and the last
    document have at least w tokens."""
    counts = [w + 1, 0, 1, max(w - 1, 1), w, 3 * w, 0, w + 2]
    n_items = sum(counts)
    lens = rng.randint(0, 71, size=n_items)
    lens[1], lens[-2] = 0, 0
    lens[-1] = 1 + (total_mod4 - 1 - int(lens[:-1].sum())) % 4 + 4 * int(rng.randint(0, 5))
    item_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rng.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8), item_offsets, doc_offsets


def cases(ctx):
    rng = np.random.RandomState(73)
    for width in (5, 56, 120):
        for mod in (1, 2, 3, 0):
            buf, doc_offsets = byte_corpus(rng, width, mod)
            assert buf.size % 4 == mod
            for bits in (32, 64):
                dev_call(ctx, buf, None, doc_offsets, width, bits, f"bytes width={width} len={buf.size} (mod 4 = {mod}) bits={bits}")
    for w in (1, 2, 5):  # token windows of about 35 w bytes: one, two and more blocks
        for mod in (1, 2, 3, 0):
            buf, item_offsets, doc_offsets = token_corpus(rng, w, mod)
            assert buf.size % 4 == mod
            for bits in (32, 64):
                dev_call(ctx, buf, item_offsets, doc_offsets, w, bits, f"tokens w={w} len={buf.size} (mod 4 = {mod}) bits={bits}")
    # one document that is one window; only short documents; an empty corpus of empty documents; empty tokens only
    for width in (5, 56, 120):
        for n in (1, width - 1, width, width + 1):
            buf = rng.randint(0, 256, size=n, dtype=np.uint8)
            dev_call(ctx, buf, None, np.array([0, n], dtype=np.int64), width, 32, f"one document of {n} bytes, width={width}")
    buf = rng.randint(0, 256, size=7, dtype=np.uint8)
    dev_call(ctx, buf, None, np.array([0, 3, 3, 5, 7, 7], dtype=np.int64), 120, 64, "short documents only")
    dev_call(ctx, buf[:0], np.zeros(4, dtype=np.int64), np.array([0, 1, 3], dtype=np.int64), 2, 32, "empty tokens only")
    # the host forms: bytes, offsets, hashes and results are pieces of exact-size scratch slots
    for width, mod in ((5, 1), (56, 2), (120, 3)):
        buf, doc_offsets = byte_corpus(rng, width, mod)
        for bits in (32, 64):
            want, set_offsets = shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="disable")
            got, got_offsets = ctx.sha1_windows(buf, doc_offsets, width, None, bits)
            _expect(got, want, f"host form hashes width={width} bits={bits}")
            _expect(got_offsets, set_offsets, f"host form set offsets width={width}")
            _done(f"host form mhx_sha1_windows bytes width={width} bits={bits}")
        m = MinHash(num_perm=64, seed=3, gpu_mode="disable")
        want = MinHash.bulk_signatures(documents=(buf, doc_offsets), shingle=width, num_perm=64, seed=3, gpu_mode="disable")
        for out_dtype in (np.uint64, np.uint32):
            got = ctx.minhash_bulk_windows(m.permutations, buf, doc_offsets, width, None, None, 32, out_dtype)
            _expect(got.astype(np.uint64), want, f"host form signatures width={width} {np.dtype(out_dtype).name}")
            _done(f"host form mhx_minhash_bulk_windows_typed bytes width={width} {np.dtype(out_dtype).name}")
        want = HyperLogLog.bulk_registers(documents=(buf, doc_offsets), shingle=width, p=8, gpu_mode="disable").view(np.uint8)
        _expect(ctx.hll_bulk_windows(buf, doc_offsets, width, 8), want, f"host form registers width={width}")
        _done(f"host form mhx_hll_bulk_windows bytes width={width}")
    for w, mod in ((2, 1), (5, 3)):
        buf, item_offsets, doc_offsets = token_corpus(rng, w, mod)
        packed = (buf, item_offsets, doc_offsets)
        want, _ = shingle.sha1_windows(buf, doc_offsets, w, item_offsets=item_offsets, bits=64, gpu_mode="disable")
        _expect(ctx.sha1_windows(buf, doc_offsets, w, item_offsets, 64)[0], want, f"host form hashes tokens w={w}")
        _done(f"host form mhx_sha1_windows tokens w={w}")
        m = MinHash(num_perm=128, seed=4, gpu_mode="disable")
        init = rng.randint(0, 2**32, size=(doc_offsets.size - 1, 128)).astype(np.uint64)
        want = np.minimum(init, MinHash.bulk_signatures(packed=packed, shingle=w, num_perm=128, seed=4, gpu_mode="disable"))
        _expect(ctx.minhash_bulk_windows(m.permutations, buf, doc_offsets, w, item_offsets, init, 32), want, f"host form signatures tokens w={w}")
        _done(f"host form mhx_minhash_bulk_windows_typed tokens w={w} with init")
        want = HyperLogLog.bulk_registers(packed=packed, shingle=w, p=8, hashfunc=sha1_hash64, hash_bits=64, gpu_mode="disable").view(np.uint8)
        _expect(ctx.hll_bulk_windows(buf, doc_offsets, w, 8, item_offsets, 64), want, f"host form registers tokens w={w}")
        _done(f"host form mhx_hll_bulk_windows tokens w={w}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"SHINGLE GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"SHINGLE GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
