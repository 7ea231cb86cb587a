"""The overlap entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run as a script in a
process of its own by tests/test_gpu_overlap_guard.py -- a kernel that over-reads kills the process).

    python tests/overlap_guard_cases.py <align>        all cases; prints "OVERLAP GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: hashes, set offsets, pairs, counts and the invalid counter of every
mhx_overlap_pairs_dev call are separate exact-size allocations from mhx_debug_guard_alloc, the counts pre-filled with a pattern;
the staging buffers of the host forms -- mhx_overlap_pairs and the three text entries -- and the pair lists and tables in the
context's scratch are exact-size allocations too.  Results are checked against datasketch_amd.overlap.overlap_counts_host.  Both key
widths; pairs of every LDS bin, at the class boundary and beyond it; with "overlap.bins" 1 and 2 and with launchers that see one
compute unit, so that every kernel walks its list in several trips.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, overlap, shingle  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect  # noqa: E402
from tests.weighted_dispatch import MI355X_LDS_PER_BLOCK  # noqa: E402


def csr(sets, dtype):
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=offsets[1:])
    return np.concatenate([np.asarray(s, dtype=dtype) for s in sets]).astype(dtype), offsets


def dev_call(ctx, hashes, offsets, pairs, what, max_set_items=None, want_invalid=0):
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_sets = offsets.size - 1
    if max_set_items is None:
        max_set_items = int(np.diff(offsets).max())
    d_hv, d_offsets, d_pairs = _dev(ctx, hashes), _dev(ctx, offsets), _dev(ctx, pairs)
    d_counts, d_bad = _alloc(ctx, 12 * pairs.shape[0]), _alloc(ctx, 8, fill=0)
    ctx.overlap_pairs_dev(d_hv.ptr if hashes.size else None, _native.MHX_U32 if hashes.dtype == np.uint32 else _native.MHX_U64, d_offsets.ptr, n_sets,
                          max_set_items, d_pairs.ptr, pairs.shape[0], d_counts.ptr, d_bad.ptr)
    ctx.synchronize()
    sizes = np.diff(offsets)
    inside = ((pairs >= 0) & (pairs < n_sets)).all(axis=1)
    inside[inside] &= (sizes[pairs[inside]] <= max_set_items).all(axis=1)
    want = np.full((pairs.shape[0], 3), -1, dtype=np.int32)
    want[inside] = overlap.overlap_counts_host(hashes, offsets, pairs[inside])
    _expect(d_counts.download((pairs.shape[0], 3), np.int32), want, what + " counts")
    _expect(d_bad.download((1,), np.int64), np.array([want_invalid]), what + " invalid")
    _done(what)


def values(rng, count, dtype):
    return rng.randint(0, np.iinfo(dtype).max, size=count, dtype=np.uint64 if dtype == np.uint64 else np.int64).astype(dtype)


def cases(ctx):
    rng = np.random.RandomState(53)
    for dtype in (np.uint32, np.uint64):
        name = np.dtype(dtype).name
        limit = _native.overlap_limits(np.dtype(dtype).itemsize * 8, MI355X_LDS_PER_BLOCK)
        top = np.iinfo(dtype).max
        # one set, one item, one pair; then sets of every small size, the empty value of the table among the items
        dev_call(ctx, *csr([[5]], dtype), [[0, 0]], f"{name} one item")
        dev_call(ctx, *csr([[top], []], dtype), [[0, 1], [1, 1], [0, 0]], f"{name} the empty value alone")
        small = [values(rng, n, dtype)[rng.randint(0, max(n, 1), n + n // 2)] if n else [] for n in (0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 256, 257)]
        small += [np.full(300, 9, dtype=dtype), np.array([0, top, 1, top], dtype=dtype), small[7]]
        hashes, offsets = csr(small, dtype)
        every = np.stack(np.meshgrid(np.arange(len(small)), np.arange(len(small)), indexing="ij"), axis=-1).reshape(-1, 2)
        dev_call(ctx, hashes, offsets, every, f"{name} small sets, every ordered pair")
        ctx.set_option("overlap.bins", 2)
        dev_call(ctx, hashes, offsets, every, f"{name} small sets, every ordered pair, a workgroup per pair")
        ctx.set_option("overlap.bins", 0)
        dev_call(ctx, hashes, offsets, every[:1], f"{name} small sets, one pair")
        # every LDS bin, the class boundary and the first pairs in scratch, in one call
        pool = values(rng, 2 * limit, dtype)
        sets = [pool[:700], pool[300:1100], pool[:1600], pool[1000:2500], pool[: limit // 2], pool[limit // 2: limit], pool[limit // 2: limit + 1],
                pool[: limit // 2 - 1], pool[:1], pool[1:limit], pool[1: limit + 1], pool[: limit + limit // 2], pool[limit // 2:]]
        hashes, offsets = csr(sets, dtype)
        pairs = np.array([[0, 1], [2, 3], [4, 5], [4, 6], [7, 5], [8, 9], [8, 10], [11, 12], [12, 12], [1, 0], [9, 8], [0, 12]], dtype=np.int64)
        totals = np.diff(offsets)[pairs].sum(axis=1)
        assert {limit - 1, limit, limit + 1, 3 * limit} <= set(totals.tolist())
        for option, v in (("overlap.bins", 0), ("overlap.bins", 1), ("overlap.bins", 2), ("debug.cus", 1)):
            ctx.set_option(option, v)
            dev_call(ctx, hashes, offsets, pairs, f"{name} bins and classes, {option}={v}")
            dev_call(ctx, hashes, offsets, np.repeat(pairs, 3, axis=0), f"{name} bins and classes x 3, {option}={v}")
            ctx.set_option(option, 0)
        # bad pairs: their rows are -1, the counter has their number; a bound below the largest set
        bad = np.array([[0, 1], [-1, 1], [0, len(sets)], [2, 3], [11, 0]], dtype=np.int64)
        dev_call(ctx, hashes, offsets, bad, f"{name} bad pairs", max_set_items=int(offsets[12] - offsets[11]) - 1, want_invalid=3)
        # the host form
        for these in (pairs, pairs[:1], every[:0]):
            _expect(overlap.overlap_counts(hashes, offsets, these, gpu_mode="always"), overlap.overlap_counts_host(hashes, offsets, these),
                    f"{name} host form, {len(these)} pairs")
            _done(f"{name} host form, {len(these)} pairs")
    # the text entries: corpora whose last window ends on the last byte of the buffer
    docs = [b"the quick brown fox", b"", b"the quick brown dog", b"ab", b"zzzzzzzzzzzzzzzz", b"the quick brown fox"]
    tokens = [[w + b" " for w in d.split(b" ") if w] for d in docs]
    flat, set_offsets = shingle.flatten(tokens)
    byte_offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in flat], out=byte_offsets[1:])
    packed = (np.frombuffer(b"".join(flat), dtype=np.uint8), byte_offsets, set_offsets)
    every = np.stack(np.meshgrid(np.arange(len(docs)), np.arange(len(docs)), indexing="ij"), axis=-1).reshape(-1, 2)
    for bits in (32, 64):
        for what, kwargs in (("bytes k=5", dict(documents=docs, shingle=5)), ("tokens", dict(packed=packed)), ("tokens w=2", dict(packed=packed, shingle=2)),
                             ("words w=2", dict(documents=docs, shingle=2, words=True)), ("bytes k=1", dict(documents=docs[:3], shingle=1))):
            these = every[(every < 3).all(axis=1)] if what == "bytes k=1" else every
            _expect(overlap.text_overlap_counts(these, bits=bits, gpu_mode="always", **kwargs),
                    overlap.text_overlap_counts(these, bits=bits, gpu_mode="disable", **kwargs), f"text {what} bits={bits}")
            _done(f"text {what} bits={bits}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"OVERLAP GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"OVERLAP GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
