"""The forest and ensemble device entry points of include/mhx.h, and two more shapes of the plain bulk query, on buffers that abut
an unmapped page (test infrastructure, run as a script in a process of its own by tests/test_gpu_forest_ensemble_guard.py -- a
kernel that over-reads kills the process).

    python tests/forest_ensemble_guard_cases.py <align>     all cases; prints "FOREST GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: the matrix, the order, the probes, the level buffers, the choice
table and every output of a call are separate exact-size allocations from mhx_debug_guard_alloc, outputs pre-filled with a
pattern, and the results are checked against np.lexsort and the numpy back ends.  mhx_lsh_forest_build_dev_typed and
mhx_lsh_forest_query_dev_typed on rows of exactly l * tree_words words -- the last key of the last row ends the matrix --,
with an all-zero and an all-ones probe whose insertion points are position 0 and position n of every tree;
mhx_lsh_ensemble_query_dev with an empty partition, one of a single row and one of 40 identical rows (every band of its block is
one run up to the block's end); mhx_lsh_query_dev over 40 identical rows and over one row.
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, lsh_bulk  # noqa: E402
from datasketch_amd import lshforest as F  # noqa: E402
from datasketch_amd._native import MHX_U32, MHX_U64, check  # noqa: E402
from datasketch_amd.lsh import _HostBands  # noqa: E402
from datasketch_amd.lshensemble import _HostEnsemble  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _begin, _dev, _done, _expect  # noqa: E402
from tests.poison_cases import _clustered, _offsets_to_pairs  # noqa: E402
from tests.test_gpu_lshforest import _corpus  # noqa: E402
from tests.test_lshforest_host import lexsort_order  # noqa: E402

_i64 = ctypes.c_int64
PATTERN = 0xA5
PATTERN32 = np.uint32(0xA5A5A5A5)


def _forest_probes(rng, sig, alpha, bases):
    """65 probes: an all-zero and an all-ones row (insertion point 0 and n in every tree: no left, no right neighbour), rows of
    the index, rows of the index redrawn from a random column on, and rows drawn like the index."""
    n, width = sig.shape
    probes, _ = _corpus(rng, 65, width, alpha, sig.dtype, bases=bases)
    probes[2:23] = sig[rng.randint(n, size=21)]
    cut = rng.randint(0, width, size=21)
    tail = np.arange(width)[None, :] >= cut[:, None]
    probes[23:44] = np.where(tail, probes[44:65], sig[rng.randint(n, size=21)])
    probes[0] = 0
    probes[1] = np.iinfo(sig.dtype).max
    return probes


def forest_cases(ctx):
    one_probe = 0
    for l, tree_words, w in ((1, 1, 1), (3, 2, 2), (8, 16, 1)):
        width = l * tree_words  # no spare column: tree l - 1 ends the row
        for dtype, code in ((np.uint32, MHX_U32), (np.uint64, MHX_U64)):
            # all rows identical, two values, the full range (uint64 without the middle one: the child's time is the host walk's)
            for alpha in (1, 2, 0) if dtype == np.uint32 else (1, 0):
                for n in (1, 2, 257):
                    rng = np.random.RandomState(1000 * l + 10 * alpha + n)
                    sig, bases = _corpus(rng, n, width, alpha, dtype)
                    shape = f"l={l} tree_words={tree_words} w={w} {np.dtype(dtype).name} alphabet={alpha} n={n}"
                    _begin("forest build " + shape)
                    d_sig, d_order = _dev(ctx, sig), _alloc(ctx, 4 * l * n)
                    ctx.lsh_forest_build_dev(d_sig.ptr, code, n, width, l, tree_words, d_order.ptr)
                    order = lexsort_order(sig, l, tree_words)
                    _expect(d_order.download((l, n), np.uint32), order, "forest build " + shape)
                    _done("forest build " + shape)
                    probes = _forest_probes(rng, sig, alpha, bases)
                    d_all = _dev(ctx, probes)
                    for k in (1, 10, 1024):
                        assert l * min(2 * k - 1, n) <= F.MAX_CANDIDATES
                        for m in (1, 65):
                            if m == 1:  # one probe alone: the all-zero row, the all-ones row and a row of the index in turn
                                q = probes[one_probe % 3 : one_probe % 3 + 1]
                                one_probe += 1
                                d_q = _dev(ctx, q)
                            else:
                                q, d_q = probes, d_all
                            what = f"forest query {shape} m={m} k={k}"
                            _begin(what)
                            d_slots, d_counts = _alloc(ctx, 4 * m * k), _alloc(ctx, 4 * m)
                            ctx.lsh_forest_query_dev(d_sig.ptr, code, n, width, l, tree_words, w, d_order.ptr, d_q.ptr, m, k, d_slots.ptr, d_counts.ptr)
                            want_slots, want_counts = F.host_query(sig, order, q, l, tree_words // w, w, k)
                            past = np.arange(k)[None, :] >= want_counts[:, None]
                            _expect(d_counts.download((m,), np.int32), want_counts, what + " counts")
                            # the cells past each count keep the pattern
                            _expect(d_slots.download((m, k), np.uint32), np.where(past, PATTERN32, want_slots), what + " slots")
                            _done(what)


def _pairs_cases(ctx, call, want_pairs, what):
    """A call that reports the total of (probe, slot) pairs and writes them when they fit, on a pair buffer of exactly the total
    and on one of half of it (nothing may be written at or past the capacity: the buffer ends there)."""
    total = len(want_pairs)
    for capacity in sorted({total, total // 2}, reverse=True):
        name = f"{what} capacity {capacity} of {total}"
        _begin(name)
        d_pairs = _alloc(ctx, max(1, 16 * capacity))
        found = call(d_pairs, capacity)
        assert found == total, (name, found)
        if capacity == total and total:
            _expect(d_pairs.download((total, 2), np.int64), want_pairs, name)
        elif capacity == 0:
            _expect(d_pairs.download((1,), np.uint8), np.full(1, PATTERN, dtype=np.uint8), name + ": a pair list of zero bytes was written")
        _done(name)


def ensemble_cases(ctx):
    k, levels = 32, [(2, 16), (4, 8)]
    sizes = [100, 0, 1, 40, 80, 79]  # one partition empty, one of a single row, one of 40 identical rows
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, n_parts, same = int(start[-1]), len(sizes), 3
    sig, probes = _clustered(61, n, 64, k, 12)
    sig[start[same]:start[same + 1]] = sig[start[same]]
    params = np.array([[0, 16], [0, 7], [1, 8], [1, 1], [1, 0]], dtype=np.int32)
    ens = _HostEnsemble(k, np.uint32, levels, start)
    ens.build(sig)
    rng = np.random.RandomState(62)
    nothing = rng.randint(0, 2**32, size=(50, k), dtype=np.uint64).astype(np.uint32)
    for name, q in (("clustered probes", probes), ("probes that hit nothing", nothing),
                    ("the identical row", np.repeat(sig[start[same]:start[same] + 1], 5, axis=0)), ("one probe", sig[n - 1:n])):
        m = q.shape[0]
        choice = rng.randint(0, params.shape[0] + 1, size=(m, n_parts)).astype(np.uint8)
        choice[choice == params.shape[0]] = 255  # the byte that skips a partition
        choice[0, 0], choice[-1, -1] = 255, 0
        if "identical" in name:
            choice[:, same] = [0, 1, 2, 3, 255]  # every band of the block, some of them, one, and not at all
        assert (choice == 255).any()
        want = _offsets_to_pairs(*ens.query(q, choice, params))
        assert (len(want) == 0) == ("nothing" in name), (name, len(want))
        if "identical" in name:
            assert len(want) >= 4 * sizes[same]

        def ensemble_query(d_pairs, capacity, q=q, choice=choice, m=m):
            bufs = [(_dev(ctx, d), _dev(ctx, rw)) for d, rw in ens.level_buffers()]
            c_levels = (_native.EnsembleLevel * len(levels))(*[_native.EnsembleLevel(d.ptr, rw.ptr, lr, lb) for (d, rw), (lr, lb) in zip(bufs, levels)])
            d_sig, d_q, d_choice = _dev(ctx, sig), _dev(ctx, q), _dev(ctx, choice)
            found = _i64(-1)
            check(ctx.lib.mhx_lsh_ensemble_query_dev(ctx.handle, c_levels, len(levels), start.ctypes.data_as(ctypes.POINTER(_i64)), n_parts, d_sig.ptr,
                                                     MHX_U32, k, d_q.ptr, m, d_choice.ptr, params.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                     params.shape[0], d_pairs.ptr, capacity, ctypes.byref(found)))
            return found.value
        _pairs_cases(ctx, ensemble_query, want, f"ensemble query, {name}")


def plain_query_cases(ctx):
    k, bands, r = 32, 8, 4
    rng = np.random.RandomState(63)
    row = rng.randint(0, 2**32, size=(1, k), dtype=np.uint64).astype(np.uint32)
    others = rng.randint(0, 2**32, size=(6, k), dtype=np.uint64).astype(np.uint32)
    others[:3, 4:] = row[0, 4:]  # rows that share all bands but the first with the index's
    q = np.concatenate([row, others])
    for name, sig in (("an index of 40 identical rows", np.repeat(row, 40, axis=0)), ("an index of one row", row)):
        n = sig.shape[0]
        dig, rows = lsh_bulk.sorted_bands(sig, bands, r, gpu_mode="disable")
        host = _HostBands(k, bands, r, np.uint32)
        host.append(sig)
        want = _offsets_to_pairs(*host.query(q))
        assert len(want) == 4 * n

        def bulk_query(d_pairs, capacity, sig=sig, n=n, dig=dig, rows=rows):
            d_dig, d_rows, d_sig, d_q = _dev(ctx, dig), _dev(ctx, rows), _dev(ctx, sig), _dev(ctx, q)
            found = _i64(-1)
            check(ctx.lib.mhx_lsh_query_dev(ctx.handle, d_dig.ptr, d_rows.ptr, n, bands, r, d_q.ptr, d_sig.ptr, MHX_U32, k, q.shape[0], d_pairs.ptr,
                                            capacity, ctypes.byref(found)))
            return found.value
        _pairs_cases(ctx, bulk_query, want, f"bulk query, {name}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    forest_cases(ctx)
    ensemble_cases(ctx)
    plain_query_cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"FOREST GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"FOREST GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
