"""The connected-components device entry points of include/mhx.h on buffers that abut an unmapped page (test infrastructure, run
as a script in a process of its own by tests/test_gpu_clusters_guard.py -- a kernel that over-reads kills the process).

    python tests/cc_guard_cases.py <align>        all cases; prints "CC GUARD OK <n> cases" and exits 0

<align> as for tests/guard_cases.py, whose helpers are used: labels, pairs, counts, digests, rows and the invalid counter of every
call are separate exact-size allocations from mhx_debug_guard_alloc, the labels pre-filled with a pattern, and the results are
checked against the host twin.  The path, the star, counts with a floor, hand-made bands and the host form (whose staging
buffers are exact-size allocations too).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, lsh_bulk  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _done, _expect  # noqa: E402


def one_call(ctx, n, what, pairs=None, counts=None, min_count=0, bands=None, want_invalid=0):
    d_labels = _alloc(ctx, 4 * n)
    d_bad = _alloc(ctx, 8, fill=0)
    ctx.cc_init_dev(d_labels.ptr, n)
    edges = []
    if pairs is not None:
        d_pairs = _dev(ctx, pairs)
        d_counts = None if counts is None else _dev(ctx, counts)
        ctx.cc_link_pairs_dev(d_labels.ptr, n, d_pairs.ptr, pairs.shape[0], None if d_counts is None else d_counts.ptr, min_count, d_bad.ptr)
        edges.append(pairs if counts is None else pairs[counts >= min_count])
    if bands is not None:
        dig, rows = bands
        d_dig, d_rows = _dev(ctx, dig), _dev(ctx, rows)
        ctx.cc_link_bands_dev(d_labels.ptr, n, d_dig.ptr, d_rows.ptr, dig.shape[1], dig.shape[0], d_bad.ptr)
        edges.append(np.stack(lsh_bulk._run_edges(dig, rows), axis=1))
    ctx.cc_finish_dev(d_labels.ptr, n)
    ctx.synchronize()
    edges = np.concatenate(edges)
    inside = ((edges >= 0) & (edges < n)).all(axis=1)
    _expect(d_labels.download((n,), np.uint32).astype(np.int64), lsh_bulk.connected_components(edges[inside], n, gpu_mode="disable"),
            what + " labels")
    _expect(d_bad.download((1,), np.int64), np.array([want_invalid]), what + " invalid")
    _done(what)


def cases(ctx):
    rng = np.random.RandomState(41)
    for n in (2, 65, 4096):
        i = np.arange(n - 1, 0, -1, dtype=np.int64)
        path = np.stack([i, i - 1], axis=1)
        one_call(ctx, n, f"path n={n}", pairs=path)
        one_call(ctx, n, f"shuffled path n={n}", pairs=path[rng.permutation(n - 1)])
        i = np.arange(n, dtype=np.int64)
        one_call(ctx, n + 1, f"star n={n + 1}", pairs=np.stack([i, np.full(n, n)], axis=1))
    for n, m in ((7, 3), (300, 257), (3000, 2001)):
        pairs = rng.randint(0, n, size=(m, 2)).astype(np.int64)
        counts = rng.randint(0, 17, size=m).astype(np.int32)
        one_call(ctx, n, f"counts n={n} m={m}", pairs=pairs, counts=counts, min_count=8)
        pairs[::5, 0] = n  # invalid edges among those the counts keep, unseen ones among those they drop
        one_call(ctx, n, f"counts + invalid n={n} m={m}", pairs=pairs, counts=counts, min_count=8,
                 want_invalid=int(np.count_nonzero(counts[::5] >= 8)))
    dig = np.array([[4, 4, 6, 7, 9], [9, 11, 11, 11, 12], [1, 2, 3, 5, 5]], dtype=np.uint64)
    rows = np.array([[0, 2, 1, 3, 4], [6, 5, 1, 3, 9], [0, 9, 4, 7, 8]], dtype=np.uint32)
    one_call(ctx, 10, "hand-made bands", bands=(dig, rows))
    one_call(ctx, 8, "hand-made bands, n = 8", bands=(dig, rows), want_invalid=1)
    one_call(ctx, 10, "hand-made bands after pairs", pairs=np.array([[9, 4], [6, 6]], dtype=np.int64), bands=(dig, rows))
    for n, b in ((1, 1), (333, 3), (2731, 3)):
        sig = rng.randint(0, 40, size=(n, b), dtype=np.uint64)
        one_call(ctx, n, f"sorted bands n={n} b={b}", bands=lsh_bulk.sorted_bands(sig, b, 1, gpu_mode="disable"))
    # the host form: pairs, counts, labels and the counter are pieces of exact-size scratch slots
    for n, m in ((1, 0), (5, 1), (3000, 2001)):
        pairs = rng.randint(0, n, size=(m, 2)).astype(np.int64)
        counts = rng.randint(0, 17, size=m).astype(np.int32)
        labels, invalid = ctx.cc_pairs(pairs, n)
        _expect(labels.astype(np.int64), lsh_bulk.connected_components(pairs, n, gpu_mode="disable"), f"host form n={n} m={m}")
        labels, invalid = ctx.cc_pairs(pairs, n, counts, 8)
        _expect(labels.astype(np.int64), lsh_bulk.connected_components(pairs, n, keep=counts >= 8, gpu_mode="disable"),
                f"host form with counts n={n} m={m}")
        assert invalid == 0
        _done(f"host form n={n} m={m}")


def main():
    align = int(sys.argv[1])
    granule, _ = _native.guard_alloc(align)  # before the first allocation of the process
    assert granule > 0
    ctx = _native.context()
    cases(ctx)
    ctx.synchronize()
    if G.FAILED:
        print(f"CC GUARD FAILED: {G.FAILED} mismatching cases of {G.CASES}", flush=True)
        sys.exit(1)
    print(f"CC GUARD OK {G.CASES} cases (align {align}, granule {granule} bytes)", flush=True)


if __name__ == "__main__":
    main()
