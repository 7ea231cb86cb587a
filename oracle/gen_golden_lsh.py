#!/usr/bin/env python3
"""Pin the bulk LSH helpers to the REAL reference's MinHashLSH: writes tests/golden/lsh_index.json.

    DATASKETCH_REFERENCE=<checkout of ekzhu/datasketch> python oracle/gen_golden_lsh.py

For every case of tests/test_lsh_bulk.py that compares with the reference's index, the reference builds the
index key by key (MinHashLSH.insert) from the test's own seeded inputs and answers the test's probes
(MinHashLSH.query).  What is stored is the (b, r) it chose, a sha256 of its dictionaries and one of its answers;
the tests recompute both from insert_bulk / query_bulk.  Nothing here is copied from the reference: it is
imported and called.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["DATASKETCH_REFERENCE"])

import datasketch as ref  # noqa: E402

from datasketch_amd import lsh_bulk as LB  # noqa: E402
from tests import test_lsh_bulk as T  # noqa: E402


def record(one, probes):
    return {"b": one.b, "r": one.r, "index_sha256": T.index_digest(one), "query_sha256": T.results_digest([one.query(p) for p in probes])}


def main():
    cases = {}
    sig = T._signatures(n=200, k=64)
    for prepickle, use_hashfunc in [(False, False), (True, False), (False, True)]:
        kw = dict(threshold=0.5, num_perm=64, prepickle=prepickle)
        if use_hashfunc:
            kw["hashfunc"] = LB.fnv1a_64
        one = ref.MinHashLSH(**kw)
        for i, row in enumerate(sig):
            one.insert(f"doc-{i}", ref.MinHash(num_perm=64, seed=1, hashvalues=row))
        cases[f"insert-{int(prepickle)}{int(use_hashfunc)}"] = record(one, [ref.MinHash(num_perm=64, seed=1, hashvalues=sig[0])])

    wm, _ = T._weighted_signatures()
    one = ref.MinHashLSH(threshold=0.5, num_perm=16)
    for i, w in enumerate(wm):
        one.insert(i, ref.WeightedMinHash(3, w.hashvalues))
    cases["weighted"] = record(one, [ref.WeightedMinHash(3, wm[3].hashvalues)])

    for prepickle in (True, False):
        sig, keys, probes = T.batch_inputs(prepickle)
        one = ref.MinHashLSH(threshold=0.6, num_perm=sig.shape[1], prepickle=prepickle)
        for key, row in zip(keys, sig):
            one.insert(key, ref.MinHash(num_perm=sig.shape[1], seed=1, hashvalues=row))
        cases[f"batches-{int(prepickle)}"] = record(one, [ref.MinHash(num_perm=sig.shape[1], seed=1, hashvalues=row) for row in probes])

    with open(T.GOLDEN_LSH, "w") as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", T.GOLDEN_LSH)


if __name__ == "__main__":
    main()
