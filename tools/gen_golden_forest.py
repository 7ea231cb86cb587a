#!/usr/bin/env python3
"""Pin MinHashLSHForest to the REAL reference's forest: writes tests/golden/lsh_forest.json.

    DATASKETCH_REFERENCE=<checkout of ekzhu/datasketch> python tools/gen_golden_forest.py

For every case of tests/test_lshforest_host.py the reference builds its MinHashLSHForest key by key from the test's own seeded
inputs, indexes it and answers the test's probes for every k of the test.  What is stored per case is the constructor arguments
and, per probe and k, the sorted positions (in insertion order) of the keys the reference returned -- the answers themselves, so
that a mismatch names the key.  Nothing here is copied from the reference: it is imported and called.
"""
from __future__ import annotations

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["DATASKETCH_REFERENCE"])

import datasketch as ref  # noqa: E402
import numpy as np  # noqa: E402

from tests import test_lshforest_host as T  # noqa: E402


def main():
    cases = {}
    for case in T.CASES:
        spec, keys, rows, probes = T.golden_inputs(case)
        if rows.ndim == 3:
            obj = lambda row: ref.WeightedMinHash(1, row)
        else:
            obj = lambda row: ref.MinHash(num_perm=spec["num_perm"], hashvalues=row.astype(np.uint64))
        forest = ref.MinHashLSHForest(num_perm=spec["num_perm"], l=spec["l"])
        for key, row in zip(keys, rows):
            forest.add(key, obj(row))
        forest.index()
        slot = {key: i for i, key in enumerate(keys)}
        answers = [[sorted(slot[key] for key in forest.query(obj(probe), k)) for k in T.KS] for probe in probes]
        cases[case] = {"num_perm": spec["num_perm"], "l": spec["l"], "ks": list(T.KS), "answers": answers}
        sizes = [(len(a), k) for per_probe in answers for a, k in zip(per_probe, T.KS)]
        print(case, "truncated", sum(n == k for n, k in sizes), "short", sum(n < k for n, k in sizes), "of", len(sizes))
    with open(T.GOLDEN_FOREST, "w") as f:
        json.dump(cases, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", T.GOLDEN_FOREST, os.path.getsize(T.GOLDEN_FOREST), "bytes")


if __name__ == "__main__":
    main()
