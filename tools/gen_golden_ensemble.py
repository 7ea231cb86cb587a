#!/usr/bin/env python3
"""Pin MinHashLSHEnsemble to the REAL reference's ensemble: writes tests/golden/lsh_ensemble.json.

    DATASKETCH_REFERENCE=<checkout of ekzhu/datasketch> python tools/gen_golden_ensemble.py

From the seeded inputs of tests/test_lshensemble_host.py the reference computes (1) its parameter table for every argument tuple of
``PARAMS``, (2) ``lowers`` / ``uppers`` for every size multiset of ``BOUNDS`` and (3), for every case of ``CASES``, its table, its
bounds and -- per probe size and probe -- the sorted positions (in input order) of the keys it answers.  Nothing here is copied
from the reference: it is imported and called.  The answers must not be vacuous: the conditions asserted at the end are asserted
again from the fixture by the test.
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

from tests import test_lshensemble_host as T  # noqa: E402


def ints(bounds):
    return [None if x is None else int(x) for x in bounds]


def main():
    out = {"params": {}, "bounds": {}, "cases": {}}
    for args in T.PARAMS:
        weights = args[3] if len(args) > 3 else (0.5, 0.5)
        index = ref.MinHashLSHEnsemble(threshold=args[0], num_perm=args[1], m=args[2], weights=weights)
        out["params"][T._params_id(args)] = index.params.tolist()
        print("params", args, index.params.tolist())
    for name in T.BOUNDS:
        num_part, sizes = T.bounds_inputs(name)
        index = ref.MinHashLSHEnsemble(threshold=0.5, num_perm=4, num_part=num_part, m=2)
        blank = ref.MinHash(num_perm=4, hashvalues=np.zeros(4, dtype=np.uint64))
        index.index([(i, blank, int(size)) for i, size in enumerate(sizes)])
        out["bounds"][name] = {"lowers": ints(index.lowers), "uppers": ints(index.uppers)}
        print("bounds", name, np.unique(sizes).size, "distinct sizes", out["bounds"][name]["uppers"])
    selected, answers = set(), []
    for case in T.CASES:
        spec, keys, rows, sizes, probes = T.golden_inputs(case)
        index, obj = T.reference_ensemble(ref, spec, keys, rows, sizes)
        position = {key: i for i, key in enumerate(keys)}
        per_size = [[sorted(position[key] for key in index.query(obj(probe), size)) for probe in probes] for size in T.PROBE_SIZES]
        out["cases"][case] = {"params": index.params.tolist(), "lowers": ints(index.lowers), "uppers": ints(index.uppers), "answers": per_size}
        mine = {tuple(int(x) for x in index._get_optimal_param(u, size)) for size in T.PROBE_SIZES for u in index.uppers if u is not None}
        selected |= {(case, br) for br in mine}
        flat = [a for one_size in per_size for a in one_size]
        answers += flat
        print(case, "selects", sorted(mine), "empty", sum(not a for a in flat), "of", len(flat), "keys", sum(map(len, flat)))
    assert len({br for _, br in selected}) >= 3
    assert any(b < T.CASES[case]["num_perm"] // r for case, (b, r) in selected)
    assert any(T.CASES["odd-r"]["num_perm"] % r for case, (b, r) in selected if case == "odd-r")
    assert sum(not a for a in answers) * 2 <= len(answers)
    assert sum(map(len, answers)) > len(answers)
    with open(T.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")
    assert os.path.getsize(T.GOLDEN) <= 64 * 1024


if __name__ == "__main__":
    main()
