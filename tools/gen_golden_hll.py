#!/usr/bin/env python3
"""Pin datasketch_amd.HyperLogLog to the REAL reference: writes tests/golden/hyperloglog.json.

    DATASKETCH_REFERENCE=<checkout of ekzhu/datasketch> python tools/gen_golden_hll.py

For every case of tests/test_hyperloglog_host.py (p in {4, 8, 11, 16}; 0, 1, 3, 300 and 5000 seeded integers through an identity
hashfunc, 40 byte tokens through the default SHA-1 functions, the hand-picked edge hashes) the reference's HyperLogLog -- and, for
the 64-bit registers, its HyperLogLogPlusPlus -- is fed token by token; recorded are the registers, for HyperLogLog its count()
and the bytes of its pickled state, and for every edge hash alone the one register it sets.  Nothing here is copied from the
reference: it is imported and called.  Registers are hex strings, rows above 256 bytes deflated first.
"""
from __future__ import annotations

import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.environ["DATASKETCH_REFERENCE"])

import datasketch as ref  # noqa: E402
import numpy as np  # noqa: E402

from tests import test_hyperloglog_host as T  # noqa: E402


def identity(x):
    return x


def sketch(bits, p, by_bytes):
    cls = ref.HyperLogLog if bits == 32 else ref.HyperLogLogPlusPlus
    return cls(p=p) if by_bytes else cls(p=p, hashfunc=identity)


def main():
    assert ref.__file__.startswith(os.environ["DATASKETCH_REFERENCE"])
    out = {"cases": {}, "edges": {}}
    warnings.simplefilter("ignore")
    for name in T.case_names():
        bits, p, tokens, _ = T.golden_tokens(name)
        h = sketch(bits, p, name.endswith("bytes"))
        for t in tokens:
            h.update(t)
        rec = {"reg": T.pack(h.reg.tobytes())}
        if bits == 32:
            rec["count"] = float(h.count())
            rec["state"] = T.pack(bytes(h.__getstate__()))
        out["cases"][name] = rec
        print(name, "nonzero", int(np.count_nonzero(h.reg)), "count", rec.get("count"))
    for kind, bits in T.KINDS.items():
        for p in T.PS:
            rows = []
            for hv in T.edge_hashes(bits, p):
                h = sketch(bits, p, False)
                h.update(hv)
                (idx,) = np.flatnonzero(h.reg).tolist()
                rows.append([str(hv), idx, int(h.reg[idx])])
            out["edges"][f"{kind}-p{p}"] = rows
    with open(T.GOLDEN, "w") as f:
        json.dump(out, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote", T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")
    assert os.path.getsize(T.GOLDEN) <= 96 * 1024


if __name__ == "__main__":
    main()
