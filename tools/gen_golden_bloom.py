"""Record tests/golden/lsh_bloom.json: the answers of the reference's MinHashLSHBloom on a small corpus.

    python tools/gen_golden_bloom.py [/path/to/reference]

The reference's class needs ``pybloomfilter``; here it runs on a stand-in whose ``BloomFilter`` is a Python ``set``, so what is
recorded is the *exact* answer -- "some band of the query equals that band of an inserted row, as band keys" -- without any
false positive of a filter.  An index of this package must answer True wherever the fixture does, and may answer True elsewhere
only at its filters' false-positive rate.  The GPU tests use the fixture where the reference is not at hand.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsh_bloom.json")


class Sig:
    """What the reference's insert / query read of a MinHash."""

    def __init__(self, hashvalues):
        self.hashvalues = np.asarray(hashvalues, dtype=np.uint64)

    def __len__(self):
        return len(self.hashvalues)


def _standin():
    mod = types.ModuleType("pybloomfilter")

    class BloomFilter:
        def __init__(self, capacity=None, error_rate=None, filename=None):
            self.items = set()

        def add(self, x):
            self.items.add(int(x))

        def __contains__(self, x):
            return int(x) in self.items

        def sync(self):
            pass

    mod.BloomFilter = BloomFilter
    return mod


def reference_module(reference: str):
    """The reference's lsh_bloom.py, imported on the stand-in, with this package's MinHash under the name it imports."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import datasketch_amd
    from datasketch_amd import minhash

    names = ("pybloomfilter", "datasketch", "datasketch.minhash")
    saved = {k: sys.modules.get(k) for k in names}
    sys.modules.update({"pybloomfilter": _standin(), "datasketch": datasketch_amd, "datasketch.minhash": minhash})
    try:
        spec = importlib.util.spec_from_file_location("_reference_lsh_bloom", os.path.join(reference, "datasketch", "lsh_bloom.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def corpus(seed: int, n_insert: int, n_query: int, num_perm: int, b: int, r: int):
    """Inserted rows and queries: a third copies, a third sharing exactly one band with an inserted row, a third unrelated."""
    rng = np.random.RandomState(seed)
    ins = rng.randint(0, 2**32, size=(n_insert, num_perm), dtype=np.uint64)
    q = rng.randint(0, 2**32, size=(n_query, num_perm), dtype=np.uint64)
    kind = np.arange(n_query) % 3
    src = rng.randint(0, n_insert, size=n_query)
    band = rng.randint(0, b, size=n_query)
    for i in range(n_query):
        if kind[i] == 0:
            q[i] = ins[src[i]]
        elif kind[i] == 1:
            q[i, band[i] * r: (band[i] + 1) * r] = ins[src[i], band[i] * r: (band[i] + 1) * r]
    return ins, q


def exact_answers(ref, ins, q, num_perm, params, n, fp):
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lsh = ref.MinHashLSHBloom(num_perm=num_perm, n=n, fp=fp, params=params)
        for row in ins:
            lsh.insert(Sig(row))
        return [bool(lsh.query(Sig(row))) for row in q]


def main():
    reference = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref = reference_module(reference)
    num_perm, params, n, fp = 16, (3, 5), 100, 1e-3
    ins, q = corpus(11, 100, 300, num_perm, *params)
    doc = {"num_perm": num_perm, "params": list(params), "n": n, "fp": fp, "inserted": ins.tolist(), "queries": q.tolist(),
           "answers": exact_answers(ref, ins, q, num_perm, params, n, fp)}
    with open(GOLDEN, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {GOLDEN}: {len(doc['answers'])} queries, {sum(doc['answers'])} positives")


if __name__ == "__main__":
    main()
