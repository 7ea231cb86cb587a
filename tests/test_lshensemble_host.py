"""datasketch_amd.MinHashLSHEnsemble on the numpy back end: the reference's parameter tables, partition bounds and answers (golden,
and live when its checkout is mounted), a dictionary model of the semantics, the exceptions, pickling, and the reference's own
test file run on this class.

The inputs of the golden cases are generated here from seeds; tools/gen_golden_ensemble.py feeds the same inputs to the reference
and writes tests/golden/lsh_ensemble.json.  ``golden_inputs``, ``bounds_inputs`` and ``check_case`` are shared with
tests/test_gpu_lshensemble.py."""
import importlib
import json
import os
import pickle
import sys
import types
import unittest

import numpy as np
import pytest

from datasketch_amd import MinHashLSHEnsemble
from datasketch_amd import lshensemble as E

REFERENCE = "/root/reference"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsh_ensemble.json")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "datasketch")), reason="reference repository not mounted")

# (threshold, num_perm, m[, weights]) of the golden parameter tables
PARAMS = [(0.5, 32, 4), (0.7, 50, 7), (0.9, 128, 8), (0.2, 64, 8, (0.3, 0.7)), (0.5, 16, 3), (0.85, 100, 8)]
PROBE_SIZES = (1, 5, 40, 300, 5000)
CASES = {
    # clustered rows: 12 random bases, a quarter of the positions redrawn
    "mixed-u32": dict(num_perm=32, m=4, num_part=4, threshold=0.5, n=300, probes=40, alpha=2**32, max_size=400, seed=21),
    "odd-r": dict(num_perm=50, m=7, num_part=4, threshold=0.7, n=150, probes=12, alpha=2**32, max_size=400, seed=22),  # r = 3 and 7 leave hash values unused
    "u64": dict(num_perm=32, m=4, num_part=3, threshold=0.5, n=120, probes=10, alpha=2**40, max_size=2000, seed=23),  # values above 2^32
    "weighted": dict(num_perm=12, m=3, num_part=3, threshold=0.5, n=120, probes=10, alpha=5, max_size=300, seed=24, weighted=True),
    "few-sizes": dict(num_perm=32, m=4, num_part=16, threshold=0.5, n=120, probes=10, alpha=2**32, sizes=(3, 9, 40, 41, 700), seed=25),
    "one-part": dict(num_perm=32, m=4, num_part=1, threshold=0.6, n=120, probes=10, alpha=2**32, max_size=400, seed=26),
}
# size multisets of the golden partition bounds: (num_part, sizes)
BOUNDS = ("one", "two", "more-parts-than-sizes", "equal-counts", "long-tail")


class _Sig:
    """Anything with ``hashvalues`` and ``len()`` is a signature to the index."""

    def __init__(self, hashvalues):
        self.hashvalues = np.asarray(hashvalues)

    def __len__(self):
        return len(self.hashvalues)


def bounds_inputs(name):
    """(num_part, sizes int64[n]) of a golden bounds case."""
    rng = np.random.RandomState({"one": 31, "two": 32, "more-parts-than-sizes": 33, "equal-counts": 34, "long-tail": 35}[name])
    if name == "one":
        return 1, rng.randint(1, 500, 80)
    if name == "two":
        return 2, rng.randint(1, 60, 200)
    if name == "more-parts-than-sizes":
        return 8, rng.choice([2, 3, 10, 50, 51], 60)
    if name == "equal-counts":  # consecutive sizes, three sets each: near-ties in the dynamic programme
        return 6, np.repeat(np.arange(1, 41), 3)
    sizes = np.minimum((rng.pareto(0.9, 800) * 8 + 1).astype(np.int64), 100000)  # skewed, long-tailed: about 150 distinct sizes
    return 16, sizes


def golden_inputs(case):
    """(spec, keys, signatures for index_bulk, sizes, probes for query_bulk) of a golden case; the weighted matrices are [N, S, 2]
    int64 (k, t) pairs with t in [-3, 2)."""
    spec = CASES[case]
    rng = np.random.RandomState(spec["seed"])
    words = 2 if spec.get("weighted") else 1
    width = spec["num_perm"] * words
    n = spec["n"]

    def clustered(count, bases):
        rows = bases[rng.randint(len(bases), size=count)]
        redraw = rng.rand(count, width) < 0.25
        rows[redraw] = rng.randint(0, spec["alpha"], int(redraw.sum()), dtype=np.int64)
        return rows

    bases = rng.randint(0, spec["alpha"], (12, width), dtype=np.int64)
    rows = clustered(n, bases)
    probes = clustered(spec["probes"], bases)
    probes[: spec["probes"] // 2] = rows[rng.randint(n, size=spec["probes"] // 2)]
    sizes = rng.choice(spec["sizes"], n) if "sizes" in spec else rng.randint(1, spec["max_size"], n)
    if words == 2:
        rows[:, 1::2] -= 3
        probes[:, 1::2] -= 3
        rows, probes = rows.reshape(-1, spec["num_perm"], 2), probes.reshape(-1, spec["num_perm"], 2)
    elif spec["alpha"] <= 2**32:
        rows, probes = rows.astype(np.uint32), probes.astype(np.uint32)
    else:
        rows, probes = rows.astype(np.uint64), probes.astype(np.uint64)
    return spec, [f"set-{i}" for i in range(n)], rows, sizes.astype(np.int64), probes


def signature(row):
    return _Sig(row if row.ndim == 2 else row.astype(np.uint64))


def constructor_args(spec):
    return dict(threshold=spec["threshold"], num_perm=spec["num_perm"], num_part=spec["num_part"], m=spec["m"])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def as_ints(bounds):
    return [None if x is None else int(x) for x in bounds]


def check_case(case, gpu_mode, gold):
    """Built entry by entry and by index_bulk: the bounds are the golden ones, every (probe, size) answer is the golden set of
    positions, in slot order and without repeats, and query_bulk equals query row by row.  Returns the bulk-built index."""
    spec, keys, rows, sizes, probes = golden_inputs(case)
    one = MinHashLSHEnsemble(gpu_mode=gpu_mode, **constructor_args(spec))
    one.index((key, signature(row), size) for key, row, size in zip(keys, rows, sizes.tolist()))
    bulk = MinHashLSHEnsemble(gpu_mode=gpu_mode, **constructor_args(spec))
    bulk.index_bulk(keys, rows, sizes)
    position = {key: i for i, key in enumerate(keys)}
    slot_of = {key: s for s, key in enumerate(bulk._keys)}
    for index in (one, bulk):
        assert index.params.tolist() == gold["params"]
        assert as_ints(index.lowers) == gold["lowers"] and as_ints(index.uppers) == gold["uppers"]
    for size, want in zip(PROBE_SIZES, gold["answers"]):
        got_bulk = bulk.query_bulk(probes, np.full(len(probes), size))
        for probe, want_positions, got in zip(probes, want, got_bulk):
            assert sorted(position[key] for key in got) == want_positions
            slots = [slot_of[key] for key in got]
            assert slots == sorted(set(slots))  # slot order, each key once
            assert list(one.query(signature(probe), size)) == got == list(bulk.query(signature(probe), size))
    return bulk


# ---------------------------------------------------------------- golden: parameter tables, bounds, answers
def _params_id(args):
    return "-".join(str(a) for a in args[:3])


@pytest.mark.parametrize("args", PARAMS, ids=_params_id)
def test_params_table_is_the_references(args):
    weights = args[3] if len(args) > 3 else (0.5, 0.5)
    index = MinHashLSHEnsemble(threshold=args[0], num_perm=args[1], m=args[2], weights=weights, gpu_mode="disable")
    assert index.params.tolist() == golden()["params"][_params_id(args)]
    assert index.params.shape == (10, 2) and np.array_equal(index.xqs, np.exp(np.linspace(-5, 5, 10)))
    assert (index.threshold, index.h, index.m) == (args[0], args[1], args[2])


def test_golden_params_are_the_ones_checked_by_hand():
    gold = golden()["params"]
    assert gold["0.5-32-4"] == [[1, 4]] * 4 + [[8, 4], [16, 2], [13, 1]] + [[32, 1]] * 3
    assert {r for _, r in gold["0.7-50-7"]} == {1, 2, 3, 7} and [17, 1] in gold["0.7-50-7"]


def _bounds_index(name, gpu_mode="disable"):
    num_part, sizes = bounds_inputs(name)
    index = MinHashLSHEnsemble(threshold=0.5, num_perm=4, num_part=num_part, m=2, gpu_mode=gpu_mode)
    index.index_bulk(range(sizes.size), np.zeros((sizes.size, 4), dtype=np.uint32), sizes)
    return index


@pytest.mark.parametrize("name", BOUNDS)
def test_partition_bounds_are_the_references(name):
    gold = golden()["bounds"][name]
    index = _bounds_index(name)
    assert as_ints(index.lowers) == gold["lowers"] and as_ints(index.uppers) == gold["uppers"]
    assert len(index.lowers) == len(index.uppers) == bounds_inputs(name)[0]


def test_golden_bounds_cover_the_shapes():
    gold = golden()["bounds"]
    assert len(gold["one"]["uppers"]) == 1 and len(gold["two"]["uppers"]) == 2
    assert gold["more-parts-than-sizes"]["uppers"][5:] == [None] * 3 and gold["more-parts-than-sizes"]["uppers"][:5] == [2, 3, 10, 50, 51]
    assert 100 <= np.unique(bounds_inputs("long-tail")[1]).size <= 200 and None not in gold["long-tail"]["uppers"]


def test_suffix_sums_give_the_same_bounds_as_slice_sums(monkeypatch):
    """Above ``_EXACT_SUMS_BELOW`` distinct sizes the interval costs are suffix sums; on the golden multisets both give the bounds."""
    for name in ("equal-counts", "long-tail", "two"):
        num_part, sizes = bounds_inputs(name)
        distinct, counts = np.unique(sizes, return_counts=True)
        exact = E._partition_bounds(distinct, counts, num_part)
        monkeypatch.setattr(E, "_EXACT_SUMS_BELOW", 0)
        assert E._partition_bounds(distinct, counts, num_part) == exact
        monkeypatch.undo()


@pytest.mark.parametrize("case", list(CASES))
def test_golden_answers(case):
    check_case(case, "disable", golden()["cases"][case])


def test_golden_answers_are_not_vacuous():
    """What the generator asserted when it wrote the fixture, asserted again from the fixture."""
    gold = golden()["cases"]
    selected, answers = set(), []
    for case, g in gold.items():
        spec = CASES[case]
        for size in PROBE_SIZES:
            for upper in g["uppers"]:
                if upper is not None:
                    i = min(int(np.searchsorted(np.exp(np.linspace(-5, 5, 10)), float(upper) / float(size), side="left")), 9)
                    selected.add((case, tuple(g["params"][i])))
        answers += [a for per_size in g["answers"] for a in per_size]
        assert len(g["answers"]) == len(PROBE_SIZES) and all(len(per_size) == spec["probes"] for per_size in g["answers"])
    assert len({br for _, br in selected}) >= 3
    assert any(b < CASES[case]["num_perm"] // r for case, (b, r) in selected)
    assert any(CASES["odd-r"]["num_perm"] % r for case, (b, r) in selected if case == "odd-r")
    assert sum(not a for a in answers) * 2 <= len(answers)
    assert sum(map(len, answers)) > len(answers)


# ---------------------------------------------------------------- live against the reference
def _reference():
    saved = {k: v for k, v in sys.modules.items() if k == "datasketch" or k.startswith("datasketch.")}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REFERENCE)
    try:
        return importlib.import_module("datasketch")
    finally:
        sys.path.remove(REFERENCE)
        for k in [k for k in sys.modules if k == "datasketch" or k.startswith("datasketch.")]:
            del sys.modules[k]
        sys.modules.update(saved)


def reference_ensemble(ref, spec, keys, rows, sizes):
    index = ref.MinHashLSHEnsemble(**constructor_args(spec))
    if rows.ndim == 3:
        obj = lambda row: ref.WeightedMinHash(1, row)
    else:
        obj = lambda row: ref.MinHash(num_perm=spec["num_perm"], hashvalues=row.astype(np.uint64))
    index.index([(key, obj(row), int(size)) for key, row, size in zip(keys, rows, sizes)])
    return index, obj


@needs_reference
def test_params_bounds_and_answers_against_the_live_reference():
    ref = _reference()
    rng = np.random.RandomState(41)
    for trial in range(6):
        spec = dict(threshold=float(rng.choice([0.3, 0.5, 0.8])), num_perm=int(rng.choice([16, 24, 30])), m=int(rng.choice([2, 3, 5])),
                    num_part=int(rng.choice([1, 2, 3, 7])))
        n = 90
        bases = rng.randint(0, 2**32, (5, spec["num_perm"]), dtype=np.int64)
        rows = bases[rng.randint(5, size=n)]
        redraw = rng.rand(n, spec["num_perm"]) < 0.2
        rows[redraw] = rng.randint(0, 2**32, int(redraw.sum()), dtype=np.int64)
        rows = rows.astype(np.uint32)
        sizes = rng.randint(1, 30 if trial % 2 else 3000, n)
        keys = list(range(n))
        theirs, obj = reference_ensemble(ref, spec, keys, rows, sizes)
        ours = MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))
        ours.index_bulk(keys, rows, sizes)
        assert ours.params.tolist() == theirs.params.tolist()
        assert as_ints(ours.lowers) == as_ints(theirs.lowers) and as_ints(ours.uppers) == as_ints(theirs.uppers)
        for size in (1, 7, 100, 4000):
            got = ours.query_bulk(rows[:25], np.full(25, size))
            for row, answer in zip(rows[:25], got):
                assert sorted(answer) == sorted(theirs.query(obj(row), size))


# ---------------------------------------------------------------- a dictionary model of the semantics
def model_answers(index, keys, mat, sizes, probes, probe_sizes):
    """Per partition and r, B dictionaries band bytes -> keys; a query reads the first b of the partition's tables for the r that
    upper / size selects.  ``mat`` / ``probes``: uint64 words matrices, ``w`` words per hash value."""
    w = mat.shape[1] // index.h
    uppers = [u for u in index.uppers if u is not None]
    tables = []
    for p, upper in enumerate(uppers):
        lower = index.lowers[p]
        members = [i for i in range(len(keys)) if lower <= sizes[i] <= upper]
        per_r = {}
        for r in sorted(set(index.params[:, 1].tolist())):
            bands = [dict() for _ in range(index.h // r)]
            for i in members:
                for j, table in enumerate(bands):
                    table.setdefault(mat[i, j * r * w : (j + 1) * r * w].tobytes(), set()).add(keys[i])
            per_r[r] = bands
        tables.append(per_r)
    out = []
    for probe, size in zip(probes, probe_sizes):
        found = set()
        for p, upper in enumerate(uppers):
            i = min(int(np.searchsorted(index.xqs, float(upper) / float(size), side="left")), 9)
            b, r = index.params[i].tolist()
            for j in range(b):
                found |= tables[p][r][j].get(probe[j * r * w : (j + 1) * r * w].tobytes(), set())
        out.append(found)
    return out


def test_answers_equal_a_dictionary_model_on_random_constructions():
    rng = np.random.RandomState(51)
    for trial in range(300):
        num_perm = int(rng.randint(4, 17))
        m = int(rng.randint(2, min(num_perm // 2, 5) + 1))
        index = MinHashLSHEnsemble(threshold=float(rng.choice([0.2, 0.5, 0.9])), num_perm=num_perm, num_part=int(rng.randint(1, 9)), m=m,
                                   gpu_mode="disable")
        n, words = int(rng.randint(1, 60)), 1 + trial % 2
        alpha = int(rng.choice([2, 3, 50]))
        mat = rng.randint(0, alpha, (n, num_perm * words)).astype(np.uint64)
        sizes = rng.randint(1, int(rng.choice([4, 40, 4000])), n)
        keys = [("k", i) for i in range(n)]
        probes = np.concatenate([mat[rng.randint(n, size=4)], rng.randint(0, alpha, (4, num_perm * words)).astype(np.uint64)])
        probe_sizes = rng.randint(1, 5000, 8)
        shaped = (lambda a: a.view(np.int64).reshape(len(a), num_perm, 2)) if words == 2 else (lambda a: a)
        index.index_bulk(keys, shaped(mat), sizes)
        got = index.query_bulk(shaped(probes), probe_sizes)
        want = model_answers(index, keys, mat, sizes, probes, probe_sizes)
        assert [set(a) for a in got] == want and all(len(a) == len(set(a)) for a in got), trial


# ---------------------------------------------------------------- exceptions
def test_constructor_checks():
    for kwargs, message in [(dict(threshold=1.5), "threshold must be in"), (dict(threshold=-0.1), "threshold must be in"),
                            (dict(num_perm=1), "Too few permutation functions"), (dict(num_part=0), "num_part must be at least 1"),
                            (dict(m=1), "m must be in the range"), (dict(num_perm=8, m=9), "m must be in the range"),
                            (dict(weights=(1.5, -0.5)), "Weight must be in"), (dict(weights=(0.5, 0.4)), "Weights must sum to 1.0"),
                            (dict(num_perm=8, m=8), "The number of bands are too small"),
                            (dict(storage_config={"type": "redis"}), "only the in-memory storage"),
                            (dict(storage_config="dict"), "only the in-memory storage"), (dict(gpu_mode="sometimes"), "gpu_mode must be")]:
        with pytest.raises(ValueError, match=message):
            MinHashLSHEnsemble(**{"num_perm": 16, "m": 2, "gpu_mode": "disable", **kwargs})
    MinHashLSHEnsemble(num_perm=16, m=2, storage_config={"type": "dict"}, gpu_mode="disable")


def _small(**kwargs):
    return MinHashLSHEnsemble(**{"threshold": 0.5, "num_perm": 16, "m": 2, "num_part": 3, "gpu_mode": "disable", **kwargs})


def test_index_and_query_checks():
    rows = np.arange(48, dtype=np.uint32).reshape(3, 16)
    entries = [(i, _Sig(rows[i]), 5 + i) for i in range(3)]
    with pytest.raises(ValueError, match="entries is empty"):
        _small().index([])
    with pytest.raises(ValueError, match="entries is empty"):
        _small().index_bulk([], np.empty((0, 16), dtype=np.uint32), [])
    for bad in (0, -3):
        with pytest.raises(ValueError, match="Set size must be positive"):
            _small().index([(0, _Sig(rows[0]), bad)])
        with pytest.raises(ValueError, match="Set size must be positive"):
            _small().index_bulk([0, 1, 2], rows, [4, bad, 4])
    with pytest.raises(ValueError, match="Expecting minhash with length 16, got 8"):
        _small().index([(0, _Sig(rows[0, :8]), 3)])
    with pytest.raises(ValueError, match="Expecting minhash with length 16, got 12"):
        _small().index_bulk([0, 1, 2], rows[:, :12], [1, 2, 3])
    with pytest.raises(ValueError, match="same length"):
        _small().index_bulk([0, 1], rows, [1, 2, 3])
    with pytest.raises(ValueError, match="same length"):
        _small().index_bulk([0, 1, 2], rows, [1, 2])
    duplicate = _small()
    with pytest.raises(ValueError, match="already exists"):
        duplicate.index([(7, _Sig(rows[0]), 1), (8, _Sig(rows[1]), 2), (7, _Sig(rows[2]), 900)])
    assert duplicate.is_empty() and duplicate.uppers == [None] * 3  # nothing was built
    index = _small()
    index.index(entries)
    for again in (lambda: index.index(entries), lambda: index.index_bulk([9], rows[:1], [1])):
        with pytest.raises(ValueError, match="Cannot call index again"):
            again()
    for bad in (0, -1):
        with pytest.raises(ValueError, match="Set size must be positive"):
            index.query(_Sig(rows[0]), bad)
        with pytest.raises(ValueError, match="Set size must be positive"):
            index.query_bulk(rows, [1, bad, 1])
    with pytest.raises(ValueError, match="Expecting minhash with length 16, got 8"):
        index.query(_Sig(rows[0, :8]), 3)
    with pytest.raises(ValueError, match="Expecting minhash with length 16, got 12"):
        index.query_bulk(rows[:, :12], [1, 2, 3])
    with pytest.raises(ValueError, match="same length"):
        index.query_bulk(rows, [1, 2])
    with pytest.raises(ValueError, match="together"):
        _small().index([(0, _Sig(rows[0]), 1), (1, _Sig(np.zeros((16, 2), dtype=np.int64)), 2)])


# ---------------------------------------------------------------- the rest of the surface
def test_query_returns_a_generator_and_membership():
    rows = np.arange(48, dtype=np.uint32).reshape(3, 16)
    for prepickle in (None, True):
        index = _small(prepickle=prepickle)
        assert index.is_empty() and ("a", 0) not in index and index.prepickle is bool(prepickle)
        index.index((("a", i), _Sig(rows[i]), 5 + i) for i in range(3))
        assert not index.is_empty() and ("a", 1) in index and ("a", 3) not in index
        answer = index.query(_Sig(rows[1]), 6)
        assert isinstance(answer, types.GeneratorType)
        assert ("a", 1) in list(answer)
        assert ("a", 1) in index.query_bulk(rows, [5, 6, 7])[1]
        assert index._keys[0] == (pickle.dumps(("a", 0)) if prepickle else ("a", 0))
    weighted = _small()
    weighted.index([(0, _Sig(np.zeros((16, 2), dtype=np.int64)), 1)])
    assert list(weighted.query(_Sig(rows[0]), 1)) == []  # a MinHash probe matches no WeightedMinHash row
    assert weighted.query_bulk(rows, [1, 1, 1]) == [[], [], []]


@pytest.mark.parametrize("case", ["mixed-u32", "weighted", "few-sizes"])
def test_pickle_round_trip_answers_identically(case):
    spec, keys, rows, sizes, probes = golden_inputs(case)
    index = MinHashLSHEnsemble(gpu_mode="disable", prepickle=case == "weighted", **constructor_args(spec))
    index.index_bulk(keys, rows, sizes)
    loaded = pickle.loads(pickle.dumps(index))
    assert as_ints(loaded.uppers) == as_ints(index.uppers) and loaded.params.tolist() == index.params.tolist()
    assert keys[3] in loaded and not loaded.is_empty()
    for (d1, r1), (d2, r2) in zip(index._backend.level_buffers(), loaded._backend.level_buffers()):
        assert np.array_equal(d1, d2) and np.array_equal(r1, r2)
    for size in PROBE_SIZES:
        assert loaded.query_bulk(probes, np.full(len(probes), size)) == index.query_bulk(probes, np.full(len(probes), size))
    empty = pickle.loads(pickle.dumps(MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))))
    assert empty.is_empty() and empty.uppers == [None] * spec["num_part"]


def test_index_bulk_takes_the_values_at_call_time():
    spec, keys, rows, sizes, probes = golden_inputs("mixed-u32")
    index = MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))
    mine = rows.copy()
    index.index_bulk(keys, mine, sizes)
    before = index.query_bulk(probes, np.full(len(probes), 40))
    mine[:] = 0
    assert index.query_bulk(probes, np.full(len(probes), 40)) == before


def test_level_buffers_are_sorted_blocks_per_partition():
    """The layout: per level and partition a block of B bands, each ascending by (digest, local row) and a permutation of the
    partition's rows."""
    spec, keys, rows, sizes, _ = golden_inputs("odd-r")
    index = MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))
    index.index_bulk(keys, rows, sizes)
    start = index._start
    assert start[0] == 0 and start[-1] == len(keys) and np.all(np.diff(start) >= 0)
    assert sorted(r for r, _ in index._backend.levels) == sorted(set(index.params[:, 1].tolist()))
    for (r, bands), (dig, slots) in zip(index._backend.levels, index._backend.level_buffers()):
        assert bands == spec["num_perm"] // r and dig.size == slots.size == bands * len(keys)
        for s0, s1 in zip(start[:-1], start[1:]):
            d = dig[bands * s0 : bands * s1].reshape(bands, s1 - s0)
            rw = slots[bands * s0 : bands * s1].reshape(bands, s1 - s0).astype(np.int64)
            assert np.array_equal(np.sort(rw, axis=1), np.broadcast_to(np.arange(s1 - s0), rw.shape))
            assert np.all((d[:, 1:] > d[:, :-1]) | ((d[:, 1:] == d[:, :-1]) & (rw[:, 1:] > rw[:, :-1])))


# ---------------------------------------------------------------- the reference's own tests on this class
@needs_reference
def test_reference_test_file_passes_on_this_class():
    """test/test_lshensemble.py of the reference, unmodified, with ``datasketch.lshensemble`` and ``datasketch.minhash`` aliased to
    this package (the Redis cases left out: storage back ends are out of scope)."""
    import datasketch_amd
    from datasketch_amd import minhash

    pattern = ("datasketch", "test")
    saved = {k: v for k, v in sys.modules.items() if k in pattern or k.startswith(tuple(p + "." for p in pattern))}
    for k in saved:
        del sys.modules[k]
    sys.modules["datasketch"] = datasketch_amd
    sys.modules["datasketch.lshensemble"] = E
    sys.modules["datasketch.minhash"] = minhash
    stubbed = "mockredis" not in sys.modules
    if stubbed:
        sys.modules["mockredis"] = types.ModuleType("mockredis")
    sys.path.insert(0, REFERENCE)
    try:
        mod = importlib.import_module("test.test_lshensemble")
        assert mod.MinHashLSHEnsemble is MinHashLSHEnsemble
        suite = unittest.TestSuite(t for group in unittest.defaultTestLoader.loadTestsFromModule(mod) for t in group
                                   if "redis" not in t.id().lower())
        assert suite.countTestCases() >= 4
        result = unittest.TextTestRunner(verbosity=0).run(suite)
        problems = [f"{t}: {tb.splitlines()[-1]}" for t, tb in result.failures + result.errors]
        assert not problems, problems
    finally:
        sys.path.remove(REFERENCE)
        if stubbed:
            del sys.modules["mockredis"]
        for k in [k for k in sys.modules if k in pattern or k.startswith(tuple(p + "." for p in pattern))]:
            del sys.modules[k]
        sys.modules.update(saved)
