"""datasketch_amd.MinHashLSH on the numpy back end: golden answers of the reference's index, a differential run against a
dict-of-sets model, cross-checks with the reference (when its checkout is mounted), pickling and the lsh_bulk hand-off.

The helpers ``golden_case`` and ``run_differential`` are shared with tests/test_gpu_minhash_lsh.py (gpu_mode='always')."""
import importlib
import os
import pickle
import sys
import types
import unittest

import numpy as np
import pytest

from datasketch_amd import MinHash, MinHashLSH, WeightedMinHash
from datasketch_amd import lsh as L
from datasketch_amd import lsh_bulk as LB
from tests.test_lsh_bulk import _signatures, _weighted_signatures, batch_inputs, lsh_golden, results_digest

REFERENCE = "/root/reference"
GOLDEN_CASES = ["insert-00", "insert-01", "insert-10", "weighted", "batches-0", "batches-1"]


class _Sig:
    """Anything with ``hashvalues`` and ``len()`` is a signature to the index."""

    def __init__(self, hashvalues):
        self.hashvalues = np.asarray(hashvalues)

    def __len__(self):
        return len(self.hashvalues)


def _golden_inputs(case):
    """(constructor kwargs, keys, signature matrix, per-key objects, probe matrix, probe objects) of a golden case."""
    if case.startswith("insert-"):
        prepickle, use_hashfunc = bool(int(case[7])), bool(int(case[8]))
        sig = _signatures(n=200, k=64)
        kw = dict(threshold=0.5, num_perm=64, prepickle=prepickle, hashfunc=LB.fnv1a_64 if use_hashfunc else None)
        keys = [f"doc-{i}" for i in range(sig.shape[0])]
        objs = [MinHash(num_perm=64, seed=1, hashvalues=row) for row in sig]
        return kw, keys, sig, objs, sig[:1], objs[:1]
    if case == "weighted":
        wm, sig = _weighted_signatures()
        return dict(threshold=0.5, num_perm=16), list(range(len(wm))), sig, wm, sig[3:4], [WeightedMinHash(3, wm[3].hashvalues)]
    prepickle = case == "batches-1"
    sig, keys, probes = batch_inputs(prepickle)
    objs = [MinHash(num_perm=64, seed=1, hashvalues=row) for row in sig]
    return dict(threshold=0.6, num_perm=64, prepickle=prepickle), keys, sig, objs, probes, [MinHash(num_perm=64, seed=1, hashvalues=p) for p in probes]


def golden_case(case, gpu_mode):
    """The index built key by key and in two bulk batches answers the golden probes as the reference's index did."""
    gold = lsh_golden(case)
    kw, keys, sig, objs, probes, probe_objs = _golden_inputs(case)
    one = MinHashLSH(gpu_mode=gpu_mode, **kw)
    assert (one.b, one.r) == (gold["b"], gold["r"])
    for key, m in zip(keys, objs):
        one.insert(key, m)
    bulk = MinHashLSH(gpu_mode=gpu_mode, params=(one.b, one.r), **{k: v for k, v in kw.items() if k != "threshold"})
    half = len(keys) // 2
    bulk.insert_bulk(keys[:half], sig[:half])
    bulk.insert_bulk(keys[half:], sig[half:])
    for index in (one, bulk):
        assert results_digest([index.query(p) for p in probe_objs]) == gold["query_sha256"]
        assert results_digest(index.query_bulk(probes)) == gold["query_sha256"]
    for a, b in zip(one._backend.bands(), bulk._backend.bands()):
        assert np.array_equal(a, b)
    return one


@pytest.mark.parametrize("case", GOLDEN_CASES)
def test_golden_answers_of_the_reference_index(case):
    golden_case(case, "disable")


# ---- differential run against a dict model ------------------------------------------------------------------------------
class DictModel:
    """The reference's dictionaries, with this index's rule for keys inserted more than once: a key owns all its rows."""

    def __init__(self, b, r, words, hashfunc=None):
        self.b, self.r, self.words, self.hashfunc = b, r, words, hashfunc
        self.rows = {}  # key -> list of word rows

    def band_keys(self, row):
        w = self.r * self.words
        return [bytes(np.asarray(row[j * w : (j + 1) * w], dtype=np.uint64).byteswap().data) for j in range(self.b)]

    def insert(self, key, row):
        self.rows.setdefault(key, []).append(self.band_keys(row))

    def remove(self, key):
        del self.rows[key]

    def query(self, row):
        hs = self.band_keys(row)
        return {k for k, rows in self.rows.items() if any(h == x[j] for x in rows for j, h in enumerate(hs))}

    def counts(self, keys=None):
        tables = [dict() for _ in range(self.b)]
        for key in self.rows if keys is None else set(keys):
            for j in range(self.b):
                for h in {x[j] for x in self.rows.get(key, [])}:
                    h = self.hashfunc(h) if self.hashfunc else h
                    tables[j].setdefault(h, set()).add(key)
        return [{h: len(s) for h, s in t.items()} for t in tables]


def _words(sig_obj_or_row):
    return LB._words_of(sig_obj_or_row)[0]


def run_differential(gpu_modes, variant, prepickle, seed=0, n_ops=2000, after_op=None):
    """A seeded sequence of operations on one index per gpu_mode, answers checked against DictModel at every query.
    variant: 'u32', 'u64' (values >= 2^32 arrive after uint32 rows) or 'weighted'.  Returns the indexes."""
    rng = np.random.RandomState(seed)
    h, b, r = 24, 6, 4
    words = 2 if variant == "weighted" else 1
    hashfunc = LB.fnv1a_64 if seed % 2 else None
    make = lambda: [MinHashLSH(num_perm=h, params=(b, r), prepickle=prepickle, hashfunc=hashfunc, gpu_mode=g) for g in gpu_modes]
    lshs = make()
    for one in lshs:
        one.buffer_size = 37
    model = DictModel(b, r, words, hashfunc)
    bases = rng.randint(0, 2**32, (12, h * words)).astype(np.uint64)
    next_key = [0]

    def new_key():
        next_key[0] += 1
        k = next_key[0]
        return ("k", k) if prepickle and k % 3 == 0 else (f"key-{k}" if k % 2 else k)

    def new_row(step):
        row = bases[rng.randint(len(bases))].copy()
        mutate = rng.rand(row.size) < rng.choice([0.05, 0.3, 0.9])
        row[mutate] = rng.randint(0, 2**32, int(mutate.sum()))
        if variant == "u64" and step > n_ops // 2 and rng.rand() < 0.5:
            row[rng.randint(row.size)] |= np.uint64(1 << 40)
        return row

    def obj(row):
        return _Sig(row.view(np.int64).reshape(h, 2) if words == 2 else row)

    def bulk_matrix(rows):
        m = np.stack(rows)
        if words == 2:
            return m.view(np.int64).reshape(len(rows), h, 2)
        return m.astype(np.uint32) if variant == "u32" and rng.rand() < 0.5 else m

    compactions = [0]
    original = MinHashLSH._compact

    def counting(self):
        if self._n_dead:
            compactions[0] += 1
        original(self)

    MinHashLSH._compact = counting
    try:
        for step in range(n_ops):
            op = rng.rand()
            live = list(model.rows)
            if op < 0.22 or not live:
                key, row = new_key(), new_row(step)
                for one in lshs:
                    one.insert(key, obj(row))
                model.insert(key, row)
            elif op < 0.32:
                keys = [new_key() for _ in range(rng.randint(1, 12))]
                rows = [new_row(step) for _ in keys]
                mat = bulk_matrix(rows)
                for one in lshs:
                    one.insert_bulk(keys, mat)
                for key, row in zip(keys, rows):
                    model.insert(key, row)
            elif op < 0.55:
                for key in [live[i] for i in rng.choice(len(live), min(len(live), rng.randint(1, 5)), replace=False)]:
                    for one in lshs:
                        one.remove(key)
                    model.remove(key)
            elif op < 0.58:
                keys = [new_key() for _ in range(rng.randint(1, 10))]
                rows = [new_row(step) for _ in keys]
                for one in lshs:
                    with one.insertion_session(buffer_size=5) as s:
                        for key, row in zip(keys, rows):
                            s.insert(key, obj(row))
                    one.buffer_size = 37
                for key, row in zip(keys, rows):
                    model.insert(key, row)
            elif op < 0.61:
                gone = [live[i] for i in rng.choice(len(live), min(len(live), rng.randint(1, 6)), replace=False)]
                for one in lshs:
                    with one.deletion_session() as s:
                        for key in gone:
                            s.remove(key)
                    one.buffer_size = 37
                for key in gone:
                    model.remove(key)
            elif op < 0.63:
                overlap = rng.rand() < 0.5 and live
                keys = [new_key() for _ in range(rng.randint(1, 15))]
                if overlap:
                    keys[0] = live[rng.randint(len(live))]
                rows = [new_row(step) for _ in keys]
                for one, other in zip(lshs, make()):
                    other.insert_bulk(keys, bulk_matrix(rows))
                    if overlap:
                        with pytest.raises(ValueError, match="overlapping"):
                            one.merge(other, check_overlap=True)
                    one.merge(other, check_overlap=not overlap)
                for key, row in zip(keys, rows):
                    model.insert(key, row)
            elif op < 0.66 and live:
                key, row = live[rng.randint(len(live))], new_row(step)  # a duplicate under check_duplication=False
                for one in lshs:
                    with pytest.raises(ValueError, match="already exists"):
                        one.insert(key, obj(row))
                    one.insert(key, obj(row), check_duplication=False)
                model.insert(key, row)
            elif op < 0.69 and live:
                key = live[rng.randint(len(live))]  # removed, then back with a new signature
                row = new_row(step)
                for one in lshs:
                    one.remove(key)
                    one.insert(key, obj(row))
                model.remove(key)
                model.insert(key, row)
            else:
                probe = new_row(step) if rng.rand() < 0.5 or not live else None
                if probe is None:
                    key = live[rng.randint(len(live))]
                    probe = new_row(step)
                    probe[: r * words] = bases[0, : r * words]
                want = model.query(probe)
                for one in lshs:
                    assert set(one.query(obj(probe))) == want, step
                    if rng.rand() < 0.3:
                        assert set(one.query_bulk(bulk_matrix([probe]))[0]) == want, step
            if step % 97 == 0:
                for one in lshs:
                    assert one.is_empty() == (not model.rows)
                    some = list(model.rows)[:3] + ["never-inserted"]
                    assert all((k in one) == (k in model.rows) for k in some)
                    assert one.get_counts() == model.counts()
                    assert one.get_subset_counts(*some) == model.counts(some)
            if after_op is not None:
                after_op(lshs, step)
    finally:
        MinHashLSH._compact = original
    assert compactions[0] >= 3 * len(lshs), compactions
    return lshs


@pytest.mark.parametrize("variant,prepickle", [("u32", False), ("u32", True), ("u64", False), ("u64", True), ("weighted", False),
                                               ("weighted", True)])
def test_differential_against_a_dict_model(variant, prepickle):
    lshs = run_differential(["disable"], variant, prepickle, seed=1 + ["u32", "u64", "weighted"].index(variant))
    dtype = lshs[0]._backend.dtype
    assert dtype == (np.uint32 if variant == "u32" else np.uint64)


# ---- the reference, where its checkout is mounted -----------------------------------------------------------------------
def _reference_lsh():
    """The reference's datasketch.lsh module, imported from its checkout and then removed from sys.modules again."""
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "datasketch" or k.startswith("datasketch.")}
    sys.path.insert(0, REFERENCE)
    try:
        return importlib.import_module("datasketch.lsh"), importlib.import_module("datasketch.minhash")
    finally:
        sys.path.remove(REFERENCE)
        for k in [k for k in sys.modules if k == "datasketch" or k.startswith("datasketch.")]:
            del sys.modules[k]
        sys.modules.update(saved)


needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "datasketch")), reason="reference repository not mounted")


@needs_reference
def test_optimal_params_equal_the_reference():
    ref, _ = _reference_lsh()
    for num_perm in (16, 64, 128, 256):
        for weights in ((0.5, 0.5), (0.3, 0.7)):
            for threshold in np.round(np.arange(0.05, 0.951, 0.1), 2):
                assert L._optimal_param(threshold, num_perm, *weights) == ref._optimal_param(threshold, num_perm, *weights), (
                    threshold, num_perm, weights)


def _error(call):
    try:
        call()
    except Exception as e:  # noqa: BLE001 -- the type and message are what is compared
        return type(e), str(e)
    return None


@needs_reference
def test_exceptions_equal_the_reference():
    ref, ref_mh = _reference_lsh()
    for kw in (dict(threshold=1.5), dict(threshold=-0.1), dict(num_perm=1), dict(weights=(1.2, -0.2)), dict(weights=(0.3, 0.3)),
               dict(num_perm=128, params=(10, 20)), dict(num_perm=128, params=(1, 4))):
        assert _error(lambda: MinHashLSH(gpu_mode="disable", **kw)) == _error(lambda: ref.MinHashLSH(**kw)), kw
    rows = np.random.RandomState(0).randint(0, 2**32, (3, 16)).astype(np.uint64)
    ours, theirs = MinHashLSH(threshold=0.5, num_perm=16, gpu_mode="disable"), ref.MinHashLSH(threshold=0.5, num_perm=16)
    for one, mh in ((ours, MinHash), (theirs, ref_mh.MinHash)):
        one.insert("a", mh(num_perm=16, hashvalues=rows[0]))
    other_params = (MinHashLSH(num_perm=16, params=(4, 4), gpu_mode="disable"), ref.MinHashLSH(num_perm=16, params=(4, 4)))
    overlapping = (MinHashLSH(threshold=0.5, num_perm=16, gpu_mode="disable"), ref.MinHashLSH(threshold=0.5, num_perm=16))
    for one, mh in zip(overlapping, (MinHash, ref_mh.MinHash)):
        one.insert("a", mh(num_perm=16, hashvalues=rows[1]))
    calls = [
        lambda one, mh, i: one.insert("b", mh(num_perm=18)),
        lambda one, mh, i: one.insert("a", mh(num_perm=16, hashvalues=rows[2])),
        lambda one, mh, i: one.query(mh(num_perm=18)),
        lambda one, mh, i: one.add_to_query_buffer(mh(num_perm=18)),
        lambda one, mh, i: one.remove("c"),
        lambda one, mh, i: one.merge(other_params[i]),
        lambda one, mh, i: one.merge(object()),
        lambda one, mh, i: one.merge(overlapping[i], check_overlap=True),
    ]
    for call in calls:
        got = _error(lambda: call(ours, MinHash, 0))
        assert got is not None and got == _error(lambda: call(theirs, ref_mh.MinHash, 1))


REFERENCE_CASES = ["TestMinHashLSH.test_init", "TestMinHashLSH.test_query", "TestMinHashLSH.test_query_buffer",
                   "TestMinHashLSH.test_query_buffer_matches_query_candidates", "TestMinHashLSH.test_pickle",
                   "TestMinHashLSH.test_get_counts", "TestWeightedMinHashLSH.test_init", "TestWeightedMinHashLSH.test_query",
                   "TestWeightedMinHashLSH.test_pickle"]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "test")), reason="reference repository not mounted")
def test_reference_lsh_cases_run_on_this_index():
    """The reference's own test/test_lsh.py cases that use only the public API, with datasketch.lsh aliased to this module."""
    import datasketch_amd
    from datasketch_amd import b_bit_minhash, hashfunc, lean_minhash, minhash, weighted_minhash

    prefixes = ("datasketch", "test")
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k.split(".")[0] in prefixes}
    sys.modules.update({"datasketch": datasketch_amd, "datasketch.minhash": minhash, "datasketch.lean_minhash": lean_minhash,
                        "datasketch.weighted_minhash": weighted_minhash, "datasketch.b_bit_minhash": b_bit_minhash,
                        "datasketch.hashfunc": hashfunc, "datasketch.lsh": L})
    stub = "mockredis" not in sys.modules
    if stub:  # not installed here; only the Redis-storage cases use it
        sys.modules["mockredis"] = types.ModuleType("mockredis")
    sys.path.insert(0, REFERENCE)
    try:
        mod = importlib.import_module("test.test_lsh")
        assert mod.MinHashLSH is MinHashLSH
        suite = unittest.TestSuite(unittest.defaultTestLoader.loadTestsFromName(name, mod) for name in REFERENCE_CASES)
        assert suite.countTestCases() == len(REFERENCE_CASES)
        result = unittest.TextTestRunner(verbosity=0).run(suite)
        problems = [f"{t}: {tb.splitlines()[-1]}" for t, tb in result.failures + result.errors]
        assert not problems, problems
    finally:
        sys.path.remove(REFERENCE)
        if stub:
            del sys.modules["mockredis"]
        for k in [k for k in sys.modules if k.split(".")[0] in prefixes]:
            del sys.modules[k]
        sys.modules.update(saved)


# ---- pickling, lsh_bulk, storage ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("prepickle", [False, True])
def test_pickle_round_trip_answers_identically(prepickle):
    sig, keys, probes = batch_inputs(prepickle)
    one = MinHashLSH(threshold=0.6, num_perm=64, prepickle=prepickle, gpu_mode="disable")
    one.insert_bulk(keys, sig)
    for key in keys[::5]:
        one.remove(key)
    one.insert(keys[1], MinHash(num_perm=64, hashvalues=sig[2]), check_duplication=False)
    two = pickle.loads(pickle.dumps(one))
    assert [sorted(map(repr, a)) for a in one.query_bulk(probes)] == [sorted(map(repr, a)) for a in two.query_bulk(probes)]
    assert one.get_counts() == two.get_counts() and (keys[1] in two) and (keys[0] not in two)
    two.remove(keys[1])
    assert keys[1] not in two and all(keys[1] not in a for a in two.query_bulk(probes))


def test_lsh_bulk_hands_the_index_to_its_own_bulk_methods():
    sig, keys, probes = batch_inputs(False)
    one = MinHashLSH(threshold=0.6, num_perm=64, gpu_mode="disable")
    two = MinHashLSH(threshold=0.6, num_perm=64, gpu_mode="disable")
    LB.insert_bulk(one, keys, sig, gpu_mode="disable")
    two.insert_bulk(keys, sig)
    assert [sorted(a) for a in LB.query_bulk(one, probes, gpu_mode="disable")] == [sorted(a) for a in two.query_bulk(probes)]
    with pytest.raises(ValueError, match="already exists"):
        LB.insert_bulk(one, keys[:1], sig[:1], gpu_mode="disable")


def test_storage_and_bulk_argument_checks():
    with pytest.raises(ValueError, match="in-memory storage"):
        MinHashLSH(threshold=0.5, num_perm=16, storage_config={"type": "redis", "redis": {}}, gpu_mode="disable")
    one = MinHashLSH(threshold=0.5, num_perm=16, storage_config={"type": "dict"}, gpu_mode="disable")
    assert one.is_empty() and one.query(MinHash(16)) == [] and one.get_counts() == [{} for _ in range(one.b)]
    sig = np.random.RandomState(0).randint(0, 2**32, (4, 16)).astype(np.uint64)
    with pytest.raises(ValueError, match="already exists"):
        one.insert_bulk(["a", "a"], sig[:2])  # twice in one batch
    with pytest.raises(ValueError, match="Expecting minhash"):
        one.insert_bulk(["a"], sig[:1, :8])
    assert one.is_empty()
    one.insert_bulk(["a", "a"], sig[:2], check_duplication=False)
    assert one.query_bulk(sig[:2]) == [["a"], ["a"]]
    one.remove("a")
    assert one.is_empty() and one.query_bulk(sig[:2]) == [[], []]


# ---- the caller's arrays, failures, key ids ---------------------------------------------------------------------------
def caller_buffer_reuse(gpu_mode, kind):
    """insert_bulk takes the values at call time: a buffer refilled between two calls (before any flush) changes nothing."""
    rng = np.random.RandomState(4)
    a = rng.randint(0, 2**32, (4, 16)).astype(np.uint64)
    b = rng.randint(0, 2**32, (4, 16)).astype(np.uint64)
    if kind == "weighted":
        a, b = a.view(np.int64).reshape(4, 8, 2), b.view(np.int64).reshape(4, 8, 2)
    elif kind == "u32":
        a, b = a.astype(np.uint32), b.astype(np.uint32)
    num_perm = 8 if kind == "weighted" else 16
    one = MinHashLSH(num_perm=num_perm, params=(4, 2), gpu_mode=gpu_mode)
    buf = a.copy()
    one.insert_bulk([f"a{i}" for i in range(4)], buf)
    buf[:] = b
    one.insert_bulk([f"b{i}" for i in range(4)], buf)
    buf[:] = 0
    assert one._pending  # both batches were still pending when the buffer changed
    assert one.query_bulk(a[:1]) == [["a0"]] and one.query_bulk(b[:1]) == [["b0"]]


@pytest.mark.parametrize("kind", ["u32", "u64", "weighted"])
def test_insert_bulk_takes_the_values_at_call_time(kind):
    caller_buffer_reuse("disable", kind)


class _StubBuffer:
    def __init__(self, nbytes):
        self.mem = np.zeros(nbytes, dtype=np.uint8)
        self.nbytes, self.ptr = nbytes, id(self)

    def upload(self, arr, offset=0):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.mem[offset : offset + raw.size] = raw

    def download(self, shape, dtype, offset=0):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.mem[offset : offset + n].copy().view(dtype).reshape(shape)


class _StubContext:
    """Device memory in host arrays; alloc fails while `fail` is set (an out-of-memory device)."""

    fail = False

    def alloc(self, nbytes):
        if self.fail:
            raise MemoryError("out of device memory")
        return _StubBuffer(nbytes)

    def synchronize(self):
        pass


def test_a_failed_widen_leaves_the_device_back_end_as_it_was():
    ctx = _StubContext()
    be = L._DeviceBands(ctx, 8, 2, 4, np.uint32)
    rows = np.arange(24, dtype=np.uint32).reshape(3, 8)
    be.d_sig, be.capacity, be.n = ctx.alloc(4 * be.row_bytes), 4, 3
    be.d_sig.upload(rows)
    before = be.d_sig
    ctx.fail = True
    with pytest.raises(MemoryError):
        be.widen()
    assert be.dtype == np.uint32 and be.d_sig is before and be.row_bytes == 32
    assert np.array_equal(be.matrix(), rows)
    ctx.fail = False
    be.widen()
    assert be.dtype == np.uint64 and be.d_sig.nbytes == 4 * 64 and np.array_equal(be.matrix(), rows.astype(np.uint64))


def test_key_ids_of_removed_keys_are_dropped():
    rng = np.random.RandomState(6)
    one = MinHashLSH(num_perm=16, params=(4, 4), gpu_mode="disable")
    live = {}
    for step in range(40):
        keys = [f"k{step}-{i}" for i in range(50)]
        sig = rng.randint(0, 2**32, (50, 16)).astype(np.uint64)
        one.insert_bulk(keys, sig)
        live.update(zip(keys, sig))
        for key in list(live)[: 45]:
            one.remove(key)
            del live[key]
        one.flush()
    assert len(one._kid_key) <= 3 * len(live) + 100  # not the 2 000 keys ever inserted
    probe = np.stack(list(live.values()))
    assert [a for a in one.query_bulk(probe)] == [[k] for k in live]
    assert one.get_counts() == DictModelFrom(live).counts()


def DictModelFrom(live):
    model = DictModel(4, 4, 1)
    for key, row in live.items():
        model.insert(key, row)
    return model
