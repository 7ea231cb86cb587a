"""Consumer-side bulk helpers (datasketch_amd/lsh_bulk.py): band keys, digests, bulk LSH insert,
candidate pairs, batched Jaccard.  The CPU tests use the numpy fallbacks.  Where the reference's own
MinHashLSH is the oracle, its index -- built key by key from the same seeded inputs -- is pinned in
tests/golden/lsh_index.json (oracle/gen_golden_lsh.py): its (b, r), a sha256 of its dictionaries and of
its answers to the probes."""
import collections
import hashlib
import json
import os
import pickle

import numpy as np
import pytest

from datasketch_amd import MinHash, prehashed
from datasketch_amd import lsh_bulk as LB

GOLDEN_LSH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lsh_index.json")


def lsh_golden(case):
    with open(GOLDEN_LSH) as f:
        return json.load(f)[case]


class _DictStore:
    """The reference's in-memory storage as insert_bulk / query_bulk recognise it: a defaultdict behind ``_dict``."""

    def __init__(self, factory):
        self._dict = collections.defaultdict(factory)

    def __contains__(self, key):
        return key in self._dict


class _DictIndex:
    """The attributes of a reference MinHashLSH over the in-memory storage, with the (b, r) the reference chose."""

    def __init__(self, h, b, r, prepickle=False, hashfunc=None):
        self.h, self.b, self.r, self.prepickle, self.hashfunc = h, b, r, prepickle, hashfunc
        self.keys = _DictStore(list)
        self.hashtables = [_DictStore(set) for _ in range(b)]


def _sha(obj):
    return hashlib.sha256(repr(obj).encode()).hexdigest()


def index_digest(lsh):
    """sha256 of an index's dictionaries in a canonical order (keys unpickled, so the pickle protocol does not enter)."""
    key = pickle.loads if lsh.prepickle else (lambda k: k)
    keys = sorted((repr(key(k)), [repr(h) for h in hs]) for k, hs in lsh.keys._dict.items())
    tables = [sorted((repr(h), sorted(repr(key(k)) for k in members)) for h, members in t._dict.items()) for t in lsh.hashtables]
    return _sha((keys, tables))


def results_digest(results):
    """sha256 of query answers, each taken as the set it is."""
    return _sha([sorted(map(repr, res)) for res in results])


def _signatures(n=300, t=40, k=64, seed=0, dup_every=7):
    rng = np.random.RandomState(seed)
    tok = rng.randint(0, 2**32, (n, t), dtype=np.uint64)
    tok[dup_every::dup_every] = tok[0:1]  # clusters of identical sets
    near = tok[1].copy()
    near[:4] = rng.randint(0, 2**32, 4, dtype=np.uint64)
    tok[2] = near  # a near duplicate of row 1
    return MinHash.bulk_signatures(tok, num_perm=k, seed=1, hashfunc=prehashed, gpu_mode="disable")


def test_band_keys_are_the_reference_key_bytes():
    sig = _signatures()
    keys = LB.band_keys(sig, 8, 8, gpu_mode="disable")
    assert keys.shape == (sig.shape[0], 8)
    for i in (0, 5, 299):
        for j in (0, 3, 7):
            assert bytes(keys[i, j]) == bytes(sig[i, j * 8 : (j + 1) * 8].byteswap().data)  # lsh.py:537-538
    assert keys.T.tolist()[2][5] == bytes(keys[5, 2])
    with pytest.raises(ValueError):
        LB.band_keys(sig, 9, 8, gpu_mode="disable")


def test_band_digests_are_fnv1a_of_the_key_bytes():
    sig = _signatures(n=50)
    dig = LB.band_digests(sig, 4, 16, gpu_mode="disable")
    keys = LB.band_keys(sig, 4, 16, gpu_mode="disable")
    for i in (0, 7, 49):
        for j in range(4):
            assert int(dig[i, j]) == LB.fnv1a_64(bytes(keys[i, j]))
    assert LB.fnv1a_64(b"") == 0xCBF29CE484222325 and LB.fnv1a_64(b"a") == 0xAF63DC4C8601EC8C  # published test vectors


def test_candidate_pairs_and_jaccard_pairs():
    sig = _signatures()
    pairs = LB.candidate_pairs(sig, 16, 4, gpu_mode="disable")
    # brute force: rows sharing any band
    bands = sig[:, : 16 * 4].reshape(sig.shape[0], 16, 4)
    want = set()
    for i in range(sig.shape[0]):
        same = np.any(np.all(bands[i][None] == bands, axis=2), axis=1)
        want.update((i, int(j)) for j in np.flatnonzero(same) if j > i)
    assert set(map(tuple, pairs.tolist())) == want and len(pairs) == len(want)
    jac = LB.jaccard_pairs(sig, pairs, gpu_mode="disable")
    for (i, j), est in list(zip(pairs.tolist(), jac))[:200]:
        a, b = MinHash(seed=1, hashvalues=sig[i]), MinHash(seed=1, hashvalues=sig[j])
        assert est == a.jaccard(b)
    assert LB.jaccard_pairs(sig, np.empty((0, 2), np.int64), gpu_mode="disable").size == 0


@pytest.mark.parametrize("prepickle,use_hashfunc", [(False, False), (True, False), (False, True)])
def test_insert_bulk_leaves_the_reference_index_in_the_same_state(prepickle, use_hashfunc):
    """insert_bulk leaves the dictionaries the reference's per-key MinHashLSH.insert leaves (threshold 0.5, num_perm 64)."""
    gold = lsh_golden(f"insert-{int(prepickle)}{int(use_hashfunc)}")
    sig = _signatures(n=200, k=64)
    keys = [f"doc-{i}" for i in range(sig.shape[0])]
    bulk = _DictIndex(64, gold["b"], gold["r"], prepickle, LB.fnv1a_64 if use_hashfunc else None)
    LB.insert_bulk(bulk, keys, sig, gpu_mode="disable")
    assert index_digest(bulk) == gold["index_sha256"]
    got = LB.query_bulk(bulk, sig[:1], gpu_mode="disable")
    assert results_digest(got) == gold["query_sha256"] and len(got[0]) > 1
    with pytest.raises(ValueError):
        LB.insert_bulk(bulk, keys[:1], sig[:1], gpu_mode="disable")  # duplicate key
    with pytest.raises(ValueError):
        LB.insert_bulk(bulk, ["x"], sig[:1, :32], gpu_mode="disable")  # wrong length
    if use_hashfunc:  # the digests are what the index stores
        dig = LB.band_digests(sig, bulk.b, bulk.r, gpu_mode="disable")
        assert set(bulk.hashtables[0]._dict) == set(int(x) for x in dig[:, 0])


def _weighted_signatures(n=60, dim=32, s=16):
    from datasketch_amd import WeightedMinHashGenerator

    g = WeightedMinHashGenerator(dim, s, seed=3, gpu_mode="disable")
    x = np.random.RandomState(0).uniform(0, 5, (n, dim)).astype(np.float32)
    x[7] = x[3]
    x[11, :4] += 1.0
    wm = g.minhash_many(x)
    return wm, np.stack([w.hashvalues for w in wm])


def test_weighted_signatures_go_through_the_same_helpers():
    """An [N, S, 2] int64 WeightedMinHash matrix: a band key is the 16*r bytes the reference builds from
    hashvalues[i*r:(i+1)*r] (lsh.py:537-538 on an [r, 2] int64 slice)."""
    wm, sig = _weighted_signatures()
    assert sig.shape == (60, 16, 2) and sig.dtype == np.int64
    keys = LB.band_keys(sig, 4, 4, gpu_mode="disable")
    for i in (0, 5, 59):
        for j in range(4):
            assert bytes(keys[i, j]) == bytes(sig[i, j * 4 : (j + 1) * 4].byteswap().data)
    dig = LB.band_digests(sig, 4, 4, gpu_mode="disable")
    assert int(dig[5, 2]) == LB.fnv1a_64(bytes(keys[5, 2]))
    pairs = LB.candidate_pairs(sig, 4, 4, gpu_mode="disable")
    assert [3, 7] in pairs.tolist()
    jac = LB.weighted_jaccard_pairs(sig, pairs)
    for (i, j), est in zip(pairs.tolist(), jac):
        assert est == wm[i].jaccard(wm[j])
    with pytest.raises(ValueError):
        LB.jaccard_pairs(sig, pairs, gpu_mode="disable")
    with pytest.raises(ValueError):
        LB.band_keys(sig, 5, 4, gpu_mode="disable")  # 5 * 4 > 16 samples


def test_insert_bulk_of_weighted_signatures_matches_the_reference_index():
    """Weighted signatures under integer keys: the reference's index of ref.WeightedMinHash(3, hashvalues) per key."""
    gold = lsh_golden("weighted")
    wm, sig = _weighted_signatures()
    bulk = _DictIndex(16, gold["b"], gold["r"])
    LB.insert_bulk(bulk, list(range(len(wm))), sig, gpu_mode="disable")
    assert index_digest(bulk) == gold["index_sha256"]
    got = LB.query_bulk(bulk, sig[3:4], gpu_mode="disable")
    assert results_digest(got) == gold["query_sha256"] and 7 in got[0]
    with pytest.raises(ValueError):
        LB.insert_bulk(bulk, ["x"], sig[:1, :8], gpu_mode="disable")  # wrong sample count


def batch_inputs(prepickle):
    """Signatures (whole rows again across the batch boundary, a big bucket, a near duplicate), keys and 1000 probes."""
    rng = np.random.RandomState(3)
    n, k = 1500, 64
    sig = rng.randint(0, 2**32, (n, k)).astype(np.uint64)
    sig[700:760] = sig[0:60]            # whole rows again, across the batch boundary
    sig[900:940, :32] = sig[5, :32]     # a big bucket in the first bands
    sig[1200, 16:] = sig[1100, 16:]     # a near duplicate inside the second batch
    keys = [("doc", i) for i in range(n)] if prepickle else [b"doc-%d" % i for i in range(n)]
    probes = sig[rng.randint(0, n, 1000)].copy()
    probes[::3, rng.randint(0, k, 20)] = 7          # perturbed probes: some bands still match
    probes[1::50] = rng.randint(0, 2**32, (20, k))  # probes that match nothing
    return sig, keys, probes


@pytest.mark.parametrize("prepickle", [True, False])
def test_insert_bulk_in_batches_and_query_bulk_equal_the_per_key_calls(prepickle):
    """Two bulk batches (the second onto a non-empty index, with band keys shared inside the batch and with the
    first batch) leave every dictionary as the reference's per-key loop does; query_bulk == [lsh.query(m) for m in
    probes] for 1000 probes (ref: datasketch/lsh.py:326-347, 370-431; storage.py:210-259)."""
    gold = lsh_golden(f"batches-{int(prepickle)}")
    sig, keys, probes = batch_inputs(prepickle)
    bulk = _DictIndex(64, gold["b"], gold["r"], prepickle)
    LB.insert_bulk(bulk, keys[:800], sig[:800], gpu_mode="disable")
    LB.insert_bulk(bulk, keys[800:], sig[800:], gpu_mode="disable")
    assert index_digest(bulk) == gold["index_sha256"]
    got = LB.query_bulk(bulk, probes, gpu_mode="disable")
    assert len(got) == 1000
    assert results_digest(got) == gold["query_sha256"]
    assert any(len(r) > 30 for r in got) and any(len(r) == 0 for r in got)
    with pytest.raises(ValueError):
        LB.query_bulk(bulk, probes[:, :32], gpu_mode="disable")
    with pytest.raises(ValueError):
        LB.insert_bulk(bulk, keys[10:12], sig[10:12], gpu_mode="disable")   # present already
    with pytest.raises(ValueError):
        LB.insert_bulk(bulk, [keys[0] + (1,) if prepickle else b"x", keys[0] + (1,) if prepickle else b"x"], sig[:2], gpu_mode="disable")  # twice in one batch


class _ListStore:
    """A storage that is NOT the in-memory dict one (no _dict): insert_bulk / query_bulk must go through
    its API key by key (what a Redis / Cassandra back end gets, ref: storage.py)."""

    def __init__(self, factory):
        self.data, self.factory, self.calls = {}, factory, 0

    def insert(self, key, *vals, **kwargs):
        self.calls += 1
        box = self.data.setdefault(key, self.factory())
        (box.extend if isinstance(box, list) else box.update)(vals)

    def get(self, key):
        return self.data.get(key, self.factory())

    def __contains__(self, key):
        return key in self.data


def test_other_storages_take_the_per_key_path():
    sig = _signatures(n=120, k=64)

    class Index:
        h, b, r, prepickle, hashfunc = 64, 8, 8, False, None

        def __init__(self):
            self.keys = _ListStore(list)
            self.hashtables = [_ListStore(set) for _ in range(8)]

    idx = Index()
    keys = [b"k%d" % i for i in range(120)]
    LB.insert_bulk(idx, keys, sig, gpu_mode="disable")
    assert idx.keys.calls == 120 and all(t.calls == 120 for t in idx.hashtables)
    bk = LB.band_keys(sig, 8, 8, gpu_mode="disable")
    assert idx.keys.data[keys[3]] == [bytes(bk[3, j]) for j in range(8)]
    assert keys[7] in idx.hashtables[2].data[bytes(bk[7, 2])]
    got = LB.query_bulk(idx, sig[:10], gpu_mode="disable")
    assert all(keys[i] in got[i] for i in range(10)) and set(got[0]) >= {keys[0], keys[7], keys[14]}  # rows 0, 7, 14 ... are identical sets
    with pytest.raises(ValueError):
        LB.insert_bulk(idx, keys[:1], sig[:1], gpu_mode="disable")


def test_insert_bulk_settle_choices(monkeypatch):
    """The new containers are settled as asked: one full collection, gc.freeze(), or nothing -- and only when the
    collector was on and the batch is big enough to matter."""
    import collections
    import gc

    class Store:
        def __init__(self, factory):
            self._dict = collections.defaultdict(factory)

    class Index:
        h, b, r, prepickle, hashfunc = 64, 8, 8, False, None

        def __init__(self):
            self.keys = Store(list)
            self.hashtables = [Store(set) for _ in range(8)]

    sig = _signatures(n=120, k=64)
    keys = [b"k%d" % i for i in range(120)]
    calls = []
    monkeypatch.setattr(gc, "collect", lambda *a: calls.append("collect") or 0)
    monkeypatch.setattr(gc, "freeze", lambda: calls.append("freeze"))
    monkeypatch.setattr(LB, "_SETTLE_MIN_KEYS", 100)
    states = []
    for settle in ("collect", "freeze", "leave"):
        idx = Index()
        LB.insert_bulk(idx, keys, sig, gpu_mode="disable", settle=settle)
        states.append(dict(idx.hashtables[3]._dict))
    assert calls == ["collect", "freeze"] and states[0] == states[1] == states[2]
    monkeypatch.setattr(LB, "_SETTLE_MIN_KEYS", 1000)
    LB.insert_bulk(Index(), keys, sig, gpu_mode="disable")
    assert calls == ["collect", "freeze"]  # small batch: left alone
    assert gc.isenabled()
    with pytest.raises(ValueError):
        LB.insert_bulk(Index(), keys, sig, gpu_mode="disable", settle="later")
