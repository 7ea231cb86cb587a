"""MinHashLSHBloom on the host: the reference's own tests, the numpy twin against a plain-Python model, the sizing, the measured
false-positive count, a differential against the reference's class on an exact stand-in filter, and the class's own behaviour."""
import importlib
import importlib.util
import json
import math
import os
import pickle
import re
import sys
import unittest
import warnings

import numpy as np
import pytest

from datasketch_amd import BloomTable, MinHash, MinHashLSHBloom, _native
from datasketch_amd import lsh_bloom as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsh_bloom.json")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "test")), reason="reference repository not mounted")

M64 = (1 << 64) - 1
M61 = (1 << 61) - 1


def _gen():
    spec = importlib.util.spec_from_file_location("gen_golden_bloom", os.path.join(ROOT, "tools", "gen_golden_bloom.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def quiet(**kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kw.setdefault("gpu_mode", "disable")
        return MinHashLSHBloom(**kw)


# ---- the reference's own test file --------------------------------------------------------------------------------------
@needs_reference
def test_reference_test_lshbloom_passes_on_this_package(tmp_path, monkeypatch):
    import datasketch_amd
    from datasketch_amd import minhash

    monkeypatch.chdir(tmp_path)  # the file writes ./test_save/
    mine = lambda k: k == "datasketch" or k.startswith("datasketch.") or k == "test" or k.startswith("test.")  # noqa: E731
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if mine(k)}
    sys.modules.update({"datasketch": datasketch_amd, "datasketch.lsh_bloom": B, "datasketch.minhash": minhash})
    sys.path.insert(0, REFERENCE)
    try:
        mod = importlib.import_module("test.test_lshbloom")
        assert mod.MinHashLSHBloom is MinHashLSHBloom and mod.BloomTable is BloomTable
        suite = unittest.defaultTestLoader.loadTestsFromModule(mod)
        assert suite.countTestCases() == 8
        result = unittest.TextTestRunner(verbosity=0).run(suite)
        problems = [f"{t}: {tb.splitlines()[-1]}" for t, tb in result.failures + result.errors]
        assert not problems, problems
    finally:
        sys.path.remove(REFERENCE)
        for k in [k for k in sys.modules if mine(k)]:
            del sys.modules[k]
        sys.modules.update(saved)
        if os.path.exists("/tmp/bloomfilter.bf"):  # written by the reference's TestBloomTable.test_save
            os.remove("/tmp/bloomfilter.bf")


# ---- the twin against a plain-Python model ------------------------------------------------------------------------------
def model_key(values):
    return (sum(int(v) for v in values) & M64) % M61


def model_bits(x, n_blocks, k):
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
        return z ^ (z >> 31)

    s = (x + 0x9E3779B97F4A7C15) & M64
    block = ((mix(s) >> 32) * n_blocks) >> 32
    words = [0] * 16
    for i in range(k):
        if i % 7 == 0:
            s = (s + 0x9E3779B97F4A7C15) & M64
            out = mix(s)
        pos = (out >> (9 * (i % 7))) & 511
        words[pos >> 5] |= 1 << (pos & 31)
    return block, words


def model_insert(sig, b, r, n_blocks, k):
    words = np.zeros((b, n_blocks, 16), dtype=np.uint32)
    for row in sig:
        for j in range(b):
            block, mask = model_bits(model_key(row[j * r: (j + 1) * r]), n_blocks, k)
            words[j, block] |= np.array(mask, dtype=np.uint32)
    return words


def edge_rows():
    """uint64 rows of 4 columns (one band of r = 4) whose sum wraps 2^64 or lands on 2^61 - 1, 2^61, 2^61 + 1, 0 and 2^64 - 1."""
    rows = [[M64, 1, 0, 0], [M64, M64, M64, M64], [1 << 63, 1 << 63, 5, 0], [M61, 0, 0, 0], [M61 - 3, 1, 1, 1], [1 << 61, 0, 0, 0],
            [(1 << 61) + 1, 0, 0, 0], [0, 0, 0, 0], [M64, 0, 0, 0], [2 * M61, 0, 0, 0], [8 * M61 + 7, 0, 0, 0], [1 << 60, 1 << 60, 1, 0]]
    return np.array(rows, dtype=np.uint64)


def test_band_keys_of_the_edge_rows_match_python_integers():
    rows = edge_rows()
    got = B.band_keys(rows, 1, 4)[:, 0].tolist()
    assert got == [model_key(r) for r in rows.tolist()]
    assert 0 in got and model_key([M61, 0, 0, 0]) == 0 and model_key([1 << 61]) == 1 and model_key([M64, 1]) == 0


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
@pytest.mark.parametrize("b,r,n_blocks,k", [(2, 1, 1, 1), (3, 5, 3, 7), (3, 5, 2, 8), (2, 4, 1000, 14), (4, 4, 3, 15), (2, 8, 7, 32)])
def test_twin_equals_the_python_model(dtype, b, r, n_blocks, k):
    rng = np.random.RandomState(b * 100 + k)
    hi = 2**32 if dtype == np.uint32 else 2**64
    sig = rng.randint(0, hi, size=(40, b * r + 1), dtype=np.uint64).astype(dtype)
    if dtype == np.uint64 and r == 4:
        sig = np.vstack([sig, np.hstack([np.tile(edge_rows(), (1, b)), np.zeros((len(edge_rows()), 1), dtype=np.uint64)])])
    words = np.zeros((b, n_blocks, 16), dtype=np.uint32)
    B.insert_host(words, sig, r, k)
    assert np.array_equal(words, model_insert(sig.tolist(), b, r, n_blocks, k))
    assert B.query_host(words, sig, r, k).all()
    for x in B.band_keys(sig, b, r).reshape(-1)[:20].tolist():
        block, mask = B.block_masks(np.array([x], dtype=np.uint64), n_blocks, k)
        assert (int(block[0]), mask[0].tolist()) == model_bits(x, n_blocks, k)


# ---- sizing -------------------------------------------------------------------------------------------------------------
SIZES = [(10, 0.01, 2, 1), (1000, 0.01, 5, 20), (20000, 0.001, 9, 606), (20000, 0.0001, 12, 857), (100000, 0.01, 6, 1933)]


@pytest.mark.parametrize("n,fp,k,n_blocks", SIZES)
def test_sizing_table(n, fp, k, n_blocks):
    assert B.bloom_size(n, fp) == (k, n_blocks)
    assert B.fp_blocked(n, n_blocks, k) <= fp
    assert n_blocks == 1 or B.fp_blocked(n, n_blocks - 1, k) > fp


def test_fp_blocked_falls_as_blocks_are_added_and_sizing_is_quick():
    for n, k in ((1000, 5), (20000, 9), (100000, 6)):
        rates = [B.fp_blocked(n, nb, k) for nb in (1, 2, 3, 10, 50, 200, 1000, 5000, 10**5, 10**7)]
        # a full block answers 1 up to the rounding of the Poisson weights (their float64 sum is 1 +- 1e-10): never rising
        # beyond that, and strictly falling once the rate has left 1
        assert all(a + 1e-9 >= b for a, b in zip(rates, rates[1:])), rates
        assert all(a > b for a, b in zip(rates, rates[1:]) if a < 0.999), rates
        assert rates[0] > 0.999 and rates[-1] < 1e-6
    k, nb = B.bloom_size(10**9, 1e-5)  # a filter of several GB per band: the search does not grow with n
    assert 1 <= k <= 32 and nb < 2**32 and B.fp_blocked(10**9, nb, k) <= 1e-5 < B.fp_blocked(10**9, nb - 1, k)


def test_measured_false_positive_count():
    n, fp, Q = 20000, 1e-3, 400000
    k, nb = B.bloom_size(n, fp)
    rng = np.random.RandomState(1)
    ins = rng.randint(0, 2**32, size=(n, 4), dtype=np.uint64)
    fresh = rng.randint(0, 2**32, size=(Q, 4), dtype=np.uint64)
    fresh[:, 0] += np.uint64(1 << 40)  # no key of the queries is a key of the inserts
    words = np.zeros((1, nb, 16), dtype=np.uint32)
    B.insert_host(words, ins, 4, k)
    assert B.query_host(words, ins, 4, k).all()
    count = int(B.query_host(words, fresh, 4, k).sum())
    print("false positives:", count)
    assert count <= Q * fp + 6 * math.sqrt(Q * fp)  # = 520


# ---- against the reference's class on an exact stand-in for pybloomfilter -----------------------------------------------
@needs_reference
def test_differential_against_the_reference_on_an_exact_filter():
    gen = _gen()
    ref = gen.reference_module(REFERENCE)
    num_perm, params, fp = 32, (8, 4), 1e-3
    ins, q = gen.corpus(5, 2000, 5000, num_perm, *params)
    exact = np.array(gen.exact_answers(ref, ins, q, num_perm, params, 2000, fp))
    lsh = quiet(num_perm=num_perm, n=2000, fp=fp, params=params)
    lsh.insert_bulk(ins)
    ours = lsh.query_bulk(q)
    assert ours[exact].all(), "a query the exact reference answers True was missed"
    m = int((~exact).sum()) * (1 - (1 - fp) ** params[0])
    extra = int((ours & ~exact).sum())
    print("exact positives", int(exact.sum()), "extra positives", extra, "allowed", m + 6 * math.sqrt(m))
    assert extra <= m + 6 * math.sqrt(m)


@needs_reference
def test_fixture_is_what_the_reference_answers():
    gen = _gen()
    doc = json.load(open(GOLDEN))
    ins, q = np.array(doc["inserted"], dtype=np.uint64), np.array(doc["queries"], dtype=np.uint64)
    ins2, q2 = gen.corpus(11, 100, 300, doc["num_perm"], *doc["params"])
    assert np.array_equal(ins, ins2) and np.array_equal(q, q2)
    assert gen.exact_answers(gen.reference_module(REFERENCE), ins, q, doc["num_perm"], tuple(doc["params"]), doc["n"], doc["fp"]) == doc["answers"]


def test_fixture_positives_are_found():
    doc = json.load(open(GOLDEN))
    lsh = quiet(num_perm=doc["num_perm"], n=doc["n"], fp=doc["fp"], params=tuple(doc["params"]))
    lsh.insert_bulk(np.array(doc["inserted"], dtype=np.uint64))
    ours = lsh.query_bulk(np.array(doc["queries"], dtype=np.uint64))
    exact = np.array(doc["answers"])
    assert exact.sum() == 200 and ours[exact].all()
    assert int((ours & ~exact).sum()) <= 3  # 100 exact negatives x (1 - (1 - 1e-3)^3) = 0.3 expected; + 6 sigma


# ---- the class ----------------------------------------------------------------------------------------------------------
def test_constructor_errors_and_warnings():
    for kw, msg in ((dict(threshold=1.5), "threshold must be in"), (dict(num_perm=1), "Too few permutation"), (dict(n=None), "n for LSHBloom"),
                    (dict(n=0), "n for LSHBloom"), (dict(fp=None), "fp must be in"), (dict(fp=1.0), "fp must be in"), (dict(fp=0.0), "fp must be in"),
                    (dict(weights=(-0.1, 1.1)), "Weight must be in"), (dict(weights=(0.5, 0.6)), "Weights must sum"),
                    (dict(params=(9, 2)), "The product of b and r in params is 9 \\* 2 = 18"), (dict(params=(1, 16)), "bands are too small")):
        args = dict(num_perm=16, n=10, fp=0.01, save_dir=None)
        args.update(kw)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(ValueError, match=msg):
                MinHashLSHBloom(gpu_mode="disable", **args)
    with pytest.raises(ValueError, match="gpu_mode"):
        quiet(num_perm=16, n=10, fp=0.01, gpu_mode="sometimes")
    with pytest.warns(RuntimeWarning, match="without save directory"):
        lsh = MinHashLSHBloom(num_perm=16, n=10, fp=0.01, params=(4, 4), gpu_mode="disable")
    assert (lsh.h, lsh.b, lsh.r) == (16, 4, 4) and len(lsh.hashtables) == 4 and lsh.hashranges == [(0, 4), (4, 8), (8, 12), (12, 16)]
    with pytest.warns(RuntimeWarning, match="no-op"):
        lsh.sync()
    with pytest.raises(ValueError, match="Expecting minhash with length 16, got 18"):
        lsh.insert(MinHash(18))

    class Weighted:
        hashvalues = np.zeros((16, 2), dtype=np.int64)

        def __len__(self):
            return 16

    with pytest.raises(ValueError, match="1-D"):
        lsh.insert(Weighted())
    with pytest.raises(ValueError, match="1-D"):
        lsh.query(Weighted())
    with pytest.raises(RuntimeError, match="Invalid length for indices, 2, expected 4"):
        lsh.hashtables[0].insert([1, 2])


def _rows(seed, n, k=16):
    return np.random.RandomState(seed).randint(0, 2**32, size=(n, k), dtype=np.uint64)


def test_staged_inserts_are_visible_and_tables_are_views():
    lsh = quiet(num_perm=16, n=100, fp=0.001, params=(4, 4))
    lsh.buffer_size = 3
    rows = _rows(1, 7)
    for i, row in enumerate(rows):
        m = MinHash(16, hashvalues=row)
        assert not lsh.query(m)
        lsh.insert(m)
        assert len(lsh._pending) == 1  # staged, and the query below flushes it
        assert lsh.query(m) and not lsh._pending
    more = _rows(9, 7)
    for i, row in enumerate(more):
        lsh.insert(MinHash(16, hashvalues=row))
        assert len(lsh._pending) == (i + 1) % 3  # flushed at buffer_size
    rows = np.vstack([rows, more])
    assert lsh.query_bulk(rows).all() and not lsh.query_bulk(_rows(2, 50)).any()
    for j, table in enumerate(lsh.hashtables):
        assert table.query(rows[0, 4 * j: 4 * j + 4]) and not table.query(rows[0, 4 * j: 4 * j + 4] + np.uint64(1))
        assert np.array_equal(table.words, lsh.words()[j])
    fresh = _rows(3, 1)[0]
    lsh.hashtables[2].insert(fresh[8:12])  # a table of the index writes the shared array
    assert lsh.query(MinHash(16, hashvalues=fresh))
    words = np.zeros((4, lsh.n_blocks, 16), dtype=np.uint32)
    B.insert_host(words, rows, 4, lsh.k)
    B.insert_host(words[2:3], fresh[8:12].reshape(1, 4), 4, lsh.k)
    assert np.array_equal(lsh.words(), words)


def test_query_insert_bulk_answers_against_the_state_before_the_call():
    lsh = quiet(num_perm=16, n=1000, fp=0.001, params=(4, 4))
    first, second = _rows(4, 100), _rows(5, 100)
    assert not lsh.query_insert_bulk(first).any()
    batch = np.vstack([first[:50], second, second])  # the repeated rows do not see each other within the call
    assert lsh.query_insert_bulk(batch).tolist() == [True] * 50 + [False] * 200
    assert lsh.query_bulk(second).all()
    uint32 = quiet(num_perm=16, n=1000, fp=0.001, params=(4, 4))
    uint32.insert_bulk(np.vstack([first, second]).astype(np.uint32))
    assert np.array_equal(uint32.words(), lsh.words())


def test_save_load_and_geometry_mismatch(tmp_path):
    d = str(tmp_path / "index")
    rows = _rows(6, 30)
    lsh = MinHashLSHBloom(num_perm=16, n=100, fp=0.001, params=(4, 4), save_dir=d, gpu_mode="disable")
    lsh.insert_bulk(rows)
    lsh.sync()
    assert sorted(os.listdir(d)) == [f"band-{i}.bf" for i in range(4)]
    assert os.path.getsize(os.path.join(d, "band-0.bf")) == 32 + lsh.n_blocks * 64
    again = MinHashLSHBloom(num_perm=16, n=100, fp=0.001, params=(4, 4), save_dir=d, gpu_mode="disable")
    assert np.array_equal(again.words(), lsh.words()) and again.query_bulk(rows).all()
    for kw in (dict(n=5000), dict(fp=0.1), dict(params=(4, 3))):
        args = dict(num_perm=16, n=100, fp=0.001, params=(4, 4), save_dir=d, gpu_mode="disable")
        args.update(kw)
        with pytest.raises(ValueError, match="the arguments ask for"):
            MinHashLSHBloom(**args)
    with open(os.path.join(d, "band-1.bf"), "wb") as f:
        f.write(b"\0" * 100)
    with pytest.raises(ValueError, match="not a datasketch_amd Bloom filter file"):
        MinHashLSHBloom(num_perm=16, n=100, fp=0.001, params=(4, 4), save_dir=d, gpu_mode="disable")
    name = str(tmp_path / "one.bf")
    table = BloomTable(10, 0.01, 3, fname=name)
    table.insert(np.array([2, 3, 31], dtype=np.uint32))
    table.sync()
    assert BloomTable(10, 0.01, 3, fname=name).query([2, 3, 31]) and not BloomTable(10, 0.01, 3, fname=name).query([2, 3, 30])


def test_pickle_and_merge():
    a, b = quiet(num_perm=16, n=100, fp=0.001, params=(4, 4)), quiet(num_perm=16, n=100, fp=0.001, params=(4, 4))
    ra, rb = _rows(7, 20), _rows(8, 20)
    a.insert_bulk(ra)
    b.insert(MinHash(16, hashvalues=rb[0]))  # still staged when merged / pickled
    b.insert_bulk(rb[1:])
    a.insert(MinHash(16, hashvalues=ra[0]))
    copy = pickle.loads(pickle.dumps(a))
    assert np.array_equal(copy.words(), a.words()) and copy.query_bulk(ra).all() and len(copy.hashtables) == 4
    assert copy.hashtables[1].query(ra[3, 4:8])
    union = a.words() | b.words()
    a.merge(b)
    assert np.array_equal(a.words(), union) and a.query_bulk(np.vstack([ra, rb])).all()
    for other in (quiet(num_perm=16, n=101, fp=0.0001, params=(4, 4)), quiet(num_perm=16, n=100, fp=0.001, params=(2, 8)), "x"):
        with pytest.raises(ValueError, match="Cannot merge"):
            a.merge(other)


def test_bloom_symbols_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_BLOOM\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_BLOOM == sorted(_native._PROTOTYPES_BLOOM) and len(declared) == 5
    lib = _native.load()
    assert all(hasattr(lib, name) for name in declared)
    assert not set(declared) & (set(_native.EXPORTED_SYMBOLS) | set(_native.EXPORTED_SYMBOLS_EXT))
