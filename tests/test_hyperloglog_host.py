"""datasketch_amd.HyperLogLog on the host: the numpy twin of the device path, pinned to the reference.

* tests/golden/hyperloglog.json (tools/gen_golden_hll.py, recorded from the real reference) pins registers, count() and the
  pickled state for seeded inputs; the inputs are rebuilt here by ``golden_tokens`` -- the generator imports this module.
* With the reference mounted, its own tests for HyperLogLog run unmodified on our class, and live comparisons cover what
  the fixture is too small for.
Nothing here needs a GPU: ``gpu_mode='disable'`` is what the GPU tests use as their expected values.
"""
import importlib
import json
import os
import pickle
import sys
import types
import unittest
import warnings
import zlib

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, prehashed, sha1_hash32, sha1_hash64
from datasketch_amd import hyperloglog as H
from tests.test_reference_suite import REFERENCE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hyperloglog.json")
KINDS = {"hll": 32, "hllpp": 64}  # HyperLogLog, and the registers of HyperLogLogPlusPlus
PS = (4, 8, 11, 16)
LENGTHS = (0, 1, 3, 300, 5000)
BYTE_TOKENS = [b"token-%d" % i for i in range(40)]
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "test")), reason="reference repository not mounted")


def edge_hashes(bits, p):
    """The hand-picked hashes: all-zero rest, all-ones index, the lowest rest bit, the top of the range, its top bit alone."""
    edges = [0, (1 << p) - 1, 1 << p, 0xFFFFFFFF, 0x80000000]
    return edges + [1 << 63, (1 << 64) - 1, 1 << 32] if bits == 64 else edges


def case_names():
    return [f"{kind}-p{p}-{what}" for kind in KINDS for p in PS for what in [f"n{n}" for n in LENGTHS] + ["bytes", "edges"]]


def golden_tokens(name):
    """(hash_bits, p, tokens, hashfunc of ours for them): integers through the identity, or byte tokens through SHA-1."""
    kind, p, what = name.split("-")
    bits, p = KINDS[kind], int(p[1:])
    if what == "bytes":
        return bits, p, BYTE_TOKENS, sha1_hash32 if bits == 32 else sha1_hash64
    if what == "edges":
        return bits, p, edge_hashes(bits, p), prehashed
    n = int(what[1:])
    rng = np.random.RandomState(1000 * p + n + bits)
    tokens = rng.randint(0, 2**32, size=n, dtype=np.uint64)
    if bits == 64:
        tokens = (tokens << np.uint64(32)) | rng.randint(0, 2**32, size=n, dtype=np.uint64)
    return bits, p, tokens.tolist(), prehashed


def pack(raw: bytes) -> str:
    """Registers as hex; long rows deflated first ("z" in front)."""
    return raw.hex() if len(raw) <= 256 else "z" + zlib.compress(raw, 9).hex()


def unpack(text: str) -> bytes:
    return zlib.decompress(bytes.fromhex(text[1:])) if text.startswith("z") else bytes.fromhex(text)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def same_float(a, b):
    return (a != a and b != b) or a == b


@pytest.mark.parametrize("name", case_names())
def test_golden_registers_counts_and_pickles(golden, name):
    rec = golden["cases"][name]
    bits, p, tokens, hashfunc = golden_tokens(name)
    want = np.frombuffer(unpack(rec["reg"]), dtype=np.int8)
    assert want.size == 1 << p
    got = HyperLogLog.bulk_registers([tokens], p=p, hashfunc=hashfunc, hash_bits=bits, gpu_mode="disable")
    assert got.dtype == np.int8 and np.array_equal(got[0], want)
    if tokens and hashfunc is prehashed:
        arr = np.array(tokens, dtype=np.uint64)
        assert np.array_equal(HyperLogLog.bulk_registers(arr.reshape(1, -1), p=p, hashfunc=prehashed, hash_bits=bits, gpu_mode="disable")[0], want)
        csr = (arr, np.array([0, 0, arr.size, arr.size]))
        assert np.array_equal(HyperLogLog.bulk_registers(csr, p=p, hashfunc=prehashed, hash_bits=bits, gpu_mode="disable"),
                              np.stack([np.zeros_like(want), want, np.zeros_like(want)]))
    if bits != 32:  # the class itself is the 32-bit sketch
        return
    one = HyperLogLog(p=p, hashfunc=hashfunc, gpu_mode="disable")
    for t in tokens:
        one.update(t)
    batch = HyperLogLog(p=p, hashfunc=hashfunc, gpu_mode="disable")
    batch.update_batch(tokens)
    batch.update_batch(tokens[: len(tokens) // 2])  # on top of a state: idempotent
    assert np.array_equal(one.reg, want) and np.array_equal(batch.reg, want) and batch.reg.dtype == np.int8
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert same_float(float(one.count()), rec["count"])
    assert same_float(float(H.count_many(want.reshape(1, -1), gpu_mode="disable")[0]), rec["count"])
    state = unpack(rec["state"])
    assert bytes(one.__getstate__()) == state
    back = pickle.loads(pickle.dumps(one))
    assert back == one and back.hashfunc is sha1_hash32  # (the reference's __setstate__ forgets the hashfunc, so does ours)
    fresh = HyperLogLog.__new__(HyperLogLog)
    fresh.__setstate__(bytearray(state))
    assert fresh.p == p and np.array_equal(fresh.reg, want)
    assert HyperLogLog.deserialize(state) == one


def test_golden_edge_hashes_one_by_one(golden):
    for key, rows in golden["edges"].items():
        kind, p = key.split("-")
        bits, p = KINDS[kind], int(p[1:])
        assert [int(r[0]) for r in rows] == edge_hashes(bits, p)
        for text, idx, rank in rows:
            reg = HyperLogLog.bulk_registers([[int(text)]], p=p, hashfunc=prehashed, hash_bits=bits, gpu_mode="disable")[0]
            assert np.flatnonzero(reg).tolist() == [idx] and reg[idx] == rank, (key, text)


# ---- the reference's own tests, and live comparisons ------------------------------------------------------------------
def _datasketch_modules():
    return [k for k in sys.modules if k == "datasketch" or k.startswith("datasketch.") or k == "test" or k.startswith("test.")]


@pytest.fixture
def ref():
    """The reference package, imported from its checkout; sys.modules is put back afterwards."""
    saved = {k: sys.modules[k] for k in _datasketch_modules()}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, REFERENCE)
    try:
        yield importlib.import_module("datasketch")
    finally:
        sys.path.remove(REFERENCE)
        for k in _datasketch_modules():
            del sys.modules[k]
        sys.modules.update(saved)


@needs_reference
def test_reference_hyperloglog_tests_pass_on_this_class(ref):
    theirs = importlib.import_module("datasketch.hyperloglog")
    shim = types.ModuleType("datasketch.hyperloglog")
    shim.HyperLogLog = HyperLogLog
    shim.HyperLogLogPlusPlus = theirs.HyperLogLogPlusPlus  # only so that the test file's import line resolves
    sys.modules["datasketch.hyperloglog"] = shim
    mod = importlib.import_module("test.test_hyperloglog")
    assert mod.HyperLogLog is HyperLogLog
    suite = unittest.TestSuite()
    for case in (mod.TestHyperLogLog, mod.TestHyperLogLogSpecific):
        suite.addTests(unittest.defaultTestLoader.loadTestsFromTestCase(case))
    assert suite.countTestCases() >= 14
    result = unittest.TextTestRunner(verbosity=0).run(suite)
    problems = [f"{t}: {tb.splitlines()[-1]}" for t, tb in result.failures + result.errors]
    assert not problems, problems


def _identity(x):
    return x


@needs_reference
@pytest.mark.parametrize("p", [4, 8, 12, 16])
def test_live_parity_with_the_reference(ref, p):
    rng = np.random.RandomState(p)
    m = 1 << p
    regs = []
    for card in (0, 1, m // 2, 2 * m, 3 * m, 40 * m if p < 16 else 4 * m):
        tokens = rng.randint(0, 2**32, size=card, dtype=np.uint64)
        theirs = ref.HyperLogLog(p=p, hashfunc=_identity)
        for t in tokens.tolist():
            theirs.update(t)
        ours = HyperLogLog(p=p, hashfunc=prehashed, gpu_mode="disable")
        ours.update_batch(tokens)
        assert np.array_equal(ours.reg, theirs.reg)
        regs.append(theirs.reg.copy())
        # pickles travel both ways
        back = ref.HyperLogLog.__new__(ref.HyperLogLog)
        back.__setstate__(ours.__getstate__())
        assert back == theirs
        mine = HyperLogLog.__new__(HyperLogLog)
        mine.__setstate__(theirs.__getstate__())
        assert mine == ours
        wide = (tokens[:2000] << np.uint64(32)) | rng.randint(0, 2**32, size=min(card, 2000), dtype=np.uint64)
        pp = ref.HyperLogLogPlusPlus(p=p, hashfunc=_identity)
        for t in wide.tolist():
            pp.update(t)
        got = HyperLogLog.bulk_registers([wide.tolist()], p=p, hashfunc=prehashed, hash_bits=64, gpu_mode="disable")[0]
        assert np.array_equal(got, pp.reg)
        assert ref.HyperLogLogPlusPlus(reg=got) == pp
    words = [b"w%d" % i for i in range(3 * m if p < 16 else 3000)]
    theirs, pp = ref.HyperLogLog(p=p), ref.HyperLogLogPlusPlus(p=p)
    for w in words:
        theirs.update(w)
        pp.update(w)
    assert np.array_equal(HyperLogLog.bulk_registers([words], p=p, gpu_mode="disable")[0], theirs.reg)
    assert np.array_equal(HyperLogLog.bulk_registers([words], p=p, hashfunc=sha1_hash64, hash_bits=64, gpu_mode="disable")[0], pp.reg)
    regs.append(theirs.reg.copy())
    regs.append(np.full(m, 32 - p - 1, dtype=np.int8))  # past 2**32 / 30: the large-range correction
    regs.append(np.full(m, 32 - p + 1, dtype=np.int8))  # saturated: nan
    regs = np.stack(regs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = [float(ref.HyperLogLog(reg=r).count()) for r in regs]
    got = H.count_many(regs, gpu_mode="disable").tolist()
    assert len(got) == len(want) and all(same_float(g, w) for g, w in zip(got, want)), (got, want)
    raw = np.array(want[:-3])
    assert np.any((raw > 0) & (raw <= 2.5 * m)) and np.any(raw > 2.5 * m) and want[-2] > 2**32 / 30 and want[-1] != want[-1]


# ---- semantics --------------------------------------------------------------------------------------------------------
def _raises_like_reference(ref_mod, call, exc):
    """``call(cls)`` raises ``exc`` for our class and, where the reference is mounted, for the reference's; the messages
    begin with the same words."""
    with pytest.raises(exc) as ours:
        call(HyperLogLog)
    if ref_mod is not None:
        with pytest.raises(exc) as theirs:
            call(ref_mod.HyperLogLog)
        assert str(ours.value).split()[:3] == str(theirs.value).split()[:3]


@pytest.fixture
def maybe_ref(request):
    if not os.path.isdir(os.path.join(REFERENCE, "test")):
        yield None
        return
    yield request.getfixturevalue("ref")


def test_errors_match_the_reference(maybe_ref):
    def union_of_one(cls):
        cls.union(cls(4))

    def merge_precisions(cls):
        cls(4).merge(cls(5))

    def overflow_update(cls):
        cls(4, hashfunc=_identity).update(1 << 32)

    def bad_reg_size(cls):
        cls(reg=np.zeros(24, dtype=np.int8))

    def bad_reg_type(cls):
        cls(reg=[0] * 16)

    def bad_p(cls):
        cls(3)

    def bad_hashfunc(cls):
        cls(4, hashfunc=3)

    def short_buffer(cls):
        cls(4).serialize(bytearray(3))

    for call in (union_of_one, merge_precisions, overflow_update, bad_reg_size, bad_reg_type, bad_p, bad_hashfunc, short_buffer):
        _raises_like_reference(maybe_ref, call, ValueError)
    with pytest.warns(DeprecationWarning):
        HyperLogLog(4, hashobj=object())
    full = np.ones(16, dtype=np.int8)
    with pytest.raises(ZeroDivisionError), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        HyperLogLog(reg=full).count()
    with pytest.raises(ZeroDivisionError, match="row 1"):
        H.count_many(np.stack([np.zeros(16, dtype=np.int8), full, full]), gpu_mode="disable")
    with pytest.warns(UserWarning, match="close to error correction threshold"):
        assert HyperLogLog(reg=np.array([1] * 8 + [5] * 8, dtype=np.int8)).count() == 0.673 * 256 / 4.25  # 40.5, the threshold is 40


def test_overflowing_hash_raises_everywhere():
    for tokens in ([1 << 32], [5, 1 << 40, 7], [1 << 64]):
        with pytest.raises(ValueError, match="Hash value overflow"):
            h = HyperLogLog(4, hashfunc=prehashed, gpu_mode="disable")
            for t in tokens:
                h.update(t)
        with pytest.raises(ValueError, match="Hash value overflow"):
            HyperLogLog(4, hashfunc=prehashed, gpu_mode="disable").update_batch(tokens)
        with pytest.raises(ValueError, match="Hash value overflow"):
            HyperLogLog.bulk_registers([[1], tokens], p=4, hashfunc=prehashed, gpu_mode="disable")
    with pytest.raises(ValueError, match="Hash value overflow"):
        HyperLogLog.bulk_registers(np.array([[1 << 32]], dtype=np.uint64), p=4, hashfunc=prehashed, gpu_mode="disable")
    assert HyperLogLog.bulk_registers([[1 << 32]], p=4, hashfunc=prehashed, hash_bits=64, gpu_mode="disable")[0, 0] == 64 - 4 - 29 + 1


def test_gpu_mode_always_needs_a_device():
    from datasketch_amd import _native

    h = HyperLogLog(4, gpu_mode="always")
    assert h.copy()._gpu_mode == "always" and HyperLogLog.union(h, h)._gpu_mode == "always"
    calls = (lambda: HyperLogLog(4, hashfunc=prehashed, gpu_mode="always").update_batch([1, 2, 3]),
             lambda: HyperLogLog.bulk_registers([[b"a"]], gpu_mode="always"),
             lambda: H.count_many(np.zeros((1, 16), dtype=np.int8), gpu_mode="always"))
    for call in calls:
        if _native.gpu_available():
            call()
        else:
            with pytest.raises(RuntimeError, match="GPU mode 'always'"):
                call()


def test_bulk_merge_many_and_union_groups():
    rng = np.random.RandomState(3)
    sets = [[b"%d" % x for x in rng.randint(0, 1000, size=n)] for n in (0, 1, 17, 300)]
    objs = HyperLogLog.bulk(sets, p=6, gpu_mode="disable")
    assert [type(o) for o in objs] == [HyperLogLog] * 4 and objs[0].is_empty() and len(objs[3]) == 64
    for o, s in zip(objs, sets):
        one = HyperLogLog(p=6)
        for t in s:
            one.update(t)
        assert o == one and o.count() == one.count()
    packed = (b"".join(t for s in sets for t in s), np.concatenate([[0], np.cumsum([len(t) for s in sets for t in s])]),
              np.concatenate([[0], np.cumsum([len(s) for s in sets])]))
    reg = HyperLogLog.bulk_registers(packed=packed, p=6, gpu_mode="disable")
    assert np.array_equal(reg, np.stack([o.reg for o in objs]))
    a, b = rng.randint(0, 27, size=(5, 64)).astype(np.int8), rng.randint(0, 27, size=(5, 64)).astype(np.int8)
    merged = H.merge_many(a, b, gpu_mode="disable")
    assert merged.dtype == np.int8 and np.array_equal(merged, np.maximum(a, b))
    with pytest.raises(ValueError):
        H.merge_many(a, b[:, :32], gpu_mode="disable")
    groups = [0, 2, 2, 3, 5]
    got = H.union_groups(a, groups, gpu_mode="disable")
    want = np.stack([np.maximum.reduce(a[0:2]), np.zeros(64, dtype=np.int8), a[2], np.maximum.reduce(a[3:5])])
    assert got.dtype == np.int8 and np.array_equal(got, want)
    assert np.array_equal(H.union_groups(a, [1, 1], gpu_mode="disable"), np.zeros((1, 64), dtype=np.int8))
    assert np.array_equal(H.union_groups(a, [1, 4], gpu_mode="disable")[0], HyperLogLog.union(*[HyperLogLog(reg=r) for r in a[1:4]]).reg)
    with pytest.raises(ValueError):
        H.union_groups(a, [0, 6], gpu_mode="disable")


def test_header_declares_the_bound_hyperloglog_entry_points():
    """What tests/test_cabi.py holds for MHX_API, for the MHX_API_EXT entries: declared, bound and exported are one list."""
    import ctypes
    import re

    from datasketch_amd import _native

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_EXT\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_EXT and len(declared) == 9 and all(name.startswith("mhx_hll_") for name in declared)
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
