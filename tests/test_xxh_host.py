"""xxHash on the host: the definition (datasketch_amd.hashfunc.xxh32_hash32 / xxh64_hash64) against known answers recorded from
the xxhash package (tests/golden/xxh_kat.json, written by tools/gen_xxh_kat.py) and, where that package imports, against it
directly; the gpu_mode='disable' paths of every text call under the two functions against a loop of MinHash.update /
HyperLogLog.update over the shingles of datasketch_amd.shingle; the hashfunc= / bits= rules of the overlap calls; pickles; and
the three-way consistency of the MHX_API_XXH family."""
import ctypes
import json
import os
import pickle
import re

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, hash_many, overlap, shingle, xxh32_hash32, xxh64_hash64
from datasketch_amd import hashfunc as HF
from datasketch_amd.hashfunc import prehashed, sha1_hash32, sha1_hash64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XXH = [xxh32_hash32, xxh64_hash64]
IDS = ["xxh32_hash32", "xxh64_hash64"]


def _bits(f):
    return 32 if f is xxh32_hash32 else 64


def test_known_answers():
    assert xxh32_hash32(b"") == 0x02CC5D05 and xxh32_hash32(b"abc") == 0x32D153FF
    assert xxh64_hash64(b"") == 0xEF46DB3751D8E999 and xxh64_hash64(b"abc") == 0x44BC2CF5AD770999
    assert xxh32_hash32(bytearray(b"abc")) == xxh32_hash32(memoryview(b"abc")) == 0x32D153FF


def test_the_definitions_equal_the_recorded_answers():
    with open(os.path.join(ROOT, "tests", "golden", "xxh_kat.json")) as f:
        kat = json.load(f)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "xxh_kat.json")) < 64 * 1024
    data = bytes((i * 131 + 7) % 256 for i in range(kat["pattern_bytes"]))
    assert kat["seed"] == 0 and len(kat["prefix_xxh32"]) == len(kat["prefix_xxh64"]) == 141 and len(kat["slices"]) == 32
    assert [xxh32_hash32(data[:n]) for n in range(141)] == kat["prefix_xxh32"]
    assert [xxh64_hash64(data[:n]) for n in range(141)] == kat["prefix_xxh64"]
    for s in kat["slices"]:
        piece = data[s["offset"]: s["offset"] + s["length"]]
        assert s["offset"] % 2 == 1 and len(piece) == s["length"]
        assert xxh32_hash32(piece) == s["xxh32"] and xxh64_hash64(piece) == s["xxh64"], s
    assert max(s["length"] for s in kat["slices"]) >= 256 and min(s["length"] for s in kat["slices"]) < 16


def test_the_definitions_equal_the_xxhash_package():
    xxhash = pytest.importorskip("xxhash")
    rng = np.random.RandomState(11)
    for n in rng.randint(0, 301, size=1000):
        data = rng.randint(0, 256, size=int(n), dtype=np.uint8).tobytes()
        assert xxh32_hash32(data) == xxhash.xxh32_intdigest(data) and xxh64_hash64(data) == xxhash.xxh64_intdigest(data), data


def test_the_one_helper_knows_the_four_functions():
    assert HF.device_hash(sha1_hash32) == (HF.HASH_SHA1, 32) and HF.device_hash(sha1_hash64) == (HF.HASH_SHA1, 64)
    assert HF.device_hash(xxh32_hash32) == (HF.HASH_XXH, 32) and HF.device_hash(xxh64_hash64) == (HF.HASH_XXH, 64)
    assert HF.device_hash(prehashed) is None and HF.device_hash(lambda t: 0) is None and HF.device_hash(None) is None
    assert (HF.HASH_SHA1, HF.HASH_XXH) == (_native.MHX_HASH_SHA1, _native.MHX_HASH_XXH) == (0, 1)
    for f in (sha1_hash32, sha1_hash64, xxh32_hash32, xxh64_hash64):
        assert HF.hash_function(*HF.device_hash(f)) is f


def _documents():
    rng = np.random.RandomState(5)
    docs = [bytes(rng.randint(97, 123, size=int(n), dtype=np.uint8)) for n in rng.randint(0, 90, size=14)]
    docs[2], docs[5], docs[7], docs[9] = b"", b"x", b"a" * 40, b"abc" * 11
    return docs


def _token_sets():
    rng = np.random.RandomState(6)
    sets = [[bytes(rng.randint(0, 256, size=int(n), dtype=np.uint8)) for n in rng.randint(0, 41, size=int(c))] for c in rng.randint(0, 9, size=12)]
    sets[1], sets[4] = [], [b""]
    return sets


def _packed(sets):
    buf, byte_offsets = _native.Context.pack_tokens([t for s in sets for t in s])
    set_offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return buf, byte_offsets, set_offsets


def _minhash_loop(sets, f, **kw):
    out = []
    for s in sets:
        m = MinHash(hashfunc=f, gpu_mode="disable", **kw)
        for t in s:
            m.update(t)
        out.append(m.hashvalues)
    return np.array(out, dtype=np.uint64)


def _hll_loop(sets, f, p):
    out = []
    for s in sets:
        h = HyperLogLog(p=p, hashfunc=f, gpu_mode="disable")
        for t in s:
            h.update(t)
        out.append(np.asarray(h.reg).astype(np.int8))
    return np.array(out, dtype=np.int8)


@pytest.mark.parametrize("f", XXH, ids=IDS)
def test_bulk_signatures_on_the_host_equal_a_loop_of_updates(f):
    kw = dict(num_perm=32, seed=3)
    call = lambda *a, **k: MinHash.bulk_signatures(*a, hashfunc=f, gpu_mode="disable", **kw, **k)  # noqa: E731
    sets, docs = _token_sets(), _documents()
    assert np.array_equal(call(sets), _minhash_loop(sets, f, **kw))
    assert np.array_equal(call(packed=_packed(sets)), _minhash_loop(sets, f, **kw))
    assert np.array_equal(call(packed=_packed(sets), shingle=3), _minhash_loop([shingle.token_shingles(s, 3) for s in sets], f, **kw))
    for k in (1, 5, 17):
        assert np.array_equal(call(documents=docs, shingle=k), _minhash_loop([shingle.byte_shingles(d, k) for d in docs], f, **kw))
    text = [b"The quick  brown fox", b"", b"jumps over the lazy dog, twice over", b"one"]
    assert np.array_equal(call(documents=text, shingle=2, words=True), _minhash_loop([shingle.word_shingles(d, 2) for d in text], f, **kw))
    # the object calls agree with the matrix
    m = MinHash(hashfunc=f, gpu_mode="disable", **kw)
    m.update_batch(sets[3])
    assert np.array_equal(m.hashvalues, _minhash_loop(sets, f, **kw)[3])
    assert np.array_equal(np.array([x.hashvalues for x in MinHash.bulk(sets, hashfunc=f, gpu_mode="disable", **kw)]), call(sets))


@pytest.mark.parametrize("f", XXH, ids=IDS)
def test_bulk_registers_on_the_host_equal_a_loop_of_updates(f):
    sets, docs = _token_sets(), _documents()
    # HyperLogLog.update is the 32-bit class: the 64-bit function is held to it on hashes cut to 32 bits by hand below
    if f is xxh32_hash32:
        call = lambda *a, **k: HyperLogLog.bulk_registers(*a, p=6, hashfunc=f, hash_bits=32, gpu_mode="disable", **k)  # noqa: E731
        assert np.array_equal(call(sets), _hll_loop(sets, f, 6))
        assert np.array_equal(call(packed=_packed(sets)), _hll_loop(sets, f, 6))
        assert np.array_equal(call(packed=_packed(sets), shingle=2), _hll_loop([shingle.token_shingles(s, 2) for s in sets], f, 6))
        assert np.array_equal(call(documents=docs, shingle=5), _hll_loop([shingle.byte_shingles(d, 5) for d in docs], f, 6))
        h = HyperLogLog(p=6, hashfunc=f, gpu_mode="disable")
        h.update_batch(sets[3])
        assert np.array_equal(np.asarray(h.reg), _hll_loop(sets, f, 6)[3])
    else:
        shingles = [shingle.byte_shingles(d, 5) for d in docs]
        got = HyperLogLog.bulk_registers(documents=docs, shingle=5, p=6, hashfunc=f, hash_bits=64, gpu_mode="disable")
        values, offsets = shingle.flatten(shingles)
        want = HyperLogLog.bulk_registers((np.array([f(t) for t in values], dtype=np.uint64), offsets), p=6, hashfunc=prehashed, hash_bits=64,
                                          gpu_mode="disable")
        assert np.array_equal(got, want) and got.any()
        with pytest.raises(ValueError, match="overflow"):  # the other pairing is a host hashfunc like any other: 64-bit values do not fit
            HyperLogLog.bulk_registers(documents=docs, shingle=5, p=6, hashfunc=f, hash_bits=32, gpu_mode="disable")


@pytest.mark.parametrize("f", XXH, ids=IDS)
def test_hash_windows_and_hash_many_on_the_host(f):
    docs = _documents()
    buf, doc_offsets = shingle.join_documents(docs)
    got, set_offsets = shingle.hash_windows(buf, doc_offsets, 4, hashfunc=f, gpu_mode="disable")
    want = [f(s) for d in docs for s in shingle.byte_shingles(d, 4)]
    assert got.dtype == (np.uint32 if _bits(f) == 32 else np.uint64) and got.tolist() == want
    assert np.array_equal(set_offsets, shingle.window_offsets(doc_offsets, 4))
    sets = _token_sets()
    pbuf, byte_offsets, tok_docs = _packed(sets)
    got, _ = shingle.hash_windows(pbuf, tok_docs, 2, item_offsets=byte_offsets, hashfunc=f, gpu_mode="disable")
    assert got.tolist() == [f(s) for st in sets for s in shingle.token_shingles(st, 2)]
    tokens = [t for s in sets for t in s]
    many = hash_many(tokens, f, gpu_mode="disable")
    assert many.dtype == got.dtype and many.tolist() == [f(t) for t in tokens]
    # sha1_windows and sha1_hash_many are what they were; hash_windows with their functions is the same thing
    a, _ = shingle.sha1_windows(buf, doc_offsets, 4, bits=_bits(f), gpu_mode="disable")
    b, _ = shingle.hash_windows(buf, doc_offsets, 4, hashfunc=sha1_hash32 if _bits(f) == 32 else sha1_hash64, gpu_mode="disable")
    assert a.dtype == b.dtype and np.array_equal(a, b)
    custom, _ = shingle.hash_windows(buf, doc_offsets, 4, hashfunc=lambda t: len(t), gpu_mode="disable")
    assert custom.dtype == np.uint64 and set(custom.tolist()) <= {1, 2, 3, 4}
    with pytest.raises(ValueError):
        shingle.hash_windows(buf, doc_offsets, 4, hashfunc=None, gpu_mode="disable")
    with pytest.raises(ValueError):
        hash_many(tokens, f, gpu_mode="never")


@pytest.mark.parametrize("f", XXH, ids=IDS)
def test_the_overlap_calls_on_the_host(f):
    docs = _documents()
    docs[11] = docs[10][:30] + b"zzzz"
    pairs = np.array([[10, 11], [11, 10], [0, 1], [2, 2], [2, 5], [7, 9], [3, 3]], dtype=np.int64)
    sets = [{f(s) for s in shingle.byte_shingles(d, 5)} for d in docs]
    want = np.array([(len(sets[i] & sets[j]), len(sets[i]), len(sets[j])) for i, j in pairs.tolist()], dtype=np.int32)
    kw = dict(documents=docs, shingle=5, hashfunc=f, gpu_mode="disable")
    got = overlap.text_overlap_counts(pairs, **kw)
    assert got.dtype == np.int32 and np.array_equal(got, want) and got[0, 0] > 0
    assert np.array_equal(overlap.exact_jaccard_pairs(pairs, **kw), overlap.jaccard_of(want))
    assert np.array_equal(overlap.exact_containment_pairs(pairs, **kw), overlap.containment_of(want))
    tsets = _token_sets()
    tpairs = np.array([[0, 2], [3, 3], [1, 4]], dtype=np.int64)
    hs = [{f(t) for t in s} for s in tsets]
    twant = np.array([(len(hs[i] & hs[j]), len(hs[i]), len(hs[j])) for i, j in tpairs.tolist()], dtype=np.int32)
    assert np.array_equal(overlap.text_overlap_counts(tpairs, packed=_packed(tsets), hashfunc=f, gpu_mode="disable"), twant)
    # hashfunc=None keeps the meaning of bits; a foreign callable runs the host definition with that callable
    for bits, sha in ((32, sha1_hash32), (64, sha1_hash64)):
        assert np.array_equal(overlap.text_overlap_counts(pairs, documents=docs, shingle=5, bits=bits, gpu_mode="disable"),
                              overlap.text_overlap_counts(pairs, documents=docs, shingle=5, hashfunc=sha, gpu_mode="disable"))
    assert overlap.text_overlap_counts(pairs, documents=docs, shingle=5, hashfunc=lambda t: 7, gpu_mode="disable")[0].tolist() == [1, 1, 1]


def test_bits_that_contradict_the_hashfunc_raise():
    docs, pairs = _documents(), [[0, 1]]
    for call in (overlap.text_overlap_counts, overlap.exact_jaccard_pairs, overlap.exact_containment_pairs):
        for f in (xxh64_hash64, sha1_hash64):
            with pytest.raises(ValueError, match="bits=32 contradicts"):
                call(pairs, documents=docs, shingle=5, bits=32, hashfunc=f, gpu_mode="disable")
            call(pairs, documents=docs, shingle=5, bits=64, hashfunc=f, gpu_mode="disable")
            call(pairs, documents=docs, shingle=5, hashfunc=f, gpu_mode="disable")
        for f in (xxh32_hash32, sha1_hash32):
            with pytest.raises(ValueError, match="bits=64 contradicts"):  # an explicit 64 is a statement, not the default
                call(pairs, documents=docs, shingle=5, bits=64, hashfunc=f, gpu_mode="disable")
            call(pairs, documents=docs, shingle=5, bits=32, hashfunc=f, gpu_mode="disable")
            call(pairs, documents=docs, shingle=5, hashfunc=f, gpu_mode="disable")
        # a foreign callable has no width to contradict; without a hashfunc the default is still 64 bits
        call(pairs, documents=docs, shingle=5, bits=32, hashfunc=lambda t: 1, gpu_mode="disable")
        assert np.array_equal(call(pairs, documents=docs, shingle=5, gpu_mode="disable"), call(pairs, documents=docs, shingle=5, bits=64, gpu_mode="disable"))
        with pytest.raises(ValueError, match="bits must be 32 or 64"):
            call(pairs, documents=docs, shingle=5, bits=16, hashfunc=xxh32_hash32, gpu_mode="disable")
        with pytest.raises(ValueError, match="callable"):
            call(pairs, documents=docs, shingle=5, hashfunc=5, gpu_mode="disable")


@pytest.mark.parametrize("f", XXH, ids=IDS)
def test_pickles_carry_the_functions(f):
    m = MinHash(num_perm=16, seed=4, hashfunc=f, gpu_mode="disable")
    m.update_batch([b"a", b"bc", b"def"])
    back = pickle.loads(pickle.dumps(m))
    assert back.hashfunc is f and back == m and np.array_equal(back.permutations[0], m.permutations[0])
    back.update(b"ghij")
    m.update(b"ghij")
    assert back == m
    assert pickle.loads(pickle.dumps(f)) is f


def test_header_declares_the_bound_xxh_symbols_and_the_library_exports_them():
    text = open(os.path.join(ROOT, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_XXH\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_XXH == sorted(_native._PROTOTYPES_XXH) and len(declared) == 11
    assert sum(name.endswith("_hashed") for name in declared) == 9
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    # every chain twin is declared beside an older entry of the same name, and takes one argument more
    older = dict(list(_native._PROTOTYPES.items()) + list(_native._PROTOTYPES_EXT.items()) + list(_native._PROTOTYPES_SHINGLE.items())
                 + list(_native._PROTOTYPES_WORDS.items()) + list(_native._PROTOTYPES_OVERLAP.items()))
    for name in declared:
        twin = name[: -len("_hashed")] if name.endswith("_hashed") else name.replace("mhx_hash_", "mhx_sha1_")
        assert len(_native._PROTOTYPES_XXH[name]) == len(older[twin]) + 1, name
    # the family is a list of its own: it extends none of the earlier ones
    for other in ("", "_EXT", "_BLOOM", "_TOPK", "_CC", "_SHINGLE", "_WORDS", "_OVERLAP"):
        assert not set(declared) & set(getattr(_native, "EXPORTED_SYMBOLS" + other))
    assert re.search(r"enum \{ MHX_HASH_SHA1 = 0, MHX_HASH_XXH = 1 \};", text)


def _walk_text(source, begin, end):
    """The walk's statements between two markers, without comments, blank lines and indentation."""
    start = source.index(begin)
    body = source[start: source.index(end, start)]
    lines = [re.sub(r"\s*//.*$", "", line).strip() for line in body.splitlines()]
    return [line for line in lines if line]


def test_the_two_texts_of_the_window_walk_stay_in_step():
    """sha1_kernels.hip keeps its own text of the walk that window_walk.h holds as a template ("xxHash in place").
    Nothing else ties them: this compares wave_owner_of whole and the trip loop from the wave's first statement to the window's
    byte range, statement by statement."""
    csrc = os.path.join(ROOT, "datasketch_amd", "csrc")
    sha1 = open(os.path.join(csrc, "sha1_kernels.hip")).read()
    walk = open(os.path.join(csrc, "window_walk.h")).read()
    owner = ("int64_t wave_owner_of(", "return lo;")
    loop = ("const int lane = (int)(threadIdx.x & 63u);", "const uintptr_t addr =")
    assert _walk_text(sha1, *owner)[1:] == _walk_text(walk, *owner)[1:] and len(_walk_text(walk, *owner)) > 8
    ours = _walk_text(walk, loop[0], "out[t] = hash(")
    assert _walk_text(sha1, *loop) == ours and len(ours) > 40
