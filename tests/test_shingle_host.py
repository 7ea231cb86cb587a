"""Shingles on the host: the definition (datasketch_amd/shingle.py), the gpu_mode='disable' paths written against it, the argument
errors, and the one piece of the C ABI that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, shingle
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_byte_shingles_by_hand():
    d = b"abcdef"
    k = 4
    assert shingle.byte_shingles(b"", k) == []  # m = 0
    assert shingle.byte_shingles(b"a", k) == [b"a"]  # m = 1
    assert shingle.byte_shingles(d[:3], k) == [b"abc"]  # m = width - 1: the whole document
    assert shingle.byte_shingles(d[:4], k) == [b"abcd"]  # m = width
    assert shingle.byte_shingles(d[:5], k) == [b"abcd", b"bcde"]  # m = width + 1
    assert shingle.byte_shingles(d, 1) == [b"a", b"b", b"c", b"d", b"e", b"f"]
    assert shingle.byte_shingles(b"aaaa", 2) == [b"aa", b"aa", b"aa"]  # repeated windows stay in
    assert shingle.byte_shingles(bytearray(b"xyz"), 2) == [b"xy", b"yz"]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            shingle.byte_shingles(d, bad)


def test_token_shingles_by_hand():
    t = [b"the ", b"quick ", b"brown ", b"fox"]
    assert shingle.token_shingles([], 3) == []
    assert shingle.token_shingles(t[:1], 3) == [b"the "]
    assert shingle.token_shingles(t[:2], 3) == [b"the quick "]  # width - 1 tokens: all of them
    assert shingle.token_shingles(t[:3], 3) == [b"the quick brown "]
    assert shingle.token_shingles(t, 3) == [b"the quick brown ", b"quick brown fox"]
    assert shingle.token_shingles(t, 1) == t
    # empty tokens are tokens: they take a place in the window and add no bytes
    assert shingle.token_shingles([b"", b"a", b"", b"b"], 2) == [b"a", b"a", b"b"]
    assert shingle.token_shingles([b"", b""], 2) == [b""]
    assert shingle.token_shingles([b"", b"", b""], 2) == [b"", b""]
    with pytest.raises(ValueError):
        shingle.token_shingles(t, 0)


def test_window_offsets_by_hand():
    w = 4
    lengths = [0, 1, w - 1, w, w + 1, 0, 0, 9]
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)])
    assert shingle.window_offsets(doc_offsets, w).tolist() == [0, 0, 1, 2, 3, 5, 5, 5, 11]
    assert shingle.window_offsets(doc_offsets, 1).tolist() == doc_offsets.tolist()
    assert shingle.window_offsets([0], 3).tolist() == [0]
    assert shingle.window_offsets(doc_offsets, w).dtype == np.int64
    with pytest.raises(ValueError):
        shingle.window_offsets([0, 5, 3], 2)
    with pytest.raises(ValueError):
        shingle.window_offsets([0, 5], 0)
    with pytest.raises(ValueError):
        shingle.window_offsets([], 2)


def test_no_window_crosses_a_document_boundary():
    """"abcd" + "efgh": a crossing window ("cdef", ...) would be new bytes and would show in the hashes."""
    docs = [b"abcd", b"efgh"]
    buf, doc_offsets = shingle.join_documents(docs)
    hashes, set_offsets = shingle.sha1_windows(buf, doc_offsets, 3, gpu_mode="disable")
    assert set_offsets.tolist() == [0, 2, 4]
    assert hashes.tolist() == [sha1_hash32(s) for s in (b"abc", b"bcd", b"efg", b"fgh")]
    assert sha1_hash32(b"cde") not in hashes.tolist() and sha1_hash32(b"def") not in hashes.tolist()
    # tokens: the documents ("a ", "b ") and ("c ", "d ") have no window "b c "
    toks = [b"a ", b"b ", b"c ", b"d "]
    item_offsets = np.concatenate([[0], np.cumsum([len(t) for t in toks])])
    hashes, set_offsets = shingle.sha1_windows(b"".join(toks), [0, 2, 4], 2, item_offsets=item_offsets, bits=64, gpu_mode="disable")
    assert hashes.dtype == np.uint64 and set_offsets.tolist() == [0, 1, 2]
    assert hashes.tolist() == [sha1_hash64(b"a b "), sha1_hash64(b"c d ")]


def _documents(seed, n=23, longest=40):
    rng = np.random.RandomState(seed)
    docs = [bytes(rng.randint(97, 101, size=rng.randint(0, longest), dtype=np.uint8)) for _ in range(n)]
    docs[3], docs[7], docs[8] = b"", b"z", b"zzzzzzzzzzzz"
    return docs


def _tokenized(seed, n=19):
    rng = np.random.RandomState(seed)
    sets = [[bytes(rng.randint(97, 100, size=rng.randint(0, 5), dtype=np.uint8)) for _ in range(rng.randint(0, 12))] for _ in range(n)]
    sets[2], sets[5] = [], [b"", b""]
    flat = [t for s in sets for t in s]
    byte_offsets = np.concatenate([[0], np.cumsum([len(t) for t in flat])]).astype(np.int64)
    set_offsets = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    return sets, (np.frombuffer(b"".join(flat), dtype=np.uint8), byte_offsets, set_offsets)


@pytest.mark.parametrize("hashfunc", [sha1_hash32, sha1_hash64, lambda t: len(t) * 1000003 + sum(t)], ids=["sha1_hash32", "sha1_hash64", "custom"])
@pytest.mark.parametrize("k", [1, 3, 12, 50])
def test_bulk_signatures_of_documents_equal_the_signatures_of_their_shingles(k, hashfunc):
    docs = _documents(k)
    kw = dict(num_perm=32, seed=3, hashfunc=hashfunc, gpu_mode="disable")
    want = MinHash.bulk_signatures([shingle.byte_shingles(d, k) for d in docs], **kw)
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=k, **kw), want)
    assert np.array_equal(MinHash.bulk_signatures(documents=shingle.join_documents(docs), shingle=k, **kw), want)
    assert np.array_equal(MinHash.bulk_signatures(documents=(b"".join(docs), np.cumsum([0] + [len(d) for d in docs])), shingle=k, **kw), want)
    got32 = MinHash.bulk_signatures(documents=docs, shingle=k, out_dtype=np.uint32, **kw)
    assert got32.dtype == np.uint32 and np.array_equal(got32, want)


@pytest.mark.parametrize("w", [1, 2, 3, 7])
def test_bulk_signatures_of_packed_tokens_equal_the_signatures_of_their_shingles(w):
    sets, packed = _tokenized(w)
    init = np.random.RandomState(1).randint(0, 2**32, size=16).astype(np.uint64)
    for extra in ({}, {"hashvalues": init}):
        kw = dict(num_perm=16, seed=5, gpu_mode="disable", **extra)
        want = MinHash.bulk_signatures([shingle.token_shingles(s, w) for s in sets], **kw)
        assert np.array_equal(MinHash.bulk_signatures(packed=packed, shingle=w, **kw), want)
    assert np.array_equal(want[2], init) and np.array_equal(want[5], np.minimum(init, MinHash.bulk_signatures([[b""]], **kw)[0]))


def test_bulk_registers_of_shingles():
    docs = _documents(11)
    for hashfunc, bits in ((sha1_hash32, 32), (sha1_hash64, 64)):
        kw = dict(p=6, hashfunc=hashfunc, hash_bits=bits, gpu_mode="disable")
        want = HyperLogLog.bulk_registers([shingle.byte_shingles(d, 5) for d in docs], **kw)
        assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=5, **kw), want)
    sets, packed = _tokenized(4)
    want = HyperLogLog.bulk_registers([shingle.token_shingles(s, 3) for s in sets], p=5, gpu_mode="disable")
    assert np.array_equal(HyperLogLog.bulk_registers(packed=packed, shingle=3, p=5, gpu_mode="disable"), want)


def test_chunks_of_whole_documents(monkeypatch):
    from datasketch_amd import minhash as M

    docs = _documents(2, n=40) + [b"q" * 500]
    want = MinHash.bulk_signatures(documents=docs, shingle=4, num_perm=16, gpu_mode="disable")
    monkeypatch.setattr(M, "_BULK_CHUNK_SETS", 7)
    monkeypatch.setattr(M, "_BULK_CHUNK_TOKENS", 60)
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=4, num_perm=16, gpu_mode="disable"), want)
    assert list(shingle.window_chunks(np.array([0, 5, 5, 105, 106, 107]), 2, 50)) == [(0, 2), (2, 3), (3, 5)]


def test_the_one_chunker_on_random_offsets():
    """What every chunked bulk call relies on: the ranges are contiguous, cover [0, n), hold at most max_sets sets, and at most
    max_tokens tokens unless a range is one set."""
    rng = np.random.RandomState(11)
    cases = [(np.zeros(1, dtype=np.int64), 3, 10), (np.zeros(6, dtype=np.int64), 2, 10)]  # no set; empty sets only
    for trial in range(60):
        n, max_sets, max_tokens = int(rng.randint(1, 40)), int(rng.randint(1, 9)), int(rng.randint(1, 30))
        lengths = rng.randint(0, 12, n) * (rng.random_sample(n) < 0.7)  # ~30 % empty sets
        lengths[rng.randint(n)] = max_tokens + int(rng.randint(1, 50))  # one set larger than max_tokens
        offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        cases.append((offsets + (trial % 2) * 17, max_sets, max_tokens))  # (a CSR pair of hashes need not start at 0)
    for offsets, max_sets, max_tokens in cases:
        n, at = offsets.size - 1, 0
        for s, e in shingle.window_chunks(offsets, max_sets, max_tokens):
            assert s == at and s < e <= n
            assert e - s <= max_sets
            assert offsets[e] - offsets[s] <= max_tokens or e - s == 1
            at = e
        assert at == n


def test_str_documents_are_shingled_over_their_utf8_bytes():
    docs = ["naïve café", "", "日本語のテキスト", "plain"]
    as_bytes = [d.encode("utf-8") for d in docs]
    kw = dict(shingle=4, num_perm=16, gpu_mode="disable")
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, **kw), MinHash.bulk_signatures(documents=as_bytes, **kw))
    assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=4, gpu_mode="disable"),
                          HyperLogLog.bulk_registers(documents=as_bytes, shingle=4, gpu_mode="disable"))


@pytest.mark.parametrize("call", [lambda **kw: MinHash.bulk_signatures(num_perm=16, gpu_mode="disable", **kw),
                                  lambda **kw: HyperLogLog.bulk_registers(gpu_mode="disable", **kw)], ids=["MinHash", "HyperLogLog"])
def test_argument_errors(call):
    docs = [b"abcdef", b"gh"]
    buf, offs = b"abcdefgh", [0, 6, 8]
    packed = (b"abcd", [0, 1, 4], [0, 1, 2])
    for kwargs in (
        {},  # no corpus
        {"b": [[b"a"]], "documents": docs, "shingle": 3},  # two corpora
        {"packed": packed, "documents": docs, "shingle": 3},
        {"b": [[b"a"]], "packed": packed},
        {"b": [[b"a"]], "shingle": 3},  # shingle with b
        {"documents": docs},  # documents without shingle
        {"documents": docs, "shingle": 0},
        {"documents": docs, "shingle": -2},
        {"documents": docs, "shingle": 2.5},
        {"documents": b"one document", "shingle": 3},
        {"documents": (buf, [1, 6, 8]), "shingle": 3},  # doc_offsets[0] != 0
        {"documents": (buf, [0, 7, 6, 8]), "shingle": 3},  # decreasing
        {"documents": (buf, [0, 6, 7]), "shingle": 3},  # does not end at the byte count
        {"documents": (buf, [0, 6, 9]), "shingle": 3},
        {"documents": (buf, []), "shingle": 3},
        {"packed": (b"abcd", [1, 2, 4], [0, 1, 2]), "shingle": 2},  # item offsets do not start at 0
        {"packed": (b"abcd", [0, 3, 2], [0, 1, 2]), "shingle": 2},  # decreasing
        {"packed": (b"abcd", [0, 1, 5], [0, 1, 2]), "shingle": 2},  # end outside buf
        {"packed": (b"abcd", [0, 1, 4], [0, 1, 3]), "shingle": 2},  # doc offsets do not end at the number of tokens
        {"packed": (b"abcd", [0, 1, 4], [0, 2, 1, 2]), "shingle": 2},
        {"packed": (b"abcd", [0, 1, 4]), "shingle": 2},  # not a triple
    ):
        with pytest.raises(ValueError):
            call(**kwargs)
    assert call(documents=docs, shingle=3).shape[0] == 2 and call(packed=packed, shingle=2).shape[0] == 2
    assert call(documents=[], shingle=3).shape[0] == 0 and call(documents=(b"", [0]), shingle=3).shape[0] == 0


def test_sha1_windows_argument_errors():
    with pytest.raises(ValueError):
        shingle.sha1_windows(b"abc", [0, 3], 2, bits=16, gpu_mode="disable")
    with pytest.raises(ValueError):
        shingle.sha1_windows(b"abc", [0, 2], 2, gpu_mode="disable")
    with pytest.raises(ValueError):
        shingle.sha1_windows(b"abc", [0, 3], 0, gpu_mode="disable")


def test_header_declares_the_bound_shingle_symbols():
    text = open(os.path.join(ROOT, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_SHINGLE\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_SHINGLE == sorted(_native._PROTOTYPES_SHINGLE) and len(declared) == 5
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    others = (_native.EXPORTED_SYMBOLS + _native.EXPORTED_SYMBOLS_EXT + _native.EXPORTED_SYMBOLS_BLOOM + _native.EXPORTED_SYMBOLS_TOPK
              + _native.EXPORTED_SYMBOLS_CC)
    assert not set(declared) & set(others)


def test_shingle_window_offsets_is_pure_host_logic():
    """mhx_shingle_window_offsets needs the library and no device, and equals shingle.window_offsets."""
    rng = np.random.RandomState(8)
    for width in (1, 2, 5, 9, 64, 1000):
        lengths = rng.randint(0, 3 * width + 2, size=200)
        lengths[:6] = [0, 1, max(width - 1, 0), width, width + 1, 0]
        doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        assert np.array_equal(_native.window_offsets(doc_offsets, width), shingle.window_offsets(doc_offsets, width)), width
    assert _native.window_offsets([0], 4).tolist() == [0]
    for doc_offsets, width in (([0, 4, 2], 3), ([0, 4], 0), ([0, 4], -1)):
        with pytest.raises(ValueError):
            _native.window_offsets(doc_offsets, width)
        assert _native.last_error()
    lib = _native.load()
    assert lib.mhx_shingle_window_offsets(None, 1, 2, None) == _native.MHX_ERR_INVALID
