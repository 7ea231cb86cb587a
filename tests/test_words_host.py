"""Word shingles on the host: the definition (word_table, words, word_shingles, normalize_words of datasketch_amd/shingle.py) held
to hand-written cases, the gpu_mode='disable' paths written against it, the argument errors, and the seventh export list."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, shingle
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_word_table_by_hand():
    t = shingle.word_table()
    assert t.dtype == np.uint8 and t.shape == (256,) and t[0] == 0
    for c in b"0123456789abcdefghijklmnopqrstuvwxyz_":
        assert t[c] == c
    for c in b"ABCDEFGHIJKLMNOPQRSTUVWXYZ":
        assert t[c] == c + 32
    assert all(t[c] == c for c in range(0x80, 0x100))
    assert not t[: ord("0")].any() and not t[ord("9") + 1: ord("A")].any() and not t[ord("Z") + 1: ord("_")].any()
    assert t[ord("`")] == 0 and not t[ord("z") + 1: 0x80].any()
    keep = shingle.word_table(lowercase=False)
    assert all(keep[c] == c for c in b"AZaz09_") and np.array_equal(keep != 0, t != 0)
    ext = shingle.word_table(extra=b"-'")
    assert ext[ord("-")] == ord("-") and ext[ord("'")] == ord("'") and ext[ord("A")] == ord("a")
    assert np.array_equal(np.flatnonzero((ext != 0) != (t != 0)), sorted(b"'-"))


def test_word_table_and_user_table_errors():
    with pytest.raises(ValueError):
        shingle.word_table(extra=b"a\0")
    good = shingle.word_table()
    bad0 = good.copy()
    bad0[0] = 1
    for bad in (bad0, good[:255], good.astype(np.int32), np.zeros((2, 128), dtype=np.uint8), list(range(256))):
        with pytest.raises(ValueError):
            shingle.words(b"abc", bad)
        with pytest.raises(ValueError):
            shingle.word_shingles(b"abc", 2, bad)
        with pytest.raises(ValueError):
            shingle.normalize_words(b"abc", [0, 3], bad, gpu_mode="disable")
    with pytest.raises(ValueError):
        shingle.word_shingles(b"abc", 0)


def test_words_by_hand():
    W = shingle.words
    assert W(b"The  cat") == W(b"the cat,") == W(b"The cat") == [b"the", b"cat"]  # case folding, runs, trailing punctuation
    assert W(b"snake_case x86_64 42") == [b"snake_case", b"x86_64", b"42"]  # _ and digits are word bytes
    assert W("Café au lait".encode()) == [b"caf\xc3\xa9", b"au", b"lait"]  # a UTF-8 word stays whole (only ASCII folds)
    assert W("日本語 text".encode()) == ["日本語".encode(), b"text"]
    assert W(b"a,.;:!?--b") == [b"a", b"b"]  # a punctuation run is one separator
    assert W(b"  \t\nlead and trail \r\n ") == [b"lead", b"and", b"trail"]
    assert W(b"") == [] and W(b" ,.\n\0\0 ") == []  # empty, separators only
    assert W(b"a\0b") == [b"a", b"b"]  # byte 0 separates
    assert W(b"it's well-known") == [b"it", b"s", b"well", b"known"]
    assert W(b"it's well-known", shingle.word_table(extra=b"'-")) == [b"it's", b"well-known"]
    assert W(b"Keep CASE", shingle.word_table(lowercase=False)) == [b"Keep", b"CASE"]
    assert W(bytearray(b"x y")) == [b"x", b"y"] and W(np.frombuffer(b"x y", dtype=np.uint8)) == [b"x", b"y"]
    # a user table: only a and b are word bytes, and b is emitted as X
    t = np.zeros(256, dtype=np.uint8)
    t[ord("a")], t[ord("b")] = ord("a"), ord("X")
    assert W(b"abc bad cab", t) == [b"aX", b"Xa", b"aX"]


def test_word_shingles_by_hand():
    S = shingle.word_shingles
    assert S(b"", 2) == [] and S(b" ,, ", 2) == []
    assert S(b"One", 2) == [b"one "]  # fewer than w words: all of them, the trailing space included
    assert S(b"one two", 2) == [b"one two "]
    assert S(b"one, two;  THREE", 2) == [b"one two ", b"two three "]
    assert S(b"one two three", 1) == [b"one ", b"two ", b"three "]
    # a shingle depends on its words alone
    assert S(b"the  cat sat", 2) == S(b"The cat, sat.", 2) == S(b"\tthe\ncat\nsat", 2)
    assert S(b"a a a a", 2) == [b"a a "] * 3  # repeated shingles stay in
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            S(b"a b", bad)


def _triple(docs, table=None):
    buf, doc_offsets = shingle.join_documents(docs)
    out, items, word_docs = shingle.normalize_words(buf, doc_offsets, table, gpu_mode="disable")
    assert out.dtype == np.uint8 and items.dtype == np.int64 and word_docs.dtype == np.int64
    return out.tobytes(), items.tolist(), word_docs.tolist()


def test_normalize_words_by_hand():
    assert _triple([b"The  cat,", b"", b" ,. ", b"sat"]) == (b"the cat sat ", [0, 4, 8, 12], [0, 2, 2, 2, 3])
    # adjacent documents with no separator between them: a word never crosses the boundary
    assert _triple([b"abc", b"def"]) == (b"abc def ", [0, 4, 8], [0, 1, 2])
    assert _triple([b"ab", b"", b"", b"cd ef"]) == (b"ab cd ef ", [0, 3, 6, 9], [0, 1, 1, 1, 3])
    assert _triple([]) == (b"", [0], [0])
    assert _triple([b"", b""]) == (b"", [0], [0, 0, 0])
    assert _triple([b"..", b"!"]) == (b"", [0], [0, 0, 0])
    assert _triple([b"x"]) == (b"x ", [0, 2], [0, 1])
    assert _triple([b"a", b"b", b"c"]) == (b"a b c ", [0, 2, 4, 6], [0, 1, 2, 3])  # one-byte documents: twice the input
    assert _triple(["Café".encode(), b"it's"], shingle.word_table(extra=b"'")) == ("café it's ".encode(), [0, 6, 11], [0, 1, 2])
    for bad_offsets in ([1, 3], [0, 2], [0, 4], [0, 2, 1, 3], []):
        with pytest.raises(ValueError):
            shingle.normalize_words(b"abc", bad_offsets, gpu_mode="disable")


def _documents(seed, n=31):
    rng = np.random.RandomState(seed)
    alphabet = np.frombuffer(b"aB ,\xc3\xa9_7", dtype=np.uint8)
    docs = [bytes(alphabet[rng.randint(0, alphabet.size, size=rng.randint(0, 60))]) for _ in range(n)]
    docs[2], docs[5], docs[6], docs[9] = b"", b" , ", b"one", b"One two THREE four five six"
    return docs


@pytest.mark.parametrize("hashfunc", [sha1_hash32, sha1_hash64, lambda t: len(t) * 1000003 + sum(t)], ids=["sha1_hash32", "sha1_hash64", "custom"])
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_round_trip_through_the_packed_path(w, hashfunc):
    """packed=normalize_words(...) with shingle=w, documents= with words=True and the signatures of word_shingles are one thing."""
    docs = _documents(w)
    init = np.random.RandomState(3).randint(0, 2**32, size=32).astype(np.uint64)
    for extra in ({}, {"hashvalues": init}):
        kw = dict(num_perm=32, seed=3, hashfunc=hashfunc, gpu_mode="disable", **extra)
        want = MinHash.bulk_signatures([shingle.word_shingles(d, w) for d in docs], **kw)
        packed = shingle.normalize_words(*shingle.join_documents(docs), gpu_mode="disable")
        assert np.array_equal(MinHash.bulk_signatures(packed=packed, shingle=w, **kw), want)
        assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=w, words=True, **kw), want)
        assert np.array_equal(MinHash.bulk_signatures(documents=shingle.join_documents(docs), shingle=w, words=shingle.word_table(), **kw), want)
    got32 = MinHash.bulk_signatures(documents=docs, shingle=w, words=True, out_dtype=np.uint32, num_perm=32, seed=3, hashfunc=hashfunc, gpu_mode="disable")
    assert got32.dtype == np.uint32
    assert np.array_equal(want[2], init)  # a document without a word keeps its init row


def test_user_table_changes_the_sets():
    docs = [b"it's well-known", b"its wellknown"]
    table = shingle.word_table(extra=b"'-")
    kw = dict(num_perm=16, gpu_mode="disable")
    got = MinHash.bulk_signatures(documents=docs, shingle=1, words=table, **kw)
    assert np.array_equal(got, MinHash.bulk_signatures([[b"it's ", b"well-known "], [b"its ", b"wellknown "]], **kw))
    assert not np.array_equal(got, MinHash.bulk_signatures(documents=docs, shingle=1, words=True, **kw))


def test_bulk_registers_of_word_shingles():
    docs = _documents(11)
    for hashfunc, bits in ((sha1_hash32, 32), (sha1_hash64, 64)):
        kw = dict(p=6, hashfunc=hashfunc, hash_bits=bits, gpu_mode="disable")
        want = HyperLogLog.bulk_registers([shingle.word_shingles(d, 3) for d in docs], **kw)
        assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=3, words=True, **kw), want)
        packed = shingle.normalize_words(*shingle.join_documents(docs), gpu_mode="disable")
        assert np.array_equal(HyperLogLog.bulk_registers(packed=packed, shingle=3, **kw), want)


def test_chunks_are_whole_documents_counted_in_bytes(monkeypatch):
    from datasketch_amd import hyperloglog as H
    from datasketch_amd import minhash as M

    docs = _documents(2, n=40) + [b"q r " * 120]
    want = MinHash.bulk_signatures(documents=docs, shingle=2, words=True, num_perm=16, gpu_mode="disable")
    want_reg = HyperLogLog.bulk_registers(documents=docs, shingle=2, words=True, p=5, gpu_mode="disable")
    monkeypatch.setattr(M, "_BULK_CHUNK_SETS", 7)
    monkeypatch.setattr(M, "_BULK_CHUNK_TOKENS", 90)
    monkeypatch.setattr(H, "_BULK_CHUNK_TOKENS", 90)
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=2, words=True, num_perm=16, gpu_mode="disable"), want)
    assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=2, words=True, p=5, gpu_mode="disable"), want_reg)


@pytest.mark.parametrize("call", [lambda **kw: MinHash.bulk_signatures(num_perm=16, gpu_mode="disable", **kw),
                                  lambda **kw: HyperLogLog.bulk_registers(gpu_mode="disable", **kw)], ids=["MinHash", "HyperLogLog"])
def test_words_argument_errors(call):
    docs = [b"one two three", b"four"]
    packed = (b"a b ", [0, 2, 4], [0, 1, 2])
    bad_table = shingle.word_table()
    bad_table[0] = 7
    for kwargs in (
        {"b": [[b"a"]], "words": True},  # words= without documents=
        {"packed": packed, "shingle": 2, "words": True},
        {"packed": packed, "shingle": 2, "words": shingle.word_table()},
        {"documents": docs, "words": True},  # no shingle
        {"documents": docs, "shingle": 0, "words": True},
        {"documents": docs, "shingle": 2, "words": bad_table},
        {"documents": docs, "shingle": 2, "words": np.zeros(255, dtype=np.uint8)},
        {"documents": docs, "shingle": 2, "words": "yes"},
        {"documents": (b"abcdef", [0, 7]), "shingle": 2, "words": True},
        {"documents": b"one document", "shingle": 2, "words": True},
    ):
        with pytest.raises(ValueError):
            call(**kwargs)
    assert call(documents=docs, shingle=2, words=True).shape[0] == 2
    assert call(documents=[], shingle=2, words=True).shape[0] == 0
    # words=None / False: the byte shingles, exactly as without the argument
    assert np.array_equal(call(documents=docs, shingle=2, words=None), call(documents=docs, shingle=2))
    assert np.array_equal(call(documents=docs, shingle=2, words=False), call(documents=docs, shingle=2))
    assert not np.array_equal(call(documents=docs, shingle=2, words=True), call(documents=docs, shingle=2))


def test_header_declares_the_bound_words_symbols():
    text = open(os.path.join(ROOT, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_WORDS\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_WORDS == sorted(_native._PROTOTYPES_WORDS) and len(declared) == 4
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    others = (_native.EXPORTED_SYMBOLS + _native.EXPORTED_SYMBOLS_EXT + _native.EXPORTED_SYMBOLS_BLOOM + _native.EXPORTED_SYMBOLS_TOPK
              + _native.EXPORTED_SYMBOLS_CC + _native.EXPORTED_SYMBOLS_SHINGLE)
    assert not set(declared) & set(others)
    assert re.search(r"MHX_ERR_CAPACITY\s*=\s*%d\b" % _native.MHX_ERR_CAPACITY, text)
