"""Exact overlap of listed pairs, the host side: datasketch_amd.overlap's definition (Python sets over the hashes) against a brute
force over sets of the raw shingle BYTES, the two 0 / 0 rules, symmetry, i == j, every ValueError, the gpu_mode='disable' paths, the
three-way consistency of the MHX_API_OVERLAP family and mhx_overlap_limits (pure host logic of the library: no device).  Every
comparison is exact integer equality."""
import ctypes
import os
import re

import numpy as np
import pytest

from datasketch_amd import _native, overlap, shingle
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64

WORDS = [w.encode() for w in "the quick brown fox jumps over a lazy dog while seven wizards quietly box Big Jugs of liquor".split()]


def text_documents(seed, n=24):
    """Short documents of words from a small vocabulary, with near copies, an empty one, a tiny one and a run of one byte."""
    rng = np.random.RandomState(seed)
    docs = []
    for d in range(n):
        if d and d % 3 == 0:  # an edited copy of an earlier document
            words = docs[rng.randint(0, d)].split(b" ")
            words[rng.randint(0, len(words))] = WORDS[rng.randint(0, len(WORDS))]
        else:
            words = [WORDS[i] for i in rng.randint(0, len(WORDS), rng.randint(3, 30))]
        docs.append(b" ".join(words))
    return docs + [b"", b"ab", b"a" * 40, docs[0]]


def packed_tokens(docs):
    tokens = [[w + b" " for w in d.split(b" ") if w] for d in docs]
    flat, set_offsets = shingle.flatten(tokens)
    byte_offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in flat], out=byte_offsets[1:])
    return np.frombuffer(b"".join(flat), dtype=np.uint8), byte_offsets, set_offsets


def all_pairs(n):
    i, j = np.triu_indices(n)
    return np.stack([i, j], axis=1).astype(np.int64)


def brute_force(sets_of_bytes, pairs):
    out = np.empty((len(pairs), 3), dtype=np.int32)
    for p, (i, j) in enumerate(pairs.tolist()):
        a, b = set(sets_of_bytes[i]), set(sets_of_bytes[j])
        out[p] = (len(a & b), len(a), len(b))
    return out


def corpus_kinds(docs):
    """name -> the keyword arguments of text_overlap_counts"""
    return {
        "bytes k=5": dict(documents=docs, shingle=5),
        "tokens": dict(packed=packed_tokens(docs)),
        "tokens w=3": dict(packed=packed_tokens(docs), shingle=3),
        "words w=2": dict(documents=docs, shingle=2, words=True),
    }


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["bytes k=5", "tokens", "tokens w=3", "words w=2"])
@pytest.mark.parametrize("seed", [11, 12])
def test_the_definition_equals_a_brute_force_over_the_shingle_bytes(seed, kind, bits):
    docs = text_documents(seed)
    kwargs = corpus_kinds(docs)[kind]
    corpus = shingle.text_corpus(kwargs.get("packed"), kwargs.get("documents"), kwargs.get("shingle"), shingle.words_argument(kwargs.get("words")))
    sets = corpus.host_sets()
    f = sha1_hash32 if bits == 32 else sha1_hash64
    flat, offsets = shingle.flatten(sets)
    hashes = np.array([f(t) for t in flat], dtype=np.uint32 if bits == 32 else np.uint64)
    assert len(set(hashes.tolist())) == len(set(flat)), "a truncated SHA-1 collision: pick another seed"
    pairs = all_pairs(len(docs))
    want = brute_force(sets, pairs)
    assert want[:, 0].max() > 0 and np.any(want[:, 1] == 0) and np.any((want[:, 0] > 0) & (want[:, 0] < want[:, 1]))
    got = overlap.overlap_counts_host(hashes, offsets, pairs)
    assert got.dtype == np.int32 and got.shape == (len(pairs), 3) and np.array_equal(got, want)
    assert np.array_equal(overlap.overlap_counts(hashes, offsets, pairs, gpu_mode="disable"), want)
    assert np.array_equal(overlap.text_overlap_counts(pairs, bits=bits, gpu_mode="disable", **kwargs), want)
    jac = overlap.exact_jaccard_pairs(pairs, bits=bits, gpu_mode="disable", **kwargs)
    con = overlap.exact_containment_pairs(pairs, bits=bits, gpu_mode="disable", **kwargs)
    assert jac.dtype == np.float64 and np.array_equal(jac, overlap.jaccard_of(want))
    assert con.dtype == np.float64 and np.array_equal(con, overlap.containment_of(want))


def test_the_two_zero_over_zero_rules_and_the_plain_quotients():
    counts = np.array([[0, 0, 0], [0, 0, 5], [0, 5, 0], [2, 4, 6], [3, 3, 3], [3, 3, 9]], dtype=np.int32)
    assert overlap.jaccard_of(counts).tolist() == [1.0, 0.0, 0.0, 2 / 8, 1.0, 3 / 9]
    assert overlap.containment_of(counts).tolist() == [1.0, 1.0, 0.0, 2 / 4, 1.0, 1.0]
    assert overlap.jaccard_of(np.empty((0, 3), dtype=np.int32)).shape == (0,)
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((1, 3, 1))):
        with pytest.raises(ValueError):
            overlap.jaccard_of(bad)
        with pytest.raises(ValueError):
            overlap.containment_of(bad)
    # near 2^31 the sums are taken in 64 bits
    big = np.array([[2**31 - 1, 2**31 - 1, 2**31 - 1]], dtype=np.int32)
    assert overlap.jaccard_of(big).tolist() == [1.0]


def hashed_sets(dtype, seed=3):
    rng = np.random.RandomState(seed)
    top = np.iinfo(dtype).max
    sets = [rng.randint(0, 50, rng.randint(0, 40)).astype(dtype) for _ in range(12)]
    sets += [np.array([], dtype=dtype), np.array([0, top, 0, 7], dtype=dtype), np.array([top], dtype=dtype), np.full(30, 9, dtype=dtype)]
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([s.size for s in sets], out=offsets[1:])
    return np.concatenate(sets), offsets


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64])
def test_symmetry_the_diagonal_repeats_and_any_order(dtype):
    hashes, offsets = hashed_sets(dtype)
    n = offsets.size - 1
    pairs = all_pairs(n)
    counts = overlap.overlap_counts_host(hashes, offsets, pairs)
    swapped = overlap.overlap_counts_host(hashes, offsets, pairs[:, ::-1])
    assert np.array_equal(swapped, counts[:, [0, 2, 1]])
    diagonal = pairs[:, 0] == pairs[:, 1]
    assert np.array_equal(counts[diagonal, 0], counts[diagonal, 1]) and np.array_equal(counts[diagonal, 1], counts[diagonal, 2])
    sizes = np.array([len(set(hashes[offsets[i]: offsets[i + 1]].tolist())) for i in range(n)])
    assert np.array_equal(counts[diagonal, 0], sizes)  # distinct values: the set of 30 nines counts 1
    order = np.random.RandomState(1).permutation(len(pairs))
    messy = np.concatenate([pairs[order], pairs[:5]])
    assert np.array_equal(overlap.overlap_counts_host(hashes, offsets, messy), np.concatenate([counts[order], counts[:5]]))
    # 0 and the all-ones value are values like any other
    both = overlap.overlap_counts_host(hashes, offsets, [[13, 14], [13, 13]])
    assert both.tolist() == [[1, 3, 1], [3, 3, 3]]
    assert overlap.overlap_counts_host(hashes, offsets, np.empty((0, 2), dtype=np.int64)).shape == (0, 3)
    assert overlap.overlap_counts_host(hashes, offsets, []).shape == (0, 3)


def test_every_value_error():
    hashes, offsets = hashed_sets(np.uint64)
    n = offsets.size - 1
    for f in (overlap.overlap_counts_host, lambda h, o, p: overlap.overlap_counts(h, o, p, gpu_mode="disable")):
        for bad in ([[0, n]], [[-1, 0]], [[n, n]]):
            with pytest.raises(ValueError, match="pair index out of range"):
                f(hashes, offsets, bad)
        for bad in ([0, 1, 2], [[0, 1, 2]], np.zeros((2, 2, 2), dtype=np.int64), np.empty((0, 3), dtype=np.int64)):
            with pytest.raises(ValueError, match="pairs is an"):
                f(hashes, offsets, bad)
        with pytest.raises(ValueError, match="uint32 or uint64"):
            f(hashes.astype(np.int64), offsets, [[0, 1]])
        for bad_offsets in (offsets[::-1], offsets + 1, np.append(offsets, hashes.size + 1), np.empty(0, dtype=np.int64)):
            with pytest.raises(ValueError, match="set_offsets"):
                f(hashes, bad_offsets, [[0, 0]])
    with pytest.raises(ValueError, match="gpu_mode"):
        overlap.overlap_counts(hashes, offsets, [[0, 1]], gpu_mode="sometimes")
    docs = text_documents(5)
    for f in (overlap.text_overlap_counts, overlap.exact_jaccard_pairs, overlap.exact_containment_pairs):
        for bits in (0, 16, 128, None):
            with pytest.raises(ValueError, match="bits must be 32 or 64"):
                f([[0, 1]], documents=docs, shingle=5, bits=bits, gpu_mode="disable")
        with pytest.raises(ValueError, match="exactly one of"):
            f([[0, 1]], gpu_mode="disable")
        with pytest.raises(ValueError, match="exactly one of"):
            f([[0, 1]], packed=packed_tokens(docs), documents=docs, shingle=5, gpu_mode="disable")
        with pytest.raises(ValueError, match="documents= needs shingle"):
            f([[0, 1]], documents=docs, gpu_mode="disable")
        with pytest.raises(ValueError, match="words= goes with documents="):
            f([[0, 1]], packed=packed_tokens(docs), shingle=2, words=True, gpu_mode="disable")
        with pytest.raises(ValueError, match="packed is a"):
            f([[0, 1]], packed=packed_tokens(docs)[:2], gpu_mode="disable")
        with pytest.raises(ValueError, match="shingle width"):
            f([[0, 1]], documents=docs, shingle=0, gpu_mode="disable")
        with pytest.raises(ValueError, match="pair index out of range"):
            f([[0, len(docs)]], documents=docs, shingle=5, gpu_mode="disable")
        with pytest.raises(ValueError, match="pair index out of range"):
            f([[-1, 0]], packed=packed_tokens(docs), gpu_mode="disable")
        with pytest.raises(ValueError, match="pairs is an"):
            f([[0, 1, 2]], documents=docs, shingle=5, gpu_mode="disable")
        with pytest.raises(ValueError, match="gpu_mode"):
            f([[0, 1]], documents=docs, shingle=5, gpu_mode="never")
        assert f(np.empty((0, 2), dtype=np.int64), documents=docs, shingle=5, gpu_mode="disable").shape[0] == 0


def test_the_package_exports_the_module():
    import datasketch_amd

    assert datasketch_amd.overlap is overlap and "overlap" in datasketch_amd.__all__


def test_header_declares_the_bound_overlap_symbols_and_the_library_exports_them():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "mhx.h")).read()
    declared = sorted(set(re.findall(r"MHX_API_OVERLAP\s+[\w\s\*]+?\b(mhx_\w+)\s*\(", text)))
    assert declared == _native.EXPORTED_SYMBOLS_OVERLAP == sorted(_native._PROTOTYPES_OVERLAP) and len(declared) == 6
    lib = ctypes.CDLL(_native.LIB_PATH)
    assert all(hasattr(lib, name) for name in declared)
    # the family is a list of its own: it extends none of the earlier ones
    for other in ("", "_EXT", "_BLOOM", "_TOPK", "_CC", "_SHINGLE", "_WORDS"):
        assert not set(declared) & set(getattr(_native, "EXPORTED_SYMBOLS" + other))


HEADER_BYTES = 64  # the pair's counters in front of an LDS table (include/mhx.h, mhx_overlap_limits)


def table_bytes(items, key_bytes):
    """keys + two bits per slot of the table of a pair of `items` items: the power of two >= max(64, 2 items) slots"""
    slots = 64
    while slots < 2 * items:
        slots *= 2
    return slots * key_bytes + 2 * (slots // 8)


@pytest.mark.parametrize("bits", [32, 64])
def test_overlap_limits_is_monotone_and_names_the_last_table_that_fits(bits):
    key_bytes = bits // 8
    sizes = sorted([0, 1, 63, 64, 500, 64 + table_bytes(1, key_bytes) - 1, 64 + table_bytes(1, key_bytes), 1 << 10, 3000, 1 << 13, 1 << 14, 40_000,
                    1 << 16, (1 << 16) + 4159, (1 << 16) + 4160, (1 << 16) + 4161, 100_000, 160 << 10, (160 << 10) + 1, 1 << 20, 1 << 24, 1 << 30])
    answers = [_native.overlap_limits(bits, lds) for lds in sizes]
    assert answers == sorted(answers) and answers[0] == 0 and answers[-1] > answers[0]
    for lds, m in zip(sizes, answers):
        if m:
            assert HEADER_BYTES + table_bytes(m, key_bytes) <= lds, (lds, m)
        assert HEADER_BYTES + table_bytes(m + 1, key_bytes) > lds, (lds, m)
    assert _native.overlap_limits(bits, 160 << 10) == (16384 if bits == 32 else 8192)  # gfx950: 160 KiB per workgroup
    lib, out = _native.load(), ctypes.c_int64(-5)
    assert lib.mhx_overlap_limits(7, 1 << 16, ctypes.byref(out)) == _native.MHX_ERR_INVALID and "hv_dtype" in _native.last_error() and out.value == -5
    assert lib.mhx_overlap_limits(_native.MHX_U64, -1, ctypes.byref(out)) == _native.MHX_ERR_INVALID and out.value == -5
    assert "lds_per_block" in _native.last_error()
    assert lib.mhx_overlap_limits(_native.MHX_U64, 1 << 16, None) == _native.MHX_ERR_INVALID and "NULL" in _native.last_error()
