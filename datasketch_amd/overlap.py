"""Exact overlap of listed pairs of sets: the verification step that follows ``candidate_pairs``.

Not in the reference.  Everything after the signatures -- ``candidate_pairs``, ``jaccard_pairs``, ``connected_components`` -- sees only
the sketch; a deduplication pipeline then verifies: for every candidate pair the true Jaccard of the two shingle sets, so that the
false positives of the LSH do not chain unrelated documents into one cluster.  :func:`overlap_counts_host`, :func:`jaccard_of` and
:func:`containment_of` ARE the definition; the device kernels (csrc/overlap_kernels.hip), the ``gpu_mode='disable'`` paths and the
tests are all written against them.

A set is the hashes of one document, ``hashes[set_offsets[i]:set_offsets[i+1]]`` (uint32 or uint64); values may repeat and any value
may occur.  For a pair ``(i, j)`` the result is three counts of **distinct** values::

    counts[p] = ( |S_i & S_j| ,  |S_i| ,  |S_j| )

so that ``union = a + b - inter``, ``jaccard = inter / union`` and ``containment = inter / a``.  Both are ``1.0`` at ``0 / 0``: two
empty documents have identical signatures and ``MinHash.jaccard`` says 1.0, and the verification must not split what the estimate
joined.  ``i == j`` gives ``(a, a, a)``; pairs may repeat and come in any order; ``(j, i)`` gives the answer of ``(i, j)`` with the
last two counts swapped.

Everything is exact on the *hashed* values.  With ``bits=64`` (``sha1_hash64``) that is the Jaccard of the shingle sets up to
collisions of SHA-1 truncated to 64 bits; with ``bits=32`` (``sha1_hash32``) it is exactly the quantity a default ``MinHash``
estimates, collisions of the 32-bit hash included.

The whole corpus' hashes must fit on the device in one call: a corpus that does not raises ``MemoryError``.  Chunking a pair list
across pieces of a corpus is out of scope here.
"""
from __future__ import annotations

import numpy as np

from datasketch_amd import _native
from datasketch_amd import shingle as _shingle
from datasketch_amd.hashfunc import HASH_SHA1, device_hash, hash_function


def _check_pairs(pairs, n_sets: int) -> np.ndarray:
    pairs = np.asarray(pairs)
    if pairs.ndim == 1 and pairs.size == 0:  # (an empty list)
        pairs = pairs.reshape(0, 2)
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError("pairs is an [P, 2] array of set indices")
    pairs = np.ascontiguousarray(pairs, dtype=np.int64)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n_sets):
        raise ValueError("pair index out of range")
    return pairs


def _check_sets(hashes, set_offsets):
    hashes = np.ascontiguousarray(hashes).reshape(-1)
    if hashes.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
        raise ValueError("hashes must be a uint32 or uint64 array")
    set_offsets = np.ascontiguousarray(set_offsets, dtype=np.int64).reshape(-1)
    if set_offsets.size < 1 or set_offsets[0] != 0 or set_offsets[-1] > hashes.size or np.any(np.diff(set_offsets) < 0):
        raise ValueError("set_offsets must start at 0, never decrease and end inside hashes")
    return hashes, set_offsets


def overlap_counts_host(hashes, set_offsets, pairs) -> np.ndarray:
    """int32 ``[P, 3]``: ``(|S_i & S_j|, |S_i|, |S_j|)`` for every listed pair, with Python sets.  The definition."""
    hashes, set_offsets = _check_sets(hashes, set_offsets)
    pairs = _check_pairs(pairs, set_offsets.size - 1)
    flat, at = hashes.tolist(), set_offsets.tolist()
    sets = {}
    for i in np.unique(pairs).tolist():
        sets[i] = set(flat[at[i]: at[i + 1]])
    out = np.empty((pairs.shape[0], 3), dtype=np.int32)
    for p, (i, j) in enumerate(pairs.tolist()):
        out[p] = (len(sets[i] & sets[j]), len(sets[i]), len(sets[j]))
    return out


def _check_counts(counts) -> np.ndarray:
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[1] != 3:
        raise ValueError("counts is an [P, 3] array of (intersection, |A|, |B|)")
    return counts.astype(np.int64)


def jaccard_of(counts) -> np.ndarray:
    """float64 ``[P]``: ``inter / (a + b - inter)``, and ``1.0`` where both sets are empty."""
    c = _check_counts(counts)
    union = c[:, 1] + c[:, 2] - c[:, 0]
    out = np.ones(c.shape[0], dtype=np.float64)
    np.divide(c[:, 0], union, out=out, where=union != 0)
    return out


def containment_of(counts) -> np.ndarray:
    """float64 ``[P]``: ``inter / a`` -- how much of the FIRST set of the pair the second one holds -- and ``1.0`` where ``a == 0``."""
    c = _check_counts(counts)
    out = np.ones(c.shape[0], dtype=np.float64)
    np.divide(c[:, 0], c[:, 1], out=out, where=c[:, 1] != 0)
    return out


def _use_gpu(gpu_mode: str) -> bool:
    from datasketch_amd.hyperloglog import _use_gpu as use

    if gpu_mode not in ("detect", "always", "disable"):
        raise ValueError("gpu_mode must be 'detect', 'always' or 'disable'")
    return use(gpu_mode)


def overlap_counts(hashes, set_offsets, pairs, gpu_mode: str = "detect") -> np.ndarray:
    """:func:`overlap_counts_host` on the device: one workgroup per pair builds a hash set of the pair in LDS (in device memory for a
    pair too large for it) and counts into it.  ``gpu_mode='disable'`` is the definition itself."""
    hashes, set_offsets = _check_sets(hashes, set_offsets)
    pairs = _check_pairs(pairs, set_offsets.size - 1)
    if pairs.shape[0] and _use_gpu(gpu_mode):
        return _native.context().overlap_pairs(hashes, set_offsets, pairs)
    return overlap_counts_host(hashes, set_offsets, pairs)


class _DefaultBits(int):
    """The default of ``bits=``: the integer 64 for everything that reads it, and an object of its own, so that a call that gives
    ``bits=64`` can be told from a call that gives nothing."""


_BITS_NOT_GIVEN = _DefaultBits(64)


def _hash_choice(hashfunc, bits):
    """``(callable, (hash_kind, bits) or None)`` of the ``hashfunc=`` / ``bits=`` pair of the text calls.  ``hashfunc=None`` keeps
    the meaning of ``bits`` (SHA-1 of that width, 64 when not given); one of the four device hashes fixes hash and width, and a
    ``bits`` that the caller gave and that says otherwise -- in either direction -- is an error; any other callable is applied on
    the host."""
    if bits not in (32, 64):
        raise ValueError("bits must be 32 or 64")
    if hashfunc is None:
        return hash_function(HASH_SHA1, int(bits)), (HASH_SHA1, int(bits))
    if not callable(hashfunc):
        raise ValueError("The hashfunc must be a callable.")
    known = device_hash(hashfunc)
    if known is not None and bits is not _BITS_NOT_GIVEN and bits != known[1]:
        raise ValueError("bits=%d contradicts hashfunc=%s, a %d-bit hash" % (bits, hashfunc.__name__, known[1]))
    return hashfunc, known


def text_overlap_counts(pairs, packed=None, documents=None, shingle=None, words=None, bits: int = _BITS_NOT_GIVEN, gpu_mode: str = "detect",
                        hashfunc=None) -> np.ndarray:
    """int32 ``[P, 3]`` overlap counts of the listed pairs of sets of a text corpus, given as in ``MinHash.bulk_signatures``:
    ``packed=(buf, byte_offsets, set_offsets)`` (a set is its tokens, or with ``shingle=w`` its shingles of ``w`` tokens),
    ``documents=`` with ``shingle=k`` (``k``-byte shingles) and, with ``words=True`` or a table, shingles of ``k`` words.  The sets
    are hashed with ``sha1_hash32`` (``bits=32``) or ``sha1_hash64`` (``bits=64``, the default).  On the device the corpus goes up once, is hashed
    there and only the counts come back; ``gpu_mode='disable'`` hashes the sets of :mod:`datasketch_amd.shingle` with hashlib and
    applies :func:`overlap_counts_host`.  The corpus is one device call (see the module docstring): ``MemoryError`` if it does not fit.

    ``hashfunc=``: ``None`` keeps the meaning of ``bits``.  One of ``sha1_hash32``, ``sha1_hash64``, ``xxh32_hash32``,
    ``xxh64_hash64`` fixes both the hash and its width (a ``bits`` that contradicts it is a ``ValueError``) and runs on the device
    like the default; any other callable (returning integers below 2**64) is applied per set element on the host."""
    f, known = _hash_choice(hashfunc, bits)
    if (packed is not None) + (documents is not None) != 1:
        raise ValueError("give the corpus as exactly one of packed=(buf, byte_offsets, set_offsets) and documents=")
    if documents is not None and shingle is None:
        raise ValueError("documents= needs shingle=k, the number of bytes per shingle")
    table = _shingle.words_argument(words)
    if table is not None and documents is None:
        raise ValueError("words= goes with documents= and shingle=w, the number of words per shingle")
    corpus = _shingle.text_corpus(packed, documents, shingle, table)
    pairs = _check_pairs(pairs, corpus.doc_offsets.size - 1)
    if pairs.shape[0] == 0:
        return np.empty((0, 3), dtype=np.int32)
    if _use_gpu(gpu_mode) and known:
        return getattr(_native.context(), "overlap_pairs_" + corpus.native)(pairs, bits=known[1], kind=known[0], **corpus.arrays())
    flat, offsets = _shingle.flatten(corpus.host_sets())
    return overlap_counts_host(np.array([f(t) for t in flat], dtype=np.uint32 if known and known[1] == 32 else np.uint64), offsets, pairs)


def exact_jaccard_pairs(pairs, packed=None, documents=None, shingle=None, words=None, bits: int = _BITS_NOT_GIVEN, gpu_mode: str = "detect",
                        hashfunc=None) -> np.ndarray:
    """float64 ``[P]``: the exact Jaccard of every listed pair (:func:`jaccard_of` of :func:`text_overlap_counts`) -- what
    ``jaccard_pairs`` estimates from the signatures.  ``connected_components(pairs, n, keep=exact >= threshold)`` takes the mask."""
    return jaccard_of(text_overlap_counts(pairs, packed, documents, shingle, words, bits, gpu_mode, hashfunc))


def exact_containment_pairs(pairs, packed=None, documents=None, shingle=None, words=None, bits: int = _BITS_NOT_GIVEN, gpu_mode: str = "detect",
                            hashfunc=None) -> np.ndarray:
    """float64 ``[P]``: the exact containment ``|A & B| / |A|`` of the first document of every listed pair in the second -- the
    quantity ``MinHashLSHEnsemble`` searches by."""
    return containment_of(text_overlap_counts(pairs, packed, documents, shingle, words, bits, gpu_mode, hashfunc))
