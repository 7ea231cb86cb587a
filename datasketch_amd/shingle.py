"""Shingles: the sliding windows that turn a document into the set MinHash and HyperLogLog summarise.

Not in the reference, which leaves the step to its caller (``for i in range(len(d) - k + 1): m.update(d[i:i+k])``).  The three
functions :func:`byte_shingles`, :func:`token_shingles` and :func:`window_offsets` ARE the definition; the device kernel
(``sha1_windows_kernel``, csrc/sha1_kernels.hip), the ``gpu_mode='disable'`` paths and the tests are all written against them.

A corpus is one byte buffer plus ``doc_offsets`` (int64, documents + 1 entries).  A window is ``width`` consecutive *items* of one
document and never crosses into the next document:

* byte mode: an item is a byte; document ``d`` owns bytes ``doc_offsets[d] .. doc_offsets[d+1]``;
* token mode: item ``i`` is ``buf[item_offsets[i]:item_offsets[i+1]]`` and document ``d`` owns items ``doc_offsets[d] ..
  doc_offsets[d+1]`` -- the ``packed=(buf, byte_offsets, set_offsets)`` layout.  A window of ``w`` tokens is the contiguous byte range
  from the start of its first token to the end of its last, so a tokenizer that keeps each word's trailing separator gets the
  natural w-word shingle.

A document of ``m`` items has ``m - width + 1`` windows, exactly one (the whole document) if ``0 < m < width`` and none if it is empty.
Repeated windows stay in (min and max are idempotent); tokens may be empty, and a window of no bytes hashes as ``sha1(b"")``.

Words: :func:`word_table`, :func:`words`, :func:`word_shingles` and :func:`normalize_words` define the w-word shingles of
normalised text -- a 256-byte translate table says which bytes separate and what the others become, a word is a maximal run of
non-separator bytes of one document, and the normal form of a byte-mode corpus is every word followed by exactly one space, as a
token-mode corpus.  ``"the  cat"``, ``"The cat"`` and ``"the cat,"`` then give the same shingle.  The device kernels
(csrc/words_kernels.hip) and ``words=`` of the bulk calls are written against these four.
"""
from __future__ import annotations

import copy
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from datasketch_amd import _native
from datasketch_amd.hashfunc import device_hash, sha1_hash32, sha1_hash64


def _check_width(width) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or width < 1:
        raise ValueError("the shingle width must be an integer >= 1")
    return int(width)


def byte_shingles(doc: bytes, k: int) -> List[bytes]:
    """The ``k``-byte windows of ``doc``, in order; the whole document if it is shorter than ``k``; nothing if it is empty."""
    k = _check_width(k)
    doc = bytes(doc)
    if len(doc) <= k:
        return [doc] if doc else []
    return [doc[i: i + k] for i in range(len(doc) - k + 1)]


def token_shingles(tokens: Sequence[bytes], w: int) -> List[bytes]:
    """The windows of ``w`` consecutive tokens of a document, each as the bytes of its tokens joined; all tokens joined if there are
    fewer than ``w``; nothing if there is no token."""
    w = _check_width(w)
    tokens = [bytes(t) for t in tokens]
    if len(tokens) <= w:
        return [b"".join(tokens)] if tokens else []
    return [b"".join(tokens[i: i + w]) for i in range(len(tokens) - w + 1)]


def window_offsets(doc_offsets, width: int) -> np.ndarray:
    """int64 [documents + 1]: the prefix sums of the per-document window counts -- the CSR offsets of the windows."""
    width = _check_width(width)
    doc_offsets = np.asarray(doc_offsets, dtype=np.int64).reshape(-1)
    if doc_offsets.size < 1:
        raise ValueError("doc_offsets has documents + 1 entries")
    items = np.diff(doc_offsets)
    if np.any(items < 0):
        raise ValueError("doc_offsets must never decrease")
    out = np.zeros(doc_offsets.size, dtype=np.int64)
    np.cumsum(np.where(items == 0, 0, np.where(items < width, 1, items - width + 1)), out=out[1:])
    return out


# ---- words: the normal form of text, and its w-word shingles ------------------------------------------------------------------
# These four ARE the definition too: words_kernels.hip, the gpu_mode='disable' paths of ``words=`` and the tests are written
# against them.
def word_table(lowercase: bool = True, extra: bytes = b"") -> np.ndarray:
    """The default translate table, uint8[256]: ``table[c] == 0`` makes byte ``c`` a separator, any other value is the byte emitted
    for ``c``.  Word bytes are ``0-9 A-Z a-z _``, every byte ``>= 0x80`` (UTF-8 letters stay inside words) and the bytes of
    ``extra``; with ``lowercase``, ``A-Z`` map to ``a-z`` and every other word byte to itself.  Byte 0 is always a separator."""
    extra = bytes(extra)
    if 0 in extra:
        raise ValueError("byte 0 is always a separator: it cannot be in extra")
    table = np.zeros(256, dtype=np.uint8)
    for c in list(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz_") + list(range(0x80, 0x100)) + list(extra):
        table[c] = c
    if lowercase:
        table[ord("A"): ord("Z") + 1] = np.arange(ord("a"), ord("z") + 1, dtype=np.uint8)
    return table


def check_table(table) -> np.ndarray:
    """``table`` (None: the default) as a checked uint8[256]; ``ValueError`` unless it is one with ``table[0] == 0``."""
    if table is None:
        return word_table()
    t = np.asarray(table)
    if t.dtype != np.uint8 or t.shape != (256,):
        raise ValueError("a word table is a uint8 array of 256 entries")
    if t[0] != 0:
        raise ValueError("table[0] must be 0: byte 0 is always a separator")
    return np.ascontiguousarray(t)


def words(doc, table=None) -> List[bytes]:
    """The words of ``doc``: its maximal runs of non-separator bytes, translated."""
    table = check_table(table)
    return [w for w in bytes(doc).translate(table.tobytes()).split(b"\0") if w]


def word_shingles(doc, w: int, table=None) -> List[bytes]:
    """The shingles of ``w`` consecutive words of ``doc``, every word followed by exactly one space -- the last one included -- so
    that a shingle depends on its words alone, never on the separators that stood between them."""
    return token_shingles([x + b" " for x in words(doc, table)], w)


def normalize_words(buf, doc_offsets, table=None, gpu_mode: str = "detect") -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(out_buf, item_offsets, word_doc_offsets)``: the normal form of a byte-mode corpus as a ``packed=`` triple.  ``out_buf`` is
    every word followed by one space; item ``i`` (``item_offsets``, int64[words + 1]) is word ``i`` with its space;
    ``word_doc_offsets`` (int64[documents + 1]) counts in words.  A word never crosses a document boundary.  Fed to ``packed=,
    shingle=w`` it gives :func:`word_shingles`.  One scan-and-compact pass on the device; ``gpu_mode='disable'`` builds it from
    :func:`words`."""
    from datasketch_amd.hyperloglog import _use_gpu

    table = check_table(table)
    buf, _, doc_offsets, _ = check_corpus(buf, None, doc_offsets, 1)
    if _use_gpu(gpu_mode):
        return _native.context().words_normalize(buf, doc_offsets, table)
    raw = buf.tobytes()
    per_doc = [words(raw[int(doc_offsets[d]): int(doc_offsets[d + 1])], table) for d in range(doc_offsets.size - 1)]
    flat = [x + b" " for doc in per_doc for x in doc]
    item_offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, flat), dtype=np.int64, count=len(flat)), out=item_offsets[1:])
    word_doc_offsets = np.zeros(len(per_doc) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, per_doc), dtype=np.int64, count=len(per_doc)), out=word_doc_offsets[1:])
    return np.frombuffer(b"".join(flat), dtype=np.uint8), item_offsets, word_doc_offsets


def words_argument(words_arg) -> Optional[np.ndarray]:
    """``words=`` of the bulk calls: None / False = no word shingles, True = the default table, anything else = a user table."""
    if words_arg is None or words_arg is False:
        return None
    return check_table(None if words_arg is True else words_arg)


# ---- what MinHash.bulk_signatures, HyperLogLog.bulk_registers and sha1_windows share ---------------------------------------
def _as_bytes_array(buf) -> np.ndarray:
    if isinstance(buf, np.ndarray):
        return np.ascontiguousarray(buf).view(np.uint8).reshape(-1)
    return np.frombuffer(memoryview(buf), dtype=np.uint8)


def join_documents(documents) -> Tuple[np.ndarray, np.ndarray]:
    """``documents=`` of the bulk calls as (uint8 buffer, int64 doc_offsets): a ``(buf, doc_offsets)`` pair as it is, or an iterable
    of ``bytes`` / ``str`` joined here (``str`` as its UTF-8 bytes)."""
    if isinstance(documents, tuple) and len(documents) == 2 and not isinstance(documents[1], (bytes, bytearray, str)):
        return _as_bytes_array(documents[0]), np.ascontiguousarray(documents[1], dtype=np.int64).reshape(-1)
    if isinstance(documents, (bytes, bytearray, str)):
        raise ValueError("documents is a (buf, doc_offsets) pair or a list of bytes / str, not one document")
    docs = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in documents]
    doc_offsets = np.zeros(len(docs) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, docs), dtype=np.int64, count=len(docs)), out=doc_offsets[1:])
    return np.frombuffer(b"".join(docs), dtype=np.uint8), doc_offsets


def check_corpus(buf, item_offsets, doc_offsets, width) -> Tuple[np.ndarray, Optional[np.ndarray], np.ndarray, int]:
    """The arrays of a corpus in their canonical types, checked; ``ValueError`` names what is wrong."""
    width = _check_width(width)
    buf = _as_bytes_array(buf)
    doc_offsets = np.ascontiguousarray(doc_offsets, dtype=np.int64).reshape(-1)
    n_items = buf.size
    if item_offsets is not None:
        item_offsets = np.ascontiguousarray(item_offsets, dtype=np.int64).reshape(-1)
        if item_offsets.size < 1 or item_offsets[0] != 0 or item_offsets[-1] > buf.size or np.any(np.diff(item_offsets) < 0):
            raise ValueError("byte_offsets must start at 0, never decrease and end inside buf")
        n_items = item_offsets.size - 1
    if doc_offsets.size < 1 or doc_offsets[0] != 0 or doc_offsets[-1] != n_items or np.any(np.diff(doc_offsets) < 0):
        raise ValueError("the document offsets must start at 0, never decrease and end at the number of %s"
                         % ("bytes of buf" if item_offsets is None else "tokens"))
    return buf, item_offsets, doc_offsets, width


def window_chunks(set_offsets: np.ndarray, max_docs: int, max_windows: int) -> Iterator[Tuple[int, int]]:
    """(s, e) ranges of whole documents: at most ``max_docs`` of them and about ``max_windows`` windows (one document may exceed
    that alone).  The one chunker: every bulk call that cuts a CSR corpus into device calls cuts it here."""
    n, s = set_offsets.size - 1, 0
    while s < n:
        e = min(n, s + max_docs)
        t0 = int(set_offsets[s])
        if int(set_offsets[e]) - t0 > max_windows:
            e = min(e, max(s + 1, int(np.searchsorted(set_offsets, t0 + max_windows, side="right")) - 1))
        yield s, e
        s = e


def corpus_piece(buf, item_offsets, doc_offsets, s: int, e: int):
    """Documents ``s .. e`` as a corpus of their own: (bytes, item offsets or None, doc offsets), offsets starting at 0."""
    i0, i1 = int(doc_offsets[s]), int(doc_offsets[e])
    local_docs = doc_offsets[s: e + 1] - i0
    if item_offsets is None:
        return buf[i0: i1], None, local_docs
    b0 = int(item_offsets[i0])
    return buf[b0: int(item_offsets[i1])], item_offsets[i0: i1 + 1] - b0, local_docs


def host_shingles(buf, item_offsets, doc_offsets, width: int) -> List[List[bytes]]:
    """The shingles of every document of a (checked) corpus, by :func:`byte_shingles` / :func:`token_shingles`."""
    raw = buf.tobytes()
    out = []
    for d in range(doc_offsets.size - 1):
        i0, i1 = int(doc_offsets[d]), int(doc_offsets[d + 1])
        if item_offsets is None:
            out.append(byte_shingles(raw[i0: i1], width))
        else:
            out.append(token_shingles([raw[int(item_offsets[i]): int(item_offsets[i + 1])] for i in range(i0, i1)], width))
    return out


# ---- a text corpus: how packed=, documents=, shingle= and words= of the bulk calls become sets -------------------------------
# Three kinds with the same members, so that MinHash.bulk_signatures and HyperLogLog.bulk_registers each have one loop and neither
# knows which kind it was handed:
#   chunks(max_sets, max_tokens)   pieces of whole sets (documents), offsets re-based to 0, cut by window_chunks
#   host_sets()                    the sets of a piece as lists of bytes: what a host hashfunc is applied to
#   native, arrays()               the device route of a piece: Context.minhash_bulk_<native> / hll_bulk_<native>(**arrays(), ...)
# All three are stored alike -- bytes, item offsets (None: an item is a byte), document offsets -- and checked by check_corpus.
class _Corpus:
    def __init__(self, buf, item_offsets, doc_offsets, width=1):
        self.buf, self.item_offsets, self.doc_offsets, self.width = check_corpus(buf, item_offsets, doc_offsets, width)

    def chunks(self, max_sets: int, max_tokens: int) -> Iterator["_Corpus"]:
        for s, e in window_chunks(self.chunk_offsets(), max_sets, max_tokens):
            piece = copy.copy(self)
            piece.buf, piece.item_offsets, piece.doc_offsets = corpus_piece(self.buf, self.item_offsets, self.doc_offsets, s, e)
            yield piece


class PackedSets(_Corpus):
    """``packed=(buf, byte_offsets, set_offsets)``: a set is its tokens."""
    native = "bytes"

    def chunk_offsets(self) -> np.ndarray:
        return self.doc_offsets

    def arrays(self) -> dict:
        return dict(buf=self.buf, byte_offsets=self.item_offsets, set_offsets=self.doc_offsets)

    def host_sets(self) -> List[List[bytes]]:
        raw, at, sets = self.buf.tobytes(), self.item_offsets.tolist(), self.doc_offsets.tolist()
        return [[raw[at[i]: at[i + 1]] for i in range(sets[j], sets[j + 1])] for j in range(len(sets) - 1)]


class Windows(_Corpus):
    """``documents=`` or ``packed=`` with ``shingle=width``: a set is the windows of ``width`` bytes or tokens of a document."""
    native = "windows"

    def chunk_offsets(self) -> np.ndarray:
        return window_offsets(self.doc_offsets, self.width)  # (a window counts as a token)

    def arrays(self) -> dict:
        return dict(buf=self.buf, doc_offsets=self.doc_offsets, width=self.width, item_offsets=self.item_offsets)

    def host_sets(self) -> List[List[bytes]]:
        return host_shingles(self.buf, self.item_offsets, self.doc_offsets, self.width)


class WordWindows(_Corpus):
    """``documents=`` with ``shingle=width`` and ``words=table``: a set is the windows of ``width`` words of a document."""
    native = "words"

    def __init__(self, buf, doc_offsets, width, table):
        super().__init__(buf, None, doc_offsets, width)
        self.table = table

    def chunk_offsets(self) -> np.ndarray:
        # by bytes: a document has no more windows than words and no more words than bytes, so the bounds hold without knowing
        # the word counts in advance
        return self.doc_offsets

    def arrays(self) -> dict:
        return dict(buf=self.buf, doc_offsets=self.doc_offsets, width=self.width, table=self.table)

    def host_sets(self) -> List[List[bytes]]:
        raw, docs = self.buf.tobytes(), self.doc_offsets.tolist()
        return [word_shingles(raw[docs[d]: docs[d + 1]], self.width, self.table) for d in range(len(docs) - 1)]


def text_corpus(packed, documents, width, table) -> _Corpus:
    """The kind of corpus that ``packed=`` / ``documents=``, ``shingle=width`` and ``words=`` (as its table) name."""
    if documents is not None:
        buf, doc_offsets = join_documents(documents)
        return Windows(buf, None, doc_offsets, width) if table is None else WordWindows(buf, doc_offsets, width, table)
    if not (isinstance(packed, tuple) and len(packed) == 3):
        raise ValueError("packed is a (buf, byte_offsets, set_offsets) triple")
    return PackedSets(*packed) if width is None else Windows(*packed, width)


def flatten(sets) -> Tuple[list, np.ndarray]:
    """(every element of every set, in order; the int64 CSR offsets of the sets into them)."""
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, sets), dtype=np.int64, count=len(sets)), out=offsets[1:])
    return [t for s in sets for t in s], offsets


def sha1_windows(buf, doc_offsets, width: int, item_offsets=None, bits: int = 32, gpu_mode: str = "detect") -> Tuple[np.ndarray, np.ndarray]:
    """``(hashes, set_offsets)``: ``sha1_hash32`` (``bits=32``, uint32) or ``sha1_hash64`` (``bits=64``, uint64) of every shingle of
    the corpus, document by document, and the CSR offsets of the documents into them (:func:`window_offsets`).  One kernel on the
    device, one thread per window, nothing materialised; ``gpu_mode='disable'`` hashes the shingles of this module with hashlib."""
    from datasketch_amd.hyperloglog import _use_gpu

    if bits not in (32, 64):
        raise ValueError("bits must be 32 or 64")
    buf, item_offsets, doc_offsets, width = check_corpus(buf, item_offsets, doc_offsets, width)
    if _use_gpu(gpu_mode):
        return _native.context().sha1_windows(buf, doc_offsets, width, item_offsets, bits)
    f = sha1_hash32 if bits == 32 else sha1_hash64
    flat = [f(s) for doc in host_shingles(buf, item_offsets, doc_offsets, width) for s in doc]
    return np.array(flat, dtype=np.uint32 if bits == 32 else np.uint64), window_offsets(doc_offsets, width)


def hash_windows(buf, doc_offsets, width: int, item_offsets=None, hashfunc=sha1_hash32, gpu_mode: str = "detect") -> Tuple[np.ndarray, np.ndarray]:
    """:func:`sha1_windows` with the hash named by its function: ``(hashes, set_offsets)`` of every shingle of the corpus under
    ``hashfunc``.  One of ``sha1_hash32``, ``sha1_hash64``, ``xxh32_hash32``, ``xxh64_hash64`` is one kernel on the device (uint32
    hashes for the 32-bit two, else uint64); any other callable, or ``gpu_mode='disable'``, is applied to the shingles of this
    module on the host."""
    from datasketch_amd.hyperloglog import _use_gpu

    if not callable(hashfunc):
        raise ValueError("The hashfunc must be a callable.")
    buf, item_offsets, doc_offsets, width = check_corpus(buf, item_offsets, doc_offsets, width)
    known = device_hash(hashfunc)
    if _use_gpu(gpu_mode) and known:
        return _native.context().hash_windows(buf, doc_offsets, width, item_offsets, known[1], known[0])
    flat = [hashfunc(s) for doc in host_shingles(buf, item_offsets, doc_offsets, width) for s in doc]
    return np.array(flat, dtype=np.uint32 if known and known[1] == 32 else np.uint64), window_offsets(doc_offsets, width)
