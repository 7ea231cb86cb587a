"""Text tokenised and normalised on the device (run on an MI355X: python -m pytest tests/test_gpu_words.py -m gpu).

Everything is compared for exact equality with the host path -- datasketch_amd.shingle.words / word_shingles / normalize_words with
gpu_mode='disable', which tests/test_words_host.py holds to the definition by hand-written cases.  The kernels of
csrc/words_kernels.hip work on granules of 16 bytes (one lane), waves of 64 granules (1024 bytes) and tiles of 256 (4096 bytes); the
corpora below put words, separator runs and document boundaries on every one of those edges.  No launcher of words_kernels.hip caps
its grid (one workgroup per tile, one thread per document offset), so there are no later trips to test under debug.cus.
"""
import ctypes

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, shingle
from datasketch_amd import hyperloglog as H
from datasketch_amd import minhash as M
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
INVALID, CAPACITY = _native.MHX_ERR_INVALID, _native.MHX_ERR_CAPACITY
TILE = 4096
ALPHABET = np.frombuffer(b"aB ,\xc3\xa9", dtype=np.uint8)
SPARE = 64
FILL = 0xA5
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _is_word(c):
    return c in b"aB\xc3\xa9"


def _corpus(slide=None):
    """About three tiles (12.6 KB) over ALPHABET, so words are short and boundaries dense:
      [0, 4070)        random bytes, a document boundary every ~20 bytes, one of them planted between two word bytes
      [4070, 4130)     separators -- the zone a 5-byte word slides through (``slide`` = its first byte, 4080 .. 4112), with a
                       document boundary exactly on the tile edge 4096: inside the word whenever it straddles the edge
      [4130, 8230)     one word longer than a tile (it crosses the tile edge 8192 in one piece)
      [8230, 12330)    a separator run longer than a tile
      [12330, 12630)   random bytes again, ending in a word byte
    and runs of three empty documents at the start, in the middle and at the end."""
    rng = np.random.RandomState(5)
    n = 12630
    buf = ALPHABET[rng.randint(0, ALPHABET.size, size=n)].copy()
    buf[4070:4130] = np.frombuffer(b" ,", dtype=np.uint8)[rng.randint(0, 2, size=60)]
    if slide is not None:
        buf[slide: slide + 5] = np.frombuffer(b"aB\xc3\xa9a", dtype=np.uint8)
    buf[4130:8230] = np.frombuffer(b"aB", dtype=np.uint8)[rng.randint(0, 2, size=4100)]
    buf[8230:12330] = np.frombuffer(b" ,", dtype=np.uint8)[rng.randint(0, 2, size=4100)]
    buf[-1] = ord("a")
    cuts = set(int(x) for x in rng.randint(1, 4070, size=200)) | set(int(x) for x in rng.randint(12330, n, size=12))
    inside = next(i for i in range(100, 4070) if _is_word(buf[i - 1]) and _is_word(buf[i]) and i not in cuts)
    cuts |= {inside, TILE, 2000}
    middle = sorted(cuts)[len(cuts) // 2]
    offsets = [0] * 4 + sorted(cuts) + [middle] * 3 + [n] * 4
    doc_offsets = np.array(sorted(offsets), dtype=np.int64)
    assert {int(o) % 4 for o in doc_offsets[:-1]} == {0, 1, 2, 3}
    assert doc_offsets[0] == doc_offsets[3] == 0 and doc_offsets[-4] == n and np.count_nonzero(doc_offsets == middle) == 4
    assert _is_word(buf[inside - 1]) and _is_word(buf[inside]) and _is_word(buf[-1])
    return buf, doc_offsets


def _truncated(n):
    """The first n bytes of the corpus, ending in a word byte, with the documents that fit (the last one cut short)."""
    buf, doc_offsets = _corpus()
    buf = buf[:n].copy()
    buf[-1] = ord("B")
    doc_offsets = np.concatenate([doc_offsets[doc_offsets < n], [n]]).astype(np.int64)
    return buf, doc_offsets


def _degenerate():
    one_byte_docs = (np.frombuffer(b"aB", dtype=np.uint8)[np.arange(TILE + 37) % 2], np.arange(TILE + 38, dtype=np.int64))
    return {
        "no bytes, three documents": (np.zeros(0, dtype=np.uint8), np.zeros(4, dtype=np.int64)),
        "all separators": (np.frombuffer(b" ,", dtype=np.uint8)[np.arange(TILE + 100) % 2], np.array([0, 5, TILE, TILE + 100], dtype=np.int64)),
        "one 1-byte word": (np.frombuffer(b"a", dtype=np.uint8), np.array([0, 1], dtype=np.int64)),
        "one-byte documents": one_byte_docs,
    }


def _same(got, want):
    assert len(got) == 3
    for g, w, name in zip(got, want, ("out_buf", "item_offsets", "word_doc_offsets")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])


def _check(key, buf, doc_offsets):
    want = _cached(key, lambda: shingle.normalize_words(buf, doc_offsets, gpu_mode="disable"))
    _same(shingle.normalize_words(buf, doc_offsets, gpu_mode="always"), want)
    return want


def test_normalize_words_equals_the_host_path():
    buf, doc_offsets = _corpus()
    out, items, word_docs = _check("corpus", buf, doc_offsets)
    lens = np.diff(items)
    assert lens.max() == 4100 + 1 and word_docs[-1] == items.size - 1 > 1000  # the long word is one word


@pytest.mark.parametrize("slide", range(4080, 4113))
def test_a_word_slides_across_granule_wave_and_tile_edges(slide):
    buf, doc_offsets = _corpus(slide)
    _check(("slide", slide), buf, doc_offsets)


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 3 * TILE - 1, 3 * TILE, 3 * TILE + 1])
def test_corpus_lengths_around_a_tile_ending_in_a_word_byte(n):
    buf, doc_offsets = _truncated(n)
    _check(("truncated", n), buf, doc_offsets)


@pytest.mark.parametrize("name", sorted(_degenerate()))
def test_degenerate_corpora(name):
    buf, doc_offsets = _degenerate()[name]
    out, items, word_docs = _check(("degenerate", name), buf, doc_offsets)
    if name == "one-byte documents":
        assert out.size == 2 * buf.size  # the bound of a tile's output
    if name in ("no bytes, three documents", "all separators"):
        assert out.size == 0 and items.tolist() == [0] and not word_docs.any()


def test_user_table_on_the_device():
    buf, doc_offsets = _corpus()
    table = np.zeros(256, dtype=np.uint8)
    table[ord(",")], table[ord("a")], table[0xA9] = ord(";"), ord("Z"), 0xA9  # ',' is a word byte now, 'B', ' ' and 0xC3 separate
    want = shingle.normalize_words(buf, doc_offsets, table, gpu_mode="disable")
    _same(shingle.normalize_words(buf, doc_offsets, table, gpu_mode="always"), want)


def test_capacity_protocol_and_alignments():
    """mhx_words_normalize_dev: the sizing call, capacities one short in either array, exact capacities with SPARE untouched
    elements behind every output -- with the input and the output text on odd addresses."""
    ctx = _native.context()
    buf, doc_offsets = _corpus()
    table = shingle.word_table()
    want = _cached("corpus", lambda: shingle.normalize_words(buf, doc_offsets, gpu_mode="disable"))
    n_docs, n_words, n_out = doc_offsets.size - 1, want[1].size - 1, want[0].size
    d_docs = ctx.to_device(doc_offsets)
    d_in = ctx.alloc(buf.size + 64)
    sizes = (n_out + SPARE + 16, 8 * (n_words + 1 + SPARE), 8 * (n_docs + 1 + SPARE))
    d_text, d_items, d_wdocs = (ctx.alloc(s) for s in sizes)

    def fill():
        for d, s in zip((d_text, d_items, d_wdocs), sizes):
            d.upload(np.full(s, FILL, dtype=np.uint8))

    def untouched():
        return all((d.download(s, np.uint8) == FILL).all() for d, s in zip((d_text, d_items, d_wdocs), sizes))

    for a_in, a_out in ((0, 0), (1, 3), (6, 0), (15, 9), (4, 16)):
        d_in.upload(buf, offset=a_in)
        fill()
        assert ctx.words_normalize_dev(d_in.ptr + a_in, buf.size, d_docs.ptr, n_docs, table) == (0, n_words, n_out)
        args = (d_in.ptr + a_in, buf.size, d_docs.ptr, n_docs, table)
        for cap_bytes, cap_words in ((n_out - 1, n_words), (n_out, n_words - 1), (0, 0)):
            got = ctx.words_normalize_dev(*args, d_text.ptr + a_out, cap_bytes, d_items.ptr, cap_words, d_wdocs.ptr)
            assert got == (CAPACITY, n_words, n_out) and _native.last_error()
        ctx.synchronize()
        assert untouched()
        assert ctx.words_normalize_dev(*args, d_text.ptr + a_out, n_out, d_items.ptr, n_words, d_wdocs.ptr) == (0, n_words, n_out)
        ctx.synchronize()
        text = d_text.download(sizes[0], np.uint8)
        assert np.array_equal(text[a_out: a_out + n_out], want[0]), (a_in, a_out)
        assert (text[:a_out] == FILL).all() and (text[a_out + n_out:] == FILL).all()
        items = d_items.download(n_words + 1 + SPARE, np.int64)
        assert np.array_equal(items[: n_words + 1], want[1]) and (items[n_words + 1:].view(np.uint8) == FILL).all()
        wdocs = d_wdocs.download(n_docs + 1 + SPARE, np.int64)
        assert np.array_equal(wdocs[: n_docs + 1], want[2]) and (wdocs[n_docs + 1:].view(np.uint8) == FILL).all()
    # capacities larger than needed are fine too
    fill()
    assert ctx.words_normalize_dev(*args, d_text.ptr, n_out + 7, d_items.ptr, n_words + 7, d_wdocs.ptr)[0] == 0
    ctx.synchronize()
    assert np.array_equal(d_text.download(n_out, np.uint8), want[0]) and (d_text.download(sizes[0], np.uint8)[n_out:] == FILL).all()


def _word_documents(w):
    """Documents of 0, 1, w-1, w and w+1 words among random text with messy separators."""
    rng = np.random.RandomState(40 + w)
    vocab = [b"the", b"Cat", b"sat", b"on", b"a", b"MAT", "café".encode(), b"x_1", b"42", b"Dog", b"ran"]
    seps = [b" ", b"  ", b", ", b".\n", b" - ", b"\t"]

    def doc(n_words):
        parts = [seps[rng.randint(len(seps))] if rng.randint(3) == 0 else b""]
        for _ in range(n_words):
            parts += [vocab[rng.randint(len(vocab))], seps[rng.randint(len(seps))]]
        return b"".join(parts)

    counts = [0, 1, max(w - 1, 0), w, w + 1, 0, 300] + [int(x) for x in rng.randint(0, 40, size=40)]
    docs = [doc(counts[i]) for i in rng.permutation(len(counts))]
    docs.insert(3, b" ,. ")
    docs.insert(9, b"")
    return docs


@pytest.mark.parametrize("num_perm", [128, 64])
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_signatures_of_word_shingles(w, num_perm):
    docs = _word_documents(w)
    assert {len(shingle.words(d)) for d in docs} >= {0, 1, w - 1, w, w + 1}
    init = np.random.RandomState(9).randint(0, 2**32, size=num_perm).astype(np.uint64)
    for hashfunc in (sha1_hash32, sha1_hash64):
        for extra in ({}, {"hashvalues": init}):
            kw = dict(documents=docs, shingle=w, words=True, num_perm=num_perm, seed=11, hashfunc=hashfunc, **extra)
            want = _cached(("sig", w, num_perm, hashfunc, bool(extra)), lambda: MinHash.bulk_signatures(gpu_mode="disable", **kw))
            for out_dtype in (np.uint64, np.uint32):
                got = MinHash.bulk_signatures(gpu_mode="always", out_dtype=out_dtype, **kw)
                assert got.dtype == out_dtype and got.shape == want.shape
                assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    # the (buf, doc_offsets) form, and the signatures of the definition itself
    kw = dict(num_perm=num_perm, seed=11)
    got = MinHash.bulk_signatures(documents=shingle.join_documents(docs), shingle=w, words=True, gpu_mode="always", **kw)
    assert np.array_equal(got, MinHash.bulk_signatures([shingle.word_shingles(d, w) for d in docs], gpu_mode="disable", **kw))


def test_signatures_with_a_user_table():
    docs = _word_documents(2) + [b"it's well-known", b"its wellknown"]
    table = shingle.word_table(lowercase=False, extra=b"'-")
    kw = dict(documents=docs, shingle=2, words=table, num_perm=128, seed=2)
    want = MinHash.bulk_signatures(gpu_mode="disable", **kw)
    assert np.array_equal(MinHash.bulk_signatures(gpu_mode="always", **kw), want)
    assert not np.array_equal(want, MinHash.bulk_signatures(documents=docs, shingle=2, words=True, num_perm=128, seed=2, gpu_mode="disable"))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_registers_of_word_shingles(w, bits):
    docs = _word_documents(w)
    kw = dict(documents=docs, shingle=w, words=True, p=8, hashfunc=sha1_hash32 if bits == 32 else sha1_hash64, hash_bits=bits)
    want = HyperLogLog.bulk_registers(gpu_mode="disable", **kw)
    assert np.array_equal(HyperLogLog.bulk_registers(gpu_mode="always", **kw), want)


def test_chunks_of_whole_documents(monkeypatch):
    docs = _word_documents(3)
    want = MinHash.bulk_signatures(documents=docs, shingle=3, words=True, num_perm=64, gpu_mode="always")
    want_reg = HyperLogLog.bulk_registers(documents=docs, shingle=3, words=True, p=6, gpu_mode="always")
    monkeypatch.setattr(M, "_BULK_CHUNK_SETS", 7)
    monkeypatch.setattr(M, "_BULK_CHUNK_TOKENS", 500)
    monkeypatch.setattr(H, "_BULK_CHUNK_TOKENS", 500)
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=3, words=True, num_perm=64, gpu_mode="always"), want)
    assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=3, words=True, p=6, gpu_mode="always"), want_reg)


def test_cabi_arguments():
    """Every invalid input of the host forms and the checks of the device form: MHX_ERR_INVALID with a message, and a valid call
    right after each succeeds."""
    ctx = _native.context()
    lib = ctx.lib
    perm = ctx.perm_handle(MinHash(num_perm=16, seed=1, gpu_mode="disable").permutations)
    buf = np.frombuffer(b"ab cd, efg", dtype=np.uint8)
    docs = np.array([0, 4, 10], dtype=np.int64)
    table = shingle.word_table()
    bad_table = table.copy()
    bad_table[0] = 1
    text, items, wdocs = np.empty(32, dtype=np.uint8), np.empty(8, dtype=np.int64), np.empty(3, dtype=np.int64)
    sig, reg = np.empty((2, 16), dtype=np.uint64), np.empty((2, 256), dtype=np.uint8)
    nw, nb = ctypes.c_int64(0), ctypes.c_int64(0)
    P = _native._ptr
    d = ctx.alloc(4096)
    image = np.zeros(4096, dtype=np.uint8)  # document offsets at 0, the bytes at 1024
    image[:24], image[1024:1034] = docs.view(np.uint8), buf
    d.upload(image)

    def arr(*values):
        return np.array(values, dtype=np.int64)

    def normalize(bytes_=buf, n_bytes=10, doc_offsets=docs, n_docs=2, t=table, o=text, cap_bytes=32, it=items, cap_words=7, wd=wdocs, c=ctx.handle,
                  p_nw=ctypes.byref(nw), p_nb=ctypes.byref(nb)):
        return lib.mhx_words_normalize(c, P(bytes_), n_bytes, P(doc_offsets), n_docs, P(t), P(o), cap_bytes, P(it), cap_words, P(wd), p_nw, p_nb)

    def minhash(bytes_=buf, n_bytes=10, doc_offsets=docs, n_docs=2, t=table, width=2, dtype=U32, c=perm, o=sig, init=None, stride=0, out_dtype=U64):
        return lib.mhx_minhash_bulk_words_typed(c, P(bytes_), n_bytes, P(doc_offsets), n_docs, P(t), width, dtype, P(init), stride, P(o), out_dtype)

    def hll(bytes_=buf, n_bytes=10, doc_offsets=docs, n_docs=2, t=table, width=2, c=ctx.handle, o=reg, bits=32, p=8, stride=0):
        return lib.mhx_hll_bulk_words(c, P(bytes_), n_bytes, P(doc_offsets), n_docs, P(t), width, bits, p, None, stride, P(o))

    def dev(c=ctx.handle, n_bytes=10, n_docs=2, t=table, d_bytes=d.ptr + 1024, d_docs=d.ptr, d_o=d.ptr + 2048, cap_bytes=32, d_it=d.ptr + 2304,
            cap_words=7, d_wd=d.ptr + 2560, p_nw=ctypes.byref(nw), p_nb=ctypes.byref(nb)):
        return lib.mhx_words_normalize_dev(c, d_bytes, n_bytes, d_docs, n_docs, P(t), d_o, cap_bytes, d_it, cap_words, d_wd, p_nw, p_nb)

    calls = {"mhx_words_normalize": normalize, "mhx_minhash_bulk_words_typed": minhash, "mhx_hll_bulk_words": hll, "mhx_words_normalize_dev": dev}
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_WORDS
    for name, call in calls.items():
        assert call() == 0, (name, _native.last_error())
    ctx.synchronize()
    # "ab c" | "d, efg": the boundary cuts "cd" in two
    assert (nw.value, nb.value) == (4, 11) and text[:11].tobytes() == b"ab c d efg " and items[:5].tolist() == [0, 3, 5, 7, 11] and wdocs.tolist() == [0, 2, 4]
    corpus_cases = (
        {"n_bytes": -1}, {"n_docs": -1}, {"t": None}, {"t": bad_table}, {"doc_offsets": None}, {"bytes_": None},
        {"doc_offsets": arr(1, 4, 10)}, {"doc_offsets": arr(0, 4, 9)}, {"doc_offsets": arr(0, 4, 11)}, {"doc_offsets": arr(0, 11, 10)}, {"c": None},
    )
    cases = {
        "mhx_words_normalize": corpus_cases + ({"p_nw": None}, {"p_nb": None}, {"cap_bytes": -1}, {"cap_words": -1}, {"o": None}, {"it": None},
                                               {"wd": None}),
        "mhx_minhash_bulk_words_typed": corpus_cases + ({"width": 0}, {"width": -2}, {"dtype": 7}, {"out_dtype": 7}, {"o": None}, {"stride": 3}),
        "mhx_hll_bulk_words": corpus_cases + ({"width": 0}, {"bits": 16}, {"p": 3}, {"p": 17}, {"o": None}, {"stride": 5}),
        "mhx_words_normalize_dev": ({"n_bytes": -1}, {"n_docs": -1}, {"t": None}, {"t": bad_table}, {"d_docs": None}, {"d_bytes": None}, {"c": None},
                                    {"p_nw": None}, {"p_nb": None}, {"cap_bytes": -1}, {"cap_words": -1}, {"d_it": None}, {"d_wd": None}, {"d_o": None}),
    }
    for name, call in calls.items():
        for case in cases[name]:
            assert call(**case) == INVALID, (name, case)
            assert _native.last_error(), (name, case)
            assert call() == 0, (name, case, _native.last_error())
    # capacities one short: the totals come back, nothing is written (the host form)
    text[:], items[:], wdocs[:] = FILL, -1, -1
    for case in ({"cap_bytes": 10}, {"cap_words": 3}):
        nw.value = nb.value = -1
        assert normalize(**case) == CAPACITY and (nw.value, nb.value) == (4, 11) and _native.last_error()
    assert (text == FILL).all() and (items == -1).all() and (wdocs == -1).all()
    assert normalize(o=None, cap_bytes=0, it=None, cap_words=0, wd=None) == 0 and (nw.value, nb.value) == (4, 11)  # the sizing call
    # n_docs == 0 is a no-op: nothing is read, the totals are 0
    nw.value = nb.value = -1
    assert normalize(bytes_=None, n_bytes=0, doc_offsets=None, n_docs=0) == 0 and (nw.value, nb.value) == (0, 0)
    assert minhash(bytes_=None, n_bytes=0, doc_offsets=None, n_docs=0, o=None) == 0 and hll(bytes_=None, n_bytes=0, doc_offsets=None, n_docs=0, o=None) == 0
    assert dev(n_bytes=0, n_docs=0, d_bytes=None, d_docs=None) == 0
    ctx.synchronize()
