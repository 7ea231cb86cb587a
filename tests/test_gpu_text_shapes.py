"""The text-to-sketch path on corpora of tiny and empty documents (run on an MI355X: python -m pytest
tests/test_gpu_text_shapes.py -m gpu).

tests/test_gpu_shingles.py and tests/test_gpu_words.py are about bytes -- SHA-1 blocks, alignments, granule and tile edges -- on
documents of many windows.  Here the documents are short lines: most give exactly one window and many give none, so that 64
consecutive windows belong to hundreds of documents.  That is where sha1_windows_kernel takes second and later batches of 64
document offsets per trip, where its 64-way search runs three and four rounds and lands behind long runs of tied offsets, and
where words_emit_kernel writes hundreds of documents that start at one byte.

The shapes are lists of per-document window counts from tests/window_owner_model.py, whose lane-by-lane model of the kernel says
what each of them reaches (tests/test_window_owner_model.py asserts it without a GPU).  Every expected hash is computed without
the code under test: the document of window t by np.searchsorted on shingle.window_offsets, its bytes sliced from the buffer,
hashlib.sha1, the first 4 or 8 digest bytes little-endian -- and once more by the gpu_mode='disable' path.  All comparisons are
exact equality.
"""
import hashlib

import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, shingle
from datasketch_amd import hyperloglog as H
from datasketch_amd import minhash as M
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64
from tests import window_owner_model as W

pytestmark = pytest.mark.gpu

TILE = 4096
SEARCH_DEPTH_DOCS = (1, 2, 64, 65, 66, 4096, 4097, 4200)
MODES = {"bytes4": ("bytes", 4), "bytes12": ("bytes", 12), "tokens3": ("tokens", 3)}  # width 4: the brief kernel; 12: the general one
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _device_cus():
    return _cached("cus", lambda: _native.context().info()["compute_units"])


def _shapes():
    shapes = {"one-window runs": W.one_window_runs, "mixed runs": W.mixed_runs, "deep search": W.deep_search}
    for run in W.RUN_LENGTHS:
        shapes["empty runs %d" % run] = lambda run=run: W.empty_runs(run, cus=(_device_cus(), 1))
    for n_docs in SEARCH_DEPTH_DOCS:
        shapes["%d documents" % n_docs] = lambda n_docs=n_docs: W.random_counts(n_docs, n_docs)
    return shapes


SHAPES = _shapes()
LARGER = ["one-window runs", "mixed runs", "deep search", "empty runs 64", "empty runs 129", "empty runs 200", "4096 documents", "4097 documents",
          "4200 documents"]


def _first8(raw, beg, end):
    return np.fromiter((int.from_bytes(hashlib.sha1(raw[b:e]).digest()[:8], "little") for b, e in zip(beg.tolist(), end.tolist())),
                       dtype=np.uint64, count=len(beg))


def _expected(buf, item_offsets, doc_offsets, width):
    """(the first 8 digest bytes of every window as a little-endian uint64, set_offsets), from the definition alone."""
    set_offsets = shingle.window_offsets(doc_offsets, width)
    t = np.arange(int(set_offsets[-1]))
    d = np.searchsorted(set_offsets[:-1], t, side="right") - 1
    first = doc_offsets[d] + (t - set_offsets[d])
    last = first + np.minimum(width, doc_offsets[d + 1] - doc_offsets[d])
    assert (last <= doc_offsets[d + 1]).all()
    if item_offsets is not None:
        first, last = item_offsets[first], item_offsets[last]
    return _first8(buf.tobytes(), first, last), set_offsets


def _as_bits(h64, bits):
    return h64 if bits == 64 else (h64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _corpus_of(shape, mode):
    """(buf, item_offsets or None, doc_offsets, width, the expected uint64 hashes, set_offsets), cached."""
    def make():
        counts = SHAPES[shape]()
        kind, width = MODES[mode]
        if kind == "bytes":
            buf, doc_offsets = W.byte_corpus(counts, width)
            item_offsets = None
            ones = np.diff(doc_offsets)[np.asarray(counts) == 1]
            assert ones.size < width or set(ones.tolist()) == set(range(1, width + 1))  # one-window documents of 1 .. width bytes
        else:
            buf, item_offsets, doc_offsets = W.token_corpus(counts, width)
            assert np.diff(item_offsets).max() == 3 and np.diff(item_offsets).min() == 0
        want, set_offsets = _expected(buf, item_offsets, doc_offsets, width)
        assert np.array_equal(set_offsets, W.set_offsets_of(counts))  # the corpus has the shape
        for bits in (32, 64):
            host, host_offsets = shingle.sha1_windows(buf, doc_offsets, width, item_offsets=item_offsets, bits=bits, gpu_mode="disable")
            assert np.array_equal(host_offsets, set_offsets) and host.dtype == _as_bits(want, bits).dtype and np.array_equal(host, _as_bits(want, bits))
        return buf, item_offsets, doc_offsets, width, want, set_offsets
    return _cached(("corpus", shape, mode), make)


def _run(shape, mode, ctx=None):
    buf, item_offsets, doc_offsets, width, want, want_offsets = _corpus_of(shape, mode)
    for bits in (32, 64):
        if ctx is None:
            got, set_offsets = shingle.sha1_windows(buf, doc_offsets, width, item_offsets=item_offsets, bits=bits, gpu_mode="always")
        else:
            got, set_offsets = ctx.sha1_windows(buf, doc_offsets, width, item_offsets, bits)
        expect = _as_bits(want, bits)
        assert got.dtype == expect.dtype and np.array_equal(set_offsets, want_offsets)
        wrong = np.flatnonzero(got != expect)
        assert wrong.size == 0, (shape, mode, bits, wrong.size, wrong[:8], (np.searchsorted(want_offsets[:-1], wrong[:8], side="right") - 1))


# ---- sha1_windows on document-shape edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shapes_on_the_default_grid(shape, mode):
    _run(shape, mode)


def test_what_the_shapes_reach_on_this_device():
    """The model at this device's CU count (tests/test_window_owner_model.py asserts the same for 256 CUs and for one): four
    batches in a trip, the corpus's last trip ending inside a batch, searches of three and four rounds, 64 tied documents in
    front of a wave's first one on the launcher's cut, and the marked documents of the deep corpus at some wave's first window."""
    cus = _device_cus()
    for c in (cus, 1):
        mixed = W.window_owners(W.set_offsets_of(SHAPES["mixed runs"]()), c)
        assert mixed.max_batches >= 4 and mixed.trips[-1][1] >= 3 and mixed.trips[-1][2]
        assert max(W.window_owners(W.set_offsets_of(SHAPES["4200 documents"]()), c).rounds) == 3
        assert max(W.window_owners(W.set_offsets_of(SHAPES["4097 documents"]()), c).rounds) == 2
        counts = SHAPES["empty runs 65"]()
        rep = W.window_owners(W.set_offsets_of(counts), c)
        assert any(w[0] > 0 and w[0] % rep.per_wave == 0 and w[3] >= 64 for w in rep.waves)
        assert any(start > 0 and start % rep.per_wave == 0 for start, _ in W.starts_of_runs(counts, 0))
        deep = W.window_owners(W.set_offsets_of(SHAPES["deep search"]()), c)
        assert max(deep.rounds) == 4 and len(deep.waves) >= 100 and set(W.deep_search_marks()) <= deep.wave_first_owners()
    assert W.launch_plan(W.EMPTY_RUNS_TOTAL, 1)[1] > 64


@pytest.fixture(scope="module")
def own_ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("shape", LARGER)
def test_larger_shapes_under_one_cu(own_ctx, shape, mode):
    """debug.cus = 1: 128 waves share the windows, several trips each, and the launcher's cut is no longer every 64 windows."""
    own_ctx.set_option("debug.cus", 1)
    try:
        _run(shape, mode, own_ctx)
    finally:
        own_ctx.set_option("debug.cus", 0)


def _brief_switch_corpus(width):
    """Documents of 10, 11, 12, 13 and 0 bytes, each on all four byte alignments, between longer ones."""
    rng = np.random.RandomState(width)
    docs, at, starts = [], 0, {}
    for length in (10, 11, 12, 13, 0):
        for alignment in (0, 1, 2, 3):
            filler = 14 + (alignment - at - 14) % 4 + 4 * int(rng.randint(0, 20))
            docs += [bytes(rng.randint(0, 256, size=filler, dtype=np.uint8)), bytes(rng.randint(0, 256, size=length, dtype=np.uint8))]
            at += filler
            starts.setdefault(length, set()).add(at % 4)
            at += length
    buf, doc_offsets = shingle.join_documents(docs)
    assert all(s == {0, 1, 2, 3} for s in starts.values()) and {int(o) % 4 for o in doc_offsets[:-1]} == {0, 1, 2, 3}
    assert {10, 11, 12, 13, 0} < set(np.diff(doc_offsets).tolist())
    return buf, doc_offsets


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("width", [10, 11, 12])
def test_byte_widths_around_the_brief_switch(width, bits):
    """Width 11 is the last that takes sha1_one_block<3> (three message words hold 11 bytes and the 0x80), 12 the first that
    does not."""
    buf, doc_offsets = _brief_switch_corpus(width)
    want, want_offsets = _cached(("brief", width), lambda: _expected(buf, None, doc_offsets, width))
    host, host_offsets = shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="disable")
    got, set_offsets = shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="always")
    expect = _as_bits(want, bits)
    assert np.array_equal(host_offsets, want_offsets) and np.array_equal(host, expect)
    assert got.dtype == expect.dtype and np.array_equal(set_offsets, want_offsets)
    assert np.array_equal(got, expect), np.flatnonzero(got != expect)[:8]


# ---- the same shapes through the sinks -------------------------------------------------------------------------------------------
K, WORDS = 5, 2  # bytes per shingle, words per shingle
SHORT = [b"a", b"ok", b"Hi", b"a b", b"x, y", b"Zed", b"no.", b"q 1", b"it", b"A"]  # at most K bytes and WORDS words: one window either way
VOCAB = [b"the", b"Cat", b"sat", b"on", b"a", b"MAT", "café".encode(), b"x_1", b"42", b"Dog", b"ran"]
SEPS = [b" ", b"  ", b", ", b".\n", b" - ", b"\t"]


def _short_lines():
    """About 2 500 documents: titles, log records, blank lines.  Some 60 % give at most one window, there are runs of 65 and
    more one-window documents and of 65 and more empty ones (at the start, inside and at the end), and five long documents."""
    def make():
        rng = np.random.RandomState(21)

        def line(n_words):
            return b"".join(VOCAB[rng.randint(len(VOCAB))] + SEPS[rng.randint(len(SEPS))] for _ in range(n_words))

        def short():
            return SHORT[rng.randint(len(SHORT))]

        docs = [b""] * 70
        for i in range(2000):
            u = rng.rand()
            docs.append(b"" if u < 0.15 else short() if u < 0.45 else b" ,. "[: rng.randint(1, 5)] if u < 0.5 else line(rng.randint(3, 9)))
            if i % 400 == 200:
                docs.append(line(300))
            if i == 700:
                docs += [short() for _ in range(90)]
            if i == 1200:
                docs += [b""] * 66 + [line(4)] + [short() for _ in range(65)] + [b""] * 130
        return docs + [b""] * 67
    return _cached("short lines", make)


def _forms():
    """The corpus as the bulk calls take it: bytes, words, and the words once more as tokens (with and without shingle=)."""
    docs = _short_lines()
    packed = _cached("normal form", lambda: shingle.normalize_words(*shingle.join_documents(docs), gpu_mode="disable"))
    return {"documents": dict(documents=docs, shingle=K), "words": dict(documents=docs, shingle=WORDS, words=True),
            "packed": dict(packed=packed, shingle=WORDS), "tokens": dict(packed=packed)}


FORMS = ("documents", "words", "packed", "tokens")


def _corpus(kw):
    return shingle.text_corpus(kw.get("packed"), kw.get("documents"), kw.get("shingle"), shingle.words_argument(kw.get("words")))


def _longest_run(flags):
    edges = np.flatnonzero(np.diff(np.concatenate([[0], np.asarray(flags, dtype=np.int8), [0]])))
    return int((edges[1::2] - edges[::2]).max()) if edges.size else 0


def test_the_short_lines_are_short():
    docs = _short_lines()
    assert 2000 < len(docs) < 3000
    for name, per_doc in (("documents", [len(shingle.byte_shingles(d, K)) for d in docs]), ("words", [len(shingle.word_shingles(d, WORDS)) for d in docs])):
        per_doc = np.array(per_doc)
        assert 0.5 < np.mean(per_doc <= 1) < 0.7, name
        assert _longest_run(per_doc == 1) >= 65 and _longest_run(per_doc == 0) >= 65 and np.count_nonzero(per_doc > 250) == 5, name
        assert per_doc[0] == per_doc[-1] == 0
    packed = _forms()["packed"]["packed"]
    assert np.array_equal(shingle.window_offsets(packed[2], WORDS), W.set_offsets_of([len(shingle.word_shingles(d, WORDS)) for d in docs]))


def _minhash_want(form, num_perm, with_init):
    kw = dict(_forms()[form], num_perm=num_perm, seed=2)
    if with_init:
        kw["hashvalues"] = np.random.RandomState(3).randint(0, 2**32, size=num_perm).astype(np.uint64)
    return kw, _cached(("minhash", form, num_perm, with_init), lambda: MinHash.bulk_signatures(gpu_mode="disable", **kw))


@pytest.mark.parametrize("with_init", [False, True], ids=["fresh", "init"])
@pytest.mark.parametrize("num_perm", [64, 128])
@pytest.mark.parametrize("form", FORMS)
def test_signatures_of_short_lines(form, num_perm, with_init):
    kw, want = _minhash_want(form, num_perm, with_init)
    for out_dtype in (np.uint64, np.uint32):
        got = MinHash.bulk_signatures(gpu_mode="always", out_dtype=out_dtype, **kw)
        assert got.dtype == out_dtype and got.shape == want.shape == (len(_short_lines()), num_perm)
        assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    if form in ("documents", "words"):  # the signatures of the definition itself
        docs = _short_lines()
        sets = [shingle.byte_shingles(d, K) for d in docs] if form == "documents" else [shingle.word_shingles(d, WORDS) for d in docs]
        rest = {k: v for k, v in kw.items() if k not in ("documents", "shingle", "words")}
        assert np.array_equal(want, MinHash.bulk_signatures(sets, gpu_mode="disable", **rest))
    if with_init:  # a row per document, through the context
        ctx, corpus = _native.context(), _corpus(kw)
        init = np.random.RandomState(4).randint(0, 2**32, size=want.shape).astype(np.uint64)
        fresh = _minhash_want(form, num_perm, False)[1]
        got = getattr(ctx, "minhash_bulk_" + corpus.native)(MinHash(num_perm=num_perm, seed=2, gpu_mode="disable").permutations, init=init, bits=32,
                                                            **corpus.arrays())
        assert np.array_equal(got, np.minimum(fresh, init))


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("form", FORMS)
def test_registers_of_short_lines(form, bits):
    p = 8
    kw = dict(_forms()[form], p=p, hashfunc=sha1_hash32 if bits == 32 else sha1_hash64, hash_bits=bits)
    want = HyperLogLog.bulk_registers(gpu_mode="disable", **kw)
    fresh = HyperLogLog.bulk_registers(gpu_mode="always", **kw)
    assert fresh.dtype == want.dtype and np.array_equal(fresh, want), np.flatnonzero((fresh != want).any(axis=1))[:8]
    if form in ("documents", "words") and bits == 32:
        docs = _short_lines()
        sets = [shingle.byte_shingles(d, K) for d in docs] if form == "documents" else [shingle.word_shingles(d, WORDS) for d in docs]
        assert np.array_equal(want, HyperLogLog.bulk_registers(sets, p=p, gpu_mode="disable"))
    # a shared and a per-document init row through the context (bulk_registers has no init argument)
    ctx, corpus = _native.context(), _corpus(kw)
    rng = np.random.RandomState(6)
    for init in (rng.randint(0, 20, size=1 << p).astype(np.uint8), rng.randint(0, 20, size=want.shape).astype(np.uint8)):
        got = getattr(ctx, "hll_bulk_" + corpus.native)(p=p, hash_bits=bits, init=init, **corpus.arrays())
        assert np.array_equal(got, np.maximum(want, init))


@pytest.mark.parametrize("form", FORMS)
def test_chunk_boundaries_inside_runs_of_empty_documents(form, monkeypatch):
    num_perm, p, max_docs, max_tokens = 64, 8, 50, 400
    kw, want = _minhash_want(form, num_perm, False)
    want_reg = _cached(("registers", form), lambda: HyperLogLog.bulk_registers(gpu_mode="disable", p=p, **_forms()[form]))
    monkeypatch.setattr(M, "_BULK_CHUNK_SETS", max_docs)
    monkeypatch.setattr(M, "_BULK_CHUNK_TOKENS", max_tokens)
    monkeypatch.setattr(H, "_BULK_CHUNK_BYTES", max_docs << p)
    monkeypatch.setattr(H, "_BULK_CHUNK_TOKENS", max_tokens)
    corpus = _corpus(kw)
    empty = np.diff(corpus.doc_offsets) == 0
    cuts = [s for s, _ in shingle.window_chunks(corpus.chunk_offsets(), max_docs, max_tokens)]
    assert len(cuts) > 40 and sum(1 for s in cuts[1:] if empty[s - 1] and empty[s]) >= 3  # cuts between two empty documents
    assert np.array_equal(MinHash.bulk_signatures(gpu_mode="always", **kw), want)
    assert np.array_equal(HyperLogLog.bulk_registers(gpu_mode="always", p=p, **_forms()[form]), want_reg)


def _no_window_corpora():
    n = 200
    nothing, zeros = np.zeros(0, dtype=np.uint8), np.zeros(n + 1, dtype=np.int64)
    seps = [b" ,.\n\t-"[i % 6: i % 6 + 1 + i % 4] for i in range(n)]
    assert all(seps) and not any(shingle.words(d) for d in seps)
    return {
        "empty documents, bytes": dict(documents=(nothing, zeros), shingle=K),
        "empty documents, words": dict(documents=(nothing, zeros), shingle=WORDS, words=True),
        "separators only, words": dict(documents=seps, shingle=WORDS, words=True),
        "no tokens, shingled": dict(packed=(nothing, np.zeros(1, dtype=np.int64), zeros), shingle=WORDS),
        "no tokens": dict(packed=(nothing, np.zeros(1, dtype=np.int64), zeros)),
    }


NORMAL = [b"the cat sat on the mat", b"", b"The  cat, sat", b"x", b"a b c d e f g h"]


@pytest.mark.parametrize("name", sorted(_no_window_corpora()))
def test_corpora_without_a_window(name):
    """max_hashes() == 0: the hash piece has no bytes and launch_sha1_windows returns before it launches; the sinks still deliver
    the empty-set rows or the init rows, and the context is fit for a normal call straight afterwards."""
    kw = _no_window_corpora()[name]
    corpus, ctx, n, k, p = _corpus(kw), _native.context(), 200, 64, 8
    assert corpus.doc_offsets.size == n + 1 and not any(corpus.host_sets())
    perms = MinHash(num_perm=k, seed=5, gpu_mode="disable").permutations
    rng = np.random.RandomState(7)
    if "shingle" in kw:
        normal = dict(kw, documents=NORMAL) if "documents" in kw else dict(kw, packed=shingle.normalize_words(*shingle.join_documents(NORMAL), gpu_mode="disable"))
    else:
        normal = dict(packed=shingle.normalize_words(*shingle.join_documents(NORMAL), gpu_mode="disable"))

    def normal_call_is_correct():
        want = MinHash.bulk_signatures(num_perm=k, seed=5, gpu_mode="disable", **normal)
        assert np.array_equal(MinHash.bulk_signatures(num_perm=k, seed=5, gpu_mode="always", **normal), want)
        assert np.array_equal(HyperLogLog.bulk_registers(p=p, gpu_mode="always", **normal), HyperLogLog.bulk_registers(p=p, gpu_mode="disable", **normal))

    for out_dtype in (np.uint64, np.uint32):
        got = MinHash.bulk_signatures(num_perm=k, seed=5, gpu_mode="always", out_dtype=out_dtype, **kw)
        assert got.dtype == out_dtype and got.shape == (n, k) and (got == M._max_hash).all()
    normal_call_is_correct()
    row = rng.randint(0, 2**32, size=k).astype(np.uint64)
    assert np.array_equal(MinHash.bulk_signatures(num_perm=k, seed=5, hashvalues=row, gpu_mode="always", **kw), np.tile(row, (n, 1)))
    normal_call_is_correct()
    for bits in (32, 64):
        for init in (row, rng.randint(0, 2**32, size=(n, k)).astype(np.uint64)):
            got = getattr(ctx, "minhash_bulk_" + corpus.native)(perms, init=init, bits=bits, **corpus.arrays())
            assert np.array_equal(got, np.broadcast_to(init, (n, k)))
        hashfunc = sha1_hash32 if bits == 32 else sha1_hash64
        got = HyperLogLog.bulk_registers(p=p, hashfunc=hashfunc, hash_bits=bits, gpu_mode="always", **kw)
        assert got.shape == (n, 1 << p) and got.dtype == HyperLogLog.bulk_registers(p=p, gpu_mode="disable", **kw).dtype and not got.any()
        normal_call_is_correct()
        for init in (rng.randint(0, 20, size=1 << p).astype(np.uint8), rng.randint(0, 20, size=(n, 1 << p)).astype(np.uint8)):
            got = getattr(ctx, "hll_bulk_" + corpus.native)(p=p, hash_bits=bits, init=init, **corpus.arrays())
            assert np.array_equal(got, np.broadcast_to(init, (n, 1 << p)))
    normal_call_is_correct()


# ---- the word normaliser: many documents at one byte --------------------------------------------------------------------------
ALPHABET = np.frombuffer(b"aB ,\xc3\xa9", dtype=np.uint8)


def _documents_at_one_byte(n_bytes, ends_in_word):
    """About 1.5 tiles (or exactly two) with 300 documents that start at byte 0, 300 at one byte in the middle of a word, 300 at
    the tile edge 4096 and 700 at n_bytes -- words_emit_kernel writes the first three runs serially from the lane that holds the
    byte, the last in passes of 256 threads of the last tile -- among a few dozen ordinary boundaries."""
    rng = np.random.RandomState(n_bytes + ends_in_word)
    buf = ALPHABET[rng.randint(0, ALPHABET.size, size=n_bytes)].copy()
    middle = 2001
    buf[middle - 1: middle + 1] = np.frombuffer(b"aB", dtype=np.uint8)
    buf[-1] = ord("a") if ends_in_word else ord(",")
    cuts = sorted(set(int(x) for x in rng.randint(1, n_bytes, size=40)) - {middle, TILE})
    doc_offsets = np.array(sorted([0] * 301 + cuts + [middle] * 300 + [TILE] * 300 + [n_bytes] * 701), dtype=np.int64)
    for at, n in ((0, 301), (middle, 300), (TILE, 300), (n_bytes, 701)):
        assert np.count_nonzero(doc_offsets == at) == n
    assert doc_offsets[0] == 0 and doc_offsets[-1] == n_bytes and {int(o) % 4 for o in cuts} == {0, 1, 2, 3}
    return buf, doc_offsets


@pytest.mark.parametrize("ends_in_word", [True, False], ids=["word", "separator"])
@pytest.mark.parametrize("n_bytes", [TILE + TILE // 2 + 37, 2 * TILE])
def test_many_documents_at_one_byte(n_bytes, ends_in_word):
    """2 * TILE: the corpus fills its last tile, so the trailing entries and bit n_bytes fall in the bitmap's extra word."""
    buf, doc_offsets = _documents_at_one_byte(n_bytes, ends_in_word)
    want = shingle.normalize_words(buf, doc_offsets, gpu_mode="disable")
    got = shingle.normalize_words(buf, doc_offsets, gpu_mode="always")
    assert len(got) == 3 and want[2][300] == 0 and want[2][-1] == want[2][-701] == want[1].size - 1 > 500
    for g, w, name in zip(got, want, ("out_buf", "item_offsets", "word_doc_offsets")):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.flatnonzero(g != w)[:8])
