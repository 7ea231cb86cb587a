"""xxHash on the device (run on an MI355X: python -m pytest tests/test_gpu_xxh.py -m gpu).

Everything is compared for exact equality with the Python definition (datasketch_amd.hashfunc.xxh32_hash32 / xxh64_hash64, which
tests/test_xxh_host.py holds to recorded answers of the xxhash package) over the shingles of datasketch_amd.shingle.  Token lengths
0 .. 140 take the XXH32 stripe loop zero, one and several times with every tail of 4-byte and 1-byte steps, and the XXH64 loop
zero, one and several times (>= 64, >= 96) with every tail of 8-, 4- and 1-byte steps; every length starts on every alignment
mod 8.  The shapes are the smallest at which the kernels can still go wrong.
"""
import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, hash_many, overlap, shingle, xxh32_hash32, xxh64_hash64

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
SHA1, XXH = _native.MHX_HASH_SHA1, _native.MHX_HASH_XXH
INVALID = _native.MHX_ERR_INVALID
FUNC = {32: xxh32_hash32, 64: xxh64_hash64}
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _aligned_tokens():
    """(buf, byte_offsets, the indices of the tokens under test): for every start alignment mod 8 and every length 0 .. 140 one
    token, each behind a pad token of 0 .. 7 bytes that puts it there (the pads are hashed too)."""
    def make():
        rng = np.random.RandomState(21)
        lens, under_test, at = [], [], 0
        for align in range(8):
            for n in range(141):
                pad = (align - at) % 8
                lens += [pad, n]
                under_test.append(len(lens) - 1)
                at += pad + n
        byte_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        starts = byte_offsets[under_test]
        assert {(int(s) % 8, n) for s, n in zip(starts, np.array(lens)[under_test])} == {(a, n) for a in range(8) for n in range(141)}
        return rng.randint(0, 256, size=int(byte_offsets[-1]), dtype=np.uint8), byte_offsets, np.array(under_test)
    return _cached("aligned", make)


def _host_tokens(buf, byte_offsets, bits):
    raw, at, f = buf.tobytes(), byte_offsets.tolist(), FUNC[bits]
    return np.array([f(raw[at[i]: at[i + 1]]) for i in range(len(at) - 1)], dtype=np.uint32 if bits == 32 else np.uint64)


@pytest.mark.parametrize("bits", [32, 64])
def test_tokens_of_every_length_on_every_alignment(bits):
    buf, byte_offsets, under_test = _aligned_tokens()
    want = _cached(("tokens", bits), lambda: _host_tokens(buf, byte_offsets, bits))
    got = _native.context().hash_tokens(buf, byte_offsets, bits, XXH)
    assert got.dtype == want.dtype and under_test.size == 8 * 141
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    # the same through the public call, from Python objects
    raw, at = buf.tobytes(), byte_offsets.tolist()
    tokens = [raw[at[i]: at[i + 1]] for i in under_test[:300].tolist()]
    assert np.array_equal(hash_many(tokens, FUNC[bits], gpu_mode="always"), want[under_test[:300]])


def _byte_corpus(width):
    """Documents of every length 0 .. 2 width + 3, each followed by 0 .. 2 empty ones; then more than 64 one-window documents
    (1 .. width bytes), more than 64 empty ones and again one-window documents, so that one trip of a wave spans several batches
    of 64 document offsets; a long document before and after, so that the runs lie inside a wave's share."""
    rng = np.random.RandomState(100 + width)
    lengths = []
    for n in range(2 * width + 4):
        lengths += [n] + [0] * (n % 3)
    lengths += [5 * width + 70] + [1 + i % width for i in range(70)] + [0] * 150 + [1 + i % width for i in range(75)] + [0] * 70 + [3 * width + 9]
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8), doc_offsets


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("width", [1, 3, 4, 5, 8, 9, 11, 12, 15, 16, 17, 31, 32, 33, 64, 70])
def test_byte_windows(width, bits):
    buf, doc_offsets = _byte_corpus(width)
    want, want_offsets = shingle.hash_windows(buf, doc_offsets, width, hashfunc=FUNC[bits], gpu_mode="disable")
    assert np.array_equal(want_offsets, shingle.window_offsets(doc_offsets, width)) and want.size > 200
    got, set_offsets = shingle.hash_windows(buf, doc_offsets, width, hashfunc=FUNC[bits], gpu_mode="always")
    assert got.dtype == want.dtype and np.array_equal(set_offsets, want_offsets)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def _token_corpus(w):
    """Tokens of every length 0 .. 40 in turn; documents of every count 0 .. 2 w + 3 of them, each followed by empty documents,
    then the runs of _byte_corpus in tokens."""
    rng = np.random.RandomState(200 + w)
    counts = []
    for n in range(2 * w + 4):
        counts += [n] + [0] * (n % 3)
    counts += [5 * w + 70] + [1 + i % w for i in range(70)] + [0] * 150 + [w + 2]
    counts = counts * 2
    n_items = sum(counts)
    lens = np.arange(n_items) % 41
    item_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return rng.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8), item_offsets, doc_offsets


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("w", [1, 3])
def test_token_windows(w, bits):
    buf, item_offsets, doc_offsets = _token_corpus(w)
    want, want_offsets = shingle.hash_windows(buf, doc_offsets, w, item_offsets=item_offsets, hashfunc=FUNC[bits], gpu_mode="disable")
    assert np.array_equal(want_offsets, shingle.window_offsets(doc_offsets, w)) and want.size > 200
    got, set_offsets = shingle.hash_windows(buf, doc_offsets, w, item_offsets=item_offsets, hashfunc=FUNC[bits], gpu_mode="always")
    assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]


# ---- the sinks: a 300-document corpus with empty and one-byte documents in it ---------------------------------------------------
def _text():
    def make():
        rng = np.random.RandomState(31)
        words = [bytes(rng.randint(97, 123, size=int(n), dtype=np.uint8)) for n in rng.randint(1, 9, size=60)]
        docs = []
        for i in range(300):
            n = int(rng.randint(0, 14))
            docs.append(b" ".join(words[j] for j in rng.randint(0, 60, size=n)) + (b"  " if i % 7 == 0 else b""))
        docs[3], docs[4], docs[17], docs[299] = b"", b"q", b"", b"z"
        docs[40] = docs[41][:-3] + b"end"  # a near-duplicate pair
        return docs
    return _cached("text", make)


def _pairs():
    rng = np.random.RandomState(32)
    return np.concatenate([[[40, 41], [3, 17], [3, 4], [4, 299], [5, 5]], rng.randint(0, 300, size=(60, 2))]).astype(np.int64)


def _packed_words(docs):
    sets = [[w + b" " for w in d.split()] for d in docs]
    buf, byte_offsets = _native.Context.pack_tokens([t for s in sets for t in s])
    return buf, byte_offsets, np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)


CORPORA = {
    "bytes": lambda docs: dict(packed=_packed_words(docs)),
    "windows": lambda docs: dict(documents=docs, shingle=5),
    "token_windows": lambda docs: dict(packed=_packed_words(docs), shingle=2),
    "words": lambda docs: dict(documents=docs, shingle=2, words=True),
}


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_the_python_calls_equal_the_host_path_bit_for_bit(corpus, bits):
    docs, f = _text(), FUNC[bits]
    kw = CORPORA[corpus](docs)
    mh = dict(num_perm=64, seed=5, hashfunc=f, **kw)
    want = MinHash.bulk_signatures(gpu_mode="disable", **mh)
    got = MinHash.bulk_signatures(gpu_mode="always", **mh)
    assert got.dtype == want.dtype and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert np.array_equal(MinHash.bulk_signatures(gpu_mode="always", out_dtype=np.uint32, **mh), want.astype(np.uint32))
    hl = dict(p=8, hashfunc=f, hash_bits=bits, **kw)
    want = HyperLogLog.bulk_registers(gpu_mode="disable", **hl)
    got = HyperLogLog.bulk_registers(gpu_mode="always", **hl)
    assert got.dtype == want.dtype and np.array_equal(got, want) and got.any()
    pairs = _pairs()
    want = overlap.text_overlap_counts(pairs, hashfunc=f, gpu_mode="disable", **kw)
    assert np.array_equal(overlap.text_overlap_counts(pairs, hashfunc=f, gpu_mode="always", **kw), want) and want[0, 0] > 0
    assert np.array_equal(overlap.exact_jaccard_pairs(pairs, hashfunc=f, gpu_mode="always", **kw), overlap.jaccard_of(want))
    assert np.array_equal(overlap.exact_containment_pairs(pairs, hashfunc=f, gpu_mode="always", **kw), overlap.containment_of(want))


@pytest.mark.parametrize("bits", [32, 64])
def test_sets_of_python_tokens_and_the_object_calls(bits):
    docs, f = _text(), FUNC[bits]
    sets = [[w + b" " for w in d.split()] for d in docs]
    kw = dict(num_perm=64, seed=5, hashfunc=f)
    want = MinHash.bulk_signatures(sets, gpu_mode="disable", **kw)
    assert np.array_equal(MinHash.bulk_signatures(sets, gpu_mode="always", **kw), want)  # the pack_sets route of _bulk_chunks
    assert np.array_equal(np.array([m.hashvalues for m in MinHash.bulk(sets[:40], gpu_mode="always", **kw)]), want[:40])
    m = MinHash(gpu_mode="always", **kw)
    m.update_batch(sets[41])
    assert np.array_equal(m.hashvalues, want[41])
    hkw = dict(p=8, hashfunc=f, hash_bits=bits)
    assert np.array_equal(HyperLogLog.bulk_registers(sets, gpu_mode="always", **hkw), HyperLogLog.bulk_registers(sets, gpu_mode="disable", **hkw))
    if bits == 32:
        a, b = HyperLogLog(p=8, hashfunc=f, gpu_mode="always"), HyperLogLog(p=8, hashfunc=f, gpu_mode="disable")
        a.update_batch(sets[41])
        b.update_batch(sets[41])
        assert np.array_equal(a.reg, b.reg) and np.any(a.reg)


def _chains(ctx, docs, bits):
    """name of the older entry -> (call(symbol, extra) -> the output array, the index at which the twin takes hash_kind)."""
    lib, P = ctx.lib, _native._ptr
    perm = ctx.perm_handle(MinHash(num_perm=64, seed=5, gpu_mode="disable").permutations)
    code = U32 if bits == 32 else U64
    pbuf, boffs, psets = _packed_words(docs)
    dbuf, ddocs = shingle.join_documents(docs)
    table = shingle.word_table()
    pairs = _pairs()
    n, n_tok, k, n_pairs = len(docs), boffs.size - 1, 64, pairs.shape[0]

    def run(symbol, args, at, kind, out):
        args = list(args)
        if kind is not None:
            args.insert(at, kind)
        rc = getattr(lib, symbol)(*args)
        assert rc == 0, (symbol, _native.last_error())
        return out

    def sig64():
        return np.full((n, k), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)

    def reg():
        return np.full((n, 256), 0xA5, dtype=np.uint8)

    def cnt():
        return np.full((n_pairs, 3), -7, dtype=np.int32)

    def entry(symbol, at, make_out, make_args):
        def call(kind):
            out = make_out()
            return run(symbol if kind is None else symbol + "_hashed", make_args(out), at, kind, out)
        return call

    return {
        "mhx_minhash_bulk_bytes_typed": entry("mhx_minhash_bulk_bytes_typed", 5, sig64, lambda o: (perm, P(pbuf), P(boffs), n_tok, code, P(psets), n, None, 0, P(o))),
        "mhx_minhash_bulk_windows_typed": entry("mhx_minhash_bulk_windows_typed", 8, sig64,
                                                lambda o: (perm, P(dbuf), None, dbuf.size, P(ddocs), n, 5, code, None, 0, P(o), U64)),
        "mhx_minhash_bulk_words_typed": entry("mhx_minhash_bulk_words_typed", 8, sig64,
                                              lambda o: (perm, P(dbuf), dbuf.size, P(ddocs), n, P(table), 2, code, None, 0, P(o), U64)),
        "mhx_hll_bulk_bytes": entry("mhx_hll_bulk_bytes", 5, reg, lambda o: (ctx.handle, P(pbuf), P(boffs), n_tok, bits, P(psets), n, 8, None, 0, P(o))),
        "mhx_hll_bulk_windows": entry("mhx_hll_bulk_windows", 8, reg, lambda o: (ctx.handle, P(dbuf), None, dbuf.size, P(ddocs), n, 5, bits, 8, None, 0, P(o))),
        "mhx_hll_bulk_words": entry("mhx_hll_bulk_words", 8, reg, lambda o: (ctx.handle, P(dbuf), dbuf.size, P(ddocs), n, P(table), 2, bits, 8, None, 0, P(o))),
        "mhx_overlap_pairs_bytes": entry("mhx_overlap_pairs_bytes", 5, cnt,
                                         lambda o: (ctx.handle, P(pbuf), P(boffs), n_tok, code, P(psets), n, P(pairs), n_pairs, P(o))),
        "mhx_overlap_pairs_windows": entry("mhx_overlap_pairs_windows", 8, cnt,
                                           lambda o: (ctx.handle, P(dbuf), None, dbuf.size, P(ddocs), n, 5, code, P(pairs), n_pairs, P(o))),
        "mhx_overlap_pairs_words": entry("mhx_overlap_pairs_words", 8, cnt,
                                         lambda o: (ctx.handle, P(dbuf), dbuf.size, P(ddocs), n, P(table), 2, code, P(pairs), n_pairs, P(o))),
    }


@pytest.mark.parametrize("bits", [32, 64])
def test_the_nine_hashed_chains(bits):
    """With MHX_HASH_SHA1 every `_hashed` twin equals the entry it is named after bit for bit; with MHX_HASH_XXH it equals the host
    path of the Python call."""
    ctx, docs, f = _native.context(), _text(), FUNC[bits]
    chains = _chains(ctx, docs, bits)
    assert sorted(name + "_hashed" for name in chains) == [s for s in _native.EXPORTED_SYMBOLS_XXH if s.endswith("_hashed")]
    for name, call in chains.items():
        old, twin = call(None), call(SHA1)
        assert np.array_equal(old, twin) and not np.array_equal(old, np.full_like(old, old.flat[0])), name
    mh = dict(num_perm=64, seed=5, hashfunc=f, gpu_mode="disable")
    hl = dict(p=8, hashfunc=f, hash_bits=bits, gpu_mode="disable")
    pairs = _pairs()
    for kind, kw in (("bytes", CORPORA["bytes"](docs)), ("windows", CORPORA["windows"](docs)), ("words", CORPORA["words"](docs))):
        assert np.array_equal(chains[f"mhx_minhash_bulk_{kind}_typed"](XXH), MinHash.bulk_signatures(**mh, **kw)), kind
        assert np.array_equal(chains[f"mhx_hll_bulk_{kind}"](XXH).view(np.int8), HyperLogLog.bulk_registers(**hl, **kw)), kind
        assert np.array_equal(chains[f"mhx_overlap_pairs_{kind}"](XXH), overlap.text_overlap_counts(pairs, hashfunc=f, gpu_mode="disable", **kw)), kind


@pytest.fixture(scope="module")
def own_ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


def test_later_trips_of_the_grid(own_ctx):
    """debug.cus = 1: 32 workgroups of 256 threads.  3 600 documents of 4 .. 12 bytes at width 2 give about 25 000 windows, 256 per
    wave: four trips each, with several document boundaries inside every trip.  16 500 tokens are more than two per thread of the
    tokens kernel's 8 192."""
    rng = np.random.RandomState(12)
    lengths = rng.randint(4, 13, size=3600)
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    buf = rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8)
    tok_lens = rng.randint(0, 21, size=16500)
    byte_offsets = np.concatenate([[0], np.cumsum(tok_lens)]).astype(np.int64)
    tok_buf = rng.randint(0, 256, size=int(byte_offsets[-1]), dtype=np.uint8)
    assert int((lengths - 1).sum()) > 2 * 8192 and tok_lens.size > 2 * 8192
    own_ctx.set_option("debug.cus", 1)
    try:
        for bits in (32, 64):
            want, want_offsets = shingle.hash_windows(buf, doc_offsets, 2, hashfunc=FUNC[bits], gpu_mode="disable")
            got, set_offsets = own_ctx.hash_windows(buf, doc_offsets, 2, None, bits, XXH)
            assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
            got = own_ctx.hash_tokens(tok_buf, byte_offsets, bits, XXH)
            assert np.array_equal(got, _host_tokens(tok_buf, byte_offsets, bits)), bits
        # the documents as runs of tokens of 1 or 2 bytes, windows of 2 tokens
        item_lens = rng.randint(1, 3, size=buf.size)
        item_offsets = np.concatenate([[0], np.cumsum(item_lens)]).astype(np.int64)
        item_offsets = item_offsets[: int(np.searchsorted(item_offsets, buf.size, side="right"))]
        n_items = item_offsets.size - 1
        tok_docs = np.concatenate([[0], np.cumsum(rng.randint(2, 7, size=n_items // 4))])
        tok_docs = np.concatenate([tok_docs[tok_docs < n_items], [n_items]]).astype(np.int64)
        want, want_offsets = shingle.hash_windows(buf, tok_docs, 2, item_offsets=item_offsets, hashfunc=xxh64_hash64, gpu_mode="disable")
        assert want.size > 8192  # 128 waves of 64 lanes: every wave takes a second trip
        got, set_offsets = own_ctx.hash_windows(buf, tok_docs, 2, item_offsets, 64, XXH)
        assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    finally:
        own_ctx.set_option("debug.cus", 0)


def test_cabi_arguments():
    """Unknown hash_kind, unknown dtype and NULL outputs on every new entry: MHX_ERR_INVALID with the exact message, the outputs
    untouched, and a valid call right after each succeeds."""
    ctx = _native.context()
    lib, P = ctx.lib, _native._ptr
    perm = ctx.perm_handle(MinHash(num_perm=16, seed=1, gpu_mode="disable").permutations)
    buf = np.frombuffer(b"abcdefghij", dtype=np.uint8)
    docs = np.array([0, 4, 10], dtype=np.int64)
    boffs = np.array([0, 2, 3, 7, 10], dtype=np.int64)
    sets = np.array([0, 1, 4], dtype=np.int64)
    table = shingle.word_table()
    pairs = np.array([[0, 1]], dtype=np.int64)
    out = np.empty(64, dtype=np.uint64)
    sig = np.empty((2, 16), dtype=np.uint64)
    reg = np.empty((2, 256), dtype=np.uint8)
    cnt = np.empty((1, 3), dtype=np.int32)
    DT = "hash_dtype must be MHX_U32 (sha1_hash32) or MHX_U64 (sha1_hash64)"
    BITS = "hash_bits must be 32 (HyperLogLog) or 64 (HyperLogLog++), not 7"

    calls = {
        "mhx_hash_tokens": (out, "bad out_dtype 7", "out is NULL",
                            lambda kind=XXH, dtype=U32, o=out: lib.mhx_hash_tokens(ctx.handle, P(buf), P(boffs), 4, kind, dtype, P(o))),
        "mhx_hash_windows": (out, "bad out_dtype 7", "out is NULL",
                             lambda kind=XXH, dtype=U32, o=out: lib.mhx_hash_windows(ctx.handle, P(buf), None, 10, P(docs), 2, 3, kind, dtype, P(o))),
        "mhx_minhash_bulk_bytes_typed_hashed": (sig, DT, "out/set_offsets is NULL", lambda kind=XXH, dtype=U32, o=sig: lib.mhx_minhash_bulk_bytes_typed_hashed(
            perm, P(buf), P(boffs), 4, dtype, kind, P(sets), 2, None, 0, P(o))),
        "mhx_minhash_bulk_windows_typed_hashed": (sig, DT, "out is NULL", lambda kind=XXH, dtype=U32, o=sig: lib.mhx_minhash_bulk_windows_typed_hashed(
            perm, P(buf), None, 10, P(docs), 2, 3, dtype, kind, None, 0, P(o), U64)),
        "mhx_minhash_bulk_words_typed_hashed": (sig, DT, "out is NULL", lambda kind=XXH, dtype=U32, o=sig: lib.mhx_minhash_bulk_words_typed_hashed(
            perm, P(buf), 10, P(docs), 2, P(table), 2, dtype, kind, None, 0, P(o), U64)),
        "mhx_hll_bulk_bytes_hashed": (reg, BITS, "out/set_offsets is NULL", lambda kind=XXH, dtype=32, o=reg: lib.mhx_hll_bulk_bytes_hashed(
            ctx.handle, P(buf), P(boffs), 4, dtype, kind, P(sets), 2, 8, None, 0, P(o))),
        "mhx_hll_bulk_windows_hashed": (reg, BITS, "out is NULL", lambda kind=XXH, dtype=32, o=reg: lib.mhx_hll_bulk_windows_hashed(
            ctx.handle, P(buf), None, 10, P(docs), 2, 3, dtype, kind, 8, None, 0, P(o))),
        "mhx_hll_bulk_words_hashed": (reg, BITS, "out is NULL", lambda kind=XXH, dtype=32, o=reg: lib.mhx_hll_bulk_words_hashed(
            ctx.handle, P(buf), 10, P(docs), 2, P(table), 2, dtype, kind, 8, None, 0, P(o))),
        "mhx_overlap_pairs_bytes_hashed": (cnt, DT, "pairs/counts is NULL", lambda kind=XXH, dtype=U32, o=cnt: lib.mhx_overlap_pairs_bytes_hashed(
            ctx.handle, P(buf), P(boffs), 4, dtype, kind, P(sets), 2, P(pairs), 1, P(o))),
        "mhx_overlap_pairs_windows_hashed": (cnt, DT, "pairs/counts is NULL", lambda kind=XXH, dtype=U32, o=cnt: lib.mhx_overlap_pairs_windows_hashed(
            ctx.handle, P(buf), None, 10, P(docs), 2, 3, dtype, kind, P(pairs), 1, P(o))),
        "mhx_overlap_pairs_words_hashed": (cnt, DT, "pairs/counts is NULL", lambda kind=XXH, dtype=U32, o=cnt: lib.mhx_overlap_pairs_words_hashed(
            ctx.handle, P(buf), 10, P(docs), 2, P(table), 2, dtype, kind, P(pairs), 1, P(o))),
    }
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_XXH
    for name, (o, bad_dtype, no_out, call) in calls.items():
        assert call() == 0, (name, _native.last_error())
        for kwargs, message in (({"kind": 2}, "unknown hash_kind 2"), ({"kind": -1}, "unknown hash_kind -1"), ({"dtype": 7}, bad_dtype),
                                ({"o": None}, no_out)):
            o.view(np.uint8)[:] = 0xC3
            assert call(**kwargs) == INVALID and _native.last_error() == message, (name, kwargs, _native.last_error())
            assert np.all(o.view(np.uint8) == 0xC3), (name, kwargs)
            assert call() == 0, (name, kwargs, _native.last_error())
        assert call(kind=SHA1) == 0, name
    # the valid calls computed something: the tokens ab | c | defg | hij and the windows of abcd | efghij at width 3
    assert calls["mhx_hash_tokens"][3]() == 0 and out.view(np.uint32)[:4].tolist() == [xxh32_hash32(t) for t in (b"ab", b"c", b"defg", b"hij")]
    assert calls["mhx_hash_windows"][3](dtype=U64) == 0
    assert out[:6].tolist() == [xxh64_hash64(s) for s in (b"abc", b"bcd", b"efg", b"fgh", b"ghi", b"hij")]
