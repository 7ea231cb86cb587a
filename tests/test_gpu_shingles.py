"""Shingles hashed in place on the device (run on an MI355X: python -m pytest tests/test_gpu_shingles.py -m gpu).

Everything is compared for exact equality with the host path -- hashlib.sha1 over datasketch_amd.shingle.byte_shingles /
token_shingles, which tests/test_shingle_host.py holds to the definition by hand-written cases.  Byte widths sit on the one / two /
three block boundaries of SHA-1 (55/56, 119/120) and on the dword multiples; documents start on all four byte alignments.
"""
import numpy as np
import pytest

from datasketch_amd import HyperLogLog, MinHash, _native, shingle
from datasketch_amd import hyperloglog as H
from datasketch_amd import minhash as M
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
INVALID = _native.MHX_ERR_INVALID
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _byte_corpus(width, seed=0, n_random=34):
    rng = np.random.RandomState(1000 * seed + width)
    lengths = [0, 1, max(width - 1, 0), width, width + 1, 0, 2, 3] + [int(x) for x in rng.randint(0, 301, size=n_random)]
    order = rng.permutation(len(lengths))
    docs = [bytes(rng.randint(0, 256, size=lengths[i], dtype=np.uint8)) for i in order]
    buf, doc_offsets = shingle.join_documents(docs)
    assert {int(o) % 4 for o in doc_offsets[:-1]} == {0, 1, 2, 3}
    return buf, doc_offsets


def _token_corpus(w, seed=0, n_docs=30):
    rng = np.random.RandomState(77 * seed + w)
    counts = [0, 1, max(w - 1, 0), w, w + 1, 0] + [int(x) for x in rng.randint(0, 25, size=n_docs - 6)]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    n_items = sum(counts)
    lens = rng.randint(0, 71, size=n_items)
    lens[rng.randint(0, max(n_items, 1), size=n_items // 6)] = 0
    lens[:4] = [70, 0, 56, 55]
    item_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    buf = rng.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8)
    return buf, item_offsets, doc_offsets


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("width", [1, 3, 4, 5, 8, 9, 55, 56, 64, 119, 120])
def test_byte_windows(width, bits):
    buf, doc_offsets = _byte_corpus(width)
    want, want_offsets = _cached(("bytes", width, bits), lambda: shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="disable"))
    got, set_offsets = shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="always")
    assert got.dtype == want.dtype and np.array_equal(set_offsets, want_offsets)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_token_windows(w, bits):
    buf, item_offsets, doc_offsets = _token_corpus(w)
    sizes = np.diff(item_offsets)
    assert sizes.min() == 0 and sizes.max() == 70
    want, want_offsets = shingle.sha1_windows(buf, doc_offsets, w, item_offsets=item_offsets, bits=bits, gpu_mode="disable")
    got, set_offsets = shingle.sha1_windows(buf, doc_offsets, w, item_offsets=item_offsets, bits=bits, gpu_mode="always")
    window_bytes = item_offsets[np.minimum(np.arange(item_offsets.size - 1) + w, item_offsets.size - 1)] - item_offsets[:-1]
    assert want.size > 100 and window_bytes.min() <= 55 and (w == 1 or window_bytes.max() >= 120)  # both sides of the block boundaries
    assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def _text_documents():
    rng = np.random.RandomState(5)
    docs = [bytes(rng.randint(97, 123, size=int(n), dtype=np.uint8)) for n in rng.randint(0, 400, size=37)]
    docs[4] = b"a" * 333          # every window identical
    docs[9] = b"abc" * 150        # period 3: three distinct windows, each repeated
    docs[11] = b""
    docs[12] = b"xy"              # shorter than the shingle
    docs[20] = b"q" * 5
    return docs


@pytest.mark.parametrize("out_dtype", [np.uint64, np.uint32], ids=["uint64", "uint32"])
@pytest.mark.parametrize("with_init", [False, True], ids=["fresh", "init"])
@pytest.mark.parametrize("num_perm", [128, 64])
def test_signatures_of_documents(num_perm, with_init, out_dtype):
    docs = _text_documents()
    k = 5
    extra = {"hashvalues": np.random.RandomState(3).randint(0, 2**32, size=num_perm).astype(np.uint64)} if with_init else {}
    kw = dict(num_perm=num_perm, seed=2, **extra)
    want = _cached(("sig", num_perm, with_init), lambda: MinHash.bulk_signatures([shingle.byte_shingles(d, k) for d in docs], gpu_mode="disable", **kw))
    got = MinHash.bulk_signatures(documents=docs, shingle=k, out_dtype=out_dtype, gpu_mode="always", **kw)
    assert got.dtype == out_dtype and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))


@pytest.mark.parametrize("num_perm", [128, 64])
def test_signatures_of_token_shingles_and_sha1_hash64(num_perm):
    buf, item_offsets, doc_offsets = _token_corpus(3, seed=2)
    raw = buf.tobytes()
    sets = [[raw[item_offsets[i]: item_offsets[i + 1]] for i in range(doc_offsets[d], doc_offsets[d + 1])] for d in range(doc_offsets.size - 1)]
    init = np.random.RandomState(4).randint(0, 2**32, size=num_perm).astype(np.uint64)
    for hashfunc in (sha1_hash32, sha1_hash64):
        for extra in ({}, {"hashvalues": init}):
            kw = dict(num_perm=num_perm, seed=9, hashfunc=hashfunc, **extra)
            want = MinHash.bulk_signatures([shingle.token_shingles(s, 3) for s in sets], gpu_mode="disable", **kw)
            got = MinHash.bulk_signatures(packed=(buf, item_offsets, doc_offsets), shingle=3, gpu_mode="always", **kw)
            assert np.array_equal(got, want)
    docs = _text_documents()
    want = MinHash.bulk_signatures([shingle.byte_shingles(d, 9) for d in docs], num_perm=num_perm, hashfunc=sha1_hash64, gpu_mode="disable")
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=9, num_perm=num_perm, hashfunc=sha1_hash64, gpu_mode="always"), want)


@pytest.mark.parametrize("bits", [32, 64])
def test_registers_of_documents(bits):
    docs = _text_documents()
    hashfunc = sha1_hash32 if bits == 32 else sha1_hash64
    kw = dict(p=8, hashfunc=hashfunc, hash_bits=bits)
    want = HyperLogLog.bulk_registers([shingle.byte_shingles(d, 5) for d in docs], gpu_mode="disable", **kw)
    got = HyperLogLog.bulk_registers(documents=docs, shingle=5, gpu_mode="always", **kw)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    buf, item_offsets, doc_offsets = _token_corpus(2, seed=3)
    packed = (buf, item_offsets, doc_offsets)
    want = HyperLogLog.bulk_registers(packed=packed, shingle=2, gpu_mode="disable", **kw)
    assert np.array_equal(HyperLogLog.bulk_registers(packed=packed, shingle=2, gpu_mode="always", **kw), want)
    # a shared and a per-document init row through the C ABI (bulk_registers has no init argument)
    ctx = _native.context()
    rng = np.random.RandomState(6)
    doc_buf, doc_offs = shingle.join_documents(docs)
    fresh = ctx.hll_bulk_windows(doc_buf, doc_offs, 5, 8, None, bits)
    for init in (rng.randint(0, 20, size=256).astype(np.uint8), rng.randint(0, 20, size=(len(docs), 256)).astype(np.uint8)):
        assert np.array_equal(ctx.hll_bulk_windows(doc_buf, doc_offs, 5, 8, None, bits, init), np.maximum(fresh, init))


def test_chunks_of_whole_documents(monkeypatch):
    docs = _text_documents() + [b"tail"]
    docs[17] = bytes(np.random.RandomState(8).randint(97, 101, size=900, dtype=np.uint8))  # more windows than the limit, alone
    buf, item_offsets, doc_offsets = _token_corpus(2, seed=5)
    whole = MinHash.bulk_signatures(documents=docs, shingle=4, num_perm=64, gpu_mode="always")
    whole_tok = MinHash.bulk_signatures(packed=(buf, item_offsets, doc_offsets), shingle=2, num_perm=64, gpu_mode="always")
    whole_reg = HyperLogLog.bulk_registers(documents=docs, shingle=4, p=8, gpu_mode="always")
    monkeypatch.setattr(M, "_BULK_CHUNK_SETS", 5)
    monkeypatch.setattr(M, "_BULK_CHUNK_TOKENS", 300)
    monkeypatch.setattr(H, "_BULK_CHUNK_BYTES", 4 * 256)
    monkeypatch.setattr(H, "_BULK_CHUNK_TOKENS", 300)
    set_offsets = shingle.window_offsets(shingle.join_documents(docs)[1], 4)
    chunks = list(shingle.window_chunks(set_offsets, 5, 300))
    assert len(chunks) > 8 and (17, 18) in chunks
    assert np.array_equal(MinHash.bulk_signatures(documents=docs, shingle=4, num_perm=64, gpu_mode="always"), whole)
    assert np.array_equal(MinHash.bulk_signatures(packed=(buf, item_offsets, doc_offsets), shingle=2, num_perm=64, gpu_mode="always"), whole_tok)
    assert np.array_equal(HyperLogLog.bulk_registers(documents=docs, shingle=4, p=8, gpu_mode="always"), whole_reg)
    assert np.array_equal(whole, MinHash.bulk_signatures(documents=docs, shingle=4, num_perm=64, gpu_mode="disable"))


@pytest.fixture(scope="module")
def own_ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


def test_later_trips_of_the_grid(own_ctx):
    """debug.cus = 1: 32 workgroups of 256 threads, 8 192 windows per trip.  3 600 documents of 4 .. 12 bytes at width 2 give about
    25 000 windows -- more than three trips, with several document boundaries inside every wave -- and a 30 000-byte document in the
    middle gives hundreds of waves with none."""
    rng = np.random.RandomState(12)
    lengths = rng.randint(4, 13, size=3600)
    lengths = np.concatenate([lengths[:1800], [30000], lengths[1800:]])
    doc_offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    buf = rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8)
    width = 2
    assert int((lengths[:1800] - width + 1).sum()) > 8192 and int((lengths - width + 1).sum()) - 29999 > 3 * 8192
    own_ctx.set_option("debug.cus", 1)
    try:
        for bits in (32, 64):
            want, want_offsets = shingle.sha1_windows(buf, doc_offsets, width, bits=bits, gpu_mode="disable")
            got, set_offsets = own_ctx.sha1_windows(buf, doc_offsets, width, None, bits)
            assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
        # the same bytes as tokens of 1 or 2 bytes, windows of 2 tokens: the documents are runs of tokens
        item_lens = rng.randint(1, 3, size=buf.size)
        item_offsets = np.concatenate([[0], np.cumsum(item_lens)]).astype(np.int64)
        item_offsets = item_offsets[: int(np.searchsorted(item_offsets, buf.size, side="right"))]
        n_items = item_offsets.size - 1
        counts = rng.randint(2, 7, size=n_items // 4)
        tok_docs = np.concatenate([[0], np.cumsum(counts)])
        tok_docs = np.concatenate([tok_docs[tok_docs < n_items], [n_items]]).astype(np.int64)
        want, want_offsets = shingle.sha1_windows(buf, tok_docs, 2, item_offsets=item_offsets, gpu_mode="disable")
        assert want.size > 3 * 8192
        got, set_offsets = own_ctx.sha1_windows(buf, tok_docs, 2, item_offsets, 32)
        assert np.array_equal(set_offsets, want_offsets) and np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    finally:
        own_ctx.set_option("debug.cus", 0)


def test_cabi_arguments():
    """Every invalid input of the host forms and the checks of the device form: MHX_ERR_INVALID with a message, and a valid call
    right after each succeeds."""
    ctx = _native.context()
    lib = ctx.lib
    perm = ctx.perm_handle(MinHash(num_perm=16, seed=1, gpu_mode="disable").permutations)
    buf = np.frombuffer(b"abcdefghij", dtype=np.uint8)
    docs = np.array([0, 4, 10], dtype=np.int64)
    items = np.array([0, 2, 3, 7, 10], dtype=np.int64)
    tok_docs = np.array([0, 1, 4], dtype=np.int64)
    out = np.empty(64, dtype=np.uint64)
    sig = np.empty((2, 16), dtype=np.uint64)
    reg = np.empty((2, 256), dtype=np.uint8)
    P = _native._ptr
    d = ctx.alloc(4096)

    def arr(*values):
        return np.array(values, dtype=np.int64)

    def sha1(bytes_=buf, item_offsets=None, n_items=10, doc_offsets=docs, n_docs=2, width=3, dtype=U32, c=ctx.handle, o=out):
        return lib.mhx_sha1_windows(c, P(bytes_), P(item_offsets), n_items, P(doc_offsets), n_docs, width, dtype, P(o))

    def minhash(bytes_=buf, item_offsets=None, n_items=10, doc_offsets=docs, n_docs=2, width=3, dtype=U32, c=perm, o=sig, init=None, stride=0,
                out_dtype=U64):
        return lib.mhx_minhash_bulk_windows_typed(c, P(bytes_), P(item_offsets), n_items, P(doc_offsets), n_docs, width, dtype, P(init), stride, P(o),
                                                  out_dtype)

    def hll(bytes_=buf, item_offsets=None, n_items=10, doc_offsets=docs, n_docs=2, width=3, dtype=U32, c=ctx.handle, o=reg, bits=32, p=8, stride=0):
        return lib.mhx_hll_bulk_windows(c, P(bytes_), P(item_offsets), n_items, P(doc_offsets), n_docs, width, bits, p, None, stride, P(o))

    def dev(c=ctx.handle, n_docs=2, n_windows=6, width=3, dtype=U32, d_docs=d.ptr, d_sets=d.ptr + 256, d_out=d.ptr + 512):
        return lib.mhx_sha1_windows_dev(c, d.ptr + 1024, None, d_docs, d_sets, n_docs, n_windows, width, dtype, d_out)

    def offsets(doc_offsets=docs, n_docs=2, width=3, o=out):
        return lib.mhx_shingle_window_offsets(P(doc_offsets), n_docs, width, P(o.view(np.int64)))

    calls = {"mhx_sha1_windows": sha1, "mhx_minhash_bulk_windows_typed": minhash, "mhx_hll_bulk_windows": hll, "mhx_sha1_windows_dev": dev,
             "mhx_shingle_window_offsets": offsets}
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_SHINGLE
    image = np.zeros(4096, dtype=np.uint8)  # document offsets at 0, set offsets at 256, the bytes at 1024
    image[:24], image[256:280], image[1024:1034] = docs.view(np.uint8), arr(0, 2, 6).view(np.uint8), buf
    d.upload(image)
    for name, call in calls.items():
        assert call() == 0, (name, _native.last_error())
    ctx.synchronize()
    host_cases = (
        {"width": 0}, {"width": -3}, {"n_docs": -1}, {"doc_offsets": None},
        {"doc_offsets": arr(1, 4, 10)},      # does not start at 0
        {"doc_offsets": arr(0, 11, 10)},     # decreases
        {"doc_offsets": arr(0, 4, 9)},       # does not end at the byte count
        {"doc_offsets": arr(0, 4, 11)},
        {"bytes_": None},
        {"item_offsets": arr(1, 2, 3, 7, 10), "n_items": 4, "doc_offsets": tok_docs},   # does not start at 0
        {"item_offsets": arr(0, 3, 2, 7, 10), "n_items": 4, "doc_offsets": tok_docs},   # decreases
        {"item_offsets": items, "n_items": 4, "doc_offsets": arr(0, 1, 5)},            # documents do not end at the number of items
        {"item_offsets": items, "n_items": -1, "doc_offsets": arr(0, 0, -1)},
        {"dtype": 7}, {"c": None}, {"o": None},
    )
    for name in ("mhx_sha1_windows", "mhx_minhash_bulk_windows_typed", "mhx_hll_bulk_windows"):
        call = calls[name]
        cases = list(host_cases)
        if name == "mhx_minhash_bulk_windows_typed":
            cases += [{"stride": 5}, {"out_dtype": 9}]
        if name == "mhx_hll_bulk_windows":
            cases = [c for c in cases if "dtype" not in c] + [{"bits": 16}, {"p": 3}, {"p": 17}, {"stride": 100}]
        for kwargs in cases:
            assert call(**kwargs) == INVALID and _native.last_error(), (name, kwargs)
            assert call() == 0, (name, kwargs, _native.last_error())
        assert call(n_docs=0, doc_offsets=arr(0), n_items=0, bytes_=None, o=None) == 0, name  # a no-op
        assert call(item_offsets=items, n_items=4, doc_offsets=tok_docs) == 0, (name, _native.last_error())
    for kwargs in ({"c": None}, {"width": 0}, {"n_docs": -1}, {"n_windows": -1}, {"dtype": 5}, {"d_docs": None}, {"d_sets": None}, {"d_out": None}):
        assert dev(**kwargs) == INVALID and _native.last_error(), kwargs
        assert dev() == 0
    assert dev(n_docs=0, d_docs=None, d_sets=None, d_out=None) == 0 and dev(n_windows=0, d_out=None) == 0
    for kwargs in ({"width": 0}, {"n_docs": -1}, {"doc_offsets": None}, {"doc_offsets": arr(0, 5, 4)}):
        assert offsets(**kwargs) == INVALID and _native.last_error(), kwargs
        assert offsets() == 0
    ctx.synchronize()
    # the valid calls computed something: the windows of "abcd" | "efghij" at width 3
    assert sha1() == 0
    out_want = [sha1_hash32(s) for s in (b"abc", b"bcd", b"efg", b"fgh", b"ghi", b"hij")]
    assert out.view(np.uint32)[:6].tolist() == out_want
    assert offsets() == 0 and out.view(np.int64)[:3].tolist() == [0, 2, 6]
    assert dev() == 0
    ctx.synchronize()
    assert d.download(4096, np.uint8)[512:536].view(np.uint32).tolist() == out_want
