"""Exact overlap of listed pairs on the device (run on an MI355X): mhx_overlap_pairs, mhx_overlap_pairs_dev and the three text
entries against datasketch_amd.overlap.overlap_counts_host (Python sets).  Every comparison is exact integer equality.

The shapes are the smallest at which the kernels can go wrong: the races on one slot (a set of one repeated value), the empty
value of the table and its neighbours as items, keys that collide under a weak slot function, the fullest LDS table, the class
boundary (read from mhx_overlap_limits, never written here) and the first pairs beyond it, a table in scratch larger than any LDS
one, both classes in one call, and -- on a context of the test's own whose launchers see 1 and 3 compute units -- enough pairs for
three trips with a partial last one of the classify pass and of every pair kernel.  Device outputs are pre-filled with 0xA5 and
carry spare elements behind the end that must keep the fill."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from datasketch_amd import _native, lsh_bulk, overlap, shingle
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64
from tests.weighted_dispatch import MI355X_LDS_PER_BLOCK

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
SPARE, FILL = 37, 0xA5
DTYPES = [np.uint32, np.uint64]


def _bits(dtype):
    return np.dtype(dtype).itemsize * 8


def lds_max_items(dtype):
    """the most items of a pair of the LDS class on this device (mhx_overlap_limits)"""
    return _native.overlap_limits(_bits(dtype), MI355X_LDS_PER_BLOCK)


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


def csr(sets, dtype):
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=offsets[1:])
    hashes = np.concatenate([np.asarray(s, dtype=dtype) for s in sets]) if sets else np.empty(0, dtype=dtype)
    return hashes.astype(dtype), offsets


def distinct_values(rng, count, dtype):
    """`count` different values spread over the whole range of dtype (an odd multiplier permutes the integers mod 2^bits)"""
    start = int(rng.randint(0, 1 << 30))
    with np.errstate(over="ignore"):
        v = (np.arange(start, start + count, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) + np.uint64(12345)
        if dtype == np.uint32:
            v = (np.arange(start, start + count, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return v.astype(dtype)


def dev_counts(ctx, hashes, offsets, pairs, max_set_items=None, n_sets=None, with_invalid=True):
    """mhx_overlap_pairs_dev on buffers of the test's own -> (counts [P, 3], invalid)"""
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    n_sets = offsets.size - 1 if n_sets is None else n_sets
    if max_set_items is None:
        max_set_items = int(np.diff(offsets).max()) if offsets.size > 1 else 0
    d_hv, d_offsets, d_pairs = ctx.to_device(hashes), ctx.to_device(offsets), ctx.to_device(pairs)
    count = 3 * pairs.shape[0]
    d_counts = ctx.alloc(4 * (count + SPARE))
    d_counts.upload(np.full(4 * (count + SPARE), FILL, dtype=np.uint8))
    d_bad = ctx.to_device(np.zeros(1, dtype=np.int64))
    ctx.overlap_pairs_dev(d_hv.ptr, U32 if hashes.dtype == np.uint32 else U64, d_offsets.ptr, n_sets, max_set_items, d_pairs.ptr, pairs.shape[0],
                          d_counts.ptr, d_bad.ptr if with_invalid else None)
    ctx.synchronize()
    raw = d_counts.download(4 * (count + SPARE), np.uint8)
    assert np.all(raw[4 * count:] == FILL), "written past the end of the counts"
    invalid = int(d_bad.download((1,), np.int64)[0])
    for buf in (d_hv, d_offsets, d_pairs, d_counts, d_bad):
        buf.free()
    return raw[: 4 * count].view(np.int32).reshape(-1, 3).copy(), invalid


def check_both_entries(ctx, sets, pairs, dtype, want=None):
    hashes, offsets = csr(sets, dtype)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    if want is None:
        want = overlap.overlap_counts_host(hashes, offsets, pairs)
    got = ctx.overlap_pairs(hashes, offsets, pairs)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    got, invalid = dev_counts(ctx, hashes, offsets, pairs)
    assert np.array_equal(got, want) and invalid == 0, np.flatnonzero((got != want).any(axis=1))[:8]
    return want


def every_ordered_pair(n):
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([i.ravel(), j.ravel()], axis=1).astype(np.int64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u32", "u64"])
def test_hand_made_sets(ctx, dtype):
    rng = np.random.RandomState(17)
    top = int(np.iinfo(dtype).max)
    wide = _bits(dtype) - 16
    a = distinct_values(rng, 100, dtype)
    sets = [
        [], [],                                                             # empty against empty and against everything else
        a, a.copy(), a[::-1].copy(), distinct_values(rng, 90, dtype),       # identical (also reversed), disjoint
        np.concatenate([a[:50], distinct_values(rng, 70, dtype)]),          # half of a
        np.full(1000, 77, dtype=dtype), np.full(1000, 78, dtype=dtype),     # the same-slot race: "aaaa..." makes every window equal
        np.full(1000, top, dtype=dtype), np.full(999, 0, dtype=dtype),      # ... on the empty value of the table, and on 0
        [0], [top], [2**32 - 1], [0, top, 5], [5, top], [5, 2**32 - 1, 0], [top, top, 0, 0, 5, 5, top - 1], [top - 1, 1],
        (np.arange(300, dtype=np.uint64) << np.uint64(16) | np.uint64(0x1234)).astype(dtype),              # equal low 16 bits
        ((np.uint64(0xBEEF) << np.uint64(wide)) | np.arange(150, 450, dtype=np.uint64)).astype(dtype),      # equal high 16 bits
        ((np.uint64(0xBEEF) << np.uint64(wide)) | np.arange(0, 300, dtype=np.uint64)).astype(dtype),
        np.arange(1000, dtype=dtype), np.arange(500, 1500, dtype=dtype),    # consecutive integers
        (np.uint64(top - 600) + np.arange(600, dtype=np.uint64)).astype(dtype), (np.uint64(top - 300) + np.arange(301, dtype=np.uint64)).astype(dtype),
    ]
    pairs = every_ordered_pair(len(sets))
    want = check_both_entries(ctx, sets, pairs, dtype)
    at = {tuple(p): w.tolist() for p, w in zip(pairs.tolist(), want)}
    assert at[(0, 1)] == [0, 0, 0] and at[(0, 2)] == [0, 0, 100] and at[(2, 3)] == [100, 100, 100] and at[(2, 4)] == [100, 100, 100]
    assert at[(2, 5)] == [0, 100, 90] and at[(2, 6)] == [50, 100, 120] and at[(7, 7)] == [1, 1, 1] and at[(7, 8)] == [0, 1, 1]
    assert at[(9, 12)] == [1, 1, 1] and at[(9, 10)] == [0, 1, 1] and at[(14, 15)] == [2, 3, 2]
    assert overlap.jaccard_of(want[:2]).tolist() == [1.0, 1.0]  # two empty documents
    # repeated pairs, in any order
    again = pairs[rng.randint(0, len(pairs), 700)]
    check_both_entries(ctx, sets, again, dtype, want=np.array([at[tuple(p)] for p in again.tolist()], dtype=np.int32))


def boundary_sets(rng, dtype, sizes):
    """for every total m: an evenly split pair and a 1 : rest pair, each half overlapping, all values distinct within a set; then the
    same totals with the two sets disjoint (the fullest table of its size)"""
    sets = []
    for m in sizes:
        for a in (m // 2, 1):
            pool = distinct_values(rng, m, dtype)  # the m items are m different values: disjoint sets
            sets += [pool[:a], pool[a:]]
            shared = min(a, m - a) // 2 + 1  # ... and a pair that shares some
            b = np.concatenate([pool[:shared], pool[a + shared:]]) if m - a > shared else pool[:shared]
            sets += [pool[:a], np.resize(b, m - a)]
    return sets


@pytest.mark.parametrize("dtype", DTYPES, ids=["u32", "u64"])
def test_the_class_boundary_the_fullest_table_and_a_table_in_scratch(ctx, dtype):
    rng = np.random.RandomState(23)
    limit = lds_max_items(dtype)
    assert limit >= 1024
    sets = boundary_sets(rng, dtype, (limit - 1, limit, limit + 1))
    big = distinct_values(rng, 2 * limit, dtype)  # 3 x the limit in all: a table in scratch larger than any in LDS
    sets += [big[: 3 * limit // 2], big[limit // 2:]]
    n_big = len(sets)
    small = [distinct_values(rng, int(c), dtype)[rng.randint(0, max(1, int(c)), int(c) + 3 if c else 0)] for c in rng.randint(0, 40, 30)]
    sets += small
    pairs = [(s, s + 1) for s in range(0, n_big, 2)]
    totals = [len(sets[i]) + len(sets[j]) for i, j in pairs]
    assert sorted(set(totals)) == [limit - 1, limit, limit + 1, 3 * limit]
    # small and large pairs interleaved: both classes in one call, results at the right indices
    mixed = []
    for p in pairs:
        mixed += [p, (n_big + rng.randint(0, 30), n_big + rng.randint(0, 30)), (p[1], p[0]), (n_big + rng.randint(0, 30), p[0])]
    want = check_both_entries(ctx, sets, mixed, dtype)
    assert want[0].tolist() == [0, (limit - 1) // 2, limit - 1 - (limit - 1) // 2]
    full = [w for p, w in zip(mixed, want.tolist()) if len(sets[p[0]]) + len(sets[p[1]]) == limit and w[0] == 0 and w[1] + w[2] == limit]
    assert len(full) >= 4  # all-distinct pairs of exactly lds_max_items items


# ---------------------------------------------------------------------------------------------------------------- capped grids
def _trips(items, per_trip):
    full, rest = divmod(items, per_trip)
    return (full + 1, rest) if rest else (full, per_trip)


@pytest.mark.parametrize("dtype", DTYPES, ids=["u32", "u64"])
@pytest.mark.parametrize("cus", [1, 3], ids=["debug_cus_1", "debug_cus_3"])
def test_every_kernel_beyond_its_first_trip(ctx, cus, dtype):
    """Launchers that see `cus` compute units: the classify pass takes 4 x 256 pairs per unit and trip, an LDS bin as many pairs
    as its tables fit the LDS of the units (eight workgroups at the most, 32 waves in the smallest bin), the global class two per unit."""
    rng = np.random.RandomState(31 + cus)
    limit = lds_max_items(dtype)
    key = np.dtype(dtype).itemsize
    tiny = [rng.randint(0, 12, rng.randint(0, 9)).astype(dtype) for _ in range(200)]
    mid = [distinct_values(rng, 800, dtype)[rng.randint(0, 800, 750)] for _ in range(6)]          # 1500 items: the second bin
    top = [distinct_values(rng, 1700, dtype)[rng.randint(0, 1700, 1500)] for _ in range(6)]       # 3000 items: the last bin
    huge = [distinct_values(rng, limit, dtype)[: limit // 2 + 1 + s] for s in range(6)]          # > limit items: scratch
    sets = tiny + mid + top + huge
    n_tiny = 1024 * cus * 2 + 300
    assert _trips(n_tiny, 1024 * cus)[0] == 3 and _trips(n_tiny, 1024 * cus)[1] < 1024 * cus
    pairs = [rng.randint(0, 200, size=(n_tiny, 2))]
    for first, per_cu in ((200, min(8, MI355X_LDS_PER_BLOCK // (64 + 4096 * key + 1024))), (206, min(8, MI355X_LDS_PER_BLOCK // (64 + 2 * limit * key + limit // 2))),
                          (212, 2)):
        n = per_cu * cus * 2 + 1
        assert _trips(n, per_cu * cus) == (3, 1)
        pairs.append(first + rng.randint(0, 6, size=(n, 2)))
    pairs = np.concatenate(pairs)[rng.permutation(sum(len(p) for p in pairs))]
    hashes, offsets = csr(sets, dtype)
    sizes = np.diff(offsets)[pairs].sum(axis=1)
    assert np.any(sizes > limit) and np.any((sizes > 2048) & (sizes <= limit)) and np.any((sizes > 512) & (sizes <= 2048)) and np.any(sizes <= 16)
    want = overlap.overlap_counts_host(hashes, offsets, pairs)
    ctx.set_option("debug.cus", cus)
    try:
        got, invalid = dev_counts(ctx, hashes, offsets, pairs)
        assert np.array_equal(got, want) and invalid == 0, np.flatnonzero((got != want).any(axis=1))[:8]
        assert np.array_equal(ctx.overlap_pairs(hashes, offsets, pairs), want)
        for bins in (1, 2):  # one launch for every LDS pair, sized for the largest; bins with a workgroup per pair in the smallest too
            ctx.set_option("overlap.bins", bins)
            got, invalid = dev_counts(ctx, hashes, offsets, pairs)
            assert np.array_equal(got, want) and invalid == 0, (bins, np.flatnonzero((got != want).any(axis=1))[:8])
    finally:
        ctx.set_option("overlap.bins", 0)
        ctx.set_option("debug.cus", 0)


# -------------------------------------------------------------------------------------------------------------------- bad pairs
@pytest.mark.parametrize("dtype", DTYPES, ids=["u32", "u64"])
def test_dev_entry_answers_bad_pairs_with_minus_one_and_counts_them(ctx, dtype):
    rng = np.random.RandomState(41)
    sets = [rng.randint(0, 60, rng.randint(0, 50)).astype(dtype) for _ in range(20)] + [rng.randint(0, 500, 300).astype(dtype)]
    hashes, offsets = csr(sets, dtype)
    n = len(sets)
    pairs = rng.randint(0, n - 1, size=(400, 2)).astype(np.int64)
    bad_rows = {3: (-1, 2), 4: (2, -1), 50: (n, 0), 51: (0, n), 77: (n + 5, -7), 120: (n - 1, 1), 121: (1, n - 1), 399: (n - 1, n - 1),
                200: (2**40, 1), 201: (1, -2**40)}
    for row, p in bad_rows.items():
        pairs[row] = p
    good = np.array([row not in bad_rows for row in range(400)])
    want = np.full((400, 3), -1, dtype=np.int32)
    want[good] = overlap.overlap_counts_host(hashes, offsets, pairs[good])
    # the last set has 300 items and the caller's bound is 49: a pair that names it is not followed
    got, invalid = dev_counts(ctx, hashes, offsets, pairs, max_set_items=49)
    assert np.array_equal(got, want) and invalid == len(bad_rows)
    got, invalid = dev_counts(ctx, hashes, offsets, pairs, max_set_items=49, with_invalid=False)  # d_invalid NULL: skipped all the same
    assert np.array_equal(got, want) and invalid == 0
    # with the bound that covers it, and fewer sets than the offsets describe: the sets beyond n_sets do not exist
    want[[120, 121, 399]] = overlap.overlap_counts_host(hashes, offsets, pairs[[120, 121, 399]])
    got, invalid = dev_counts(ctx, hashes, offsets, pairs, max_set_items=300)
    assert np.array_equal(got, want) and invalid == len(bad_rows) - 3
    got, invalid = dev_counts(ctx, hashes, offsets, pairs, max_set_items=300, n_sets=10)
    beyond = (pairs >= 10).any(axis=1) | ~good
    assert np.all(got[beyond] == -1) and np.array_equal(got[~beyond], want[~beyond]) and invalid == int(beyond.sum())
    # offsets that decrease make a set of negative size: never followed either (the probe loops are bounded whatever the arrays hold)
    broken = offsets.copy()
    broken[5] = broken[4] - 3
    got, invalid = dev_counts(ctx, hashes, broken, [[4, 0], [0, 0]], max_set_items=300)
    assert got.tolist() == [[-1, -1, -1], want_of(hashes, broken, 0)] and invalid == 1
    # the host form refuses instead, and writes nothing
    counts = np.full((400, 3), 7, dtype=np.int32)
    rc = ctx.lib.mhx_overlap_pairs(ctx.handle, hashes.ctypes.data, U32 if dtype == np.uint32 else U64, offsets.ctypes.data, n, pairs.ctypes.data, 400,
                                   counts.ctypes.data)
    assert rc == _native.MHX_ERR_INVALID and "pair index out of range" in _native.last_error() and np.all(counts == 7)
    with pytest.raises(ValueError, match="pair index out of range"):
        overlap.overlap_counts(hashes, offsets, pairs, gpu_mode="always")


def want_of(hashes, offsets, i):
    size = len(set(hashes[offsets[i]: offsets[i + 1]].tolist()))
    return [size, size, size]


# ------------------------------------------------------------------------------------------------------------------------ text
TEMPLATES = [
    "The committee met on {0} to discuss the budget for the coming year, and agreed that {1} would chair the next session.",
    "Shipping update: your order {0} left the warehouse in {1}; expect delivery within five working days, signature required.",
    "def handler(request_{0}):\n    # TODO({1}): validate input\n    return respond(request_{0}.body, status=200)\n",
    "{0} {0} {1} -- lorem ipsum dolor sit amet, consectetur adipiscing elit, sed do eiusmod tempor incididunt ut labore.",
]


def text_corpus_documents(seed=7, n=200):
    rng = np.random.RandomState(seed)
    names = ["Monday", "Tuesday", "Rotterdam", "Ms. Okafor", "Dr. Lindqvist", "A-1042", "B-77", "x", "payload", "QA"]
    docs = [b"", b"ab", b"a", b"z" * 64, b"z" * 3, b"  ", b"", b"one two"]  # empty, shorter than any width, one repeated byte, separators only
    while len(docs) < n:
        text = TEMPLATES[rng.randint(0, len(TEMPLATES))].format(names[rng.randint(0, 10)], names[rng.randint(0, 10)])
        words = text.split(" ")
        for _ in range(rng.randint(0, 4)):  # edits: a word replaced, dropped or doubled
            at = rng.randint(0, len(words))
            words[at: at + 1] = [[names[rng.randint(0, 10)]], [], [words[at], words[at]]][rng.randint(0, 3)]
        docs.append(" ".join(words).encode())
    docs[30], docs[31], docs[150] = docs[10], docs[3], docs[12]  # equal documents, among the first 40 and beyond
    return docs


def packed_words(docs):
    tokens = [[w + b" " for w in d.split(b" ") if w] for d in docs]
    flat, set_offsets = shingle.flatten(tokens)
    byte_offsets = np.zeros(len(flat) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in flat], out=byte_offsets[1:])
    return np.frombuffer(b"".join(flat), dtype=np.uint8), byte_offsets, set_offsets


_TEXT = {}


def text_case(kind, bits):
    """(keyword arguments, pairs, the counts of the definition): computed once per kind and width of the hash"""
    if "docs" not in _TEXT:
        _TEXT["docs"] = text_corpus_documents()
        i, j = np.triu_indices(40)  # all i < j of the first 40 documents, and i == j
        _TEXT["pairs"] = np.stack([i, j], axis=1).astype(np.int64)
    docs, pairs = _TEXT["docs"], _TEXT["pairs"]
    if (kind, bits) not in _TEXT:
        kwargs = {"bytes k=5": dict(documents=docs, shingle=5), "tokens w=3": dict(packed=packed_words(docs), shingle=3),
                  "tokens": dict(packed=packed_words(docs)), "words w=2": dict(documents=docs, shingle=2, words=True)}[kind]
        corpus = shingle.text_corpus(kwargs.get("packed"), kwargs.get("documents"), kwargs.get("shingle"), shingle.words_argument(kwargs.get("words")))
        f = sha1_hash32 if bits == 32 else sha1_hash64
        flat, offsets = shingle.flatten(corpus.host_sets())
        hashes = np.array([f(t) for t in flat], dtype=np.uint32 if bits == 32 else np.uint64)
        _TEXT[(kind, bits)] = (kwargs, overlap.overlap_counts_host(hashes, offsets, pairs))
    return _TEXT[(kind, bits)] + (pairs,)


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("kind", ["bytes k=5", "tokens w=3", "tokens", "words w=2"])
def test_text_entries_equal_the_definition_over_the_hashed_shingles(kind, bits):
    kwargs, want, pairs = text_case(kind, bits)
    docs = _TEXT["docs"]
    assert len(docs) == 200 and b"" in docs[:40] and docs[30] == docs[10]
    assert want[:, 0].max() > 5 and np.any(want[:, 1] == 0) and np.any((want[:, 0] > 0) & (want[:, 0] < np.minimum(want[:, 1], want[:, 2])))
    got = overlap.text_overlap_counts(pairs, bits=bits, gpu_mode="always", **kwargs)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]
    assert np.array_equal(overlap.text_overlap_counts(pairs, bits=bits, gpu_mode="disable", **kwargs), want)
    assert np.array_equal(overlap.exact_jaccard_pairs(pairs, bits=bits, gpu_mode="always", **kwargs), overlap.jaccard_of(want))
    assert np.array_equal(overlap.exact_containment_pairs(pairs[:, ::-1], bits=bits, gpu_mode="always", **kwargs), overlap.containment_of(want[:, [0, 2, 1]]))
    # every document against itself and the pairs of the whole corpus' equal documents
    n = len(docs)
    same = np.stack([np.arange(n), np.arange(n)], axis=1)
    counts = overlap.text_overlap_counts(same, bits=bits, gpu_mode="always", **kwargs)
    assert np.array_equal(counts, overlap.text_overlap_counts(same, bits=bits, gpu_mode="disable", **kwargs))
    assert np.array_equal(counts[:, 0], counts[:, 1]) and np.array_equal(counts[:, 1], counts[:, 2])


def test_overlap_counts_on_hashes_from_sha1_windows():
    _, want, pairs = text_case("bytes k=5", 64)
    buf, doc_offsets = shingle.join_documents(_TEXT["docs"])
    hashes, offsets = shingle.sha1_windows(buf, doc_offsets, 5, bits=64, gpu_mode="always")
    assert np.array_equal(overlap.overlap_counts(hashes, offsets, pairs, gpu_mode="always"), want)
    assert overlap.overlap_counts(hashes, offsets, np.empty((0, 2), dtype=np.int64), gpu_mode="always").shape == (0, 3)


def test_verified_clusters_of_the_example_equal_the_host_chain():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "verified_near_duplicates.py")
    spec = importlib.util.spec_from_file_location("verified_near_duplicates", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    docs, _ = mod.synthetic_text(1500)
    pairs, exact, labels, sig = mod.verified_clusters(docs, 9, {}, 128, 32, 4, 0.7, "always")
    pairs_h, exact_h, labels_h, sig_h = mod.verified_clusters(docs, 9, {}, 128, 32, 4, 0.7, "disable")
    assert np.array_equal(sig, sig_h) and np.array_equal(pairs, pairs_h) and len(pairs) > 500
    assert np.array_equal(exact, exact_h) and np.array_equal(labels, labels_h)
    keep = exact >= 0.7
    assert 0 < keep.sum() < len(pairs) and np.array_equal(labels, lsh_bulk.connected_components(pairs[keep], len(docs), gpu_mode="disable"))
    # the verification is not the estimate: some pair lies on the other side of the threshold
    est = lsh_bulk.jaccard_pairs(sig_h, pairs, gpu_mode="disable")
    assert np.any((est >= 0.7) != keep)


# ------------------------------------------------------------------------------------------------------------- argument checks
def test_cabi_arguments(ctx):
    lib, h = ctx.lib, ctx.handle
    hashes, offsets = csr([[1, 2, 3], [2, 3, 4], []], np.uint64)
    pairs = np.array([[0, 1], [2, 2]], dtype=np.int64)
    counts = np.full((2, 3), 7, dtype=np.int32)
    P = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def refused(rc, text):
        assert rc == _native.MHX_ERR_INVALID and text in _native.last_error(), (rc, _native.last_error())
        assert np.all(counts == 7), "an output was written"

    # mhx_overlap_pairs
    ok = lambda **kw: lib.mhx_overlap_pairs(*[kw.get(k, v) for k, v in dict(ctx=h, hv=P(hashes), dtype=U64, offsets=P(offsets), n=3, pairs=P(pairs),  # noqa: E731
                                                                          m=2, counts=P(counts)).items()])
    refused(ok(ctx=None), "ctx is NULL")
    refused(ok(dtype=5), "bad hv_dtype")
    refused(ok(n=-1), "n_sets must be >= 0")
    refused(ok(m=-1), "n_pairs must be in")
    refused(ok(m=1 << 31), "n_pairs must be in")
    refused(ok(pairs=None), "NULL host pointer")
    refused(ok(counts=None), "NULL host pointer")
    refused(ok(offsets=None), "NULL host pointer")
    refused(ok(hv=None), "NULL host pointer")
    refused(ok(n=0), "pair index out of range")
    refused(ok(offsets=P(np.array([1, 3, 6, 6], dtype=np.int64))), "set_offsets[0] must be 0")
    refused(ok(offsets=P(np.array([0, 3, 2, 6], dtype=np.int64))), "set_offsets must be non-decreasing (set 1)")
    refused(ok(pairs=P(np.array([[0, 1], [3, 0]], dtype=np.int64))), "pair index out of range (pair 1")
    refused(ok(pairs=P(np.array([[0, -1], [1, 0]], dtype=np.int64))), "pair index out of range (pair 0")
    huge = np.array([0, 1 << 31, (1 << 31) + 1, (1 << 31) + 1], dtype=np.int64)
    refused(ok(offsets=P(huge)), "a set of 2^31 or more items")
    assert ok(m=0, pairs=None, counts=None, hv=None, offsets=None) == 0 and np.all(counts == 7)
    assert ok() == 0 and counts.tolist() == [[2, 3, 3], [0, 0, 0]]
    counts[:] = 7

    # mhx_overlap_pairs_dev: no array is looked at
    dev = ctx.to_device(np.zeros(64, dtype=np.int64))
    d = dev.ptr
    okd = lambda **kw: lib.mhx_overlap_pairs_dev(*[ctypes.c_void_p(v) if k in ("ctx", "hv", "offsets", "pairs", "counts", "invalid") else v  # noqa: E731
                                                   for k, v in {**dict(ctx=h, hv=d, dtype=U64, offsets=d, n=1, most=0, pairs=d, m=1, counts=d + 256, invalid=None), **kw}.items()])
    refused(okd(ctx=None), "ctx is NULL")
    refused(okd(dtype=9), "bad hv_dtype")
    refused(okd(n=-1), "n_sets must be >= 0")
    refused(okd(m=-2), "n_pairs must be in")
    refused(okd(most=-1), "max_set_items must be in")
    refused(okd(most=1 << 31), "fewer than 2^31 items")
    refused(okd(offsets=None), "NULL device pointer")
    refused(okd(pairs=None), "NULL device pointer")
    refused(okd(counts=None), "NULL device pointer")
    refused(okd(hv=None, most=1), "NULL device pointer")
    assert okd(m=0, hv=None, offsets=None, pairs=None, counts=None) == 0 and okd(n=0, hv=None, offsets=None, pairs=None, counts=None) == 0
    assert okd(hv=None) == 0  # sets of no items need no hashes: offsets 0, 0 -> (0, 0, 0)
    ctx.synchronize()
    assert dev.download((3,), np.int32, offset=256).tolist() == [0, 0, 0]
    dev.free()

    # the three text entries: the checks of their twins, then the pairs
    docs = [b"hello world", b"hello there world", b""]
    buf, doc_offsets = shingle.join_documents(docs)
    table = shingle.word_table()
    tok_buf, tok_offsets, tok_sets = packed_words(docs)
    entries = {
        "windows": (lib.mhx_overlap_pairs_windows, dict(ctx=h, bytes=P(buf), items=None, n_items=buf.size, docs=P(doc_offsets), n=3, width=4, dtype=U64,
                                                        pairs=P(pairs), m=2, counts=P(counts))),
        "words": (lib.mhx_overlap_pairs_words, dict(ctx=h, bytes=P(buf), n_bytes=buf.size, docs=P(doc_offsets), n=3, table=P(table), width=1, dtype=U64,
                                                    pairs=P(pairs), m=2, counts=P(counts))),
        "bytes": (lib.mhx_overlap_pairs_bytes, dict(ctx=h, bytes=P(tok_buf), boffs=P(tok_offsets), n_tokens=tok_offsets.size - 1, dtype=U64,
                                                    docs=P(tok_sets), n=3, pairs=P(pairs), m=2, counts=P(counts))),
    }
    decreasing = np.array([0, 20, 11, buf.size], dtype=np.int64)
    for name, (entry, args) in entries.items():
        call = lambda **kw: entry(*{**args, **kw}.values())  # noqa: E731
        refused(call(ctx=None), "ctx is NULL")
        refused(call(dtype=3), "hash_dtype must be")
        refused(call(m=-1), "n_pairs must be in")
        refused(call(pairs=None), "pairs/counts is NULL")
        refused(call(counts=None), "pairs/counts is NULL")
        refused(call(n=-1), "must be >= 0")
        refused(call(n=0), "pair index out of range")
        refused(call(pairs=P(np.array([[0, 3], [0, 0]], dtype=np.int64))), "pair index out of range (pair 0")
        refused(call(docs=None), "NULL")
        if name != "bytes":
            refused(call(width=0), "width")
            refused(call(bytes=None), "bytes is NULL")
            refused(call(docs=P(decreasing)), "non-decreasing" if name == "words" else "doc_offsets")
        else:
            refused(call(boffs=None), "byte_offsets is NULL")
            refused(call(docs=P(np.array([0, 3, 2, 5], dtype=np.int64))), "set_offsets must be non-decreasing")
        if name == "words":
            refused(call(table=None), "table is NULL")
        assert call(m=0, pairs=None, counts=None) == 0 and np.all(counts == 7)
        assert call() == 0, _native.last_error()
        want = overlap.text_overlap_counts(pairs, gpu_mode="disable", bits=64,
                                           **{"windows": dict(documents=docs, shingle=4), "words": dict(documents=docs, shingle=1, words=True),
                                              "bytes": dict(packed=(tok_buf, tok_offsets, tok_sets))}[name])
        assert np.array_equal(counts, want), name
        counts[:] = 7
    for bad in (3, -1):
        with pytest.raises(ValueError, match="overlap.bins must be 0, 1 or 2"):
            ctx.set_option("overlap.bins", bad)
