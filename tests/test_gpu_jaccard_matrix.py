"""All-pairs Jaccard on the MI355X through the C ABI (mhx_jaccard_matrix*, mhx_jaccard_threshold_pairs*, and the b-bit
twins): every count equal to numpy's, the threshold lists equal to np.argwhere in (i, j) order, the capacity protocol, and
one 200k-row self-join at scale (ref: datasketch/minhash.py:299-324, b_bit_minhash.py:53-72)."""
import numpy as np
import pytest

from datasketch_amd import _native, b_bit_minhash, lsh_bulk
from oracle import oracle as O

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    return _native.context()


def _counts(a, b, chunk=64):
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.int32)
    for i in range(0, a.shape[0], chunk):
        out[i : i + chunk] = np.count_nonzero(a[i : i + chunk, None, :] == b[None, :, :], axis=2)
    return out


def _planted(rng, m, n, k, dtype=np.uint32, high=False):
    """A [m, k] random; B [n, k] whose rows copy a row of A with a random number of positions (0..k) replaced."""
    top = 1 << 32
    a = rng.randint(0, top, size=(m, k), dtype=np.uint64)
    b = rng.randint(0, top, size=(n, k), dtype=np.uint64)
    src = rng.randint(0, m, size=n)
    for j in range(n):
        keep = rng.random_sample(k) < rng.random_sample()
        b[j, keep] = a[src[j], keep]
    if high:  # uint64 values: some agree only in the low word
        a |= rng.randint(0, 2, size=a.shape).astype(np.uint64) << np.uint64(40)
        b |= rng.randint(0, 2, size=b.shape).astype(np.uint64) << np.uint64(40)
    return a.astype(dtype), b.astype(dtype)


def _dev_matrix(ctx, a, b, k, ldc=None, code=U32):
    d_a = ctx.to_device(a)
    d_b = None if b is None else ctx.to_device(b)
    n_b = a.shape[0] if b is None else b.shape[0]
    ldc = n_b if ldc is None else ldc
    d_c = ctx.alloc(4 * a.shape[0] * ldc)
    d_c.upload(np.full(a.shape[0] * ldc, -7, dtype=np.int32))
    ctx.jaccard_matrix_dev(d_a.ptr, a.shape[0], None if d_b is None else d_b.ptr, n_b, code, k, d_c.ptr, ldc)
    return d_c.download((a.shape[0], ldc), np.int32)


SHAPES = [(1, 1, 1), (2, 63, 3), (63, 64, 64), (64, 65, 100), (65, 127, 128), (127, 129, 256), (129, 2, 320),
          (1000, 65, 128), (4097, 129, 64), (129, 4097, 3)]


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_matrix_counts_equal_numpy_both_dtypes(ctx, m, n, k):
    rng = np.random.RandomState(m * 7 + n + k)
    a, b = _planted(rng, m, n, k)
    want = _counts(a, b)
    assert np.array_equal(_dev_matrix(ctx, a, b, k, code=U32), want)
    assert np.array_equal(_dev_matrix(ctx, a.astype(np.uint64), b.astype(np.uint64), k, code=U64), want)
    assert np.array_equal(ctx.jaccard_matrix(a.astype(np.uint64), b.astype(np.uint64)), want)
    if m == 1000:
        assert set(np.unique(want)) >= {0, k}


@pytest.mark.parametrize("k", [3, 64, 128])
def test_uint64_values_that_differ_only_in_the_high_word_are_not_equal(ctx, k):
    rng = np.random.RandomState(k)
    a, b = _planted(rng, 130, 140, k, dtype=np.uint64, high=True)
    want = _counts(a, b)
    assert not np.array_equal(want, _counts(a & np.uint64(0xFFFFFFFF), b & np.uint64(0xFFFFFFFF)))
    assert np.array_equal(_dev_matrix(ctx, a, b, k, code=U64), want)
    # rows whose high words are zero except in one position of one row: the chunk with it takes the 64-bit comparison
    lo_a, lo_b = a & np.uint64(0xFFFFFFFF), (b & np.uint64(0xFFFFFFFF)).copy()
    lo_b[5, k - 1] = lo_a[3, k - 1] | (np.uint64(1) << np.uint64(63))
    assert np.array_equal(_dev_matrix(ctx, lo_a, lo_b, k, code=U64), _counts(lo_a, lo_b))


def test_self_join_and_a_wider_ldc(ctx):
    rng = np.random.RandomState(3)
    a, _ = _planted(rng, 300, 1, 128)
    a[150:] = a[:150]
    a[150:, :40] ^= 1
    want = _counts(a, a)
    got = _dev_matrix(ctx, a, None, 128, ldc=307)
    assert np.array_equal(got[:, :300], want)
    assert np.all(got[:, 300:] == -7)  # the columns between n_b and ldc are not written
    assert np.array_equal(ctx.jaccard_matrix(a.astype(np.uint64)), want)


def _dev_threshold(ctx, a, b, k, min_count, capacity, code=U32, extra=64):
    d_a = ctx.to_device(a)
    d_b = None if b is None else ctx.to_device(b)
    n_b = 0 if b is None else b.shape[0]
    d_p = ctx.alloc(16 * (capacity + extra))
    d_c = ctx.alloc(4 * (capacity + extra))
    d_p.upload(np.full(2 * (capacity + extra), -5, dtype=np.int64))
    d_c.upload(np.full(capacity + extra, -5, dtype=np.int32))
    total = ctx.jaccard_threshold_pairs_dev(d_a.ptr, a.shape[0], None if d_b is None else d_b.ptr, n_b, code, k, min_count,
                                            d_p.ptr, d_c.ptr, capacity)
    return total, d_p.download((capacity + extra, 2), np.int64), d_c.download(capacity + extra, np.int32)


def _want_pairs(counts, t, self_join):
    keep = counts >= t
    if self_join:
        keep = np.triu(keep, k=1)
    ij = np.argwhere(keep)
    return ij, counts[ij[:, 0], ij[:, 1]]


@pytest.mark.parametrize("m,n,k,t", [(65, 129, 64, 20), (1000, 1000, 128, 64), (4097, 129, 100, 30), (130, 200, 3, 0)])
def test_threshold_pairs_equal_argwhere(ctx, m, n, k, t):
    rng = np.random.RandomState(m + n + k)
    a, b = _planted(rng, m, n, k)
    counts = _counts(a, b)
    ij, c = _want_pairs(counts, t, False)
    total, p, cc = _dev_threshold(ctx, a, b, k, t, len(ij))
    assert total == len(ij)
    assert np.array_equal(p[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c)
    hp, hc = ctx.jaccard_threshold_pairs(a.astype(np.uint64), b.astype(np.uint64), t, capacity=1)  # retry inside
    assert np.array_equal(hp, ij) and np.array_equal(hc, c)
    # the self-join: i < j only
    aa = np.concatenate([a, b])
    full = _counts(aa, aa)
    ij, c = _want_pairs(full, t, True)
    total, p, cc = _dev_threshold(ctx, aa, None, k, t, len(ij) + 3)
    assert total == len(ij) and np.array_equal(p[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c)
    total, p, cc = _dev_threshold(ctx, aa.astype(np.uint64), None, k, t, len(ij), code=U64)
    assert total == len(ij) and np.array_equal(p[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c)


def test_threshold_capacity_overflow_keeps_the_tail_and_reports_the_total(ctx):
    rng = np.random.RandomState(11)
    a, b = _planted(rng, 300, 500, 64)
    ij, c = _want_pairs(_counts(a, b), 10, False)
    assert len(ij) > 200
    for cap in (0, 1, 100, len(ij) - 1):
        total, p, cc = _dev_threshold(ctx, a, b, 64, 10, cap)
        assert total == len(ij)
        assert np.all(p[cap:] == -5) and np.all(cc[cap:] == -5), cap
    total, p, cc = _dev_threshold(ctx, a, b, 64, 10, len(ij))
    assert np.array_equal(p[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c) and np.all(p[len(ij):] == -5)


def test_empty_inputs_and_out_of_range_thresholds(ctx):
    a = np.zeros((5, 16), dtype=np.uint32)
    d_a, d_p, d_c = ctx.to_device(a), ctx.alloc(16 * 4), ctx.alloc(4 * 4)
    assert ctx.jaccard_threshold_pairs_dev(d_a.ptr, 5, d_a.ptr, 0, U32, 16, 1, d_p.ptr, d_c.ptr, 4) == 0
    assert ctx.jaccard_threshold_pairs_dev(d_a.ptr, 0, None, 0, U32, 16, 1, d_p.ptr, d_c.ptr, 4) == 0
    assert _dev_threshold(ctx, a, None, 16, 17, 4)[0] == 0
    total, p, c = _dev_threshold(ctx, a, None, 16, -3, 10)
    assert total == 10 and np.array_equal(p[:10], np.argwhere(np.triu(np.ones((5, 5), bool), k=1))) and np.all(c[:10] == 16)
    assert ctx.jaccard_matrix(np.zeros((0, 8), np.uint64), np.zeros((3, 8), np.uint64)).shape == (0, 3)
    with pytest.raises(ValueError):
        ctx.jaccard_matrix_dev(1, 4, None, 4, U32, 0, 1, 4)  # num_perm <= 0
    with pytest.raises(ValueError):
        ctx.jaccard_matrix_dev(1, 4, 1, 5, U32, 8, 1, 4)  # ldc < n_b


def _bbit_counts(a, b, bits):
    mask = np.uint64((1 << bits) - 1)
    return _counts(a & mask, b & mask)


@pytest.mark.parametrize("bits", [1, 2, 3, 4, 8, 16, 32])
def test_bbit_counts_equal_numpy(ctx, bits):
    k = 100  # not a multiple of the values per block for any b
    rng = np.random.RandomState(bits)
    a, b = _planted(rng, 130, 257, k, dtype=np.uint64)
    pa, pb = ctx.bbit_pack(a, bits), ctx.bbit_pack(b, bits)
    assert np.array_equal(pa, b_bit_minhash.pack_matrix(a, bits, gpu_mode="disable"))
    want = _bbit_counts(a, b, bits)
    assert np.array_equal(ctx.bbit_jaccard_matrix(pa, pb, k, bits), want)
    d_a, d_b = ctx.to_device(pa), ctx.to_device(pb)
    d_c = ctx.alloc(4 * 130 * 260)
    ctx.bbit_jaccard_matrix_dev(d_a.ptr, 130, d_b.ptr, 257, k, bits, d_c.ptr, 260)
    assert np.array_equal(d_c.download((130, 260), np.int32)[:, :257], want)
    t = int(np.percentile(want, 90))
    ij, c = _want_pairs(want, t, False)
    hp, hc = ctx.bbit_jaccard_threshold_pairs(pa, pb, k, bits, t)
    assert np.array_equal(hp, ij) and np.array_equal(hc, c)
    selfc = _bbit_counts(a, a, bits)
    ij, c = _want_pairs(selfc, t, True)
    d_p, d_cc = ctx.alloc(16 * (len(ij) + 1)), ctx.alloc(4 * (len(ij) + 1))
    total = ctx.bbit_jaccard_threshold_pairs_dev(d_a.ptr, 130, None, 0, k, bits, t, d_p.ptr, d_cc.ptr, len(ij) + 1)
    assert total == len(ij)
    assert np.array_equal(d_p.download((len(ij), 2), np.int64), ij) and np.array_equal(d_cc.download(len(ij), np.int32), c)


def test_public_functions_on_the_gpu_equal_the_numpy_path(ctx):
    rng = np.random.RandomState(2)
    a, b = _planted(rng, 200, 150, 128, dtype=np.uint64)
    assert np.array_equal(lsh_bulk.jaccard_matrix(a, b, gpu_mode="always"), lsh_bulk.jaccard_matrix(a, b, gpu_mode="disable"))
    for t in (0.5, 0.3):
        g = lsh_bulk.similar_pairs(np.concatenate([a, b]), threshold=t, gpu_mode="always")
        h = lsh_bulk.similar_pairs(np.concatenate([a, b]), threshold=t, gpu_mode="disable")
        assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])
    blocks = b_bit_minhash.pack_matrix(a, 2)
    g = b_bit_minhash.similar_pairs(blocks, None, 128, 2, threshold=0.4, r=0.1, r_b=0.3)
    h = b_bit_minhash.similar_pairs(blocks, None, 128, 2, threshold=0.4, r=0.1, r_b=0.3, gpu_mode="disable")
    assert np.array_equal(g[0], h[0]) and np.array_equal(g[1], h[1])
    assert np.array_equal(b_bit_minhash.jaccard_matrix(blocks, blocks[:9], 128, 2),
                          b_bit_minhash.jaccard_matrix(blocks, blocks[:9], 128, 2, gpu_mode="disable"))


def _signatures_on_device(ctx, tok, k, seed=1):
    n, t = tok.shape
    pa, pb = O.np_init_permutations(k, seed)
    d_tok, d_sig = ctx.to_device(tok), ctx.alloc(n * k * 4)
    ctx.minhash_bulk_dev((pa, pb), d_tok.ptr, U64, None, t, n, n * t, None, 0, d_sig.ptr, U32)
    return d_sig


def test_dev_forms_on_uint32_signatures_from_the_bulk_kernel(ctx):
    rng = np.random.RandomState(4)
    k, n = 128, 700
    tok = rng.randint(0, 2**32, size=(n, 64), dtype=np.uint64)
    tok[350:] = tok[:350]
    tok[350:, :10] = rng.randint(0, 2**32, size=(350, 10), dtype=np.uint64)  # near-duplicates of the first half
    d_sig = _signatures_on_device(ctx, tok, k)
    sig = d_sig.download((n, k), np.uint32)
    want = _counts(sig, sig)
    d_c = ctx.alloc(4 * n * n)
    ctx.jaccard_matrix_dev(d_sig.ptr, n, None, n, U32, k, d_c.ptr, n)
    assert np.array_equal(d_c.download((n, n), np.int32), want)
    ij, c = _want_pairs(want, 64, True)
    assert len(ij) >= 300
    d_p, d_cc = ctx.alloc(16 * len(ij)), ctx.alloc(4 * len(ij))
    assert ctx.jaccard_threshold_pairs_dev(d_sig.ptr, n, None, 0, U32, k, 64, d_p.ptr, d_cc.ptr, len(ij)) == len(ij)
    assert np.array_equal(d_p.download((len(ij), 2), np.int64), ij) and np.array_equal(d_cc.download(len(ij), np.int32), c)


def test_self_join_at_scale_finds_every_planted_pair(ctx):
    rng = np.random.RandomState(8)
    n, k, t = 200_000, 128, 64
    sig = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64).astype(np.uint32)
    heads = rng.choice(n, size=2000, replace=False)
    members = {}
    for h in heads[:1000]:  # 1000 clusters of 2..4 rows: copies of a head with a quarter of the positions replaced
        others = [x for x in rng.randint(0, n, size=3) if x not in members and x not in heads]
        for o in others:
            sig[o] = sig[h]
            sig[o, rng.random_sample(k) < 0.25] = rng.randint(0, 2**32, dtype=np.uint64)
            members[o] = h
    d_sig = ctx.to_device(sig)
    cap = 1 << 16
    d_p, d_cc = ctx.alloc(16 * cap), ctx.alloc(4 * cap)
    total = ctx.jaccard_threshold_pairs_dev(d_sig.ptr, n, None, 0, U32, k, t, d_p.ptr, d_cc.ptr, cap)
    assert 0 < total <= cap
    pairs, counts = d_p.download((total, 2), np.int64), d_cc.download(total, np.int32)
    assert np.all(pairs[:, 0] < pairs[:, 1]) and np.all(np.diff(pairs[:, 0] * n + pairs[:, 1]) > 0)
    found = set(map(tuple, pairs.tolist()))
    for o, h in members.items():
        assert (min(o, h), max(o, h)) in found
    assert np.array_equal(ctx.jaccard_pairs(sig.astype(np.uint64), pairs), counts)
    assert np.all(counts >= t)
    rows = rng.choice(n, size=64, replace=False)
    d_rows = ctx.to_device(np.ascontiguousarray(sig[rows]))
    d_m = ctx.alloc(4 * 64 * n)
    ctx.jaccard_matrix_dev(d_rows.ptr, 64, d_sig.ptr, n, U32, k, d_m.ptr, n)
    got = d_m.download((64, n), np.int32)
    for r in range(0, 64, 8):
        assert np.array_equal(got[r : r + 8], _counts(sig[rows[r : r + 8]], sig, chunk=8))
