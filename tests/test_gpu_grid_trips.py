"""Every capped-grid kernel beyond the first trip of its grid-stride loop, at small shapes (run on an MI355X: python -m pytest
tests -m gpu).

Almost every launcher of datasketch_amd/csrc sizes its grid as min(work, CUs * C) and lets the kernel walk the rest in an outer
loop.  With 256 CUs that cap is 2 048 .. 32 768 workgroups, so at test sizes the loop makes one trip.  Context option
"debug.cus" makes the launchers size grids, chunks and segments as if the device had that many CUs; here it is 1 and 3 (with 3
the trips divide unevenly), on a Context of this module's own, so that a failing test cannot leave the option set for the
modules that share _native.context().

Shapes are the smallest that give at least three trips with a partial last one at debug.cus = 1 for the kernel a test is named
after; each docstring states the per-trip amount read from the launch line and the trips the shape gives.  Launches that merely
ride along in a call fall short of that rule in places, and the docstrings say where: the forest search at its first shape
(two trips), the scatter pass of the LSH sort at 10 001 rows (48 items, three full trips of 16), its big bin pass (128 bins: four
full trips at one CU, a ragged second one at three), wgen_transpose_kernel (two full trips at (64, 64), 256 full
ones at (4096, 128)).  Results are compared for exact equality with the
reference the family's own test uses (all of them are integers).  Device outputs are filled with 0xA5 bytes first and carry SPARE
elements behind the end, which must still hold the fill afterwards.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from datasketch_amd import _native, lsh_bulk
from datasketch_amd import hyperloglog as H
from datasketch_amd import lsh_bloom as B
from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64
from datasketch_amd.lsh import _DeviceBands, _HostBands
from datasketch_amd.lshensemble import _DeviceEnsemble, _HostEnsemble
from datasketch_amd.weighted_minhash import WeightedMinHashGenerator
from oracle import oracle as O
from tests.test_gpu_jaccard_matrix import _counts, _dev_matrix, _dev_threshold, _want_pairs
from tests.test_gpu_jaccard_topk import _case, _check, _dev_topk, _tie_at_k, _want
from tests.test_gpu_lshforest import _build, _corpus, _query_case
from tests.test_lshforest_host import lexsort_order
from tests.weighted_dispatch import dense_walk_launch

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
SPARE = 37      # elements behind the end of every device output
FILL = 0xA5     # the byte they hold
_CACHE = {}     # references computed once for both CU counts


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


@pytest.fixture(params=[1, 3], ids=["debug_cus_1", "debug_cus_3"])
def cus(ctx, request):
    ctx.set_option("debug.cus", request.param)
    yield request.param
    ctx.set_option("debug.cus", 0)


def _options(ctx, **values):
    """Context manager: the options (dots written as __) set for the block, 0 afterwards."""
    class Set:
        def __enter__(self):
            for key, v in values.items():
                ctx.set_option(key.replace("__", "."), v)

        def __exit__(self, *exc):
            for key in values:
                ctx.set_option(key.replace("__", "."), 0)
    return Set()


def _filled(ctx, count, dtype, lead=0, spare=SPARE):
    """A device buffer of `lead` bytes + count + spare elements of dtype, every byte FILL."""
    nbytes = lead + (count + spare) * np.dtype(dtype).itemsize
    buf = ctx.alloc(nbytes)
    buf.upload(np.full(nbytes, FILL, dtype=np.uint8))
    return buf


def _taken(buf, count, dtype, lead=0, spare=SPARE):
    """The first `count` elements the call wrote; the bytes in front of and behind them must be untouched."""
    size = np.dtype(dtype).itemsize
    raw = buf.download(lead + (count + spare) * size, np.uint8)
    assert np.all(raw[:lead] == FILL), "written in front of the output"
    assert np.all(raw[lead + count * size:] == FILL), "written past the end of the output"
    return raw[lead: lead + count * size].view(dtype).copy()


def _trips(items, per_trip):
    """(trips, items of the last trip) of a grid that takes per_trip items at a time."""
    full, rest = divmod(items, per_trip)
    return (full + 1, rest) if rest else (full, per_trip)


def _three_ragged_trips(items, per_trip):
    trips, last = _trips(items, per_trip)
    return trips >= 3 and last < per_trip


def _csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- HyperLogLog
HLL_LENGTHS = (0, 1, 63, 64, 65, 257, 1025, 5000)  # 257 / 1025: more than the four prefetched tokens per lane of a wave / a workgroup
HLL_COMBOS = ((np.uint32, 32), (np.uint64, 64))


def _hashes(rng, n, dtype, bits):
    """n random hashes of dtype that fit `bits`, with long runs of leading zeros among them (high ranks)."""
    wide = dtype == np.uint64 and bits == 64
    hv = rng.randint(0, 2**32, size=n, dtype=np.uint64)
    if wide:
        hv = (hv << np.uint64(32)) | rng.randint(0, 2**32, size=n, dtype=np.uint64)
    hv >>= rng.randint(0, 64 if wide else 32, size=n).astype(np.uint64)
    return hv.astype(dtype)


def _hll_bulk_dev(ctx, hv, offsets, fixed_len, n, p, bits, init):
    m = 1 << p
    d_hv = ctx.to_device(hv)
    d_off = None if offsets is None else ctx.to_device(offsets)
    d_init = None if init is None else ctx.to_device(init)
    d_out = _filled(ctx, n * m, np.uint8)
    d_ovf = ctx.to_device(np.zeros(1, dtype=np.int64))
    total = int(offsets[-1]) if offsets is not None else n * fixed_len
    _native.check(ctx.lib.mhx_hll_bulk_dev(ctx.handle, d_hv.ptr, U32 if hv.dtype == np.uint32 else U64, None if d_off is None else d_off.ptr,
                                           fixed_len, n, total, p, bits, None if d_init is None else d_init.ptr, 0 if init is None else m,
                                           d_out.ptr, d_ovf.ptr))
    ctx.synchronize()
    assert int(d_ovf.download(1, np.int64)[0]) == 0
    return _taken(d_out, n * m, np.uint8).reshape(n, m)


@pytest.mark.parametrize("p", [4, 8, 9, 13, 14, 16])
def test_hll_bulk_kernel_hands_the_prefetched_set_to_the_next_trip(ctx, cus, p):
    """hll_bulk_kernel (hll_kernels.hip, launch_bulk_layout): grid = min(ceil(n_sets / per_block), CUs * 32).  Wave layout (p = 4, 8;
    per_block = 4): 32 workgroups x 4 sets = 128 sets per trip, 259 sets = 128 + 128 + 3: three trips, the last with one workgroup
    of which three waves have a set.  Words and bytes layouts (p = 9 .. 16; per_block = 1): 32 sets per trip, 67 = 32 + 32 + 3.
    Every trip re-initialises the LDS registers (zero or the set's init row), folds the tokens fetched during the trip before
    (cur = next) and fetches the next set's."""
    wave = _native.hll_layout(p) == 0
    assert wave == (p <= 8)
    n, per_trip = (259, 128) if wave else (67, 32)
    assert _three_ragged_trips(n, per_trip)
    lengths = [HLL_LENGTHS[i % len(HLL_LENGTHS)] for i in range(n)]
    offsets = _csr(lengths)
    for dtype, bits in HLL_COMBOS:
        def make():
            rng = np.random.RandomState(100 * p + bits)
            hv = _hashes(rng, int(offsets[-1]), dtype, bits)
            init = rng.randint(0, 9, size=(n, 1 << p)).astype(np.uint8)
            return hv, init, H._registers_host(hv, offsets, 0, n, p, bits, None), H._registers_host(hv, offsets, 0, n, p, bits, init)
        hv, init, want, want_init = _cached(("hll_bulk", p, bits), make)
        got = _hll_bulk_dev(ctx, hv, offsets, 0, n, p, bits, None)
        assert np.array_equal(got, want), (p, bits, np.argwhere(got != want)[:5].tolist())
        got = _hll_bulk_dev(ctx, hv, offsets, 0, n, p, bits, init)
        assert np.array_equal(got, want_init), (p, bits, np.argwhere(got != want_init)[:5].tolist())


def _split_lengths():
    """600 sets: 0 .. 269 short ones of 0 .. 20 tokens, every 37th set (36, 73, ... 591) long, 74 long beside 73, the last set long,
    109 empty in front of the long 110 (same start offset).  The long sets up to 258 have 250 .. 300 tokens; from 270 on every set
    but the long ones is empty and those have 65 .. 75 tokens, so that the last eighth of the tokens spans more than 256 sets."""
    rng = np.random.RandomState(37)
    lengths = rng.randint(0, 21, size=600)
    lengths[270:599] = 0
    long_ones = sorted(set(range(36, 600, 37)) | {74, 599})
    for i in long_ones:
        lengths[i] = rng.randint(65, 76) if i >= 270 else rng.randint(250, 301)
    lengths[109] = 0
    return lengths, long_ones


@pytest.mark.parametrize("p", [4, 16])
def test_hll_split_kernel_with_many_long_sets_per_workgroup_and_more_than_one_tile_of_sets(ctx, cus, p):
    """hll_split_kernel with hll.split_tokens = 64: workgroup b owns tokens [b * chunk, (b + 1) * chunk), chunk = max(split,
    ceil(total / (CUs * 8))): at one CU eight workgroups share the whole array instead of one per 64 tokens, so a workgroup meets
    many long sets of one 256-set tile (the while (bits) loop), and the one whose tokens lie in the run of empty sets walks more
    than one tile (tile += 256; the others leave at any_past).  CSR form with per-row init, and the fixed-length form where every set
    splits (600 sets of 70 tokens: 75 long sets per workgroup)."""
    lengths, long_ones = _split_lengths()
    offsets = _csr(lengths)
    total = int(offsets[-1])
    assert 74 in long_ones and any(i >= 256 for i in long_ones) and any(i >= 512 for i in long_ones) and lengths[599] > 64
    assert lengths[109] == 0 and offsets[109] == offsets[110] and lengths[110] > 64
    chunk = max(64, -(-total // (cus * 8)))
    spans = [int(np.searchsorted(offsets, min(t0 + chunk, total), "left")) - max(int(np.searchsorted(offsets, t0, "right")) - 1, 0)
             for t0 in range(0, total, chunk)]
    if cus == 1:
        assert len(spans) == 8 and max(spans) > 256, spans
    with _options(ctx, hll__split_tokens=64):
        for dtype, bits in HLL_COMBOS:
            def make():
                rng = np.random.RandomState(p + bits)
                hv = _hashes(rng, max(total, 600 * 70), dtype, bits)
                init = rng.randint(0, 9, size=(600, 1 << p)).astype(np.uint8)
                return hv, init, H._registers_host(hv, offsets, 0, 600, p, bits, init), H._registers_host(hv, None, 70, 600, p, bits, init)
            hv, init, want, want_fixed = _cached(("hll_split", p, bits), make)
            got = _hll_bulk_dev(ctx, hv, offsets, 0, 600, p, bits, init)
            assert np.array_equal(got, want), (p, bits, np.flatnonzero((got != want).any(axis=1))[:8].tolist())
            got = _hll_bulk_dev(ctx, hv, None, 70, 600, p, bits, init)
            assert np.array_equal(got, want_fixed), (p, bits, np.flatnonzero((got != want_fixed).any(axis=1))[:8].tolist())


@pytest.mark.parametrize("p", [4, 10])
def test_hll_histogram_kernel_clears_its_counts_between_rows(ctx, cus, p):
    """hll_histogram_kernel: grid = min(ceil(n / 4), CUs * 32), one wave per row: 128 rows per trip, 259 rows = 128 + 128 + 3;
    h[wave][lane] is reused by every trip."""
    n, m = 259, 1 << p
    assert _three_ragged_trips(n, 32 * 4)
    reg = np.random.RandomState(p).randint(0, 30, size=(n, m)).astype(np.uint8)
    reg[0] = 0
    want = _cached(("hll_hist", p), lambda: H._histogram_host(reg))
    bad = reg.copy()
    bad[-1, 5], bad[-1, m - 1], bad[130, 0] = 64, 255, 200  # three registers above 63: counted, in no bin
    want_bad = want.copy()
    for row, col in ((n - 1, 5), (n - 1, m - 1), (130, 0)):
        want_bad[row, reg[row, col]] -= 1
    for rows, hist, invalid in ((reg, want, 0), (bad, want_bad, 3)):
        d_reg = ctx.to_device(rows)
        d_hist, d_invalid = _filled(ctx, n * 64, np.uint32), ctx.to_device(np.zeros(1, dtype=np.int64))
        _native.check(ctx.lib.mhx_hll_histogram_dev(ctx.handle, d_reg.ptr, n, p, d_hist.ptr, d_invalid.ptr))
        ctx.synchronize()
        assert np.array_equal(_taken(d_hist, n * 64, np.uint32).reshape(n, 64), hist), invalid
        assert int(d_invalid.download(1, np.int64)[0]) == invalid


@pytest.mark.parametrize("shift", [0, 1], ids=["16_bytes_per_lane", "byte_by_byte"])
def test_hll_merge_kernel(ctx, cus, shift):
    """hll_merge_kernel: grid_for(ceil(count / 16), 32) = 32 workgroups x 256 lanes = 8 192 lanes per trip.  count = 2 x 131 072 + 53
    bytes: 16 387 sixteen-byte items = 8 192 + 8 192 + 3 and five bytes behind them; with d_a moved by one byte the same grid walks
    the array byte by byte (33 trips, the last with 53 bytes)."""
    count = 2 * 131072 + 53
    assert _three_ragged_trips(count >> 4, 8192) and _three_ragged_trips(count, 8192)
    rng = np.random.RandomState(3)
    a, b = (rng.randint(0, 64, size=count).astype(np.uint8) for _ in range(2))
    lead = 16 + shift
    d_a = _filled(ctx, count, np.uint8, lead=lead)
    d_a.upload(a, offset=lead)
    d_b = ctx.to_device(b)
    assert (d_a.ptr + 16) % 16 == 0 and d_b.ptr % 16 == 0
    _native.check(ctx.lib.mhx_hll_merge_dev(ctx.handle, d_a.ptr + lead, d_b.ptr, count))
    ctx.synchronize()
    assert np.array_equal(_taken(d_a, count, np.uint8, lead=lead), np.maximum(a, b))
    assert np.array_equal(d_b.download(count, np.uint8), b)


def test_hll_union_kernel(ctx, cus):
    """hll_union_kernel: one thread per four registers of one group, grid_for(n_groups * m / 4, 32) = 8 192 quads per trip.  p = 8 and
    300 groups: 19 200 quads = 8 192 + 8 192 + 2 816.  Empty and single-row groups among them."""
    p, n_groups = 8, 300
    m = 1 << p
    assert _three_ragged_trips(n_groups * m // 4, 8192)
    rng = np.random.RandomState(8)
    sizes = rng.choice([0, 1, 2, 5], size=n_groups, p=[0.2, 0.3, 0.3, 0.2])
    sizes[0], sizes[1], sizes[-1] = 0, 1, 0
    offsets = _csr(sizes)
    reg = rng.randint(0, 30, size=(int(offsets[-1]), m)).astype(np.uint8)
    want = H.union_groups(reg, offsets, gpu_mode="disable").view(np.uint8)
    d_reg, d_off, d_out = ctx.to_device(reg), ctx.to_device(offsets), _filled(ctx, n_groups * m, np.uint8)
    _native.check(ctx.lib.mhx_hll_union_groups_dev(ctx.handle, d_reg.ptr, reg.shape[0], p, d_off.ptr, n_groups, d_out.ptr))
    ctx.synchronize()
    got = _taken(d_out, n_groups * m, np.uint8).reshape(n_groups, m)
    assert np.array_equal(got, want) and not got[0].any() and np.array_equal(got[1], reg[0])


# ---------------------------------------------------------------------------------------------------------------- Bloom filters
def _sigs(seed, n, num_perm, dtype):
    hi = 2**32 if dtype == np.uint32 else 2**64
    return np.random.RandomState(seed).randint(0, hi, size=(n, num_perm), dtype=np.uint64).astype(dtype)


def _bloom_dev(ctx, sig, d_filter, b, r, k, nb, query, then_insert=False):
    """mhx_bloom_insert_dev / mhx_bloom_query_dev on device rows; the answers of a query."""
    d_sig = ctx.to_device(sig)
    code = U32 if sig.dtype == np.uint32 else U64
    n, num_perm = sig.shape
    if not query:
        _native.check(ctx.lib.mhx_bloom_insert_dev(ctx.handle, d_sig.ptr, code, n, num_perm, b, r, k, nb, d_filter.ptr))
        ctx.synchronize()
        return None
    d_hit = _filled(ctx, n, np.uint8)
    _native.check(ctx.lib.mhx_bloom_query_dev(ctx.handle, d_sig.ptr, code, n, num_perm, b, r, k, nb, d_filter.ptr, d_hit.ptr, 1 if then_insert else 0))
    ctx.synchronize()
    return _taken(d_hit, n, np.uint8).view(np.bool_)


@pytest.mark.parametrize("lanes", [16, 1], ids=["16_lanes_per_key", "1_lane_per_key"])
@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("num_perm,b,r,k,nb", [(16, 3, 5, 7, 50), (128, 9, 13, 14, 997)])
def test_bloom_kernel_insert_query_and_query_then_insert(ctx, cus, lanes, dtype, num_perm, b, r, k, nb):
    """bloom_kernel: tiles of 64 rows, grid = min(tiles, CUs * 16): 16 tiles x 64 = 1 024 rows per trip.  2 113 rows are 34 tiles
    = 16 + 16 + 2, the last of one row; tile_hit is cleared and written out per tile.  The insert goes into a non-zero filter;
    the probes are the inserted rows, rows sharing one band with them and fresh rows (6 339 rows: 100 tiles, seven trips)."""
    n = 2113
    assert _three_ragged_trips((n + 63) // 64, 16) and n % 64 == 1

    def make():
        old = np.random.RandomState(n + b).randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101)
        sig = _sigs(n + k, n, num_perm, dtype)
        shared = _sigs(n + 7, n, num_perm, dtype)
        shared[:, (b - 1) * r: b * r] = sig[:, (b - 1) * r: b * r]
        probes = np.vstack([sig, shared, _sigs(n + 9, n, num_perm, dtype)])
        want = old.copy()
        B.insert_host(want, sig, r, k)
        batch = _sigs(n + 11, n, num_perm, dtype)
        batch[::3] = sig[::3]
        after = want.copy()
        B.insert_host(after, batch, r, k)
        return old, sig, probes, want, B.query_host(want, probes, r, k), batch, B.query_host(want, batch, r, k), after
    old, sig, probes, want, want_hit, batch, want_batch, after = _cached(("bloom", num_perm, np.dtype(dtype).name), make)
    words = b * nb * 16
    spare = 48  # whole 64-byte blocks behind the filter: it stays 64-byte aligned when allocations end at a guard page
    with _options(ctx, bloom__lanes=lanes):
        d = _filled(ctx, words, np.uint32, spare=spare)
        d.upload(old)
        _bloom_dev(ctx, sig, d, b, r, k, nb, query=False)
        got = _taken(d, words, np.uint32, spare=spare).reshape(b, nb, 16)
        assert np.array_equal(got, want) and np.array_equal(got & old, old)
        hit = _bloom_dev(ctx, probes, d, b, r, k, nb, query=True)
        assert hit[: 2 * n].all() and np.array_equal(hit, want_hit)
        assert np.array_equal(_taken(d, words, np.uint32, spare=spare).reshape(b, nb, 16), want)  # a query writes nothing
        hit = _bloom_dev(ctx, batch, d, b, r, k, nb, query=True, then_insert=True)
        assert np.array_equal(hit, want_batch) and want_batch[::3].all()
        assert np.array_equal(_taken(d, words, np.uint32, spare=spare).reshape(b, nb, 16), after)
        d.free()


def test_bloom_union_kernel(ctx, cus):
    """bloom_union_kernel (bloom_kernels.hip:212): 16 bytes per lane, grid_for(words / 4, 32) = 8 192 quads per trip.  Two non-zero
    filters of 9 bands x 997 blocks x 16 words: 35 892 quads = 4 x 8 192 + 3 124, five trips with a partial last one.  dst |= src
    against np.bitwise_or, src unchanged; 48 spare words (whole 64-byte blocks) behind dst."""
    b, nb, spare = 9, 997, 48
    words = b * nb * 16
    assert _three_ragged_trips(words // 4, 8192) and _trips(words // 4, 8192) == (5, 3124)
    rng = np.random.RandomState(997)
    x, y = (rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32)
            for _ in range(2))
    d_x = _filled(ctx, words, np.uint32, spare=spare)
    d_x.upload(x)
    d_y = ctx.to_device(y)
    assert d_x.ptr % 64 == 0 and d_y.ptr % 64 == 0
    ctx.bloom_union(d_x, d_y, b, nb)
    ctx.synchronize()
    assert np.array_equal(_taken(d_x, words, np.uint32, spare=spare).reshape(b, nb, 16), np.bitwise_or(x, y))
    assert np.array_equal(d_y.download((b, nb, 16), np.uint32), y)


# ---------------------------------------------------------------------------------------------------------------- SHA-1
@pytest.mark.parametrize("bits", [32, 64])
def test_sha1_tokens_kernel(ctx, cus, bits):
    """sha1_tokens_kernel: one thread per token, grid = min(ceil(n / 256), CUs * 32): 32 x 256 = 8 192 tokens per trip;
    2 x 8 192 + 257 tokens: three trips, the last of two workgroups.  Token lengths cycle through 0 .. 130 bytes (one to three
    SHA-1 blocks)."""
    n = 2 * 8192 + 257
    assert _three_ragged_trips(n, 8192)

    def make():
        offsets = _csr(np.arange(n) % 131)
        buf = np.random.RandomState(131).randint(0, 256, size=int(offsets[-1]), dtype=np.uint8)
        return buf, offsets, [buf[offsets[i]: offsets[i + 1]].tobytes() for i in range(n)]
    buf, offsets, tokens = _cached("sha1_tokens", make)
    f, dtype = (sha1_hash32, np.uint32) if bits == 32 else (sha1_hash64, np.uint64)
    want = _cached(("sha1", bits), lambda: np.array([f(t) for t in tokens], dtype=dtype))
    d_buf, d_off, d_out = ctx.to_device(buf), ctx.to_device(offsets), _filled(ctx, n, dtype)
    _native.check(ctx.lib.mhx_sha1_tokens_dev(ctx.handle, d_buf.ptr, d_off.ptr, n, U32 if bits == 32 else U64, d_out.ptr))
    ctx.synchronize()
    assert np.array_equal(_taken(d_out, n, dtype), want)


# ---------------------------------------------------------------------------------------------------------------- dense Jaccard
@pytest.mark.parametrize("dtype,code", [(np.uint32, U32), (np.uint64, U64)], ids=["u32", "u64"])
def test_jaccard_tile_kernel_and_the_threshold_list(ctx, cus, dtype, code):
    """jaccard_tile_kernel (launch_tiles): grid = min(tiles, CUs * 16) tiles of 128 x 128: 641 x 641 rows are 6 x 6 = 36 tiles
    = 16 + 16 + 4.  ldc 644 takes the 16-byte stores, ldc 641 the scalar ones; the columns between n_b and ldc keep their fill.
    The threshold list of the same rows: the self-join walks the 21 tiles of the triangle (16 + 5), the pairs against B all 36, and
    unpack_threshold_pairs_kernel (jaccard_kernels.hip:240, min(ceil(m / 256), CUs * 16): 4 096 pairs per trip) writes more than
    2 x 4 096 pairs: the floor is the count of the 9 000th best pair of the reference."""
    n, k = 641, 64
    assert _three_ragged_trips(6 * 6, 16)

    def make():
        rng = np.random.RandomState(641)
        base = rng.randint(0, 2**32, size=(30, k), dtype=np.uint64)  # families of rows: about 641 x 641 / 30 pairs agree somewhere

        def family(count):
            rows = base[rng.randint(0, 30, size=count)]
            redraw = rng.random_sample(rows.shape) < rng.uniform(0, 0.7, size=(count, 1))
            rows[redraw] = rng.randint(0, 2**32, size=int(redraw.sum()), dtype=np.uint64)
            return rows
        a, b = family(n), family(n)
        counts, self_counts = _counts(a, b), _counts(a, a)
        floor = int(np.sort(counts.ravel())[-9000])
        return a, b, counts, self_counts, floor
    a, b, counts, self_counts, floor = _cached("jaccard_matrix", make)
    a, b = a.astype(dtype), b.astype(dtype)
    for ldc in (644, 641):
        got = _dev_matrix(ctx, a, b, k, ldc=ldc, code=code)
        assert np.array_equal(got[:, :n], counts) and np.all(got[:, n:] == -7), ldc
    assert np.array_equal(_dev_matrix(ctx, a, None, k, code=code), self_counts)
    ij, c = _want_pairs(counts, floor, False)
    assert _three_ragged_trips(len(ij), 4096), len(ij)
    total, pairs, cc = _dev_threshold(ctx, a, b, k, floor, len(ij), code=code)
    assert total == len(ij) and np.array_equal(pairs[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c)
    assert np.all(pairs[len(ij):] == -5) and np.all(cc[len(ij):] == -5)
    ij, c = _want_pairs(self_counts, floor, True)
    assert len(ij) > 4096
    total, pairs, cc = _dev_threshold(ctx, a, None, k, floor, len(ij), code=code)
    assert total == len(ij) and np.array_equal(pairs[: len(ij)], ij) and np.array_equal(cc[: len(ij)], c)
    assert np.all(pairs[len(ij):] == -5)


# ---------------------------------------------------------------------------------------------------------------- top-k
@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("m,n,k_perm,path", [(130, 4097, 64, 1), (3, 4097, 64, 2), (130, 12293, 16, 1), (3, 20001, 16, 2)])
def test_topk_with_the_segment_count_left_to_the_launcher(ctx, cus, m, n, k_perm, path, k):
    """launch_jaccard_topk takes its automatic segment counts from the CU count.  Strip kernel (path 1): min(ceil(2 CUs / tiles_m),
    max(1, tiles_n / 32)) segments -- (130, 4097): 33 tiles of B, one segment at any count; (130, 12293): 97 tiles of B and two of A, as
    many segments as CUs up to three: one at debug.cus = 1, three at 3 and at the device's count.  Stream kernel (path 2): min(12 CUs, ceil(n_b / 1024)) -- (3, 4097): five; (3, 20001):
    twenty at the device's count, twelve at one CU.  The lists do not depend on the cut."""
    a, b, counts = _case(m, n, k_perm)
    assert _tie_at_k(counts, k)
    with _options(ctx, jaccard__topk_path=path):
        _check(_dev_topk(ctx, a, b, k_perm, k, code=U32, extra=SPARE), _want(counts, k), f"path {path}")


def test_topk_merge_kernel_past_its_grid_of_2_to_the_20_rows(ctx):
    """jaccard_topk_merge_kernel: one workgroup per row of A, grid = min(n_a, 2^20), rows i, i + 2^20, ...; folded[][] is reused
    from row to row.  No option reaches this cap: n_a = 2^20 + 3 probes of four values (16 MB) against three rows, k = 2, at the
    device's own CU count -- the first three workgroups take a second row.  Probes are drawn from an alphabet of three values, so
    nearly every list has a tie at the second place that the row number decides."""
    n_a, k_perm, k = (1 << 20) + 3, 4, 2
    rng = np.random.RandomState(20)
    a = rng.randint(0, 3, size=(n_a, k_perm)).astype(np.uint32)
    a[-3:] = a[:3][::-1]  # the rows of the second trip are not the first trip's
    b = np.array([[0, 1, 2, 0], [0, 1, 0, 0], [2, 1, 2, 1]], dtype=np.uint32)
    counts = np.count_nonzero(a[:, None, :] == b[None, :, :], axis=2).astype(np.int32)
    assert _tie_at_k(counts, k)
    got = _dev_topk(ctx, a, b, k_perm, k, code=U32, extra=SPARE)
    _check(got, _want(counts, k), "2^20 + 3 probes")


# ---------------------------------------------------------------------------------------------------------------- LSH Forest
def test_forest_search_and_build(ctx, cus):
    """forest_search_kernel: one thread per (probe, tree), grid_for(m * l, 32) = 8 192 items per trip.  1 100 probes x 8 trees over
    500 rows: 8 800 items = 8 192 + 608 (two trips); 2 100 probes: 16 800 = 8 192 + 8 192 + 416 (three).  forest_keys_kernel
    (the build, one launch per half-word of a tree's key): grid_for(l * n, 32): 2 100 rows x 8 trees = 16 800 keys, three trips;
    the 500-row index is built in one.  uint32 rows."""
    l, tree_words = 8, 4
    width = l * tree_words
    assert _trips(1100 * l, 8192) == (2, 608) and _three_ragged_trips(2100 * l, 8192)
    rng = np.random.RandomState(5)
    sig, bases = _corpus(rng, 500, width, 3, np.uint32)
    d_sig, d_order, order = _build(ctx, sig, l, tree_words)
    assert np.array_equal(order, lexsort_order(sig, l, tree_words))
    probes, _ = _corpus(rng, 2100, width, 3, np.uint32, bases=bases)
    probes[:700] = sig[rng.randint(500, size=700)]
    _query_case(ctx, sig, d_sig, d_order, order, probes[:1100], l, tree_words, 1, 10)
    _query_case(ctx, sig, d_sig, d_order, order, probes, l, tree_words, 2, 3)
    big, _ = _corpus(rng, 2100, width, 3, np.uint32, bases=bases)
    d_big, d_big_order, big_order = _build(ctx, big, l, tree_words)
    assert np.array_equal(big_order, lexsort_order(big, l, tree_words))
    _query_case(ctx, big, d_big, d_big_order, big_order, probes[:300], l, tree_words, 1, 10)


# ---------------------------------------------------------------------------------------------------------------- LSH sort
# the option sets of tests/test_gpu_round5.py::test_bucketing_passes_in_both_layouts_equal_numpy_and_the_radix_sort (written inline
# there, lines 110-116): a change of either list belongs in both
_SORT_OPTIONS = (("lds", {}), ("two_levels", {"lsh.levels": 2}), ("radix", {"lsh.sort": 1}), ("band_major_two_levels", {"lsh.levels": 2}),
                 ("band_major", {}), ("band_major_radix", {"lsh.sort": 1}), ("band_major_gather", {"lsh.sort": 1, "lsh.gather": 1}),
                 ("big_bins", {"lsh.bigbins": 2}), ("band_major_big_bins", {"lsh.bigbins": 2}), ("band_major_never_big", {"lsh.bigbins": 1}),
                 ("band_major_teams_256", {"lsh.team": 256}), ("band_major_teams_1024", {"lsh.team": 1024}),
                 ("band_major_teams_1024_two_levels", {"lsh.team": 1024, "lsh.levels": 2}))


@pytest.mark.parametrize("n", [10_001, 70_001])
def test_lsh_sort_passes_in_both_layouts(ctx, cus, n):
    """mhx_lsh_sort_digests_dev / _layout_dev with the option sets of the bucketing test, 16 bands (lsh_kernels.hip 507 .. 696).
    At one CU: digests_to_band_major_kernel takes 16 tiles of 2 048 (row, band) pairs per trip -- 160 016 pairs are 79 tiles, five
    trips; the scatter pass takes at most 2 x per_cu <= 16 items of 4 096 (8 192) rows of one band: 48 items at 10 001 rows, 288
    at 70 001; the bin pass min(bins, 96) bins per trip -- 64 bins at 10 001 rows (one trip), 512 at 70 001 (5.3 trips), its big
    form min(bins, 32): 128 bins, four trips at one CU and 1.3 at three; the radix path's key and unpack kernels grid_for(n * 16)
    = 4 096 keys per trip.  "items2 >= 8 CUs" also sends the 10 001-row case to the one team of 1 024 threads at one CU."""
    rng = np.random.RandomState(n)
    bands = 16
    assert _three_ragged_trips((n * bands + 2047) // 2048, 16) and _three_ragged_trips(n * bands, 4096)

    def make():
        dig = rng.randint(0, 2**63, (n, bands), dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, (n, bands)).astype(np.uint64)
        dig[rng.randint(0, n, min(n // 7, 600)), 3] = dig[0, 3]
        dig[rng.randint(0, n, n // 7), 7] = dig[1, 7]
        dup = rng.randint(0, n, n // 3)
        dig[dup, 5] = dig[(dup * 7) % n, 5]
        order = np.stack([np.lexsort((np.arange(n), dig[:, j])) for j in range(bands)])
        return dig, order.astype(np.uint32), np.take_along_axis(dig.T, order, axis=1)
    dig, want_rows, want_dig = _cached(("lsh_sort", n), make)
    d_dig, d_dig_bm = ctx.to_device(dig), ctx.to_device(np.ascontiguousarray(dig.T))
    for name, opts in _SORT_OPTIONS:
        d_sd, d_sr = _filled(ctx, n * bands, np.uint64), _filled(ctx, n * bands, np.uint32)
        for key, v in opts.items():
            ctx.set_option(key, v)
        try:
            if name.startswith("band_major"):
                _native.check(ctx.lib.mhx_lsh_sort_digests_layout_dev(ctx.handle, d_dig_bm.ptr, n, bands, _native.BAND_MAJOR, d_sd.ptr, d_sr.ptr))
            else:
                _native.check(ctx.lib.mhx_lsh_sort_digests_dev(ctx.handle, d_dig.ptr, n, bands, d_sd.ptr, d_sr.ptr))
            ctx.synchronize()
        finally:
            for key in opts:
                ctx.set_option(key, 0)
        assert np.array_equal(_taken(d_sr, n * bands, np.uint32).reshape(bands, n), want_rows), name
        assert np.array_equal(_taken(d_sd, n * bands, np.uint64).reshape(bands, n), want_dig), name
        d_sd.free()
        d_sr.free()


# ---------------------------------------------------------------------------------------------------------------- LSH queries
def _clustered(seed, n, n_probes, k, bases, dtype=np.uint32):
    """n index rows and n_probes probes that are copies of `bases` base rows with a few values redrawn: every probe shares bands
    with about n / bases rows."""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 2**32, size=(bases, k), dtype=np.uint64)

    def draw(count):
        rows = base[rng.randint(0, bases, size=count)]
        redraw = rng.random_sample(rows.shape) < 0.05
        rows[redraw] = rng.randint(0, 2**32, size=int(redraw.sum()), dtype=np.uint64)
        return rows.astype(dtype)
    return draw(n), draw(n_probes)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
def test_lsh_index_query_compaction_and_candidate_pairs(ctx, cus, dtype):
    """The grid_for launches of lsh_query_kernels.hip and lsh_index_kernels.hip (16 workgroups x 256 = 4 096 items per trip at one CU)
    against the numpy back end of MinHashLSH (gpu_mode = "disable"), 32 bands of 4:
    query_ranges_kernel / query_emit_kernel: 300 probes x 32 bands = 9 600 items = 4 096 + 4 096 + 1 408; band_digest_kernel of the
    probes the same 9 600; unpack_pairs_kernel: more than 2 x 4 096 (probe, row) pairs (asserted); rows_compact_kernel: 1 000 rows x
    32 sixteen-byte units (uint32 rows) = 32 000 items, eight trips; run_position_kernel / emit_pairs_kernel of the candidate
    pairs: 1 000 x 32 = 32 000 entries.  The index is built in two batches (a merge) and compacted after a removal."""
    n, m, k, b, r = 1000, 300, 128, 32, 4
    assert _three_ragged_trips(m * b, 4096)
    sig, probes = _clustered(7, n, m, k, 30, dtype)
    host, dev = _HostBands(k, b, r, dtype), _DeviceBands(ctx, k, b, r, dtype)
    for one in (host, dev):
        one.append(sig[:600])
        one.append(sig[600:])
    hd, hr = host.bands()
    dd, dr = dev.bands()
    assert np.array_equal(dd, hd) and np.array_equal(dr, hr)
    want, got = host.query(probes), dev.query(probes)
    assert _three_ragged_trips(int(want[0][-1]), 4096), int(want[0][-1])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    live = np.random.RandomState(9).random_sample(n) < 0.7
    for one in (host, dev):
        one.compact(live)
    assert np.array_equal(dev.matrix(), host.matrix())
    hd, hr = host.bands()
    dd, dr = dev.bands()
    assert np.array_equal(dd, hd) and np.array_equal(dr, hr)
    want, got = host.query(probes), dev.query(probes)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    pairs, raw = ctx.lsh_candidate_pairs(sig, b, r)
    want_pairs = lsh_bulk.candidate_pairs(sig, b, r, gpu_mode="disable")
    assert _three_ragged_trips(len(want_pairs), 4096) and raw >= len(want_pairs)
    assert np.array_equal(pairs, want_pairs)


@pytest.mark.parametrize("items", [0, 16], ids=["merge_items_auto", "merge_items_16"])
def test_bands_merge_partition_kernel_with_more_bands_than_a_trip_takes(ctx, cus, items):
    """bands_merge_partition_kernel (lsh_index_kernels.hip:215): one item per (band, tile boundary), grid_for(bands * (tiles + 1)) =
    4 096 items per trip.  The items grow with the bands: 4 097 bands of n_a = 3 and n_b = 2 entries are one tile each, 8 194 items
    = 4 096 + 4 096 + 2, on 20 485 entries.  Per band the stable merge by digest of the two sorted runs (A's entries first among
    equal digests, B's rows + row_offset_b), as the numpy back end of MinHashLSH merges; digests from an alphabet of six values, so
    that runs tie within and across the two sides."""
    bands, n_a, n_b, offset = 4097, 3, 2, 1000
    assert _three_ragged_trips(bands * 2, 4096)
    rng = np.random.RandomState(4097)
    dig_a, dig_b = (np.sort(rng.randint(0, 6, size=(bands, n)).astype(np.uint64) << np.uint64(40), axis=1) for n in (n_a, n_b))
    rows_a, rows_b = (np.stack([rng.permutation(n) for _ in range(bands)]).astype(np.uint32) for n in (n_a, n_b))
    dig = np.concatenate([dig_a, dig_b], axis=1)
    order = np.argsort(dig, axis=1, kind="stable")
    want_dig = np.take_along_axis(dig, order, axis=1)
    want_rows = np.take_along_axis(np.concatenate([rows_a, rows_b + np.uint32(offset)], axis=1), order, axis=1)
    assert np.any(dig_a[:, -1] == dig_b[:, 0]) and np.any(dig_a[:, 0] > dig_b[:, -1])
    n_out = bands * (n_a + n_b)
    d = [ctx.to_device(v) for v in (dig_a, rows_a, dig_b, rows_b)]
    d_dig, d_rows = _filled(ctx, n_out, np.uint64), _filled(ctx, n_out, np.uint32)
    with _options(ctx, lsh__merge_items=items):
        ctx.lsh_bands_merge_dev(d[0].ptr, d[1].ptr, n_a, d[2].ptr, d[3].ptr, n_b, offset, bands, d_dig.ptr, d_rows.ptr)
        ctx.synchronize()
    assert np.array_equal(_taken(d_dig, n_out, np.uint64).reshape(bands, n_a + n_b), want_dig)
    assert np.array_equal(_taken(d_rows, n_out, np.uint32).reshape(bands, n_a + n_b), want_rows)


def test_lsh_ensemble_query(ctx, cus):
    """launch_lsh_ensemble_query against the numpy back end of MinHashLSHEnsemble: ensemble_items_kernel grid_for(m * n_parts):
    600 probes x 16 partitions = 9 600 (probe, partition) pairs = 4 096 + 4 096 + 1 408; ensemble_ranges_kernel and
    ensemble_emit_kernel grid_for(n_items), one item per band searched: at least as many."""
    n, m, k, n_parts = 800, 600, 64, 16
    assert _three_ragged_trips(m * n_parts, 4096)
    sig, probes = _clustered(11, n, m, k, 25)
    levels = [(2, 32), (4, 16)]
    start = np.linspace(0, n, n_parts + 1).astype(np.int64)
    start[3] = start[2]  # an empty partition
    params = np.array([[0, 32], [0, 7], [1, 16], [1, 1], [1, 0]], dtype=np.int32)
    choice = np.random.RandomState(12).randint(0, params.shape[0] + 1, size=(m, n_parts)).astype(np.uint8)  # (one past the table: partition skipped)
    host, dev = _HostEnsemble(k, np.uint32, levels, start), _DeviceEnsemble(ctx, k, np.uint32, levels, start)
    host.build(sig)
    dev.build(sig)
    for (hd, hr), (dd, dr) in zip(host.level_buffers(), dev.level_buffers()):
        assert np.array_equal(dd, hd) and np.array_equal(dr, hr)
    want, got = host.query(probes, choice, params), dev.query(probes, choice, params)
    assert int(want[0][-1]) > 0
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------------------------------------------------------- packers
def test_row_kernels_of_the_packers(ctx, cus):
    """row_grid (pack_kernels.hip:529): min(ceil(n / 4), CUs * 8) workgroups of four waves, a row per wave: 32 rows per trip, 67 rows
    = 32 + 32 + 3.  bbit_pack_kernel (k = 100), bbit1_wide_kernel and bbit_wide_kernel (k = 256: 16-byte loads), band_keys_kernel
    (bands * r < k), lean_serialize_kernel / lean_deserialize_kernel, jaccard_pairs_kernel (67 pairs)."""
    n = 67
    assert _three_ragged_trips(n, 32)
    rng = np.random.RandomState(67)
    for k in (100, 256):
        sig = rng.randint(0, 2**32, (n, k), dtype=np.uint64)
        for b in (1, 2, 5, 8, 16, 32):
            assert np.array_equal(ctx.bbit_pack(sig, b), O.c_bbit_pack(sig, b)), (k, b)
            d_sig = ctx.to_device(sig.astype(np.uint32))
            nb = O.c_bbit_pack(sig[:1], b).shape[1]
            d_out = _filled(ctx, n * nb, np.uint64)
            _native.check(ctx.lib.mhx_bbit_pack_dev_typed(ctx.handle, d_sig.ptr, U32, n, k, b, d_out.ptr))
            ctx.synchronize()
            assert np.array_equal(_taken(d_out, n * nb, np.uint64).reshape(n, nb), O.c_bbit_pack(sig, b)), (k, b)
        assert np.array_equal(ctx.band_keys(sig, 3, 7), O.c_band_keys(sig, 3, 7))
        raw = ctx.lean_serialize(sig, -12345)
        assert np.array_equal(raw, O.c_lean_serialize(sig, -12345))
        seeds, back = ctx.lean_deserialize(raw, k)
        assert np.array_equal(back, sig) and np.all(seeds == -12345)
        pairs = np.stack([rng.randint(0, n, n), rng.randint(0, n, n)], axis=1).astype(np.int64)
        sig[pairs[::2, 1], : k // 2] = sig[pairs[::2, 0], : k // 2]
        assert np.array_equal(ctx.jaccard_pairs(sig, pairs), np.count_nonzero(sig[pairs[:, 0]] == sig[pairs[:, 1]], axis=1))


def test_flat_and_tiled_kernels_of_the_packers(ctx, cus):
    """bswap_flat_kernel (pack_kernels.hip:618): min(ceil(n2 / 1024), CUs * 32) workgroups, four 16-byte items per thread and trip:
    32 768 items per trip; 1 027 rows x 128 uint64 = 65 728 items = 32 768 + 32 768 + 192.
    bbit_digest_fused_kernel (:581) and band_digest_bm_kernel (:635): tiles of 2 048 (row, band) pairs, min(tiles, CUs * 16): at 32
    bands 16 tiles = 1 024 rows per trip, 2 053 rows = 1 024 + 1 024 + 5.  band_digest_kernel (:631, a lane per pair, 4 096 pairs per
    trip): 2 053 x 32 = 65 696 = 16 x 4 096 + 160.  bbit_unpack_kernel (:713, a thread per four values, min(.., CUs * 32) = 8 192
    groups per trip): 517 rows x 32 groups = 16 544 = 8 192 + 8 192 + 160.  bbit_jaccard_kernel (:672, eight lanes per pair at k = 128,
    b = 4: eight pairs per wave, 32 waves per trip): 517 pairs = 256 + 256 + 5."""
    rng = np.random.RandomState(1027)
    sig = rng.randint(0, 2**63, (1027, 128), dtype=np.uint64)
    assert _three_ragged_trips(1027 * 128 // 2, 32768)
    assert np.array_equal(ctx.band_keys(sig, 32, 4), O.c_band_keys(sig, 32, 4))
    n, k, bands, r = 2053, 128, 32, 4
    assert _three_ragged_trips(n * bands, 16 * 2048) and _trips(n * bands, 4096) == (17, 160)
    sig = rng.randint(0, 2**32, (n, k), dtype=np.uint64)
    want_dig = lsh_bulk.band_digests(sig, bands, r, gpu_mode="disable")
    for dtype in (np.uint32, np.uint64):
        for b in (1, 4, 32):
            blocks, dig, fused = ctx.bbit_pack_band_digests(sig.astype(dtype), b, bands, r)
            assert fused and np.array_equal(blocks, O.c_bbit_pack(sig, b)) and np.array_equal(dig, want_dig), (dtype, b)
            blocks, dig, fused = ctx.bbit_pack_band_digests(sig.astype(dtype), b, bands, r, layout=_native.BAND_MAJOR)
            assert fused and np.array_equal(blocks, O.c_bbit_pack(sig, b)) and np.array_equal(dig, want_dig.T), (dtype, b)
        with _options(ctx, pack__fused=1):  # the two kernels: bbit pack by rows, band_digest_kernel / band_digest_bm_kernel
            blocks, dig, fused = ctx.bbit_pack_band_digests(sig.astype(dtype), 4, bands, r)
            assert not fused and np.array_equal(blocks, O.c_bbit_pack(sig, 4)) and np.array_equal(dig, want_dig)
            dig_bm = ctx.bbit_pack_band_digests(sig.astype(dtype), 4, bands, r, layout=_native.BAND_MAJOR)[1]
            assert np.array_equal(dig_bm, want_dig.T)
    assert np.array_equal(ctx.band_digests(sig, bands, r), want_dig)
    m = 517
    assert _three_ragged_trips(m * 32, 8192) and _three_ragged_trips(m, 256)
    for b in (1, 4, 7, 32):
        blocks = O.c_bbit_pack(sig[:m], b)
        assert np.array_equal(ctx.bbit_unpack(blocks, k, b), (sig[:m] & np.uint64((1 << b) - 1)).astype(np.uint32)), b
    pairs = np.stack([np.arange(m), rng.randint(0, m, m)], axis=1).astype(np.int64)
    low = sig[:m] & np.uint64(15)
    assert np.array_equal(ctx.bbit_jaccard_pairs(O.c_bbit_pack(sig[:m], 4), k, 4, pairs), np.count_nonzero(low[pairs[:, 0]] == low[pairs[:, 1]], axis=1))


# ---------------------------------------------------------------------------------------------------------------- MinHash
def _minhash_dev(ctx, perm, hv, offsets, fixed_len, n, k, out_dtype=np.uint64):
    d_hv = ctx.to_device(hv)
    d_off = None if offsets is None else ctx.to_device(offsets)
    d_out = _filled(ctx, n * k, out_dtype)
    total = int(offsets[-1]) if offsets is not None else n * fixed_len
    ctx.minhash_bulk_dev(perm, d_hv.ptr, U32 if hv.dtype == np.uint32 else U64, None if d_off is None else d_off.ptr, fixed_len, n, total,
                         None, 0, d_out.ptr, U32 if np.dtype(out_dtype) == np.uint32 else U64)
    ctx.synchronize()
    return _taken(d_out, n * k, out_dtype).reshape(n, k)


@pytest.mark.parametrize("tok_dtype", [np.uint32, np.uint64], ids=["u32_tokens", "u64_tokens"])
def test_minhash_bulk_with_flagged_sets_and_sets_split_over_waves(ctx, cus, tok_dtype):
    """launch_typed (minhash_kernels.hip 1507 .. 1711), num_perm = 128 (two permutations per lane): max_blocks = CUs * 64 workgroups
    of four waves, a set per wave: 256 sets per trip; 1 103 ragged sets = 4 x 256 + 79.  The launches for the flagged sets take
    resident_grid(flag groups of 64 sets) = min(18, CUs * occupancy) workgroups that stride over the 18 groups; every third set
    repeats its own tokens, so that sets are flagged (asserted) and those launches have work on later trips.
    Sets split over waves: three sets of 5 000 tokens (the launcher's own choice: fewer sets than CUs * 16 waves), and 300 ragged
    sets with minhash.split = 2 -- minhash_fill_state_kernel min(ceil(n * 128 / 256), max_blocks): 150 workgroups = 64 + 64 + 22;
    the slices follow from CUs * 32 waves.  minhash_merge_kernel (:1711): min(.., CUs * 32) workgroups x 1 024 pairs of values:
    65 536 values per trip, 131 331 = 2 x 65 536 + 259 (odd: the last value goes alone)."""
    k = 128
    a, b = O.np_init_permutations(k, 1)
    perm = (a, b)
    n = 1103
    assert _three_ragged_trips(n, 256)

    def make():
        rng = np.random.RandomState(1103)
        lengths = rng.choice([0, 1, 5, 63, 64, 65, 200, 257, 480], size=n)
        offsets = _csr(lengths)
        top = 2**32 if tok_dtype == np.uint32 else 2**61
        hv = rng.randint(0, top, size=int(offsets[-1]), dtype=np.uint64)
        for i in range(0, n, 3):  # duplicate-heavy sets: the second half repeats tokens of the first (equal tokens at the minimum defeat the first proof)
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            half = (hi - lo) // 2
            if half:
                hv[lo + half: hi] = hv[lo: lo + half][rng.randint(0, half, size=hi - lo - half)]
        few = rng.randint(0, top, size=3 * 5000, dtype=np.uint64)
        return (hv.astype(tok_dtype), offsets, O.c_minhash_bulk(hv, offsets, a, b), few.astype(tok_dtype),
                O.c_minhash_bulk_dense(few.reshape(3, 5000), a, b))
    hv, offsets, want, few, want_few = _cached(("minhash", np.dtype(tok_dtype).name), make)
    ctx.minhash_mode(reset=True)  # a fresh context's first launch: the one-candidate proof
    got = _minhash_dev(ctx, perm, hv, offsets, 0, n, k)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8].tolist()
    flags = ctx.minhash_flags(n)
    assert flags.max() >= 1 and np.flatnonzero(flags)[-1] >= 256, "no set of a later trip was flagged"
    got = _minhash_dev(ctx, perm, hv, offsets, 0, n, k, out_dtype=np.uint32)
    assert np.array_equal(got, want.astype(np.uint32))
    assert np.array_equal(_minhash_dev(ctx, perm, few, None, 5000, 3, k), want_few)
    with _options(ctx, minhash__split=2):
        assert _three_ragged_trips(300 * k // 256, 64)
        got = _minhash_dev(ctx, perm, hv, offsets[:301], 0, 300, k)
        assert np.array_equal(got, want[:300])
    with _options(ctx, minhash__path=1):  # the exact fold for every set: the full launch on the capped grid
        assert np.array_equal(_minhash_dev(ctx, perm, hv, offsets, 0, n, k), want)
    count = 2 * 65536 + 259
    assert _three_ragged_trips(count, 65536)
    x, y = (np.random.RandomState(s).randint(0, 2**32, size=count, dtype=np.uint64) for s in (1, 2))
    d_x, d_y, d_out = ctx.to_device(x), ctx.to_device(y), _filled(ctx, count, np.uint64)
    _native.check(ctx.lib.mhx_minhash_merge_dev(ctx.handle, d_x.ptr, d_y.ptr, count, d_out.ptr))
    ctx.synchronize()
    assert np.array_equal(_taken(d_out, count, np.uint64), np.minimum(x, y))


# ---------------------------------------------------------------------------------------------------------------- weighted MinHash
def _weighted_rows(rng, n, dim):
    """Rows of mixed density (entry-by-entry rows, shared-out lists and walked rows side by side) and two rows that store nothing."""
    x = rng.lognormal(0, 2.0, (n, dim)).astype(np.float32)
    dens = rng.choice([0.02, 0.09, 0.3, 1.0], size=(n, 1), p=[0.2, 0.2, 0.3, 0.3])
    x[rng.random_sample(x.shape) >= dens] = 0
    x[7] = 0
    x[n - 2] = 0
    return x


@pytest.mark.parametrize("dim,s", [(64, 64), (4096, 128)])
def test_weighted_launchers(ctx, cus, dim, s):
    """weighted_kernels.hip 2071 .. 2359 against the C oracle, host logs in (parity mode) and values in: the device's log, whose
    reference takes its logs from the oracle's restatement of numpy's float32 loop (oracle/np_logf.c), so that nothing here depends
    on which loop this host's numpy runs.  Rows per trip
    at one CU, from tests/weighted_dispatch.py and the launch lines: the dense walk (one wave per row, or at (4096, 128) the
    fetcher / walker kernel: one workgroup per CU of seven stripes) and the workgroup-per-row kernel (weighted.kernel = 1) take
    rows_per_turn of dense_walk_launch(cus = 1); dense_count_kernel / dense_compact_kernel (weighted.path = 2) min(ceil(n / 4), CUs *
    32) x 4 = 128 rows; weighted_rows_kernel and weighted_prepare's consumers (:2359) CUs * 8 x 4 = 32 rows; the CSR walk
    (weighted_csr_direct_kernel, :2317) max(1, CUs * 16 / chunks) x 4 <= 64 rows, weighted_walk_csr_kernel (:2331) at most 8 rows;
    weighted_log_kernel (:2282) 4 096 values.  n = 3 x the largest of these + 5 rows.  wgen_transpose_kernel (:2071, 2 048 entries per
    trip) runs when the generator is created, under the option: dim x s_pad = 4 096 entries (two trips) and 524 288."""
    launches = [dense_walk_launch(dim, s, logs, options=o, cus=1) for logs in (True, False) for o in ({}, {"weighted.kernel": 1})]
    per_trip = max([128] + [launch.rows_per_turn for launch in launches])
    n = 3 * per_trip + 5
    g = WeightedMinHashGenerator(dim, s, seed=11, gpu_mode="disable")

    def make():
        x = _weighted_rows(np.random.RandomState(dim + s), n, dim)
        csr = sp.csr_matrix(x)
        csr.sort_indices()
        with np.errstate(invalid="ignore", divide="ignore"):
            want, wn = O.c_weighted_minhash_many(csr.indptr, csr.indices, csr.data, g.rs, g.ln_cs, g.betas)
            logs = np.log(x)
            want_v, wn_v = O.c_weighted_minhash_many(csr.indptr, csr.indices, csr.data, g.rs, g.ln_cs, g.betas, logs=O.c_np_logf(csr.data))
        assert np.array_equal(wn_v, wn)
        return x, csr, logs, want, wn, want_v
    x, csr, logs, want, wn, want_v = _cached(("weighted", dim, s), make)
    assert not wn[7] and not wn[n - 2] and wn.sum() > n // 2
    handle = ctx.wgen_create(g.rs, g.ln_cs, g.betas)

    def same(got, what, ref=want):
        out, ne = got
        assert np.array_equal(ne.astype(bool), wn), what
        assert np.array_equal(out[wn], ref[wn]) and not out[~wn].any(), what

    try:
        for options in ({}, {"weighted.kernel": 1}, {"weighted.path": 2}, {"weighted.path": 1}):
            for key, v in options.items():
                ctx.set_option(key, v)
            try:
                same(ctx.weighted_minhash_many_dense(handle, s, logs, True), (options, "dense, logs in"))
                same(ctx.weighted_minhash_many(handle, s, csr.indptr, csr.indices, np.log(csr.data), True), (options, "CSR, logs in"))
                same(ctx.weighted_minhash_many_dense(handle, s, x, False), (options, "dense, values in"), want_v)
                same(ctx.weighted_minhash_many(handle, s, csr.indptr, csr.indices, csr.data, False), (options, "CSR, values in"), want_v)
            finally:
                for key in options:
                    ctx.set_option(key, 0)
        assert _three_ragged_trips(3 * 4096 + 5, 4096)
        v = np.random.RandomState(1).lognormal(0, 3.0, 3 * 4096 + 5).astype(np.float32)
        assert np.array_equal(ctx.weighted_logf(v).view(np.uint32), O.c_np_logf(v).view(np.uint32))
    finally:
        ctx.wgen_destroy(handle)
