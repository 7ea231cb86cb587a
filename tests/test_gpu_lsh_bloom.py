"""The Bloom-filter kernels and MinHashLSHBloom on an MI355X: filter words and answers against the numpy twin (exact: OR does not
depend on the order), both lane mappings, every shape at which the kernels take another turn, and the argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest

from datasketch_amd import MinHash, MinHashLSHBloom, _native
from datasketch_amd import lsh_bloom as B
from datasketch_amd._native import MHX_U32, MHX_U64
from tests.test_lsh_bloom_host import edge_rows, quiet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [(16, 2, 1), (16, 3, 5), (128, 9, 13), (128, 32, 4), (128, 128, 1)]  # (num_perm, b, r): an ignored tail, more than 64 bands
ROWS = [1, 63, 64, 65, 1000]
KS = [1, 7, 8, 14, 15, 32]
BLOCKS = [1, 2, 3, 1000]


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    return _native.context()


@pytest.fixture(params=[16, 1, 0], ids=["16_lanes_per_key", "1_lane_per_key", "auto"])
def lanes(ctx, request):
    ctx.set_option("bloom.lanes", request.param)
    yield request.param
    ctx.set_option("bloom.lanes", 0)


def sigs(seed, n, num_perm, dtype):
    hi = 2**32 if dtype == np.uint32 else 2**64
    return np.random.RandomState(seed).randint(0, hi, size=(n, num_perm), dtype=np.uint64).astype(dtype)


def dev_filter(ctx, words):
    return ctx.to_device(words)


def download(d, b, nb):
    return d.download((b, nb, 16), np.uint32)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("num_perm,b,r", SHAPES)
def test_insert_and_query_equal_the_twin(ctx, lanes, dtype, num_perm, b, r):
    """Every row count, with k and n_blocks cycling through their lists; an insert into a non-zero filter keeps the old bits;
    queries of inserted, one-band-shared and fresh rows.  The product rows x k x n_blocks is sampled, not crossed, here: every
    value of each list meets every shape and dtype, test_every_k_and_block_count crosses k with n_blocks at one shape, and
    tests/bloom_guard_cases.py runs further combinations."""
    for i, n in enumerate(ROWS):
        k, nb = KS[(i + b) % len(KS)], BLOCKS[(i + r) % len(BLOCKS)]
        old = np.random.RandomState(n).randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101)
        sig = sigs(n + k, n, num_perm, dtype)
        want = old.copy()
        B.insert_host(want, sig, r, k)
        d = dev_filter(ctx, old)
        ctx.bloom_insert(sig, d, b, r, k, nb)
        got = download(d, b, nb)
        assert np.array_equal(got, want), (n, k, nb)
        assert np.array_equal(got & old, old)
        shared = sigs(n + 7, n, num_perm, dtype)
        shared[:, (b - 1) * r: b * r] = sig[:, (b - 1) * r: b * r]
        probes = np.vstack([sig, shared, sigs(n + 9, max(n, 70), num_perm, dtype)])
        hit = ctx.bloom_query(probes, d, b, r, k, nb)
        assert hit[: 2 * n].all() and np.array_equal(hit, B.query_host(want, probes, r, k)), (n, k, nb)
        d.free()


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nb", BLOCKS)
def test_every_k_and_block_count(ctx, lanes, k, nb):
    sig = sigs(k * 10 + nb, 65, 16, np.uint32)
    want = np.zeros((3, nb, 16), dtype=np.uint32)
    B.insert_host(want, sig, 5, k)
    d = dev_filter(ctx, np.zeros_like(want))
    ctx.bloom_insert(sig, d, 3, 5, k, nb)
    assert np.array_equal(download(d, 3, nb), want)
    probes = sigs(k * 10 + nb + 1, 200, 16, np.uint32)
    assert np.array_equal(ctx.bloom_query(probes, d, 3, 5, k, nb), B.query_host(want, probes, 5, k))
    d.free()


def test_identical_rows_contend_for_the_same_words(ctx, lanes):
    sig = np.repeat(sigs(3, 1, 128, np.uint64), 1000, axis=0)
    want = np.zeros((32, 3, 16), dtype=np.uint32)
    B.insert_host(want, sig[:1], 4, 14)
    d = dev_filter(ctx, np.zeros_like(want))
    ctx.bloom_insert(sig, d, 32, 4, 14, 3)
    ctx.bloom_insert(sig, d, 32, 4, 14, 3)  # all bits present: reads only
    assert np.array_equal(download(d, 32, 3), want)
    d.free()


def test_wrapping_and_modulo_keys(ctx, lanes):
    rows = edge_rows()
    sig = np.hstack([rows, rows[::-1]])  # two bands of r = 4
    want = np.zeros((2, 7, 16), dtype=np.uint32)
    B.insert_host(want, sig, 4, 8)
    d = dev_filter(ctx, np.zeros_like(want))
    ctx.bloom_insert(sig, d, 2, 4, 8, 7)
    assert np.array_equal(download(d, 2, 7), want)
    assert ctx.bloom_query(sig, d, 2, 4, 8, 7).all()
    d.free()


@pytest.mark.parametrize("n", [1, 65, 1000])
def test_query_then_insert(ctx, lanes, n):
    b, r, k, nb = 9, 13, 12, 50
    first, batch = sigs(1, 400, 128, np.uint32), sigs(2, n, 128, np.uint32)
    batch[::3] = first[: len(batch[::3])]
    want = np.zeros((b, nb, 16), dtype=np.uint32)
    B.insert_host(want, first, r, k)
    d = dev_filter(ctx, want)
    expect = B.query_host(want, batch, r, k)
    assert np.array_equal(ctx.bloom_query(batch, d, b, r, k, nb, then_insert=True), expect) and expect[::3].all()
    B.insert_host(want, batch, r, k)
    assert np.array_equal(download(d, b, nb), want)
    d.free()


@pytest.mark.parametrize("b,nb", [(1, 1), (3, 3), (9, 1000)])
def test_union_is_or(ctx, b, nb):
    rng = np.random.RandomState(b)
    x, y = (rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) for _ in range(2))
    d_x, d_y = dev_filter(ctx, x), dev_filter(ctx, y)
    ctx.bloom_union(d_x, d_y, b, nb)
    assert np.array_equal(download(d_x, b, nb), x | y) and np.array_equal(download(d_y, b, nb), y)
    d_x.free()
    d_y.free()


def test_class_on_the_device_agrees_with_the_host_and_covers_the_fixture():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "lsh_bloom.json")))
    ins, q = np.array(doc["inserted"], dtype=np.uint64), np.array(doc["queries"], dtype=np.uint64)
    args = dict(num_perm=doc["num_perm"], n=doc["n"], fp=doc["fp"], params=tuple(doc["params"]))
    dev, host = quiet(gpu_mode="always", **args), quiet(gpu_mode="disable", **args)
    assert dev.on_device and not host.on_device
    for lsh in (dev, host):
        lsh.insert_bulk(ins[:50])
        for row in ins[50:60]:
            lsh.insert(MinHash(doc["num_perm"], hashvalues=row))
        lsh.hashtables[1].insert(ins[60, 5:10])
    assert np.array_equal(dev.query_insert_bulk(ins[60:]), host.query_insert_bulk(ins[60:]))
    assert np.array_equal(dev.words(), host.words())
    answers = dev.query_bulk(q)
    assert np.array_equal(answers, host.query_bulk(q)) and answers[np.array(doc["answers"])].all()
    assert dev.query(MinHash(doc["num_perm"], hashvalues=q[0])) == bool(answers[0])
    assert dev.hashtables[2].query(ins[3, 10:15]) and np.array_equal(dev.hashtables[2].words, host.words()[2])
    other = quiet(gpu_mode="always", **args)
    extra = sigs(9, 40, doc["num_perm"], np.uint32)
    other.insert_bulk(extra)
    host.insert_bulk(extra)
    dev.merge(other)
    assert np.array_equal(dev.words(), host.words())
    host2 = quiet(gpu_mode="disable", **args)
    host2.merge(dev)  # device into host, and host into device
    other.merge(host2)
    assert np.array_equal(host2.words(), host.words()) and np.array_equal(other.words(), host.words())


def test_detect_moves_the_filter_to_the_device_with_the_first_large_call():
    lsh = quiet(num_perm=16, n=5000, fp=0.001, params=(4, 4), gpu_mode="detect")
    host = quiet(num_perm=16, n=5000, fp=0.001, params=(4, 4), gpu_mode="disable")
    small, large = sigs(1, 10, 16, np.uint32), sigs(2, B.DETECT_DEVICE_KEYS // 4, 16, np.uint32)
    lsh.insert_bulk(small)
    assert not lsh.on_device
    lsh.insert_bulk(large)
    assert lsh.on_device
    host.insert_bulk(np.vstack([small, large]))
    assert np.array_equal(lsh.words(), host.words())


# ---- the argument checks of the five entry points ------------------------------------------------------------------------
def test_rejected_arguments(ctx):
    lib, INVALID = ctx.lib, _native.MHX_ERR_INVALID
    dev = ctx.to_device(np.zeros(4096, dtype=np.uint64))
    host = np.zeros(4096, dtype=np.uint64)
    hit = np.zeros(64, dtype=np.uint8)
    calls = set()

    def bad(entry, message, *argv):
        calls.add(entry)
        before = download(dev, 1, 512)
        assert getattr(lib, entry)(*argv) == INVALID, (entry, message)
        assert message in _native.last_error(), (entry, message, _native.last_error())
        assert np.array_equal(download(dev, 1, 512), before)

    def cases(entry, sig, extra):
        # (ctx, sig, dtype, n, num_perm, bands, r, k, n_blocks, d_filter, *extra)
        ok = [ctx.handle, sig, MHX_U64, 4, 16, 3, 5, 7, 2, dev.ptr] + extra
        where = "device" if entry.endswith("_dev") else "host"

        def change(**kw):
            names = ["ctx", "sig", "dtype", "n", "num_perm", "bands", "r", "k", "n_blocks", "d_filter", "hit", "then_insert"]
            argv = list(ok)
            for name, v in kw.items():
                argv[names.index(name)] = v
            return argv

        bad(entry, "ctx is NULL", *change(ctx=None))
        bad(entry, f"NULL {where} pointer", *change(sig=None))
        bad(entry, "d_filter is NULL", *change(d_filter=None))
        bad(entry, "d_filter must be 64-byte aligned", *change(d_filter=dev.ptr + 4))
        if extra:
            bad(entry, f"NULL {where} pointer", *change(hit=None))
        for k in (0, 33, -1):
            bad(entry, "k must be in [1, 32]", *change(k=k))
        for nb in (0, -1, 2**32):
            bad(entry, "n_blocks must be in [1, 2^32-1]", *change(n_blocks=nb))
        bad(entry, "bands*r must be in (0, num_perm]", *change(bands=4, r=5))
        bad(entry, "bands*r must be in (0, num_perm]", *change(bands=0))
        bad(entry, "bands*r must be in (0, num_perm]", *change(r=0))
        bad(entry, "bad sig_dtype 7", *change(dtype=7))
        bad(entry, "n must be >= 0", *change(n=-1))
        assert getattr(lib, entry)(*change(n=0, sig=None)) == _native.MHX_OK

    cases("mhx_bloom_insert_dev", dev.ptr + 2048, [])
    cases("mhx_bloom_insert", host.ctypes.data, [])
    cases("mhx_bloom_query_dev", dev.ptr + 2048, [dev.ptr + 16384, 0])
    cases("mhx_bloom_query", host.ctypes.data, [hit.ctypes.data, 1])
    entry = "mhx_bloom_union_dev"
    bad(entry, "ctx is NULL", None, dev.ptr, dev.ptr + 8192, 1, 2)
    bad(entry, "NULL device pointer", ctx.handle, None, dev.ptr + 8192, 1, 2)
    bad(entry, "NULL device pointer", ctx.handle, dev.ptr, None, 1, 2)
    bad(entry, "d_dst must be 64-byte aligned", ctx.handle, dev.ptr + 4, dev.ptr + 8192, 1, 2)
    bad(entry, "d_src must be 64-byte aligned", ctx.handle, dev.ptr, dev.ptr + 8200, 1, 2)
    bad(entry, "bands must be in [1, 2^24]", ctx.handle, dev.ptr, dev.ptr + 8192, 0, 2)
    bad(entry, "n_blocks must be in [1, 2^32-1]", ctx.handle, dev.ptr, dev.ptr + 8192, 1, 0)
    bad(entry, "n_blocks must be in [1, 2^32-1]", ctx.handle, dev.ptr, dev.ptr + 8192, 1, 2**32)
    assert sorted(calls) == _native.EXPORTED_SYMBOLS_BLOOM
    with pytest.raises(ValueError, match="bloom.lanes must be 0, 1 or 16"):
        ctx.set_option("bloom.lanes", 8)
    ctx.synchronize()
    dev.free()
