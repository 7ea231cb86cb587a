"""Every value of every context option against the reference, at a shape whose launcher reads it (run on an MI355X: python -m
pytest tests -m gpu).

include/mhx.h says of the tuning keys of mhx_ctx_set_option that timings depend on them, results never.  tests/option_cases.py
lists, per key, every value of a listed domain and both ends and an inner value of a range, each with the smallest input that
makes the launcher look at the option (tests/test_option_ledger.py holds that list to the sources).  Here each case runs its
operation under the defaults and then with the option set: both results equal the reference byte for byte -- the C oracle for
MinHash and weighted MinHash, the numpy twins for the rest --, device outputs are filled with 0xA5 first and the spare elements
behind them keep it.  Where the library shows an effect of the option the test asserts it (the hand-over flags that
minhash.path != 0 and split sets do not keep, the exact redos of minhash.path 2, the `fused` answer of the packer).  Values
outside a domain are refused with a message that names the key, and the option keeps the value it had.

All of it on a Context of this module's own, every option put back in `finally`, so that nothing set here reaches the context the
other modules share.
"""
import ctypes

import numpy as np
import pytest

from datasketch_amd import _native
from tests import option_cases as C
from tests.test_gpu_grid_trips import SPARE, _bloom_dev, _filled, _hll_bulk_dev, _minhash_dev, _taken
from tests.test_gpu_jaccard_topk import _dev_topk
from tests.test_gpu_overlap import dev_counts
from tests.test_gpu_weighted_jaccard import _dev_topk as _dev_topk_weighted

pytestmark = pytest.mark.gpu

U32, U64 = _native.MHX_U32, _native.MHX_U64
OK, INVALID = _native.MHX_OK, _native.MHX_ERR_INVALID


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    own = _native.Context(_native.default_device())
    yield own
    own.close()


class _set:
    """The options of a case for the block; every one of them back at its default afterwards, whatever happened."""

    def __init__(self, ctx, options):
        self.ctx, self.options = ctx, dict(options)

    def __enter__(self):
        try:
            for key, value in self.options.items():
                self.ctx.set_option(key, value)
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for key in self.options:
            self.ctx.set_option(key, C.DEFAULTS[key])


def _code(arr):
    return U32 if arr.dtype == np.uint32 else U64


def _rows(got, want):
    return f"rows differing: {np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))[:8].tolist()}"


# ------------------------------------------------------------------------------------------------------------------ the operations
def _run_minhash(ctx, shape, d, what):
    fixed = shape["layout"] == "fixed"
    got = _minhash_dev(ctx, (d["a"], d["b"]), d["hv"], None if fixed else d["offsets"], shape["fixed_len"] if fixed else 0, shape["n_sets"], shape["num_perm"])
    assert np.array_equal(got, d["want"]), (what, _rows(got, d["want"]))


def _run_minhash_host(ctx, shape, d, what):
    out = np.full((shape["n_sets"] + 1, shape["num_perm"]), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    ctx.minhash_bulk((d["a"], d["b"]), d["hv"], None, shape["fixed_len"], shape["n_sets"], out=out[:-1])
    assert np.array_equal(out[:-1], d["want"]), (what, _rows(out[:-1], d["want"]))
    assert np.all(out[-1] == 0xA5A5A5A5A5A5A5A5), "written past the end of the output"


def _run_weighted(ctx, shape, d, what):
    n, s = shape["n_rows"], shape["samples"]
    wn = d["nonempty"]
    handle = ctx.wgen_create(d["rs"], d["ln_cs"], d["betas"])  # under the option: the tables of a fresh generator
    try:
        for is_logs, want in ((True, d["want"]), (False, d["want_values"])):
            d_out, d_ne = _filled(ctx, n * s * 2, np.int64), _filled(ctx, n, np.uint8)
            if shape["layout"] == "dense":
                d_x = ctx.to_device(d["logs"] if is_logs else d["x"])
                assert d_x.ptr % 16 == 0
                _native.check(ctx.lib.mhx_weighted_minhash_many_dense_dev(handle, d_x.ptr, int(is_logs), n, d_out.ptr, d_ne.ptr))
            else:
                bufs = [ctx.to_device(v) for v in (d["indptr"], d["indices"], d["data_logs"] if is_logs else d["data"])]
                _native.check(ctx.lib.mhx_weighted_minhash_many_dev(handle, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, int(is_logs), n, int(d["indptr"][-1]),
                                                                    d_out.ptr, d_ne.ptr))
            ctx.synchronize()
            ne = _taken(d_ne, n, np.uint8).astype(bool)
            out = _taken(d_out, n * s * 2, np.int64).reshape(n, s, 2)
            assert np.array_equal(ne, wn), (what, is_logs)
            assert np.array_equal(out[wn], want[wn]), (what, "logs in" if is_logs else "values in", _rows(out[wn], want[wn]))
            assert not out[~wn].any(), (what, "rows that store nothing hold zeros")
    finally:
        ctx.wgen_destroy(handle)


def _run_lsh_sort(ctx, shape, d, what):
    n, bands = shape["n"], shape["bands"]
    d_sd, d_sr = _filled(ctx, n * bands, np.uint64), _filled(ctx, n * bands, np.uint32)
    if shape["source"] == "signatures":
        d_in = ctx.to_device(d["sig"])
        ctx.lsh_sort_bands_dev(d_in.ptr, _code(d["sig"]), n, shape["num_perm"], bands, shape["r"], d_sd.ptr, d_sr.ptr)
    elif shape["source"] == "band_major":
        d_in = ctx.to_device(d["dig_bm"])
        _native.check(ctx.lib.mhx_lsh_sort_digests_layout_dev(ctx.handle, d_in.ptr, n, bands, _native.BAND_MAJOR, d_sd.ptr, d_sr.ptr))
    else:
        d_in = ctx.to_device(d["dig"])
        _native.check(ctx.lib.mhx_lsh_sort_digests_dev(ctx.handle, d_in.ptr, n, bands, d_sd.ptr, d_sr.ptr))
    ctx.synchronize()
    got_rows, got_dig = _taken(d_sr, n * bands, np.uint32).reshape(bands, n), _taken(d_sd, n * bands, np.uint64).reshape(bands, n)
    assert np.array_equal(got_rows, d["want_rows"]), (what, _rows(got_rows, d["want_rows"]))
    assert np.array_equal(got_dig, d["want_dig"]), (what, _rows(got_dig, d["want_dig"]))
    for buf in (d_sd, d_sr, d_in):
        buf.free()


def _run_lsh_merge(ctx, shape, d, what):
    bands, n_a, n_b = shape["bands"], shape["n_a"], shape["n_b"]
    n_out = bands * (n_a + n_b)
    bufs = [ctx.to_device(d[v]) for v in ("dig_a", "rows_a", "dig_b", "rows_b")]
    d_dig, d_rows = _filled(ctx, n_out, np.uint64), _filled(ctx, n_out, np.uint32)
    ctx.lsh_bands_merge_dev(bufs[0].ptr, bufs[1].ptr, n_a, bufs[2].ptr, bufs[3].ptr, n_b, int(d["offset"]), bands, d_dig.ptr, d_rows.ptr)
    ctx.synchronize()
    assert np.array_equal(_taken(d_dig, n_out, np.uint64).reshape(bands, n_a + n_b), d["want_dig"]), what
    assert np.array_equal(_taken(d_rows, n_out, np.uint32).reshape(bands, n_a + n_b), d["want_rows"]), what


def _run_pack_digests(ctx, shape, d, what):
    n, k, bands = shape["n"], shape["num_perm"], shape["bands"]
    nb = d["want_blocks"].shape[1]
    fused = []
    for layout, want_dig in ((0, d["want_dig"]), (_native.BAND_MAJOR, d["want_dig"].T)):
        d_sig = ctx.to_device(d["sig"])
        d_blk, d_dig = _filled(ctx, n * nb, np.uint64), _filled(ctx, n * bands, np.uint64)
        fused.append(ctx.bbit_pack_band_digests_dev(d_sig.ptr, _code(d["sig"]), n, k, shape["b"], bands, shape["r"], d_blk.ptr, d_dig.ptr, layout))
        ctx.synchronize()
        assert np.array_equal(_taken(d_blk, n * nb, np.uint64).reshape(n, nb), d["want_blocks"]), (what, layout)
        assert np.array_equal(_taken(d_dig, n * bands, np.uint64).reshape(want_dig.shape), want_dig), (what, layout)
    return {"fused": fused}


def _run_hll(ctx, shape, d, what):
    n, p, bits = shape["n_sets"], shape["p"], int(d["bits"])
    for init, want in ((None, d["want"]), (d["init"], d["want_init"])):
        got = _hll_bulk_dev(ctx, d["hv"], d["offsets"], 0, n, p, bits, init)
        assert np.array_equal(got, want), (what, init is not None, _rows(got, want))


def _run_bloom(ctx, shape, d, what):
    b, r, k, nb = shape["bands"], shape["r"], shape["k"], shape["n_blocks"]
    words, spare = b * nb * 16, 48  # (whole 64-byte blocks behind the filter)
    d_f = _filled(ctx, words, np.uint32, spare=spare)
    d_f.upload(d["old"])
    _bloom_dev(ctx, d["sig"], d_f, b, r, k, nb, query=False)
    assert np.array_equal(_taken(d_f, words, np.uint32, spare=spare).reshape(b, nb, 16), d["want"]), (what, "insert")
    hit = _bloom_dev(ctx, d["probes"], d_f, b, r, k, nb, query=True)
    assert np.array_equal(hit, d["want_hit"]) and hit[: 2 * shape["n"]].all(), (what, "query")
    assert np.array_equal(_taken(d_f, words, np.uint32, spare=spare).reshape(b, nb, 16), d["want"]), (what, "a query writes nothing")
    d_f.free()


def _run_topk(ctx, shape, d, what):
    if shape["rows"] == "weighted":
        got = _dev_topk_weighted(ctx, d["a"], d["b"], shape["k"], extra=SPARE)
    elif shape["rows"] == "bbit":
        got = _dev_topk(ctx, d["a"], d["b"], shape["k_perm"], shape["k"], bbit=4, extra=SPARE)
    else:
        got = _dev_topk(ctx, d["a"], d["b"], shape["k_perm"], shape["k"], code=U32, extra=SPARE)
    assert np.array_equal(got[0], d["want_rows"]), (what, _rows(got[0], d["want_rows"]))
    assert np.array_equal(got[1], d["want_counts"]), (what, _rows(got[1], d["want_counts"]))


def _run_topk_host(ctx, shape, d, what):
    rows, counts = ctx.jaccard_topk(d["a"], d["b"], shape["k"])
    assert np.array_equal(rows, d["want_rows"]) and np.array_equal(counts, d["want_counts"]), what


def _run_overlap(ctx, shape, d, what):
    got, invalid = dev_counts(ctx, d["hashes"], d["offsets"], d["pairs"])
    assert invalid == 0 and np.array_equal(got, d["want"]), (what, _rows(got, d["want"]))


_RUN = {"minhash": _run_minhash, "minhash_host": _run_minhash_host, "weighted": _run_weighted, "lsh_sort": _run_lsh_sort, "lsh_merge": _run_lsh_merge,
        "pack_digests": _run_pack_digests, "hll": _run_hll, "bloom": _run_bloom, "topk": _run_topk, "topk_host": _run_topk_host, "overlap": _run_overlap}


def _keeps_flags(ctx, n_sets):
    """Whether the last MinHash call kept its hand-over flags (mhx_ctx_minhash_flags answers MHX_ERR_INVALID when it did not)."""
    flags = np.empty(max(1, n_sets), dtype=np.uint8)
    rc = ctx.lib.mhx_ctx_minhash_flags(ctx.handle, n_sets, flags.ctypes.data_as(ctypes.c_void_p))
    assert rc in (OK, INVALID), _native.last_error()
    return (rc == OK), flags[:n_sets]


def _value(ctx, case):
    """debug.cus: the upper end of its range is this device's own count."""
    return min(case.value, ctx.info()["compute_units"]) if case.key == "debug.cus" else case.value


# ------------------------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_result_equals_the_reference_under_the_defaults_and_with_the_option_set(ctx, case):
    assert case.applies(), "the launcher does not read the option at this shape"
    shape, data = dict(case.shape), C.build(case)
    run = _RUN[case.op]
    value = _value(ctx, case)
    with _set(ctx, case.with_options):
        if case.op == "minhash":
            ctx.minhash_mode(reset=True)  # a fresh context's first launch, whatever ran before
        effect = run(ctx, shape, data, "defaults")
        kept, flags = _keeps_flags(ctx, shape["n_sets"]) if case.op == "minhash" else (None, None)
        with _set(ctx, {case.key: value}):
            effect_set = run(ctx, shape, data, f"{case.key} = {value}")
            kept_set, _ = _keeps_flags(ctx, shape["n_sets"]) if case.op == "minhash" else (None, None)
        run(ctx, shape, data, "defaults again")  # the option is back: nothing of it stays in the context's scratch or tables
    # what the library shows of the option's effect
    if case.op == "minhash":
        split_default, split_set = C.minhash_split(shape), C.minhash_split(shape, {case.key: value})
        assert kept == (not split_default), "the hand-over flags under the defaults"
        assert kept_set == (not split_set and not (case.key == "minhash.path" and value != 0)), "the hand-over flags with the option set"
        if shape["corpus"] == "repeats" and kept:
            assert flags.max() >= 1, "no set of the corpus left the first launch: nothing for the later launches to do"
    if case.key == "pack.fused":
        assert effect["fused"] == [True, True] and effect_set["fused"] == [False, False]


def test_minhash_path_2_redoes_sets_with_the_exact_fold_and_the_counters_show_it(ctx):
    """minhash.path 2 folds with 32-bit arithmetic and redoes a set with the exact fold when a minimum comes out too close to zero to be
    told from a wrapped one.  The near_zero corpus plants tokens whose hash has a low word of 0 .. 6 before the reduction's carry is
    added, so some of them end that close (not all: the carry moves the others away).  mhx_ctx_counters counts the redone sets
    (out[1]): at least one, and no sieve block, under minhash.path 2; the defaults run the sieve.  The results equal the oracle
    either way."""
    case = next(c for c in C.CASES if c.key == "minhash.path" and c.value == 2 and c.shape["corpus"] == "near_zero")
    shape, data = dict(case.shape), C.build(case)
    assert int(data["planted"]) >= 20
    try:
        ctx.counters(True)
        _run_minhash(ctx, shape, data, "defaults, counting")
        under_defaults = ctx.counters(True)
        with _set(ctx, {"minhash.path": 2}):
            _run_minhash(ctx, shape, data, "minhash.path = 2, counting")
            with_path_2 = ctx.counters(True)
    finally:
        ctx.counters(False)
    print(f"planted {int(data['planted'])}; defaults {under_defaults}; minhash.path 2 {with_path_2}")
    assert under_defaults["sieve_blocks"] > 0
    assert 1 <= with_path_2["exact_sets_redone"] <= shape["n_sets"] and with_path_2["sieve_blocks"] == 0 and with_path_2["sieve_sets_redone"] == 0


# ------------------------------------------------------------------------------------------------------------------ exclusions, refusals
def _small_case(key):
    """The cheapest case of a key, to run right after a refusal."""
    cases = [c for c in C.CASES if c.key == key]
    return min(cases, key=lambda c: (c.op == "weighted", c.shape.get("n", 0) + c.shape.get("n_sets", 0))) if cases else None


def test_excluded_values_are_accepted_and_nothing_runs_with_them(ctx):
    """weighted.debug 1 / 2 / 4 / 8 and minhash.alias >= 0 are in their domains but no reference holds them (option_cases.EXCLUDED): each is
    set and set back at once, no operation in between."""
    lib = ctx.lib
    for what, reason in C.EXCLUDED.items():
        key, values = (what, C.value_needs_case(what)) if isinstance(what, str) else (what[0], (what[1],))
        assert reason
        for v in values:
            try:
                assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), v) == OK, (key, v, _native.last_error())
            finally:
                assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), C.DEFAULTS[key]) == OK
    case = _small_case("minhash.prefetch")
    _RUN[case.op](ctx, dict(case.shape), C.build(case), "after the excluded values were set and set back")


@pytest.mark.parametrize("key", sorted(C.DOMAIN))
def test_values_outside_the_domain_are_refused_and_the_option_keeps_its_value(ctx, key):
    lib, dom = ctx.lib, C.DOMAIN[key]
    bad = C.outside(key)
    if key == "debug.cus":
        bad = (-1, ctx.info()["compute_units"] + 1)
    if key == "blocks_per_cu":
        bad = (-1, 0xFFFFFFFF // (512 * ctx.info()["compute_units"]) + 1)
    if key == "host.chunk_bytes":
        assert bad == (), "every int64 is a value of host.chunk_bytes"
        return
    assert len(bad) >= 2, (key, bad)
    if key == "debug.cus":
        named = [str(ctx.info()["compute_units"])]
    elif key == "blocks_per_cu":
        named = [str(bad[1] - 1)]
    else:  # every value of a listed domain, the finite ends of a range
        named = [str(x) for x in ((dom.lo, dom.hi) if isinstance(dom, C.Range) else dom) if abs(x) < 1 << 62]
    case = _small_case(key)
    valid = next(v for v in C.value_needs_case(key)) if case is None else case.value
    try:
        with _set(ctx, case.with_options if case else {}):
            assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), _value(ctx, case) if case else valid) == OK, _native.last_error()
            for v in bad:
                assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), v) == INVALID, (key, v)
                message = _native.last_error()
                assert key in message and "must be" in message, message
                assert all(str(x) in message for x in named), (message, named)
            # the refused values changed nothing: the option still holds the valid value set before them -- the case run now equals the
            # reference (with -1 or 2^40 in the option it would not get this far) -- and takes another valid value
            if case is not None:
                _RUN[case.op](ctx, dict(case.shape), C.build(case), f"{key} = {case.value} after refused values")
            assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), C.DEFAULTS[key]) == OK
            if case is not None:
                _RUN[case.op](ctx, dict(case.shape), C.build(case), f"{key} back at its default after refused values")
    finally:
        assert lib.mhx_ctx_set_option(ctx.handle, key.encode(), C.DEFAULTS[key]) == OK
