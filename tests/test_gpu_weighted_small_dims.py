"""Dense weighted sketches of 4 .. 1020 columns against the C oracle (run on an MI355X: python -m pytest tests -m gpu -q).

Since round 6 (weighted.min_dim 4) every dense row whose width is a multiple of 4 runs weighted_walk_wave_kernel, NV = 4
below 1024 columns, and rows of 2, 3, 4 or 6 chunks of 64 samples its fetcher / walker form (SPLIT = 2).  Small widths take
paths wide rows do not: lanes past the row's end load and store a copy of its last four entries, the cached walk positions
(8, 12 or 16 per chunk) are cut to the width, the list holds max(64, dim / 8) columns here and max(64, dim / 4) in the
workgroup-per-row kernel, a row of 8 columns or fewer is never "few stored", and a row of 5 or more chunks walks its last
chunks from global memory.  Every case runs one launch over at least three turns of its grid and a ragged remainder
(tests/weighted_dispatch.py sizes the turn), logs in and values in (the log taken on the device), against the oracle: fed
np.log of the data for logs in, the device's own log (ctx.weighted_logf, pinned to numpy by
test_device_log_equals_numpy_log_for_every_float32) for values in.  The same classes run the workgroup-per-row kernel
(weighted.kernel 1) and the chunk-after-chunk wave kernel (weighted.kernel 2) against the oracle, and every row of each is
compared with the evaluate-every-element path (weighted.path 2).

Instantiations below 1024 columns (tests/weighted_dispatch.py; LOGS both ways) and the widths each runs at; the test ids
name them:

    walk_wave_NV4_PAIRS_true_FETCH0_SPLIT0   1, 5 or 9 chunks of samples      4 8 12 16 20 32 60 64 100 252 256 260 516 1020
    walk_wave_NV4_PAIRS_false_FETCH2_SPLIT2  2, 3, 4 or 6 chunks              4 8 12 16 20 32 60 64 100 252 256 260 516 1020
    walk_wave_NV4_PAIRS_false_FETCH0_SPLIT0  weighted.kernel 2, every count   4 8 12 16 20 32 60 64 100 252 256 260 516 1020
    walk_dense_AHEAD_true                    weighted.kernel 1                4 8 12 16 20 32 60 64 100 252 256 260 516 1020
                                             weighted.min_dim 64              60
    walk_dense_AHEAD_false                   a matrix at a 4-byte offset      4 60 256 1020
"""
import contextlib
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import scipy.sparse as sp

from datasketch_amd import WeightedMinHashGenerator, _native
from oracle import oracle as O
from tests.weighted_dispatch import dense_walk_launch

pytestmark = pytest.mark.gpu

_THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
_FULL_CHECK = 2e9   # rows x dim x samples up to which the oracle sees every row
_SPECIALS = [np.nan, np.inf, -0.0, -1.5, 1e-42]


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    c = _native.context()
    c.set_option("host.chunk_bytes", -1)  # one launch sees every row (the host entry feeds large matrices in pieces otherwise)
    yield c
    c.set_option("host.chunk_bytes", 0)


@contextlib.contextmanager
def _options(wctx, options):
    for key, value in options.items():
        wctx.set_option(key, value)
    try:
        yield
    finally:
        for key in options:
            wctx.set_option(key, 0)


def _logs(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.log(x)


def _oracle(g, x, rows, logs_of):
    """The C oracle on rows `rows` of the dense values x (stored: nonzero, as scipy keeps them -- NaN stays, -0.0 goes), fed
    logs_of(stored values) as the logs; the rows shared out among host threads (ctypes releases the GIL)."""
    csr = sp.csr_matrix(x[rows])
    csr.sort_indices()
    indptr, indices = csr.indptr.astype(np.int64), csr.indices.astype(np.int32)
    logs = logs_of(csr.data.astype(np.float32))

    def piece(lo, hi):
        return O.c_weighted_minhash_many(indptr[lo : hi + 1] - indptr[lo], indices[indptr[lo] : indptr[hi]], None, g.rs, g.ln_cs, g.betas,
                                         logs=logs[indptr[lo] : indptr[hi]])

    n = len(rows)
    cuts = np.linspace(0, n, min(_THREADS, n) + 1).astype(np.int64)
    with ThreadPoolExecutor(_THREADS) as pool:
        parts = list(pool.map(lambda i: piece(cuts[i], cuts[i + 1]), range(len(cuts) - 1)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _odd(x):
    """Rows with a NaN, an infinity or a negative value (its log is a NaN): floor(NaN), floor(inf) cast to int64 platform by
    platform, so only the winning columns are compared with the oracle."""
    return (~np.isfinite(x) | (x < 0)).any(axis=1)


def _assert_oracle(got, ne, want, wn, odd):
    assert np.array_equal(ne.astype(bool), wn)
    assert np.array_equal(got[wn & ~odd], want[wn & ~odd]) and not got[~wn].any()
    assert np.array_equal(got[wn & odd][:, :, 0], want[wn & odd][:, :, 0])


def _generator(dim, s, seed):
    g = WeightedMinHashGenerator(dim, s, seed=seed, gpu_mode="always")
    wctx, handle = g._device_handle()
    return g, wctx, handle


def _sketch(wctx, handle, s, x, values_in):
    """One launch over every row: values in (the log on the device) or np.log(x) in."""
    return wctx.weighted_minhash_many_dense(handle, s, x if values_in else _logs(x), not values_in)


def _base_rows(rng, n, dim):
    """Uniform, lognormal (sigma 2) and Pareto rows, each stored at 100, 60, 30, 12 or 5 % of the columns -- 4 columns included."""
    kind = rng.randint(0, 3, n)
    x = rng.uniform(0, 100, (n, dim)).astype(np.float32)
    heavy = kind == 1
    x[heavy] = rng.lognormal(0, 2.0, (int(heavy.sum()), dim))
    pareto = kind == 2
    x[pareto] = rng.pareto(1.1, (int(pareto.sum()), dim)) + 1e-3
    dens = rng.choice([1.0, 0.6, 0.3, 0.12, 0.05], size=(n, 1), p=[0.4, 0.15, 0.15, 0.15, 0.15])
    x[rng.random_sample(x.shape) >= dens] = 0
    return x


def _special_rows(rng, dim):
    """Empty rows, one stored entry in the first or last column, floor(dim / 10) and one more stored entries (both sides of
    the few-stored rule), and NaN, +inf, -0.0, a negative and a denormal value in column 0, in each of the last four columns
    (the ones the lanes behind the row's end copy) and in the middle."""
    rows = []
    zero = np.zeros(dim, np.float32)
    rows.append(zero.copy())
    for col in (0, dim - 1):
        r = zero.copy()
        r[col] = rng.uniform(0.5, 50)
        rows.append(r)
        r = zero.copy()
        r[col] = 1e-42
        rows.append(r)
    for k in (dim // 10, dim // 10 + 1):
        r = zero.copy()
        r[rng.choice(dim, k, replace=False)] = rng.uniform(0.5, 50, k)
        rows.append(r)
    places = sorted({0, dim // 2} | {dim - 4 + i for i in range(4)})
    for value in _SPECIALS:
        for col in places:
            r = rng.uniform(0.5, 100, dim).astype(np.float32)
            r[col] = value
            rows.append(r)
    return np.array(rows, dtype=np.float32)


def _matrix(rng, n, dim, turn):
    """n rows of mixed kinds, the special rows at the start, across the first two turn boundaries and at the ragged end;
    returns the matrix and the special rows' indices."""
    x = _base_rows(rng, n, dim)
    sp_rows = _special_rows(rng, dim)
    m = len(sp_rows)
    starts = sorted(a for a in {0, turn - m // 2, 2 * turn - m // 2, n - m} if 0 <= a and a + m <= n)
    for at in starts:
        x[at : at + m] = sp_rows
    return x, np.unique(np.concatenate([np.arange(at, at + m) for at in starts]))


def _check_rows(n, dim, s, turn, must):
    """Every row when the oracle can afford it, else a spread sample with the first and last rows of every turn and `must`."""
    if n * dim * s <= _FULL_CHECK:
        return np.arange(n)
    budget = int(_FULL_CHECK // (dim * s))
    edges = np.concatenate([[t * turn - 1, t * turn, t * turn + 1] for t in range(n // turn + 1)] + [np.arange(n - 4, n)])
    rows = np.concatenate([np.linspace(0, n - 1, budget).astype(np.int64), edges, must])
    return np.unique(rows[(rows >= 0) & (rows < n)])


# (dim, samples): every width with 1, 5 or 9 chunks of samples (the one-wave-per-row form) and with 2, 3, 4 or 6 (fetcher / walker)
_CASES = [(4, 1), (8, 63), (12, 64), (16, 257), (20, 300), (32, 513), (60, 1), (64, 300), (100, 64), (252, 257), (256, 1), (260, 513), (516, 300), (1020, 63),
          (4, 128), (8, 65), (12, 192), (16, 384), (20, 256), (32, 129), (60, 128), (64, 65), (100, 192), (252, 256), (256, 128), (260, 384), (516, 129), (1020, 256)]


_VARIANTS = [{}, {"weighted.kernel": 1}, {"weighted.kernel": 2}]   # the launcher's choice, the workgroup-per-row kernel, chunk after chunk
_MAIN = [(d, s, o) for o in _VARIANTS for d, s in _CASES]


def _case_id(dim, s, options=None, aligned=True):
    return f"{dense_walk_launch(dim, s, True, aligned, options).name}-dim{dim}-S{s}-chunks{(s + 63) // 64}"


@pytest.mark.parametrize("dim,s,options", _MAIN, ids=[_case_id(d, s, o) for d, s, o in _MAIN])
def test_small_widths_against_the_oracle(ctx, dim, s, options):
    """Three turns of the kernel's grid and a ragged remainder of mixed and special rows, logs and values in: the oracle on
    every row (past 2e9 evaluations a spread sample with every turn's edges and every special row), and every row equal to
    the evaluate-every-element path (weighted.path 2)."""
    launch = dense_walk_launch(dim, s, True, options=options, cus=ctx.info()["compute_units"])
    assert dense_walk_launch(dim, s, False, options=options).name == launch.name
    turn = launch.rows_per_turn
    n = 3 * turn + 37
    rng = np.random.RandomState(zlib.crc32(f"small/{dim}/{s}/{launch.kernel}".encode()))
    x, special = _matrix(rng, n, dim, turn)
    odd = _odd(x)
    rows = _check_rows(n, dim, s, turn, special)
    g, wctx, handle = _generator(dim, s, seed=dim + s)
    for values_in in (False, True):
        with _options(wctx, options):
            got, ne = _sketch(wctx, handle, s, x, values_in)
        want, wn = _oracle(g, x, rows, wctx.weighted_logf if values_in else _logs)
        _assert_oracle(got[rows], ne[rows], want, wn, odd[rows])
        with _options(wctx, {"weighted.path": 2}):
            every, ne2 = _sketch(wctx, handle, s, x, values_in)
        assert np.array_equal(ne2, ne) and np.array_equal(every, got)


def _band_rows(rng, dim, counts, zeros):
    """Rows with exactly m entries far above any cut (1e6 .. 1e7), the other columns far below it or not stored."""
    rows = []
    for m in counts:
        r = np.zeros(dim, np.float32) if zeros else rng.uniform(1e-6, 1e-5, dim).astype(np.float32)
        r[rng.choice(dim, m, replace=False)] = rng.uniform(1e6, 1e7, m)
        rows.append(r)
    return np.array(rows, dtype=np.float32)


@pytest.mark.parametrize("dim,s", [(12, 128), (12, 300), (64, 128), (64, 300), (1020, 128), (1020, 300)])
def test_every_cut_at_small_widths(ctx, dim, s):
    """weighted.tail 1 .. 5 (the cut at the 0.5 .. 8 % quantile of the sampled logs), each on a fresh generator so that the
    forced cut is the one the tables are built for, on lognormal and Pareto rows; logs and values in, every row against the
    oracle.  At 1020 columns the rows include 65 .. 256 entries above the cut: up to 127 the wave kernel lists them, beyond
    it goes entry by entry where the workgroup kernel (list of 255) still walks -- checked with weighted.kernel 1 as well."""
    rng = np.random.RandomState(zlib.crc32(f"cut/{dim}/{s}".encode()))
    n = 1500
    x = np.where(rng.random_sample((n, 1)) < 0.5, rng.lognormal(0, 2.0, (n, dim)), rng.pareto(1.1, (n, dim)) + 1e-3).astype(np.float32)
    x[rng.random_sample(x.shape) < 0.1] = 0
    if dim == 1020:
        counts = [65, 100, 127, 128, 129, 200, 254, 255, 256]
        x[101 : 101 + 2 * len(counts)] = np.concatenate([_band_rows(rng, dim, counts, False), _band_rows(rng, dim, counts, True)])
    odd = _odd(x)
    rows = np.arange(n)
    for tail in (1, 2, 3, 4, 5):
        g, wctx, handle = _generator(dim, s, seed=tail)
        with _options(wctx, {"weighted.tail": tail}):
            for values_in in (False, True):
                want, wn = _oracle(g, x, rows, wctx.weighted_logf if values_in else _logs)
                got, ne = _sketch(wctx, handle, s, x, values_in)
                _assert_oracle(got, ne, want, wn, odd)
                if tail == 5:
                    with _options(wctx, {"weighted.kernel": 1}):
                        got1, ne1 = _sketch(wctx, handle, s, x, values_in)
                    _assert_oracle(got1, ne1, want, wn, odd)


@pytest.mark.parametrize("dim", [4, 8, 12, 16, 100])
@pytest.mark.parametrize("s", [128, 192, 256, 384])
def test_fetcher_walker_settings_at_small_widths(ctx, dim, s):
    """The fetcher / walker kernel with fewer rows than fetchers, stripes or workgroups and with a ragged last round (1 .. 257
    rows): auto against the oracle, and weighted.refill 13 (no split), 5, 6, 8, 9 (other stripe, fetcher and cache
    settings) against auto -- logs and values in."""
    assert dense_walk_launch(dim, s, True).split == 2
    rng = np.random.RandomState(zlib.crc32(f"split/{dim}/{s}".encode()))
    g, wctx, handle = _generator(dim, s, seed=7)
    sp_rows = _special_rows(rng, dim)
    for n in (1, 3, 5, 7, 13, 255, 257):
        x = _base_rows(rng, n, dim)
        if n >= 5:
            x[2] = 0
        if n >= 7:
            x[5, 0], x[6, dim - 1] = np.nan, np.inf
        if n > len(sp_rows):
            x[n - len(sp_rows) :] = sp_rows
        odd = _odd(x)
        for values_in in (False, True):
            got, ne = _sketch(wctx, handle, s, x, values_in)
            want, wn = _oracle(g, x, np.arange(n), wctx.weighted_logf if values_in else _logs)
            _assert_oracle(got, ne, want, wn, odd)
            for code in (13, 5, 6, 8, 9):
                with _options(wctx, {"weighted.refill": code}):
                    other, ne2 = _sketch(wctx, handle, s, x, values_in)
                assert np.array_equal(ne2, ne) and np.array_equal(other, got), (n, code)


@pytest.mark.parametrize("dim", [32, 60, 256])
@pytest.mark.parametrize("s", [128, 300])
def test_rescue_settings_at_small_widths(ctx, dim, s):
    """weighted.rescue -1 (off), 0 (auto: 8), 1 and 8 lanes on lognormal rows, whose slowest lanes walk past the cached
    positions: every row against the oracle, logs and values in."""
    rng = np.random.RandomState(zlib.crc32(f"rescue/{dim}/{s}".encode()))
    n = 3 * dense_walk_launch(dim, s, True).rows_per_turn // 4 + 37
    x = rng.lognormal(0, 2.0, (n, dim)).astype(np.float32)
    x[rng.random_sample(x.shape) < 0.05] = 0
    odd = _odd(x)
    g, wctx, handle = _generator(dim, s, seed=3)
    for values_in in (False, True):
        want, wn = _oracle(g, x, np.arange(n), wctx.weighted_logf if values_in else _logs)
        for rescue in (-1, 0, 1, 8):
            with _options(wctx, {"weighted.rescue": rescue}):
                got, ne = _sketch(wctx, handle, s, x, values_in)
            _assert_oracle(got, ne, want, wn, odd)


def _bin_top(log):
    """The largest float32 of the plan's histogram bin that holds `log` (sign, exponent and 5 mantissa bits): the cuts the
    plan can choose are these."""
    b = int(np.float32(log).view(np.uint32))
    o = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
    top = (((o >> 18) + 1) << 18) - 1
    return np.uint32(top ^ (0x80000000 if top >> 31 else 0xFFFFFFFF)).view(np.float32)


@pytest.mark.parametrize("dim,s", [(64, 128), (60, 300)])
def test_values_in_cut_shortcut_near_the_cut(ctx, dim, s):
    """Values in, the wave kernel asks "above the cut?" of the value (v > vcut, vcut = exp of the cut less 1e-5 relative;
    0 below a cut of -87, FLT_MAX above 88).  Rows of a constant c whose log is the top of a histogram bin -- a cut the
    plan can choose -- with entries 1 .. 64 ulp above and below c straddle that cut.  Every weighted.tail, from log c = -100
    (denormal values: a cut at or below -88) to 88.3 (the bin of [88, 90): a cut above 88), every row against the oracle on
    the device's logs."""
    rng = np.random.RandomState(zlib.crc32(f"vcut/{dim}/{s}".encode()))
    n = 512
    for target in (-100.0, -88.5, -86.5, -30.0, -1.0, -0.01, 0.3, 3.0, 40.0, 87.5, 88.3):
        edge = _bin_top(target)
        c = np.float32(np.exp(np.float64(edge)) if edge < 88.72 else np.exp(np.float64(target)))  # (the top of [88, 90) has no float32 exp)
        c_bits = int(c.view(np.uint32))
        bits = c_bits - rng.randint(0, 65, (n, dim)) * (rng.random_sample((n, dim)) < 0.3)
        up = rng.random_sample((n, dim)) < 0.02
        bits[up] = c_bits + rng.randint(1, 65, int(up.sum()))
        x = np.clip(bits, 1, 0x7F7FFFFF).astype(np.uint32).view(np.float32)
        x[:8] = np.uint32(c_bits).view(np.float32)  # constant rows
        for tail in (0, 1, 2, 3, 4, 5):
            g, wctx, handle = _generator(dim, s, seed=tail + 1)
            with _options(wctx, {"weighted.tail": tail}):
                got, ne = _sketch(wctx, handle, s, x, True)
            want, wn = _oracle(g, x, np.arange(n), wctx.weighted_logf)
            assert np.array_equal(ne, wn) and np.array_equal(got, want), (target, tail)


_OFFSET_CASES = [(4, 128), (60, 1), (256, 300), (1020, 129)]


@pytest.mark.parametrize("dim,s", _OFFSET_CASES, ids=[_case_id(d, s, aligned=False) for d, s in _OFFSET_CASES])
def test_matrix_at_a_four_byte_offset(ctx, dim, s):
    """A matrix that does not start on 16 bytes goes to the workgroup-per-row kernel without its 16-byte loads
    (walk_dense_AHEAD_false): the matrix sits at byte 4 of a buffer 16 bytes longer than it, and the sketch equals the
    aligned call's and the oracle's -- logs and values in."""
    assert dense_walk_launch(dim, s, True, aligned=False).name == "walk_dense_AHEAD_false"
    turn = dense_walk_launch(dim, s, True, aligned=False, cus=ctx.info()["compute_units"]).rows_per_turn
    n = 3 * turn + 37
    rng = np.random.RandomState(zlib.crc32(f"offset/{dim}/{s}".encode()))
    x, special = _matrix(rng, n, dim, turn)
    odd = _odd(x)
    rows = _check_rows(n, dim, s, turn, special)
    g, wctx, handle = _generator(dim, s, seed=9)
    lib = wctx.lib
    for values_in in (False, True):
        data = np.ascontiguousarray(x if values_in else _logs(x), dtype=np.float32)
        d_x = wctx.alloc(data.nbytes + 16)
        d_o, d_ne = wctx.alloc(n * s * 16), wctx.alloc(n)
        try:
            results = []
            for offset in (0, 4):
                d_x.upload(data, offset=offset)
                _native.check(lib.mhx_weighted_minhash_many_dense_dev(handle, d_x.ptr + offset, int(not values_in), n, d_o.ptr, d_ne.ptr))
                results.append((d_o.download((n, s, 2), np.int64), d_ne.download((n,), np.uint8)))
        finally:
            for d in (d_x, d_o, d_ne):
                d.free()
        (aligned, ne_a), (shifted, ne_s) = results
        assert np.array_equal(ne_s, ne_a) and np.array_equal(shifted, aligned)
        want, wn = _oracle(g, x, rows, wctx.weighted_logf if values_in else _logs)
        _assert_oracle(shifted[rows], ne_s[rows], want, wn, odd[rows])


_MIN_DIM = {"weighted.min_dim": 64}
_MIN_DIM_CASES = [(60, 128), (64, 128), (60, 300), (64, 300)]


@pytest.mark.parametrize("dim,s", _MIN_DIM_CASES, ids=[_case_id(d, s, _MIN_DIM) + "-min_dim64" for d, s in _MIN_DIM_CASES])
def test_min_dim_option_edge(ctx, dim, s):
    """weighted.min_dim 64: 60 columns go to the workgroup-per-row kernel, 64 stay with the wave kernel; both equal the oracle."""
    launch = dense_walk_launch(dim, s, True, options=_MIN_DIM, cus=ctx.info()["compute_units"])
    assert launch.kernel == ("walk_dense" if dim < 64 else "walk_wave")
    n = 3 * launch.rows_per_turn + 37
    rng = np.random.RandomState(zlib.crc32(f"min_dim/{dim}/{s}".encode()))
    x, _ = _matrix(rng, n, dim, launch.rows_per_turn)
    odd = _odd(x)
    g, wctx, handle = _generator(dim, s, seed=13)
    for values_in in (False, True):
        with _options(wctx, _MIN_DIM):
            got, ne = _sketch(wctx, handle, s, x, values_in)
        want, wn = _oracle(g, x, np.arange(n), wctx.weighted_logf if values_in else _logs)
        _assert_oracle(got, ne, want, wn, odd)
