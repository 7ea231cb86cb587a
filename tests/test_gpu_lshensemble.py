"""The device side of datasketch_amd.MinHashLSHEnsemble: mhx_lsh_ensemble_query_dev against a numpy model (answers, the overflow
contract, a guard behind the output, refused arguments), the level buffers against mhx_lsh_sort_bands per (level, partition), the
device back end against the numpy one on the golden cases and on 20 000 random rows, bulk against single queries, and widening."""
import ctypes

import numpy as np
import pytest

from datasketch_amd import MinHashLSHEnsemble, _native, lsh_bulk
from datasketch_amd.lsh import _DeviceBands, _HostBands
from datasketch_amd.lshensemble import _DeviceEnsemble, _HostEnsemble
from tests.test_lshensemble_host import CASES, PROBE_SIZES, check_case, constructor_args, golden, golden_inputs, signature

pytestmark = pytest.mark.gpu

GUARD = 4096  # bytes past the output that must keep their fill byte
K = 16        # hash values per row in the entry point tests
# levels r = 1, 2, 3 hash values: 16, 8 and 5 bands (r = 3 leaves one value unused); the table's (level, b) rows: whole levels,
# true prefixes, b = 1 and b = 0
LEVEL_R = (1, 2, 3)
TABLE = np.array([(0, 16), (0, 5), (1, 8), (1, 3), (2, 5), (2, 1), (1, 0)], dtype=np.int32)
PARTITIONS = [(1,), (1, 1, 1), (1, 7, 300), (2047, 2049)]
ROW_TYPES = ["u32", "u64", "two-word"]


@pytest.fixture(scope="module")
def ctx():
    return _native.context()


def _guarded(ctx, nbytes):
    buf = ctx.alloc(nbytes + GUARD)
    buf.upload(np.full(nbytes + GUARD, 0xA5, dtype=np.uint8))
    return buf


def _untouched(buf, first, nbytes):
    return bool(np.all(buf.download(nbytes, np.uint8, offset=first) == 0xA5))


class Resident:
    """A hand-built ensemble on the device: the matrix, the level buffers made by numpy, and a dictionary model of them."""

    def __init__(self, ctx, parts, row_type):
        self.ctx, self.words = ctx, 2 if row_type == "two-word" else 1
        rng = np.random.RandomState(sum(parts) + len(row_type))
        n = self.n = sum(parts)
        self.start = np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)
        self.alpha = max(3, n // 8)
        dtype = np.uint32 if row_type == "u32" else np.uint64
        sig = rng.randint(0, self.alpha, (n, K * self.words)).astype(dtype)
        if row_type != "u32":
            sig += np.uint64(2**40)  # every value beyond uint32
        if max(parts) >= 300:  # 200 identical rows in the last partition: a run far past the first galloping steps
            sig[self.start[-2] + 50 : self.start[-2] + 250] = sig[self.start[-2] + 50]
        self.sig, self.dtype = sig, dtype
        self.code = _native.MHX_U32 if dtype == np.uint32 else _native.MHX_U64
        self.d_sig = ctx.to_device(sig)
        self.levels, self.buffers, self.model = [], [], []
        for r in LEVEL_R:
            rw, bands = r * self.words, K // r
            dig, rows = np.empty(bands * n, dtype=np.uint64), np.empty(bands * n, dtype=np.uint32)
            tables = []
            for s0, s1 in zip(self.start[:-1], self.start[1:]):
                d = lsh_bulk.band_digests(sig[s0:s1], bands, rw, gpu_mode="disable").T
                order = np.argsort(d, axis=1, kind="stable")
                dig[bands * s0 : bands * s1] = np.take_along_axis(d, order, axis=1).reshape(-1)
                rows[bands * s0 : bands * s1] = order.reshape(-1)
                per_band = []
                for j in range(bands):
                    table = {}
                    for slot in range(s0, s1):
                        table.setdefault(sig[slot, j * rw : (j + 1) * rw].tobytes(), []).append(slot)
                    per_band.append(table)
                tables.append(per_band)
            self.model.append(tables)
            self.buffers.append((ctx.to_device(dig), ctx.to_device(rows)))
            self.levels.append((self.buffers[-1][0].ptr, self.buffers[-1][1].ptr, rw, bands))

    def probes(self, m, seed):
        rng = np.random.RandomState(seed)
        probes = rng.randint(0, self.alpha, (m, K * self.words)).astype(self.dtype)
        if self.dtype == np.uint64:
            probes += np.uint64(2**40)
        copies = rng.rand(m) < 0.5
        probes[copies] = self.sig[rng.randint(self.n, size=int(copies.sum()))]
        # every row of the table, 255 (an unused partition) and a byte that is no row either
        choice = rng.choice(np.r_[np.arange(len(TABLE)), 255, 100], size=(m, len(self.start) - 1)).astype(np.uint8)
        probes[0], choice[0, -1] = self.sig[-1], 0  # the first probe meets at least the last row
        return probes, choice

    def expected(self, probes, choice):
        pairs = set()
        for q in range(probes.shape[0]):
            for p in range(len(self.start) - 1):
                if choice[q, p] >= len(TABLE):
                    continue
                level, b = TABLE[choice[q, p]].tolist()
                rw = LEVEL_R[level] * self.words
                for j in range(b):
                    for slot in self.model[level][p][j].get(probes[q, j * rw : (j + 1) * rw].tobytes(), ()):
                        pairs.add((q, slot))
        return np.array(sorted(pairs), dtype=np.int64).reshape(-1, 2)

    def call(self, probes, choice, d_pairs, capacity, levels=None, table=TABLE, start=None, null=(), **overrides):
        """One raw call: (status, n_pairs after the call).  levels, table and start replace the resident ones, overrides replace
        single arguments by name, and the arguments named in null are passed as NULL."""
        levels = self.levels if levels is None else levels
        start = np.ascontiguousarray(self.start if start is None else start, dtype=np.int64)
        table = np.ascontiguousarray(table, dtype=np.int32)
        m = probes.shape[0]
        self._keep = (self.ctx.to_device(probes) if m else None, self.ctx.to_device(choice) if choice.size else None)
        args = dict(ctx=self.ctx.handle,
                    levels=(_native.EnsembleLevel * len(levels))(*[_native.EnsembleLevel(d, rw, r, b) for d, rw, r, b in levels]),
                    n_levels=len(levels), start=start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n_parts=start.size - 1,
                    d_index_sig=self.d_sig.ptr, sig_dtype=self.code, row_words=K * self.words,
                    d_query_sig=self._keep[0].ptr if m else None, n_queries=m, d_choice=self._keep[1].ptr if choice.size else None,
                    params=table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n_params=table.shape[0], d_pairs=d_pairs,
                    capacity=capacity)
        found = ctypes.c_int64(-7)
        args["n_pairs"] = ctypes.byref(found)
        assert set(overrides) | set(null) <= set(args), (overrides, null)
        args.update(overrides)
        args.update(dict.fromkeys(null))
        rc = self.ctx.lib.mhx_lsh_ensemble_query_dev(*args.values())
        self.ctx.synchronize()
        return rc, found.value


_residents = {}


def resident(ctx, parts, row_type):
    if (parts, row_type) not in _residents:
        _residents[parts, row_type] = Resident(ctx, parts, row_type)
    return _residents[parts, row_type]


# ---------------------------------------------------------------- 1. the entry point against a numpy model
@pytest.mark.parametrize("m", [1, 257, 3000])
@pytest.mark.parametrize("row_type", ROW_TYPES)
@pytest.mark.parametrize("parts", PARTITIONS, ids=lambda p: "x".join(map(str, p)))
def test_entry_point_equals_the_model(ctx, parts, row_type, m):
    index = resident(ctx, parts, row_type)
    probes, choice = index.probes(m, seed=m)
    want = index.expected(probes, choice)
    assert len(want) > 0
    if m == 3000:
        assert set(np.unique(choice)) == set(range(len(TABLE))) | {100, 255}
    cap = len(want)
    exact = _guarded(ctx, cap * 16)
    if cap > 1:  # one pair short: the count comes back and nothing is written
        short = _guarded(ctx, (cap - 1) * 16)
        rc, found = index.call(probes, choice, short.ptr, cap - 1)
        assert (rc, found) == (_native.MHX_OK, cap)
        assert _untouched(short, 0, (cap - 1) * 16 + GUARD)
    rc, found = index.call(probes, choice, exact.ptr, cap)
    assert (rc, found) == (_native.MHX_OK, cap), _native.last_error()
    assert np.array_equal(exact.download((cap, 2), np.int64), want)  # ascending and unique, as the sorted set is
    assert _untouched(exact, cap * 16, GUARD)


RUNS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 64, 65, 129)  # around every galloping step 1, 2, 4, ... and its closing search


def _runs_index(bands=4, r=2):
    """(index rows, probes, digests of the probes): per band every length of RUNS as one run of equal band keys, the run of 129 at
    the band's first position and the run of 65 at its last; the probes are the keys of all runs and, per band, one key whose
    digest lies below every digest of the band, one above, and one between two runs that is in no run."""
    rng = np.random.RandomState(7)
    pool = rng.randint(0, 2**32, (len(RUNS) + 3, bands * r)).astype(np.uint32)
    dig = lsh_bulk.band_digests(pool, bands, r, gpu_mode="disable")
    sig = np.empty((sum(RUNS), bands * r), dtype=np.uint32)
    for j in range(bands):
        order = np.argsort(dig[:, j])
        below, first, absent, last, above = order[0], order[1], order[len(order) // 2], order[-2], order[-1]
        rest = [p for p in rng.permutation(order).tolist() if p not in (below, first, absent, last, above)]
        at = 0
        for length in rng.permutation(RUNS).tolist():  # another tiling of the rows in every band
            key = first if length == 129 else last if length == 65 else rest.pop()
            sig[at : at + length, j * r : (j + 1) * r] = pool[key, j * r : (j + 1) * r]
            at += length
    return sig, pool, dig


@pytest.mark.parametrize("entry", ["ensemble", "plain"])
def test_long_runs_are_found_whole(ctx, entry):
    """A probe equal to the 200 identical rows meets all of them in every band: the galloping upper bound and its closing search.
    Then runs of every length of RUNS, at a band's two ends and inside, an index that is one run, and probes that fall below,
    above and between the runs: both entry points against numpy's searchsorted left / right (the numpy back ends)."""
    if entry == "ensemble":
        index = resident(ctx, (1, 7, 300), "u32")
        probes = index.sig[index.start[2] + 60][None, :].copy()
        choice = np.array([[255, 255, 0]], dtype=np.uint8)
        want = index.expected(probes, choice)
        assert len(want) >= 200
        out = _guarded(ctx, len(want) * 16)
        assert index.call(probes, choice, out.ptr, len(want)) == (_native.MHX_OK, len(want))
        assert np.array_equal(out.download((len(want), 2), np.int64), want)
    bands, r = 4, 2
    sig, probes, pdig = _runs_index(bands, r)
    ranks = np.argsort(np.argsort(pdig, axis=0), axis=0)
    inner = int(np.flatnonzero(np.all((ranks > 0) & (ranks < len(probes) - 1), axis=1))[0])  # a key with probes below and above it in every band
    one_run = np.repeat(probes[inner : inner + 1], 129, axis=0)
    for rows in (sig, one_run):
        n = rows.shape[0]
        if entry == "plain":
            host, device = _HostBands(bands * r, bands, r, np.uint32), _DeviceBands(ctx, bands * r, bands, r, np.uint32)
            host.append(rows)
            device.append(rows)
            want, got = host.query(probes), device.query(probes)
        else:
            start, table = np.array([0, n], dtype=np.int64), np.array([(0, bands)], dtype=np.int32)
            host, device = _HostEnsemble(bands * r, np.uint32, [(r, bands)], start), _DeviceEnsemble(ctx, bands * r, np.uint32, [(r, bands)], start)
            host.build(rows)
            device.build(rows)
            choice = np.zeros((probes.shape[0], 1), dtype=np.uint8)
            want, got = host.query(probes, choice, table), device.query(probes, choice, table)
        print(f"{entry} n={n}: {want[1].size} (probe, row) pairs, per probe {np.diff(want[0]).tolist()}")
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        idig = np.sort(lsh_bulk.band_digests(rows, bands, r, gpu_mode="disable"), axis=0)
        for j in range(bands):  # what the probes meet in this band, from the digests alone
            lo, hi = np.searchsorted(idig[:, j], pdig[:, j], side="left"), np.searchsorted(idig[:, j], pdig[:, j], side="right")
            assert np.any((hi == 0)) and np.any(lo == n)                            # below all, above all
            if rows is sig:
                assert sorted((hi - lo)[hi > lo].tolist()) == sorted(RUNS)            # every run, whole
                assert np.any((hi == lo) & (lo > 0) & (lo < n))                       # absent, between two runs
                assert (hi - lo)[lo == 0].max() == 129 and (hi - lo)[hi == n].max() == 65  # the runs at the two ends
    assert np.diff(want[0])[inner] == 129  # (the one-run index: its key meets all of it)


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64], ids=["u32", "u64"])
@pytest.mark.parametrize("m", [1, 257])
@pytest.mark.parametrize("n", [1, 2, 300, 5000])
def test_plain_query_equals_an_ensemble_of_one_partition(ctx, n, m, dtype):
    """mhx_lsh_query_dev and mhx_lsh_ensemble_query_dev on the same resident bands -- one level, start = [0, n], table [(0, bands)],
    every choice byte 0 -- return the same count and the same bytes: the two share the search and the verification."""
    bands, r, k = 16, 4, 64
    rng = np.random.RandomState(n + m)
    sig = rng.randint(0, 3, (n, k)).astype(dtype)  # 81 keys per band: buckets of n / 81 rows
    probes = rng.randint(0, 3, (m, k)).astype(dtype)
    probes[::3] = sig[rng.randint(0, n, len(probes[::3]))]
    code = _native.MHX_U32 if dtype == np.uint32 else _native.MHX_U64
    d_sig, d_q, d_choice = ctx.to_device(sig), ctx.to_device(probes), ctx.to_device(np.zeros(m, dtype=np.uint8))
    d_dig, d_rows = ctx.alloc(bands * n * 8), ctx.alloc(bands * n * 4)
    ctx.lsh_sort_bands_dev(d_sig.ptr, code, n, k, bands, r, d_dig.ptr, d_rows.ptr)
    cap = m * n
    plain, ens = _guarded(ctx, cap * 16), _guarded(ctx, cap * 16)
    found_p, found_e = ctypes.c_int64(-7), ctypes.c_int64(-7)
    _native.check(ctx.lib.mhx_lsh_query_dev(ctx.handle, d_dig.ptr, d_rows.ptr, n, bands, r, d_q.ptr, d_sig.ptr, code, k, m, plain.ptr, cap,
                                            ctypes.byref(found_p)))
    level = (_native.EnsembleLevel * 1)(_native.EnsembleLevel(d_dig.ptr, d_rows.ptr, r, bands))
    start, table = np.array([0, n], dtype=np.int64), np.array([(0, bands)], dtype=np.int32)
    _native.check(ctx.lib.mhx_lsh_ensemble_query_dev(ctx.handle, level, 1, start.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1, d_sig.ptr,
                                                     code, k, d_q.ptr, m, d_choice.ptr, table.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), 1,
                                                     ens.ptr, cap, ctypes.byref(found_e)))
    ctx.synchronize()
    print(f"n={n} m={m}: plain {found_p.value} pairs, ensemble {found_e.value}")
    assert found_p.value == found_e.value and 0 < found_p.value <= cap
    assert np.array_equal(plain.download(cap * 16 + GUARD, np.uint8), ens.download(cap * 16 + GUARD, np.uint8))


def test_entry_point_through_the_binding(ctx):
    index = resident(ctx, (2047, 2049), "two-word")
    probes, choice = index.probes(500, seed=9)
    want = index.expected(probes, choice)
    for capacity in (None, 1):  # the default first guess, and one that forces the second call
        offsets, slots = ctx.lsh_ensemble_query_dev(index.levels, index.start, index.d_sig.ptr, index.code, K * index.words, probes, choice,
                                                    TABLE, capacity)
        assert np.array_equal(np.repeat(np.arange(500), np.diff(offsets)), want[:, 0]) and np.array_equal(slots, want[:, 1])


def test_nothing_to_do_returns_zero(ctx):
    index = resident(ctx, (1, 7, 300), "u32")
    probes, choice = index.probes(5, seed=1)
    out = _guarded(ctx, 16)
    assert index.call(probes[:0], choice[:0], out.ptr, 1) == (_native.MHX_OK, 0)                      # M = 0
    assert index.call(probes, choice[:, :1], out.ptr, 1, start=[0, 0]) == (_native.MHX_OK, 0)         # N = 0
    assert index.call(probes, np.full_like(choice, 255), out.ptr, 1) == (_native.MHX_OK, 0)           # every partition skipped
    assert index.call(probes, np.full_like(choice, 6), out.ptr, 1) == (_native.MHX_OK, 0)             # b = 0
    assert _untouched(out, 0, 16 + GUARD)


def test_refused_arguments(ctx):
    index = resident(ctx, (1, 7, 300), "u32")
    probes, choice = index.probes(5, seed=2)
    out = _guarded(ctx, 1024)
    levels = index.levels
    # (every refusal with its message and what it leaves in n_pairs: tests/test_gpu_cabi_arguments.py; here one of each stage of the
    # checks -- scalars, the host tables, the levels' buffers -- on a real index, for the guard)
    bad = [
        dict(null=["n_pairs"]), dict(null=["d_pairs"]), dict(sig_dtype=7), dict(n_levels=17),
        dict(table=np.array([(0, 4), (2, 6)], dtype=np.int32)),     # b > B of its level (5 bands)
        dict(levels=[(None, levels[0][1], 1, 16), levels[1], levels[2]]),
        dict(start=[0, 9, 8, 308]),
    ]
    for overrides in bad:
        rc, found = index.call(probes, choice, out.ptr, **{"capacity": 64, **overrides})
        assert rc == _native.MHX_ERR_INVALID, (overrides, rc)
        assert _native.last_error()
    assert _untouched(out, 0, 1024 + GUARD)
    assert index.call(probes, choice, None, 0)[0] == _native.MHX_OK  # no room asked for: the count alone


# ---------------------------------------------------------------- 2. every (level, partition) block
@pytest.mark.parametrize("case", ["odd-r", "weighted", "few-sizes"])
def test_blocks_are_sort_bands_of_the_partitions_rows(ctx, case):
    spec, keys, rows, sizes, _ = golden_inputs(case)
    index = MinHashLSHEnsemble(gpu_mode="always", **constructor_args(spec))
    index.index_bulk(keys, rows, sizes)
    backend = index._backend
    mat, start = backend.matrix().astype(np.uint64), index._start
    assert len(backend.levels) == len(set(index.params[:, 1].tolist()))
    for (r, bands), (dig, slots) in zip(backend.levels, backend.level_buffers()):
        for s0, s1 in zip(start[:-1].tolist(), start[1:].tolist()):
            if s1 == s0:
                continue
            want_dig, want_rows = ctx.lsh_sort_bands(mat[s0:s1], bands, r)
            assert np.array_equal(dig[bands * s0 : bands * s1], want_dig.reshape(-1))
            assert np.array_equal(slots[bands * s0 : bands * s1], want_rows.reshape(-1))


# ---------------------------------------------------------------- 3. 'always' against 'disable'
def _same_levels(a, b):
    assert np.array_equal(a._backend.matrix(), b._backend.matrix()) and a._backend.dtype == b._backend.dtype
    for (d1, r1), (d2, r2) in zip(a._backend.level_buffers(), b._backend.level_buffers()):
        assert np.array_equal(d1, d2) and np.array_equal(r1, r2)


@pytest.mark.parametrize("case", list(CASES))
def test_golden_cases_on_the_device(case):
    device = check_case(case, "always", golden()["cases"][case])
    spec, keys, rows, sizes, probes = golden_inputs(case)
    host = MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))
    host.index_bulk(keys, rows, sizes)
    _same_levels(device, host)
    for size in PROBE_SIZES:
        assert device.query_bulk(probes, np.full(len(probes), size)) == host.query_bulk(probes, np.full(len(probes), size))


@pytest.fixture(scope="module")
def random_pair():
    """20 000 clustered rows of 128 values, default arguments but threshold 0.5 (four levels), on both back ends."""
    rng = np.random.RandomState(61)
    n, k = 20_000, 128
    bases = rng.randint(0, 2**32, (300, k), dtype=np.int64)
    def draw(count):
        rows = bases[rng.randint(len(bases), size=count)]
        redraw = rng.rand(count, k) < rng.choice([0.02, 0.1, 0.3], size=count)[:, None]
        rows[redraw] = rng.randint(0, 2**32, int(redraw.sum()), dtype=np.int64)
        return rows.astype(np.uint32)
    rows, probes = draw(n), draw(2000)
    sizes = np.minimum((rng.pareto(1.0, n) * 20 + 1).astype(np.int64), 50_000)
    probe_sizes = np.exp(rng.uniform(0, np.log(10_000), 2000)).astype(np.int64)
    pair = []
    for gpu_mode in ("always", "disable"):
        index = MinHashLSHEnsemble(threshold=0.5, gpu_mode=gpu_mode)
        index.index_bulk(range(n), rows, sizes)
        pair.append(index)
    return pair[0], pair[1], probes, probe_sizes


def test_random_rows_on_both_back_ends(random_pair):
    device, host, probes, probe_sizes = random_pair
    assert len(device._backend.levels) >= 3 and None not in device.uppers
    _same_levels(device, host)
    got = device.query_bulk(probes, probe_sizes)
    assert got == host.query_bulk(probes, probe_sizes)
    assert sum(map(len, got)) > len(got) and sum(not a for a in got) * 2 <= len(got)


# ---------------------------------------------------------------- 4. bulk against single queries
def test_query_bulk_equals_query_row_by_row(random_pair):
    device, _, probes, probe_sizes = random_pair
    got = device.query_bulk(probes[:60], probe_sizes[:60])
    for probe, size, answer in zip(probes[:60], probe_sizes[:60].tolist(), got):
        assert list(device.query(signature(probe), size)) == answer


# ---------------------------------------------------------------- 5. widening
def test_a_wide_probe_widens_a_uint32_index():
    spec, keys, rows, sizes, probes = golden_inputs("mixed-u32")
    device = MinHashLSHEnsemble(gpu_mode="always", **constructor_args(spec))
    device.index_bulk(keys, rows, sizes)
    assert device._backend.dtype == np.uint32
    before = device.query_bulk(probes, np.full(len(probes), 40))
    wide = probes.astype(np.uint64)
    wide[0, -1] = 2**32 + 5  # the last band of r = 1, 2 and 4 no longer matches; the others still do
    host = MinHashLSHEnsemble(gpu_mode="disable", **constructor_args(spec))
    host.index_bulk(keys, rows, sizes)
    want = host.query_bulk(wide, np.full(len(wide), 40))
    got = device.query_bulk(wide, np.full(len(wide), 40))
    assert device._backend.dtype == np.uint64 and np.array_equal(device._backend.matrix(), rows[np.argsort(sizes, kind="stable")])
    assert got == want and got[1:] == before[1:] and set(got[0]) <= set(before[0]) and len(got[0]) > 0
    assert device.query_bulk(probes, np.full(len(probes), 40)) == before
