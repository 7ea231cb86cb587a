"""``MinHashLSHEnsemble`` with the reference's public surface (ref: datasketch/lshensemble.py), held as sorted bands.

The reference answers a *containment* query -- which indexed sets contain most of the probe -- with ``num_part`` partitions by
set size, each holding one ``MinHashLSH`` per distinct ``r`` of a table of ten ``(b, r)`` rows; a query picks a row of the table
per partition from ``upper bound / probe size`` and reads the first ``b`` tables of that partition's ``MinHashLSH`` of ``r`` rows
(ref: lshensemble.py:230-249, lsh.py:545-557).

Here the rows are sorted stably by size into ONE signature matrix (:mod:`_index_rows`), so partition ``p`` is the slot range
``[start[p], start[p + 1])``.  Every distinct ``r`` is a *level* of ``B = h // r`` bands: two buffers ``digests u64`` /
``rows u32`` of ``B * N`` entries in which partition ``p`` owns ``[B * start[p], B * start[p + 1])`` -- inside that block band ``j``
starts at ``j * n_p`` and is ascending by ``(digest, row)`` with rows local to the partition: byte for byte what
``mhx_lsh_sort_bands_dev_typed`` writes for the partition's rows, which is how the device back end builds it.  A batch of
probes is answered in one call of ``mhx_lsh_ensemble_query_dev`` (csrc/lsh_query_kernels.hip); which row of the table a
(probe, partition) pair uses is floating point and is decided here, in numpy float64: the device gets a byte per pair.

``gpu_mode`` is the seam of ``MinHashLSH``: ``'always'`` / ``'detect'`` keep the index on an MI355X, ``'disable'`` (or
``'detect'`` without a device) keeps the same level buffers in numpy.

Differences from the reference: no ``indexes`` attribute; sizes ``<= 0`` raise ``ValueError`` everywhere; a key
given twice raises ``ValueError`` before anything is built; keys come back in slot order (ascending partition, then the stable
order by size); only the in-memory storage.
"""
from __future__ import annotations

import functools
import pickle
from typing import Hashable, Iterable, List, Optional

import numpy as np
from scipy.integrate import quad

from datasketch_amd import _native, lsh_bulk
from datasketch_amd._index_rows import DeviceRows, HostRows

__all__ = ["MinHashLSHEnsemble"]

_UNUSED = 255  # the choice byte of a partition that holds nothing: no row of the parameter table


# ---------------------------------------------------------------- the parameter table
def _collision(t: float, xq: float, r: float, b: float) -> float:
    """Probability that a set whose containment of the probe is ``t`` shares one of ``b`` bands of ``r`` rows with it, the set
    being ``xq`` times the probe's size: the Jaccard similarity is then ``t / (1 + xq - t)``."""
    return 1 - (1 - (t / (1 + xq - t)) ** r) ** b


def _weighted_error(threshold: float, b: int, r: int, xq: float, fp_weight: float, fn_weight: float) -> float:
    """False positives: collisions at containments below the threshold (containment cannot exceed ``xq``); false negatives: misses
    between the threshold and ``min(xq, 1)`` (the integrals as ref: lshensemble.py:17-38 takes them)."""
    fr, fb = float(r), float(b)
    fp, _ = quad(lambda t: _collision(t, xq, fr, fb), 0.0, threshold if xq >= threshold else xq)
    fn = 0.0
    if xq >= threshold:
        fn, _ = quad(lambda t: 1 - _collision(t, xq, fr, fb), threshold, 1.0 if xq >= 1.0 else xq)
    return fp * fp_weight + fn * fn_weight


@functools.lru_cache(maxsize=None)
def _params_table(threshold: float, num_perm: int, m: int, fp_weight: float, fn_weight: float):
    """The ten ``(b, r)`` rows: per ``xq`` a grid search over ``b`` ascending, then ``r`` in ``1 .. m`` ascending, with
    ``b * r <= num_perm``, keeping the first strict minimum (the reference's choice, ref: lshensemble.py:41-58)."""
    rows = []
    for xq in np.exp(np.linspace(-5, 5, 10)):
        best, opt = float("inf"), (0, 0)
        for b in range(1, num_perm + 1):
            for r in range(1, min(m, num_perm // b) + 1):
                err = _weighted_error(threshold, b, r, xq, fp_weight, fn_weight)
                if err < best:
                    best, opt = err, (b, r)
        rows.append(opt)
    return tuple(rows)


# ---------------------------------------------------------------- the size partitions
_EXACT_SUMS_BELOW = 256  # distinct sizes below which interval costs are summed slice by slice (see _interval_costs)


def _interval_costs(sizes: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """``cost[l, u]`` (``l <= u``) of one partition over the distinct sizes ``l .. u``: the expected false positives of taking the
    upper bound for every size in it, ``sum((sizes[u] - sizes[i]) / sizes[u] * counts[i])`` (ref: lshensemble_partition.py:54-70).

    Two partitionings can tie exactly, and then rounding decides.  Below ``_EXACT_SUMS_BELOW`` distinct sizes every interval is
    summed on its own with ``numpy.sum`` over the slice, the very additions the reference makes, so a tie falls as it does there;
    above, the terms of an upper bound are summed once from the right (suffix sums): one pass per upper bound instead of one per
    interval, rounding that differs in the last bits."""
    s = sizes.size
    cost = np.zeros((s, s))
    fsizes = sizes.astype(np.float64)
    for u in range(s):
        terms = (float(sizes[u]) - fsizes[: u + 1]) / float(sizes[u]) * counts[: u + 1]
        if s < _EXACT_SUMS_BELOW:
            for l in range(u + 1):
                cost[l, u] = np.sum(terms[l:])
        else:
            cost[: u + 1, u] = np.cumsum(terms[::-1])[::-1]
    return cost


def _first_min(values: np.ndarray) -> int:
    return int(np.argmin(values))  # the first of equal minima: the smallest upper bound index, as the reference's min() over tuples


def _partition_bounds(sizes: np.ndarray, counts: np.ndarray, num_part: int) -> list:
    """``[(lower, upper), ...]`` (inclusive set sizes) for ``num_part`` partitions over the ascending distinct ``sizes`` with
    ``counts`` sets each: the reference's dynamic programme (ref: lshensemble_partition.py:95-196), its shortcuts and its
    back-tracking reproduced as they behave.

    ``best[u, p - 2]`` is the least total cost of ``p`` partitions over sizes ``0 .. u`` (``p = 2 .. num_part - 1``; zero where
    ``u < p - 1``, which the back-tracking reads like any other entry).  The last partition's lower bound minimises
    ``best[u1, num_part - 3] + cost[u1 + 1, last]``; walking back with ``p = num_part - 1 .. 2`` partitions left over ``0 .. u``,
    the next bound minimises ``best[u1, p - 2] + cost[u1 + 1, u]`` over ``u1 = p - 2 .. u - 1`` -- column ``p - 2``, as the
    reference takes it."""
    s = sizes.size
    if num_part < 2:
        return [(sizes[0], sizes[-1])]
    if num_part >= s:
        return [(x, x) for x in sizes]
    cost = _interval_costs(sizes, counts)
    last = s - 1
    if num_part == 2:
        u = _first_min(cost[0, :last] + cost[np.arange(1, s), last])
        return [(sizes[0], sizes[u]), (sizes[u + 1], sizes[-1])]
    # after[u1, u] = cost[u1 + 1, u]: what the partition behind bound u1 costs when it ends at u (u1 < u)
    after = np.full((s, s), np.inf)
    after[:-1, :] = cost[1:, :]
    after[np.tril_indices(s)] = np.inf
    best = np.zeros((s, num_part - 2))
    prev = cost[0, :]  # one partition over 0 .. u1
    for p in range(2, num_part):
        total = prev[:, None] + after  # [u1, u]
        total[: p - 2, :] = np.inf     # u1 >= p - 2: p - 1 partitions need that many sizes
        best[p - 1 :, p - 2] = total[:, p - 1 :].min(axis=0)
        prev = best[:, p - 2]
    u1s = np.arange(num_part - 2, last)
    u = int(u1s[_first_min(best[u1s, num_part - 3] + cost[u1s + 1, last])])
    bounds = [(sizes[u + 1], sizes[-1])]
    for p in range(num_part - 1, 1, -1):
        u1s = np.arange(p - 2, u)
        u1 = int(u1s[_first_min(best[u1s, p - 2] + cost[u1s + 1, u])])
        bounds.insert(0, (sizes[u1 + 1], sizes[u]))
        u = u1
    bounds.insert(0, (sizes[0], sizes[u]))
    return bounds


# ---------------------------------------------------------------- the two back ends
class _HostEnsemble(HostRows):
    """The numpy back end: the size-sorted matrix and, per level, the level buffers ``digests u64[B * N]`` / ``rows u32[B * N]``
    in host memory, built with a stable ``argsort`` per (partition, band) and queried with ``searchsorted``."""

    def __init__(self, kw: int, dtype, levels: list, start: np.ndarray):
        super().__init__(kw, dtype)
        self.levels, self.start = levels, start  # levels: (r in words, bands)
        self.dig, self.rows = [], []

    def build(self, sig: np.ndarray) -> None:
        self.upload(sig)
        n = self.n
        for r, bands in self.levels:
            dig, rows = np.empty(bands * n, dtype=np.uint64), np.empty(bands * n, dtype=np.uint32)
            for s0, s1 in zip(self.start[:-1].tolist(), self.start[1:].tolist()):
                if s1 == s0:
                    continue
                d = lsh_bulk.band_digests(sig[s0:s1], bands, r, gpu_mode="disable").T
                order = np.argsort(d, axis=1, kind="stable")
                dig[bands * s0 : bands * s1] = np.take_along_axis(d, order, axis=1).reshape(-1)
                rows[bands * s0 : bands * s1] = order.reshape(-1)
            self.dig.append(dig)
            self.rows.append(rows)

    def query(self, probes: np.ndarray, choice: np.ndarray, params: np.ndarray):
        m = probes.shape[0]
        found_p, found_s = [], []
        pdig = {}
        for p in range(self.start.size - 1):
            s0, n_p = int(self.start[p]), int(self.start[p + 1] - self.start[p])
            for c in np.unique(choice[:, p]).tolist():
                if c >= params.shape[0] or n_p == 0:
                    continue
                level, b = params[c].tolist()
                r, bands = self.levels[level]
                if level not in pdig:
                    pdig[level] = lsh_bulk.band_digests(probes, bands, r, gpu_mode="disable")
                who = np.flatnonzero(choice[:, p] == c)
                for j in range(b):
                    at = bands * s0 + j * n_p
                    pid, slot = lsh_bulk.band_hits(self.dig[level][at : at + n_p], self.rows[level][at : at + n_p], pdig[level][who, j], who,
                                                   self.sig[:, j * r : (j + 1) * r], probes[:, j * r : (j + 1) * r], s0)
                    found_p.append(pid)
                    found_s.append(slot)
        return lsh_bulk._pairs_to_lists(found_p, found_s, m, self.n)

    def level_buffers(self):
        return list(zip(self.dig, self.rows))


class _DeviceEnsemble(DeviceRows):
    """The device back end: the ``[N, K]`` matrix and the level buffers resident on one MI355X.  Every (level, partition) block is
    one ``mhx_lsh_sort_bands_dev_typed`` call on the partition's slice of the resident matrix, written straight into its place."""

    def __init__(self, ctx, kw: int, dtype, levels: list, start: np.ndarray):
        super().__init__(ctx, kw, dtype)
        self.levels, self.start = levels, start
        self.d_dig, self.d_rows = [], []

    def build(self, sig: np.ndarray) -> None:
        self.upload(sig)
        n = self.n
        for r, bands in self.levels:
            d_dig, d_rows = self.ctx.alloc(bands * n * 8), self.ctx.alloc(bands * n * 4)
            for s0, s1 in zip(self.start[:-1].tolist(), self.start[1:].tolist()):
                if s1 > s0:
                    self.ctx.lsh_sort_bands_dev(self.d_sig.ptr + s0 * self.row_bytes, self.code, s1 - s0, self.kw, bands, r,
                                                d_dig.ptr + bands * s0 * 8, d_rows.ptr + bands * s0 * 4)
            self.d_dig.append(d_dig)
            self.d_rows.append(d_rows)
        self.ctx.synchronize()

    def native_levels(self) -> list:
        return [(d.ptr, rw.ptr, r, bands) for d, rw, (r, bands) in zip(self.d_dig, self.d_rows, self.levels)]

    def query(self, probes: np.ndarray, choice: np.ndarray, params: np.ndarray, capacity: Optional[int] = None):
        if lsh_bulk.needs_widening(self.dtype, probes):
            self.widen()  # a probe value no uint32 row can hold: compare on the full width (the digests do not change)
        return self.ctx.lsh_ensemble_query_dev(self.native_levels(), self.start, self.d_sig.ptr, self.code, self.kw,
                                               np.ascontiguousarray(probes, dtype=self.dtype), choice, params, capacity)

    def level_buffers(self):
        n = self.n
        return [(d.download((bands * n,), np.uint64), rw.download((bands * n,), np.uint32))
                for d, rw, (_, bands) in zip(self.d_dig, self.d_rows, self.levels)]


# ---------------------------------------------------------------- the index
class MinHashLSHEnsemble:
    """The LSH Ensemble index (ref: datasketch/lshensemble.py ``MinHashLSHEnsemble``), in the reference's terms: ``threshold`` is the
    containment threshold, ``num_perm``, ``num_part``, ``m``, ``weights`` and ``prepickle`` mean what they mean there;
    ``storage_config`` takes only the in-memory storage.  ``gpu_mode`` (``'always'`` | ``'detect'`` | ``'disable'``) and ``device``
    choose where the index lives.  Beyond the reference: :meth:`index_bulk` and :meth:`query_bulk`."""

    def __init__(self, threshold: float = 0.9, num_perm: int = 128, num_part: int = 16, m: int = 8, weights=(0.5, 0.5),
                 storage_config=None, prepickle: Optional[bool] = None, gpu_mode: str = "detect", device: Optional[int] = None) -> None:
        storage_config = storage_config if storage_config else {"type": "dict"}
        if not isinstance(storage_config, dict) or storage_config.get("type") != "dict":
            raise ValueError("datasketch_amd.MinHashLSHEnsemble supports only the in-memory storage: storage_config None or {'type': 'dict'}")
        lsh_bulk._check_gpu_mode(gpu_mode)
        if threshold > 1.0 or threshold < 0.0:
            raise ValueError("threshold must be in [0.0, 1.0]")
        if num_perm < 2:
            raise ValueError("Too few permutation functions")
        if num_part < 1:
            raise ValueError("num_part must be at least 1")
        if m < 2 or m > num_perm:
            raise ValueError("m must be in the range of [2, num_perm]")
        if any(w < 0.0 or w > 1.0 for w in weights):
            raise ValueError("Weight must be in [0.0, 1.0]")
        if sum(weights) != 1.0:
            raise ValueError("Weights must sum to 1.0")
        self.threshold = threshold
        self.h = num_perm
        self.m = m
        self.xqs = np.exp(np.linspace(-5, 5, 10))
        self.params = np.array(_params_table(float(threshold), int(num_perm), int(m), float(weights[0]), float(weights[1])), dtype=int)
        if any(self.h // int(r) < 2 for r in self.params[:, 1]):  # (the reference's per-partition MinHashLSH(params=(h // r, r)) raises it)
            raise ValueError("The number of bands are too small (b < 2)")
        self.lowers = [None] * num_part
        self.uppers = [None] * num_part
        self.prepickle = False if prepickle is None else prepickle
        self.gpu_mode, self.device = gpu_mode, device
        if gpu_mode == "always" and not _native.gpu_available():
            raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
        rs = sorted(set(int(r) for r in self.params[:, 1]))
        self._level_r = rs                                                  # level -> r in hash values
        self._table = np.array([(rs.index(int(r)), int(b)) for b, r in self.params], dtype=np.int32)  # table row -> (level, b)
        self._words = None      # uint64 words per hash value: 1 MinHash, 2 WeightedMinHash
        self._backend = None
        self._keys: list = []   # slot -> stored key
        self._key_set = frozenset()
        self._start = None      # int64[num_part + 1]: partition p is the slots [start[p], start[p + 1])

    # ---------------------------------------------------------------- building
    def _stored_key(self, key):
        return pickle.dumps(key) if self.prepickle else key

    @staticmethod
    def _checked_sizes(sizes) -> np.ndarray:
        arr = np.asarray(sizes)
        if arr.ndim != 1:
            raise ValueError("sizes must be one-dimensional")
        if arr.size and not np.all(arr > 0):
            raise ValueError("Set size must be positive")
        return arr

    def index(self, entries: Iterable) -> None:
        """Index all sets given as ``(key, minhash, size)``; it can be called once (ref: lshensemble.py:189-228).  ``minhash`` is
        anything with ``hashvalues`` and ``len()``: a MinHash, LeanMinHash or WeightedMinHash."""
        if not self.is_empty():
            raise ValueError("Cannot call index again on a non-empty index")
        keys, rows, sizes, words = [], [], [], None
        for key, minhash, size in entries:
            if size <= 0:
                raise ValueError("Set size must be positive")
            if len(minhash) != self.h:
                raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
            row, w = lsh_bulk._words_of(minhash.hashvalues)
            words = lsh_bulk._same_words(words, w)
            keys.append(key)
            rows.append(row)
            sizes.append(size)
        if not keys:
            raise ValueError("entries is empty")
        mat = np.stack(rows)
        if words == 1 and int(mat.max()) <= 0xFFFFFFFF:
            mat = mat.astype(np.uint32)
        self._build(keys, mat, words, np.asarray(sizes))

    def index_bulk(self, keys, signatures, sizes) -> None:
        """``index(zip(keys, map(MinHash, signatures), sizes))`` for a ``[N, K]`` uint32 / uint64 matrix, or a WeightedMinHash matrix
        ``[N, S, 2]`` int64.  The matrix's values are taken at call time."""
        if not self.is_empty():
            raise ValueError("Cannot call index again on a non-empty index")
        mat, words = lsh_bulk._words_matrix(signatures)
        n, k = mat.shape
        if k != self.h * words:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, k // words))
        keys = list(keys)
        sizes = self._checked_sizes(sizes)
        if len(keys) != n or sizes.size != n:
            raise ValueError("keys, signatures and sizes must have the same length")
        if n == 0:
            raise ValueError("entries is empty")
        if mat.dtype != np.uint32 and words == 1 and int(mat.max()) <= 0xFFFFFFFF:
            mat = mat.astype(np.uint32)
        self._build(keys, mat, words, sizes)

    def _build(self, keys: list, mat: np.ndarray, words: int, sizes: np.ndarray) -> None:
        stored = list(map(pickle.dumps, keys)) if self.prepickle else keys
        key_set = frozenset(stored)
        if len(key_set) != len(stored):
            raise ValueError("The given key already exists")
        distinct, counts = np.unique(sizes, return_counts=True)
        bounds = _partition_bounds(distinct, counts, len(self.lowers))
        order = np.argsort(sizes, kind="stable")
        uppers = np.array([u for _, u in bounds])
        start = np.zeros(len(self.lowers) + 1, dtype=np.int64)
        start[1 : len(bounds) + 1] = np.searchsorted(sizes[order], uppers, side="right")
        start[len(bounds) + 1 :] = sizes.size
        self._install([stored[i] for i in order.tolist()], mat[order], words, start)  # (fancy indexing: a copy of the caller's matrix)
        for i, (lower, upper) in enumerate(bounds):
            self.lowers[i], self.uppers[i] = lower, upper

    def _install(self, stored: list, mat: np.ndarray, words: int, start: np.ndarray) -> None:
        """The size-sorted rows, their stored keys and the partition starts become the index: the levels are built from them."""
        levels = [(r * words, self.h // r) for r in self._level_r]
        kw = self.h * words
        if lsh_bulk._use_gpu(self.gpu_mode):
            backend = _DeviceEnsemble(_native.context(self.device), kw, mat.dtype, levels, start)
        else:
            backend = _HostEnsemble(kw, mat.dtype, levels, start)
        backend.build(np.ascontiguousarray(mat))
        self._backend, self._words, self._start = backend, words, start
        self._keys, self._key_set = stored, frozenset(stored)

    # ---------------------------------------------------------------- queries
    def _choice(self, sizes: np.ndarray) -> np.ndarray:
        """``uint8[M][P]``: the row of the parameter table each (probe, partition) pair uses -- ``searchsorted(xqs, upper / size,
        'left')`` clipped to the last row (ref: lshensemble.py:178-182) -- and 255 for a partition that holds nothing."""
        choice = np.full((sizes.size, len(self.uppers)), _UNUSED, dtype=np.uint8)
        used = [p for p, u in enumerate(self.uppers) if u is not None]
        if used and sizes.size:
            uppers = np.array([float(self.uppers[p]) for p in used], dtype=np.float64)
            ratio = uppers[None, :] / sizes.astype(np.float64)[:, None]
            choice[:, used] = np.minimum(np.searchsorted(self.xqs, ratio, side="left"), len(self.params) - 1).astype(np.uint8)
        return choice

    def _answers(self, probes: Optional[np.ndarray], sizes: np.ndarray) -> List[list]:
        m = sizes.size
        if probes is None or self._backend is None or m == 0:
            return [[] for _ in range(m)]
        offsets, slots = self._backend.query(probes, self._choice(sizes), self._table)
        keys = list(map(self._keys.__getitem__, slots.tolist()))
        if self.prepickle:
            keys = list(map(pickle.loads, keys))
        bounds = offsets.tolist()
        return [keys[a:b] for a, b in zip(bounds[:-1], bounds[1:])]

    def query(self, minhash, size):
        """A generator of the keys of the sets whose containment of the probe set exceeds the threshold, as the ensemble estimates
        it (ref: lshensemble.py:230-249): per partition, the sets sharing one of the first ``b`` bands of ``r`` rows."""
        if size <= 0:
            raise ValueError("Set size must be positive")
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        row, words = lsh_bulk._words_of(minhash.hashvalues)
        probes = row[None, :] if self._words is None or words == self._words else None
        answer = self._answers(probes, np.asarray([size]))[0]
        return (key for key in answer)

    def query_bulk(self, signatures, sizes) -> List[list]:
        """``[list(query(MinHash(hashvalues=row), size)) for row, size in zip(signatures, sizes)]`` for an ``[M, K]`` (or
        ``[M, S, 2]``) matrix."""
        mat, words = lsh_bulk._words_matrix(signatures)
        m, k = mat.shape
        if k != self.h * words:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, k // words))
        sizes = self._checked_sizes(sizes)
        if sizes.size != m:
            raise ValueError("signatures and sizes must have the same length")
        if self._words is not None and words != self._words:
            return [[] for _ in range(m)]
        return self._answers(mat, sizes)

    def __contains__(self, key: Hashable) -> bool:
        return self._stored_key(key) in self._key_set

    def is_empty(self) -> bool:
        return not self._keys

    # ---------------------------------------------------------------- pickling
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if not k.startswith("_")}
        state["_level_r"], state["_table"], state["_words"] = self._level_r, self._table, self._words
        state["_stored"], state["_start"] = self._keys, self._start
        state["_matrix"] = self._backend.matrix().copy() if self._backend is not None else None
        return state

    def __setstate__(self, state) -> None:
        stored, mat, start, words = state.pop("_stored"), state.pop("_matrix"), state.pop("_start"), state.pop("_words")
        self.__dict__.update(state)
        self._words, self._backend, self._keys, self._key_set, self._start = None, None, [], frozenset(), None
        if mat is not None:
            self._install(stored, mat, words, start)
