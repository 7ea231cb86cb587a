"""``MinHashLSH`` with the reference's public surface (ref: datasketch/lsh.py), held as sorted bands.

The reference keeps one dictionary per band, band key -> set of keys (ref: lsh.py:326-347 insert, :370-431 query).  Here the
index is what :class:`lsh_bulk.SortedBandsIndex` queries: a signature matrix of *slots* and, per band, the 64-bit digests of
every slot's band key in ascending ``(digest, slot)`` order with the slots beside them -- every bucket is a run of equal digests,
and a candidate is confirmed by comparing the band's hash values themselves, so answers are the reference's dictionaries'.

Updates never sort the index again:

* inserts are staged on the host and *flushed* as one batch -- upload into the slots after the last used one, sort the batch's
  bands alone, **merge** them into the index's (``mhx_lsh_bands_merge_dev``);
* ``remove`` only marks the key's slots dead (answers drop dead slots on the host); once dead slots exceed a quarter of the used
  ones the next flush or query **compacts**: slots are renumbered by an order-preserving remap, the bands are rewritten without
  the dead entries and the live signature rows are gathered (``mhx_lsh_bands_compact_dev``, ``mhx_rows_compact_dev``).

A flush happens on any query, ``get_counts``, pickling, ``merge``, :meth:`MinHashLSH.flush`, the end of a session, or when
``buffer_size`` rows are pending.  ``gpu_mode`` is the seam of ``MinHash``: ``'always'`` / ``'detect'`` keep the index on an
MI355X, ``'disable'`` (or ``'detect'`` without a device) keeps the same sorted bands in numpy.  Both back ends hold the same
bands, byte for byte, after the same operations.

Differences from the reference: only the in-memory storage (``storage_config`` ``None`` or ``{"type":
"dict"}``); no ``keys`` / ``hashtables`` storage objects; a key inserted more than once (``check_duplication=False``, or
``merge`` with ``check_overlap=False``) owns all of its rows and ``remove`` drops every one of them -- the reference drops only
the buckets of the first insertion (ref: lsh.py:509-528 pairs the stored band keys with the ``b`` tables), so the buckets of
the later ones stay behind there.  Bucketing is exact on band values whatever ``hashfunc`` is; ``hashfunc`` only names the
buckets :meth:`MinHashLSH.get_counts` reports.
"""
from __future__ import annotations

import itertools
import pickle
from typing import Callable, Hashable, List, Optional

import numpy as np
from scipy.integrate import quad

from datasketch_amd import _native, lsh_bulk
from datasketch_amd._index_rows import DeviceRows, HostRows

__all__ = ["MinHashLSH", "MinHashLSHInsertionSession", "MinHashLSHDeletionSession"]

def _weighted_error(threshold: float, b: int, r: int, fp_weight: float, fn_weight: float) -> float:
    """Weighted false positive + false negative probability of ``b`` bands of ``r`` rows at ``threshold``: a pair of
    similarity ``s`` collides in some band with probability ``1 - (1 - s^r)^b``.  False positives are the collisions below
    the threshold, false negatives the misses above it (the integrands as ref: lsh.py:21-30 evaluates them)."""
    fr, fb = float(r), float(b)
    fp, _ = quad(lambda s: 1 - (1 - s**fr) ** fb, 0.0, threshold)
    fn, _ = quad(lambda s: 1 - (1 - (1 - s**fr) ** fb), threshold, 1.0)
    return fp * fp_weight + fn * fn_weight


def _optimal_param(threshold: float, num_perm: int, fp_weight: float, fn_weight: float):
    """``(b, r)`` with ``b * r <= num_perm`` minimising :func:`_weighted_error`: a grid search over ``b`` ascending, then
    ``r`` ascending, keeping the first strict minimum (the reference's choice, ref: lsh.py:33-48)."""
    best, opt = float("inf"), (0, 0)
    for b in range(1, num_perm + 1):
        for r in range(1, num_perm // b + 1):
            err = _weighted_error(threshold, b, r, fp_weight, fn_weight)
            if err < best:
                best, opt = err, (b, r)
    return opt


class _HostBands(HostRows):
    """The numpy back end: the signature slots and the sorted bands in host memory.  A merge is a stable ``argsort`` by digest
    of A||B, compaction a mask plus a remap, a query ``searchsorted`` per band with the band's words compared."""

    def __init__(self, k: int, b: int, r: int, dtype):
        super().__init__(k, dtype)
        self.b, self.r = b, r
        self.dig = np.empty((b, 0), dtype=np.uint64)
        self.rows = np.empty((b, 0), dtype=np.uint32)

    def _merge_bands(self, dig_b: np.ndarray, rows_b: np.ndarray) -> None:
        """Merge in the sorted bands of rows that take the slots after the last used one."""
        dig = np.concatenate([self.dig, dig_b], axis=1)
        order = np.argsort(dig, axis=1, kind="stable")
        rows = np.concatenate([self.rows, rows_b + np.uint32(self.n)], axis=1)
        self.dig = np.take_along_axis(dig, order, axis=1)
        self.rows = np.take_along_axis(rows, order, axis=1)

    def append(self, sig: np.ndarray) -> None:
        dig = lsh_bulk.band_digests(sig, self.b, self.r, gpu_mode="disable").T
        self._merge_bands(dig, np.broadcast_to(np.arange(sig.shape[0], dtype=np.uint32), dig.shape))
        self.upload(sig)

    def merge_from(self, other: "_HostBands") -> None:
        self._merge_bands(other.dig, other.rows)
        self.copy_from(other)

    def compact(self, live: np.ndarray) -> None:
        n_live = int(np.count_nonzero(live))
        remap = (np.cumsum(live, dtype=np.int64) - 1).astype(np.uint32)
        keep = live[self.rows]
        self.dig = self.dig[keep].reshape(self.b, n_live)
        self.rows = remap[self.rows[keep]].reshape(self.b, n_live)
        self.sig = self.sig[live]

    def query(self, probes: np.ndarray):
        m, r = probes.shape[0], self.r
        pdig = lsh_bulk.band_digests(probes, self.b, r, gpu_mode="disable")
        who = np.arange(m, dtype=np.int64)
        hits = [lsh_bulk.band_hits(self.dig[j], self.rows[j], pdig[:, j], who, self.sig[:, j * r : (j + 1) * r],
                                   probes[:, j * r : (j + 1) * r]) for j in range(self.b)]
        return lsh_bulk._pairs_to_lists([p for p, _ in hits], [s for _, s in hits], m, self.n)

    def bands(self):
        return self.dig, self.rows

    def clusters(self, threshold, extra, words: int = 1) -> np.ndarray:
        return lsh_bulk.bands_clusters_host(self.sig, self.dig, self.rows, threshold, extra, words=words)


class _DeviceBands(DeviceRows):
    """The device back end: the ``[capacity, K]`` signature matrix and the sorted bands ``digests u64[b][n]`` / ``rows u32[b][n]``
    (the layout of ``mhx_lsh_sort_bands_dev_typed``), all resident on one MI355X."""

    def __init__(self, ctx, k: int, b: int, r: int, dtype):
        super().__init__(ctx, k, dtype)
        self.b, self.r = b, r
        self.d_dig = self.d_rows = None

    def _merge_bands(self, d_dig_b: int, d_rows_b: int, m: int):
        """New buffers holding this index's bands merged with the sorted bands of m rows that take slots n .. n+m-1."""
        dig = self.ctx.alloc((self.n + m) * self.b * 8)
        rows = self.ctx.alloc((self.n + m) * self.b * 4)
        if self.n:
            self.ctx.lsh_bands_merge_dev(self.d_dig.ptr, self.d_rows.ptr, self.n, d_dig_b, d_rows_b, m, self.n, self.b, dig.ptr, rows.ptr)
        else:  # nothing to merge with: a copy
            self.ctx.copy_dev(dig.ptr, d_dig_b, m * self.b * 8)
            self.ctx.copy_dev(rows.ptr, d_rows_b, m * self.b * 4)
        return dig, rows

    def append(self, sig: np.ndarray) -> None:
        first, m = self.n, sig.shape[0]
        self.upload(sig)
        self.n = first  # the rows count once their bands are merged in: a failure below leaves the index as it was
        d_dig = self.ctx.alloc(m * self.b * 8)
        d_rows = self.ctx.alloc(m * self.b * 4)
        self.ctx.lsh_sort_bands_dev(self.d_sig.ptr + first * self.row_bytes, self.code, m, self.kw, self.b, self.r, d_dig.ptr, d_rows.ptr)
        dig, rows = self._merge_bands(d_dig.ptr, d_rows.ptr, m) if first else (d_dig, d_rows)
        self.ctx.synchronize()
        self.d_dig, self.d_rows, self.n = dig, rows, first + m

    def merge_from(self, other: "_DeviceBands") -> None:
        """The other index's rows copied device to device after this one's, its bands merged in with that row offset."""
        first, m = self.n, other.n
        self.copy_from(other)
        self.n = first  # as in append
        dig, rows = self._merge_bands(other.d_dig.ptr, other.d_rows.ptr, m)
        self.ctx.synchronize()
        self.d_dig, self.d_rows, self.n = dig, rows, first + m

    def compact(self, live: np.ndarray) -> None:
        n_live = int(np.count_nonzero(live))
        words = np.zeros((self.n + 31) // 32 * 4, dtype=np.uint8)
        packed = np.packbits(live, bitorder="little")
        words[: packed.size] = packed
        d_bits = self.ctx.to_device(words.view(np.uint32))
        cap = max(1024, n_live + n_live // 4)  # the live rows and a quarter of headroom, not the old capacity
        sig = self.ctx.alloc(cap * self.row_bytes)
        kept = self.ctx.rows_compact_dev(self.d_sig.ptr, self.row_bytes, self.n, d_bits.ptr, sig.ptr)
        if kept != n_live:
            raise _native.MhxError(f"row compaction kept {kept} rows, not {n_live}")
        dig = self.ctx.alloc(max(1, n_live * self.b * 8))
        rows = self.ctx.alloc(max(1, n_live * self.b * 4))
        self.ctx.lsh_bands_compact_dev(self.d_dig.ptr, self.d_rows.ptr, self.n, self.b, d_bits.ptr, n_live, dig.ptr, rows.ptr)
        self.d_sig, self.capacity, self.d_dig, self.d_rows, self.n = sig, cap, dig, rows, n_live

    def query(self, probes: np.ndarray, capacity: Optional[int] = None):
        if probes.shape[0] == 0 or self.n == 0:
            return np.zeros(probes.shape[0] + 1, dtype=np.int64), np.empty(0, dtype=np.int64)
        if lsh_bulk.needs_widening(self.dtype, probes):
            self.widen()  # a probe value no uint32 row can hold: compare on the full width
        return self.ctx.lsh_query_dev(self.d_dig.ptr, self.d_rows.ptr, self.n, self.b, self.r, self.d_sig.ptr, self.code, self.kw,
                                      np.ascontiguousarray(probes, dtype=self.dtype), capacity)

    def bands(self):
        if self.n == 0:
            return np.empty((self.b, 0), dtype=np.uint64), np.empty((self.b, 0), dtype=np.uint32)
        return self.d_dig.download((self.b, self.n), np.uint64), self.d_rows.download((self.b, self.n), np.uint32)

    def clusters(self, threshold, extra, words: int = 1) -> np.ndarray:
        return lsh_bulk.rows_clusters(self, self.d_dig.ptr, self.d_rows.ptr, self.b, self.kw, threshold, extra, words=words)


class MinHashLSH:
    """The MinHash LSH index (ref: datasketch/lsh.py ``MinHashLSH``), in the reference's terms: ``threshold``, ``num_perm``,
    ``weights``, ``params``, ``prepickle`` and ``hashfunc`` mean what they mean there; ``storage_config`` takes only the in-memory
    storage.  ``gpu_mode`` (``'always'`` | ``'detect'`` | ``'disable'``) and ``device`` choose where the sorted bands live.

    A key inserted more than once (``check_duplication=False``, or :meth:`merge` with ``check_overlap=False``) owns all of its
    rows: :meth:`query` reports it once and :meth:`remove` drops every row of it.  (The reference's ``remove`` drops only the
    buckets of the key's first insertion.)  Beyond the reference: :meth:`insert_bulk`, :meth:`query_bulk`, :meth:`flush` and
    :meth:`compact`."""

    def __init__(self, threshold: float = 0.9, num_perm: int = 128, weights=(0.5, 0.5), params=None, storage_config=None,
                 prepickle: Optional[bool] = None, hashfunc: Optional[Callable[[bytes], object]] = None, gpu_mode: str = "detect",
                 device: Optional[int] = None) -> None:
        storage_config = storage_config if storage_config else {"type": "dict"}
        if storage_config.get("type") != "dict":
            raise ValueError("datasketch_amd.MinHashLSH supports only the in-memory storage: storage_config None or {'type': 'dict'}")
        lsh_bulk._check_gpu_mode(gpu_mode)
        self._buffer_size = 50000
        if threshold > 1.0 or threshold < 0.0:
            raise ValueError("threshold must be in [0.0, 1.0]")
        if num_perm < 2:
            raise ValueError("Too few permutation functions")
        if any(w < 0.0 or w > 1.0 for w in weights):
            raise ValueError("Weight must be in [0.0, 1.0]")
        if sum(weights) != 1.0:
            raise ValueError("Weights must sum to 1.0")
        self.h = num_perm
        if params is not None:
            self.b, self.r = params
            if self.b * self.r > num_perm:
                raise ValueError(
                    "The product of b and r in params is "
                    f"{self.b} * {self.r} = {self.b * self.r} -- it must be less than num_perm {num_perm}. "
                    "Did you forget to specify num_perm?"
                )
        else:
            self.b, self.r = _optimal_param(threshold, num_perm, weights[0], weights[1])
        if self.b < 2:
            raise ValueError("The number of bands are too small (b < 2)")
        self.prepickle = False if prepickle is None else prepickle
        self.hashfunc = hashfunc
        self.hashranges = [(i * self.r, (i + 1) * self.r) for i in range(self.b)]
        self.gpu_mode, self.device = gpu_mode, device
        if gpu_mode == "always" and not _native.gpu_available():
            raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
        self._reset()

    def _reset(self) -> None:
        self._words = None        # uint64 words per hash value: 1 MinHash, 2 WeightedMinHash (set by the first insert)
        self._backend = None
        self._kid = {}            # stored key -> key id
        self._kid_key = []        # key id -> stored key (None once removed)
        self._kid_slot = np.empty(0, dtype=np.int64)   # key id -> its first slot (-1 once removed)
        self._n_dead_kids = 0     # removed key ids not yet renumbered away
        self._extra = {}          # key id -> its further slots (a key inserted more than once)
        self._slot_kid = np.empty(0, dtype=np.int64)   # slot -> key id, -1 when dead
        self._n_slots = 0         # slots handed out: flushed + pending
        self._n_flushed = 0
        self._n_dead = 0          # dead among the flushed slots
        self._n_dead_pending = 0
        self._pending = []        # rows staged for the next flush (1-D or 2-D arrays of words)
        self._query_buffer = []

    # ---------------------------------------------------------------- attributes of the reference
    @property
    def buffer_size(self) -> int:
        return self._buffer_size

    @buffer_size.setter
    def buffer_size(self, value: int) -> None:
        self._buffer_size = value

    # ---------------------------------------------------------------- bookkeeping
    def _use_gpu(self) -> bool:
        return lsh_bulk._use_gpu(self.gpu_mode)

    def _ensure_backend(self, words: int) -> None:
        self._words = lsh_bulk._same_words(self._words, words)
        if self._backend is None:
            k, r = self.h * words, self.r * words
            dtype = np.uint32 if words == 1 else np.uint64
            if self._use_gpu():
                self._backend = _DeviceBands(_native.context(self.device), k, self.b, r, dtype)
            else:
                self._backend = _HostBands(k, self.b, r, dtype)

    @staticmethod
    def _grown(arr: np.ndarray, need: int) -> np.ndarray:
        if need <= arr.size:
            return arr
        out = np.full(max(need, 2 * arr.size, 1024), -1, dtype=np.int64)
        out[: arr.size] = arr
        return out

    def _register(self, stored_keys: list, fresh: bool) -> None:
        """Key ids and slots for rows that take the next ``len(stored_keys)`` slots.  ``fresh``: the keys are new and distinct."""
        m = len(stored_keys)
        s0 = self._n_slots
        self._slot_kid = self._grown(self._slot_kid, s0 + m)
        if fresh:
            k0 = len(self._kid_key)
            self._kid_slot = self._grown(self._kid_slot, k0 + m)
            self._kid.update(zip(stored_keys, range(k0, k0 + m)))
            self._kid_key.extend(stored_keys)
            self._kid_slot[k0 : k0 + m] = np.arange(s0, s0 + m)
            self._slot_kid[s0 : s0 + m] = np.arange(k0, k0 + m)
        else:
            for i, key in enumerate(stored_keys):
                kid = self._kid.get(key)
                if kid is None:
                    kid = len(self._kid_key)
                    self._kid[key] = kid
                    self._kid_key.append(key)
                    self._kid_slot = self._grown(self._kid_slot, kid + 1)
                    self._kid_slot[kid] = s0 + i
                else:
                    self._extra.setdefault(kid, []).append(s0 + i)
                self._slot_kid[s0 + i] = kid
        self._n_slots += m

    def _stage(self, stored_keys: list, rows, fresh: bool, borrowed: bool = False) -> None:
        """Stage rows for the next flush.  ``borrowed``: ``rows`` is (or views) the caller's array -- whatever is still pending
        when this returns is copied, so the caller may reuse the array; the values are taken at call time."""
        self._register(stored_keys, fresh)
        self._pending.append(rows)
        try:
            if self._n_slots - self._n_flushed >= self._buffer_size:
                self.flush()
        finally:
            if borrowed and self._pending and self._pending[-1] is rows:
                self._pending[-1] = np.array(rows)

    def _upload_pending(self) -> None:
        if not self._pending:
            return
        rows = lsh_bulk._stacked(self._pending)
        backend = self._backend
        if lsh_bulk.needs_widening(backend.dtype, rows):
            backend.widen()
        backend.append(np.ascontiguousarray(rows, dtype=backend.dtype))
        self._pending = []
        self._n_flushed = self._n_slots
        self._n_dead += self._n_dead_pending
        self._n_dead_pending = 0

    def _compact(self) -> None:
        n = self._n_flushed
        if not self._n_dead:
            return
        live = self._slot_kid[:n] >= 0
        self._backend.compact(live)
        keep = np.ones(self._n_slots, dtype=bool)
        keep[:n] = live
        new_slot = np.cumsum(keep, dtype=np.int64) - 1
        kept = int(np.count_nonzero(keep))
        self._slot_kid[:kept] = self._slot_kid[: self._n_slots][keep]
        self._slot_kid[kept : self._n_slots] = -1
        ks = self._kid_slot[: len(self._kid_key)]
        valid = ks >= 0
        ks[valid] = new_slot[ks[valid]]
        for kid, slots in self._extra.items():
            self._extra[kid] = [int(new_slot[s]) for s in slots]
        self._n_slots, self._n_flushed, self._n_dead = kept, n - self._n_dead, 0
        if 2 * self._n_dead_kids > len(self._kid_key):
            self._renumber_keys()

    def _renumber_keys(self) -> None:
        """Drop the ids of removed keys (order-preserving), so that host memory follows the live keys, not every key ever seen."""
        nk = len(self._kid_key)
        alive = self._kid_slot[:nk] >= 0
        new_id = np.cumsum(alive, dtype=np.int64) - 1
        self._kid_key = list(itertools.compress(self._kid_key, alive.tolist()))
        n_alive = len(self._kid_key)
        kid_slot = np.full(max(1024, n_alive), -1, dtype=np.int64)
        kid_slot[:n_alive] = self._kid_slot[:nk][alive]
        self._kid_slot = kid_slot
        self._extra = {int(new_id[kid]): slots for kid, slots in self._extra.items()}
        used = self._slot_kid[: self._n_slots]
        owned = used >= 0
        used[owned] = new_id[used[owned]]
        self._kid = dict(zip(self._kid_key, range(n_alive)))
        self._n_dead_kids = 0

    def _sync(self) -> None:
        """Compact when dead slots exceed a quarter of the used ones, then flush what is pending."""
        if self._backend is None:
            return
        if 4 * self._n_dead > self._n_flushed:
            self._compact()
        self._upload_pending()

    def flush(self) -> None:
        """Push the pending inserts into the index (compacting first when that is due)."""
        self._sync()

    def compact(self) -> None:
        """Flush, then drop every dead slot now."""
        self._sync()
        if self._backend is not None:
            self._compact()

    # ---------------------------------------------------------------- inserts
    def _stored_key(self, key):
        return pickle.dumps(key) if self.prepickle else key

    def insert(self, key: Hashable, minhash, check_duplication: bool = True) -> None:
        """Insert a key with the MinHash (or WeightedMinHash, LeanMinHash: anything with ``hashvalues`` and ``len()``) of its set."""
        self._insert(key, minhash, check_duplication=check_duplication)

    def _insert(self, key: Hashable, minhash, check_duplication: bool = True) -> None:
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        if self.prepickle:
            key = pickle.dumps(key)
        if check_duplication and key in self._kid:
            raise ValueError("The given key already exists")
        row, words = lsh_bulk._words_of(minhash.hashvalues)
        self._ensure_backend(words)
        self._stage([key], row, fresh=key not in self._kid)

    def insert_bulk(self, keys, signatures, check_duplication: bool = True) -> None:
        """``insert(key, MinHash(hashvalues=row))`` for every row: ``signatures`` ``[N, K]`` uint32 / uint64, or a
        WeightedMinHash matrix ``[N, S, 2]`` int64.  With ``check_duplication`` a key present already, or twice in ``keys``,
        raises ``ValueError`` and nothing is inserted."""
        mat, words = lsh_bulk._words_matrix(signatures)
        n, k = mat.shape
        if k != self.h * words:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, k // words))
        keys = list(keys)
        if len(keys) != n:
            raise ValueError("keys and signatures must have the same length")
        if self.prepickle:
            keys = list(map(pickle.dumps, keys))
        distinct = len(set(keys)) == n
        fresh = distinct and self._kid.keys().isdisjoint(keys)
        if check_duplication and not fresh:
            raise ValueError("The given key already exists")
        if n == 0:
            return
        self._ensure_backend(words)
        self._stage(keys, mat, fresh, borrowed=np.shares_memory(mat, np.asarray(signatures)))

    def _stage_stored(self, stored_keys: list, mat: np.ndarray, words: int) -> None:
        """Rows whose keys are stored keys already (pickled where prepickle is on): unpickling, merging through the host."""
        self._ensure_backend(words)
        self._stage(stored_keys, mat, fresh=len(set(stored_keys)) == len(stored_keys) and self._kid.keys().isdisjoint(stored_keys))

    # ---------------------------------------------------------------- removal
    def remove(self, key: Hashable) -> None:
        """Remove the key and every row inserted under it.  ``ValueError`` if it does not exist."""
        self._remove(key)

    def _remove(self, key: Hashable) -> None:
        if self.prepickle:
            key = pickle.dumps(key)
        kid = self._kid.pop(key, None)
        if kid is None:
            raise ValueError("The given key does not exist")
        for s in [int(self._kid_slot[kid])] + self._extra.pop(kid, []):
            self._slot_kid[s] = -1
            if s < self._n_flushed:
                self._n_dead += 1
            else:
                self._n_dead_pending += 1
        self._kid_slot[kid] = -1
        self._kid_key[kid] = None
        self._n_dead_kids += 1

    def __contains__(self, key: Hashable) -> bool:
        if self.prepickle:
            key = pickle.dumps(key)
        return key in self._kid

    def is_empty(self) -> bool:
        return not self._kid

    # ---------------------------------------------------------------- queries
    def _probe_matrix(self, minhashes) -> Optional[np.ndarray]:
        rows = []
        for m in minhashes:
            if len(m) != self.h:
                raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(m)))
            row, words = lsh_bulk._words_of(m.hashvalues)
            if self._words is not None and words != self._words:
                return None
            rows.append(row)
        return np.stack(rows) if rows else np.empty((0, self.h), dtype=np.uint64)

    def _answers(self, probes: Optional[np.ndarray], m: int, stored: bool = False) -> List[list]:
        """Keys (``stored``: as stored, pickled where prepickle is on) per probe row of a words matrix (``None``: probes that
        can match nothing)."""
        self._sync()
        if probes is None or self._backend is None or self._n_flushed == 0 or m == 0:
            return [[] for _ in range(m)]
        offsets, slots = self._backend.query(probes)
        kids = self._slot_kid[slots]
        probe = np.repeat(np.arange(m, dtype=np.int64), np.diff(offsets))
        live = kids >= 0
        nk = max(len(self._kid_key), 1)
        code = np.unique(probe[live] * nk + kids[live])
        starts = lsh_bulk._starts(np.bincount(code // nk, minlength=m)).tolist()
        keys = list(map(self._kid_key.__getitem__, (code % nk).tolist()))
        if self.prepickle and not stored:
            keys = list(map(pickle.loads, keys))
        return [keys[a:b] for a, b in zip(starts[:-1], starts[1:])]

    def query(self, minhash) -> list:
        """The keys sharing at least one band key with ``minhash`` (ref: lsh.py:370-431), each once."""
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        return self._answers(self._probe_matrix([minhash]), 1)[0]

    def query_bulk(self, signatures) -> List[list]:
        """``[query(MinHash(hashvalues=row)) for row in signatures]`` for an ``[M, K]`` (or ``[M, S, 2]``) matrix."""
        mat, words = lsh_bulk._words_matrix(signatures)
        m, k = mat.shape
        if k != self.h * words:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, k // words))
        if self._words is not None and words != self._words:
            return [[] for _ in range(m)]
        return self._answers(mat, m)

    def nearest_bulk(self, signatures, k: int, threshold: Optional[float] = None) -> List[list]:
        """Per row of an ``[M, K]`` matrix of probes the ``k`` keys nearest by ``MinHash.jaccard``: a list of up to ``k``
        ``(key, jaccard)``, best first, ties by the earlier insertion; keys as :meth:`query` returns them.  Exact -- every live
        row of the index is compared, no banding in front.  ``threshold``: only keys whose Jaccard is ``>= threshold``.  A key
        inserted more than once is reported once, with its nearest row: the scan asks for ``k`` + (live rows - live keys)
        rows, which must not exceed 64.  Pending inserts are flushed first; removed rows are masked, not compacted.  An index
        of WeightedMinHash signatures takes ``[M, S, 2]`` probes and ranks by ``WeightedMinHash.jaccard``; probes of the other
        kind than the index's are a ``ValueError``."""
        mat, words = lsh_bulk._words_matrix(signatures)
        if self._words is not None and words != self._words:
            raise ValueError("Cannot compare MinHash and WeightedMinHash signatures: the index holds %s ones"
                             % ("WeightedMinHash" if self._words == 2 else "MinHash"))
        m, kw = mat.shape
        if kw != self.h * words:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, kw // words))
        k = lsh_bulk._check_topk(k)
        self._sync()
        n = self._n_flushed
        if self._backend is None or n == 0 or m == 0:
            return [[] for _ in range(m)]
        kids = self._slot_kid[:n]
        live = kids >= 0
        want = k + int(np.count_nonzero(live)) - len(self._kid)
        if want > _native.MHX_TOPK_MAX:
            raise ValueError("k plus the rows of keys inserted more than once is %d: it must not exceed %d" % (want, _native.MHX_TOPK_MAX))
        backend = self._backend
        if lsh_bulk.needs_widening(backend.dtype, mat):
            backend.widen()  # a probe value no uint32 row can hold: compare on the full width
        rows, counts = lsh_bulk.rows_nearest(backend, np.ascontiguousarray(mat, dtype=backend.dtype), want, threshold,
                                             None if self._n_dead == 0 else live, words=words)
        out = []
        for row, count in zip(rows.tolist(), counts.tolist()):
            seen, best = set(), []
            for slot, c in zip(row, count):
                if slot < 0 or len(best) == k:
                    break
                kid = int(kids[slot])
                if kid not in seen:
                    seen.add(kid)
                    key = self._kid_key[kid]
                    best.append((pickle.loads(key) if self.prepickle else key, c / float(self.h)))
            out.append(best)
        return out

    def nearest(self, minhash, k: int, threshold: Optional[float] = None) -> list:
        """``[(key, jaccard)]`` of the up to ``k`` keys nearest to ``minhash``, best first (:meth:`nearest_bulk` of one probe)."""
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        hv = np.asarray(minhash.hashvalues)
        return self.nearest_bulk(hv[None], k, threshold)[0]

    def duplicate_clusters(self, threshold: Optional[float] = None, min_size: int = 2) -> List[list]:
        """The near-duplicate clusters of the indexed keys: lists of keys (as :meth:`query` returns them) of at least
        ``min_size`` keys each (``min_size=1`` includes the keys that are alone).  ``threshold=None``: keys are one cluster when
        a chain of shared band keys joins them -- the connected components of what :meth:`query` reports for the keys
        themselves.  With a ``threshold`` two rows that share a band key are joined only when their ``MinHash.jaccard`` estimate
        is ``>= threshold`` (on an index of WeightedMinHash signatures: their ``WeightedMinHash.jaccard``, as
        ``lsh_bulk.weighted_duplicate_clusters`` does), as ``lsh_bulk.duplicate_clusters`` does.  A key inserted more than once
        joins the clusters of all its rows.  Clusters come ordered by their first inserted key, the keys inside a cluster in
        insertion order (by slot).  Calls :meth:`compact` first: removed keys are gone before anything is linked."""
        min_size = int(min_size)
        if min_size < 1:
            raise ValueError("min_size must be at least 1")
        self.compact()
        n = self._n_flushed
        if self._backend is None or n == 0:
            return []
        extra = [(int(self._kid_slot[kid]), s) for kid, slots in self._extra.items() for s in slots]
        labels = self._backend.clusters(threshold, np.asarray(extra, dtype=np.int64).reshape(-1, 2), self._words)
        kids = self._slot_kid[:n]
        first = np.flatnonzero(self._kid_slot[kids] == np.arange(n))  # one slot per key: its first
        order = first[np.argsort(labels[first], kind="stable")]       # by (cluster's smallest slot, slot)
        sizes = np.unique(labels[order], return_counts=True)[1]
        keys = list(map(self._kid_key.__getitem__, kids[order].tolist()))
        if self.prepickle:
            keys = list(map(pickle.loads, keys))
        starts = lsh_bulk._starts(sizes).tolist()
        return [keys[a:b] for a, b in zip(starts[:-1], starts[1:]) if b - a >= min_size]

    def add_to_query_buffer(self, minhash) -> None:
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        self._query_buffer.append(minhash)

    def collect_query_buffer(self) -> list:
        """The keys every buffered probe would get from :meth:`query` (the intersection, as ref: lsh.py:455-483)."""
        buffered, self._query_buffer = self._query_buffer, []
        if not buffered:
            return []
        probes = self._probe_matrix(buffered)
        sets = [set(a) for a in self._answers(probes, len(buffered), stored=True)]
        common = set.intersection(*sets)
        return [pickle.loads(k) for k in common] if self.prepickle else list(common)

    # ---------------------------------------------------------------- counts
    def _bucket_counts(self, slots: np.ndarray) -> list:
        tables = [dict() for _ in range(self.b)]
        if self._backend is None or slots.size == 0:
            return tables
        mat = self._backend.matrix()[slots]
        kids = self._slot_kid[slots].tolist()
        cols = lsh_bulk.band_keys(mat, self.b, self.r * self._words, gpu_mode="disable").T.tolist()
        for j, col in enumerate(cols):
            if self.hashfunc is not None:
                col = list(map(self.hashfunc, col))
            counts = tables[j]
            for h, _kid in set(zip(col, kids)):
                counts[h] = counts.get(h, 0) + 1
        return tables

    def get_counts(self) -> list:
        """Per band, bucket key -> number of distinct keys in it (bucket keys: the band key bytes, through ``hashfunc`` if set)."""
        self._sync()
        return self._bucket_counts(np.flatnonzero(self._slot_kid[: self._n_flushed] >= 0))

    def get_subset_counts(self, *keys: Hashable) -> list:
        """:meth:`get_counts` restricted to ``keys`` (keys not in the index count nothing)."""
        self._sync()
        slots = []
        for key in set(keys):
            kid = self._kid.get(self._stored_key(key))
            if kid is not None:
                slots.append(int(self._kid_slot[kid]))
                slots.extend(self._extra.get(kid, []))
        return self._bucket_counts(np.asarray(sorted(slots), dtype=np.int64))

    # ---------------------------------------------------------------- merge, sessions, pickling
    def merge(self, other: "MinHashLSH", check_overlap: bool = False) -> None:
        """Make this index the union of both (ref: lsh.py:349-368).  Keys present in both own the rows of both."""
        if type(self) is not type(other):
            raise ValueError(f"Cannot merge type MinHashLSH and type {type(other).__name__}.")
        if (self.h, self.b, self.r) != (other.h, other.b, other.r) or (
                self._words is not None and other._words is not None and self._words != other._words):
            raise ValueError("Cannot merge MinHashLSH with different initialization parameters.")
        if check_overlap and not self._kid.keys().isdisjoint(other._kid.keys()):
            raise ValueError("The keys are overlapping, duplicate key exists.")
        if other._backend is None or not other._kid:
            return
        other.compact()
        self._sync()
        n_o = other._n_flushed
        stored = list(map(other._kid_key.__getitem__, other._slot_kid[:n_o].tolist()))
        self._ensure_backend(other._words)
        mine, theirs = self._backend, other._backend
        same_home = type(mine) is type(theirs) and (isinstance(mine, _HostBands) or mine.ctx is theirs.ctx)
        if same_home and mine.dtype.itemsize < theirs.dtype.itemsize:
            mine.widen()
        if same_home and (mine.dtype == theirs.dtype or isinstance(mine, _HostBands)):
            mine.merge_from(theirs)  # rows copied, bands merged with the row offset: nothing is sorted again
            self._register(stored, fresh=len(set(stored)) == n_o and self._kid.keys().isdisjoint(stored))
            self._n_flushed = self._n_slots
        else:  # different back end or device: through the host
            self._stage_stored(stored, theirs.matrix()[:n_o].astype(np.uint64), other._words)
            self._sync()

    def insertion_session(self, buffer_size: int = 50000) -> "MinHashLSHInsertionSession":
        return MinHashLSHInsertionSession(self, buffer_size=buffer_size)

    def deletion_session(self, buffer_size: int = 50000) -> "MinHashLSHDeletionSession":
        return MinHashLSHDeletionSession(self, buffer_size=buffer_size)

    def __getstate__(self):
        self.compact()
        n = self._n_flushed
        state = {k: v for k, v in self.__dict__.items() if not k.startswith("_")}
        state["_buffer_size"] = self._buffer_size
        state["_words"] = self._words
        state["_stored"] = list(map(self._kid_key.__getitem__, self._slot_kid[:n].tolist()))
        state["_matrix"] = self._backend.matrix()[:n].copy() if self._backend is not None else None
        state["_dtype"] = self._backend.dtype.str if self._backend is not None else None
        return state

    def __setstate__(self, state) -> None:
        stored, mat, words, dtype = state.pop("_stored"), state.pop("_matrix"), state.pop("_words"), state.pop("_dtype")
        self.__dict__.update(state)
        self._reset()
        if words is not None:
            self._ensure_backend(words)
            if np.dtype(dtype) == np.uint64 and self._backend.dtype == np.uint32:
                self._backend.widen()
            if len(stored):
                self._stage_stored(stored, mat, words)
            self._sync()


class MinHashLSHInsertionSession:
    """Context manager for batch insertion (ref: lsh.py ``MinHashLSHInsertionSession``): rows are staged and flushed every
    ``buffer_size`` rows and at the end of the session."""

    def __init__(self, lsh: MinHashLSH, buffer_size: int):
        self.lsh = lsh
        self.lsh.buffer_size = buffer_size

    def __enter__(self) -> "MinHashLSHInsertionSession":
        return self

    def __exit__(self, exc_type, exc_val, exc_tb) -> None:
        self.close()

    def close(self) -> None:
        self.lsh.flush()

    def insert(self, key: Hashable, minhash, check_duplication=True) -> None:
        self.lsh._insert(key, minhash, check_duplication=check_duplication)


class MinHashLSHDeletionSession:
    """Context manager for batch deletion (ref: lsh.py ``MinHashLSHDeletionSession``)."""

    def __init__(self, lsh: MinHashLSH, buffer_size: int):
        self.lsh = lsh
        self.lsh.buffer_size = buffer_size

    def __enter__(self) -> "MinHashLSHDeletionSession":
        return self

    def __exit__(self, exc_type, exc_val, exc_tb) -> None:
        self.close()

    def close(self) -> None:
        self.lsh.flush()

    def remove(self, key: Hashable) -> None:
        self.lsh._remove(key)
