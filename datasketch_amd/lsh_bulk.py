"""Bulk helpers on the consumer side of the signature matrix.

The reference's ``MinHashLSH`` stays what it is -- host-side control plane that duck-types on
``.hashvalues`` -- and keeps working on our objects unchanged.  What this module adds is the
whole-matrix form of the three per-object steps around it, so that 10^6 signatures do not cost 10^6
Python round trips:

* :func:`band_keys` / :func:`band_digests` -- every band key of every signature in one pass
  (ref: datasketch/lsh.py:199,344,537-543), as the exact key bytes or as 64-bit FNV-1a digests of them;
* :func:`insert_bulk` -- ``MinHashLSH.insert`` for a whole matrix (ref: lsh.py:326-347), leaving the index
  in exactly the state the per-key loop would: for the in-memory storage (``storage.py:210-259``) every band's
  ``defaultdict(set)`` is built by ONE ``dict.update`` over C-level iterators instead of N ``insert`` calls;
  other back ends (Redis, Cassandra) go through the index's own storage API key by key;
* :func:`query_bulk` -- ``MinHashLSH.query`` (ref: lsh.py:370-431) for a whole matrix of probes;
  :class:`SortedBandsIndex` -- the same question answered on the device against an index held as sorted
  bands (binary search of M x b probe digests, exact band-key verification, sort + unique);
* :func:`sorted_bands` / :func:`candidate_pairs` -- LSH bucketing by sort: per band the digests in
  ascending order with their rows (device radix sort), and from that the pairs of rows that share at
  least one band (what ``query`` would find), without probing dictionaries -- on the device the
  whole chain (digests, sorts, run detection, pair emission, sort + unique) is one call;
* :func:`jaccard_pairs` -- ``MinHash.jaccard`` for a list of pairs (ref: datasketch/minhash.py:299-324);
* :func:`jaccard_matrix` / :func:`similar_pairs` -- ``MinHash.jaccard`` of every row of A against every row of B
  (or of A against itself), as a dense matrix or as the pairs at or above a threshold: exhaustive near-duplicate
  search with no LSH banding in front, so no pair is missed by design;
* :func:`nearest_neighbors` -- per row of A the ``k`` rows of B with the largest ``MinHash.jaccard``, by an exact scan
  that never forms the matrix (:meth:`SortedBandsIndex.nearest`, ``MinHashLSH.nearest_bulk``: the same against an index);
* :func:`connected_components` / :func:`duplicate_clusters` -- the step after the pairs: the near-duplicate clusters as
  ``labels[i]`` = the smallest row of ``i``'s connected component, by a lock-free union-find on the device that reads listed
  pairs or the sorted bands themselves (:meth:`SortedBandsIndex.clusters`, ``MinHashLSH.duplicate_clusters``).

The banding helpers also take a WeightedMinHash matrix ``[N, S, 2]`` int64 (``WeightedMinHashGenerator.minhash_many_arrays``):
its band keys are the reference's too (16*r bytes per band).  The Jaccard steps have weighted twins of their own, since a position
of such a row is a ``(k, t)`` pair: :func:`weighted_jaccard_pairs`, :func:`weighted_jaccard_matrix`, :func:`weighted_similar_pairs`,
:func:`weighted_nearest_neighbors` and :func:`weighted_duplicate_clusters` are ``WeightedMinHash.jaccard`` (ref:
weighted_minhash.py:45-60) for listed pairs, every pair, the pairs at a threshold, the ``k`` nearest and the clusters;
:class:`SortedBandsIndex` and ``MinHashLSH`` built on weighted rows answer ``nearest`` and thresholded clusters with them.
"""
from __future__ import annotations

import pickle
from typing import Hashable, Iterable, List, Optional, Sequence

import numpy as np

from datasketch_amd import _native
from datasketch_amd._index_rows import DeviceRows, HostRows

_FNV_OFFSET = np.uint64(0xCBF29CE484222325)
_FNV_PRIME = np.uint64(0x100000001B3)


def fnv1a_64(data: bytes) -> int:
    """64-bit FNV-1a of a byte string.  ``MinHashLSH(hashfunc=fnv1a_64)`` stores exactly the values
    :func:`band_digests` computes."""
    h = 0xCBF29CE484222325
    for byte in bytes(data):
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def _use_gpu(gpu_mode: str) -> bool:
    if gpu_mode == "always":
        if not _native.gpu_available():
            raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
        return True
    return gpu_mode == "detect" and _native.gpu_detected()


def _matrix(signatures) -> np.ndarray:
    """``[N, K]`` uint64 view of a signature matrix.  A WeightedMinHash matrix ``[N, S, 2]`` int64 (rows of
    ``(k, t)`` pairs, ref: weighted_minhash.py:11-30) is viewed as ``[N, 2S]`` words: the reference's band
    key of ``hashvalues[i*r:(i+1)*r]`` is then the key of ``2r`` consecutive words (see :func:`_words`)."""
    sig = np.asarray(signatures)
    if sig.ndim == 3 and sig.shape[2] == 2:
        sig = np.ascontiguousarray(sig, dtype=np.int64).view(np.uint64).reshape(sig.shape[0], 2 * sig.shape[1])
        return sig
    sig = np.ascontiguousarray(sig, dtype=np.uint64)
    if sig.ndim != 2:
        raise ValueError("signatures must be an [N, K] matrix (or [N, S, 2] for WeightedMinHash)")
    return sig


def _words(signatures) -> int:
    """uint64 words per hash value: 2 for a WeightedMinHash matrix ``[N, S, 2]``, else 1."""
    return 2 if np.ndim(signatures) == 3 else 1


def _words_of(hashvalues):
    """(uint64 words of one signature, words per hash value): a MinHash's ``[h]`` values, or a WeightedMinHash's ``[h, 2]``
    int64 ``(k, t)`` pairs viewed as ``2h`` words -- the reference's band key bytes are the big-endian bytes of those words."""
    a = np.asarray(hashvalues)
    if a.ndim == 2:
        return np.ascontiguousarray(a, dtype=np.int64).view(np.uint64).reshape(-1).copy(), 2
    return np.array(a, dtype=np.uint64), 1


def _words_matrix(signatures):
    """(words matrix, words per hash value) of a bulk argument ``[N, K]`` / ``[N, S, 2]``: :func:`_matrix`, except that a uint32
    matrix is kept as it is (the indexes hold uint32 rows while every value fits)."""
    sig = np.asarray(signatures)
    mat = np.ascontiguousarray(sig) if sig.ndim == 2 and sig.dtype == np.uint32 else _matrix(sig)
    return mat, _words(sig)


def needs_widening(dtype, rows: np.ndarray) -> bool:
    """Whether an index holding rows of ``dtype`` has to become uint64 before it stores ``rows`` or is compared with them: it is
    uint32 and some value of ``rows`` is one no uint32 row can hold."""
    return dtype == np.uint32 and rows.dtype != np.uint32 and rows.size > 0 and int(rows.max()) > 0xFFFFFFFF


def _check_gpu_mode(gpu_mode: str) -> None:
    if gpu_mode not in ("always", "detect", "disable"):
        raise ValueError("gpu_mode must be 'always', 'detect' or 'disable'")


def _same_words(have: Optional[int], words: int) -> int:
    """The words per hash value of an index that holds ``have`` (``None``: nothing yet) and now takes rows of ``words``."""
    if have is not None and words != have:
        raise ValueError("Cannot index MinHash and WeightedMinHash signatures together")
    return words


def _stacked(pending: list) -> np.ndarray:
    """The staged rows (1-D or 2-D arrays of words) as one matrix; a single staged matrix is returned as it is."""
    return pending[0] if len(pending) == 1 and pending[0].ndim == 2 else np.vstack(pending)


def _check_params(k: int, b: int, r: int) -> None:
    if b <= 0 or r <= 0 or b * r > k:
        raise ValueError("b*r must be in (0, num_perm]")


def band_keys(signatures, b: int, r: int, gpu_mode: str = "detect") -> np.ndarray:
    """``[N, b]`` array of ``numpy.void`` items of ``8*r`` bytes: item ``[i, j]`` holds exactly
    ``MinHashLSH._H(hashvalues[j*r:(j+1)*r])`` of row ``i`` (big-endian words, ref: lsh.py:537-538).
    ``.tolist()`` gives nested lists of ``bytes``; ``bytes(out[i, j])`` one key."""
    sig, r = _matrix(signatures), r * _words(signatures)
    n, k = sig.shape
    _check_params(k, b, r)
    if _use_gpu(gpu_mode):
        swapped = _native.context().band_keys(sig, b, r)
    else:
        swapped = sig[:, : b * r].byteswap()
    swapped = np.ascontiguousarray(swapped).reshape(n, b * r)
    return swapped.view(np.dtype((np.void, 8 * r))).reshape(n, b)


def band_digests(signatures, b: int, r: int, gpu_mode: str = "detect") -> np.ndarray:
    """``[N, b]`` uint64: FNV-1a-64 of every band key.  Equal band keys give equal digests; different band keys
    give different digests except for 64-bit hash collisions (one expected among ~6*10^9 keys of one band).
    :func:`sorted_bands` / :func:`candidate_pairs` group by digest, so such a collision would add one candidate
    pair the reference's byte-keyed dictionaries would not report -- harmless where candidates are verified
    with :func:`jaccard_pairs` afterwards; :class:`SortedBandsIndex` compares the band's values themselves."""
    sig, r = _matrix(signatures), r * _words(signatures)
    n, k = sig.shape
    _check_params(k, b, r)
    if _use_gpu(gpu_mode):
        return _native.context().band_digests(sig, b, r)
    key_bytes = np.ascontiguousarray(sig[:, : b * r].byteswap()).view(np.uint8).reshape(n, b, 8 * r)
    h = np.full((n, b), _FNV_OFFSET, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(8 * r):
            h = (h ^ key_bytes[:, :, c].astype(np.uint64)) * _FNV_PRIME
    return h


def _starts(counts: np.ndarray) -> np.ndarray:
    out = np.zeros(counts.size + 1, dtype=np.int64)
    np.cumsum(counts, out=out[1:])
    return out


def band_hits(col: np.ndarray, rows: np.ndarray, want: np.ndarray, who: np.ndarray, sig_band: np.ndarray, probe_band: np.ndarray,
              slot0: int = 0):
    """The numpy back ends' lookup in ONE sorted band: ``col`` its ascending digests with ``rows`` beside them, ``want`` the
    wanted digests of the probes ``who`` (ids into the probe matrix), ``sig_band`` / ``probe_band`` the band's columns of the
    index and probe matrices, ``slot0`` the slot of row 0.  Every probe's bucket is the run between ``searchsorted`` left and
    right; returns ``(probe ids, slots)`` of the bucket entries whose band words equal the probe's."""
    lo = np.searchsorted(col, want, side="left")
    cnt = np.searchsorted(col, want, side="right") - lo
    total = int(cnt.sum())
    pid = np.repeat(who, cnt)
    pos = np.arange(total, dtype=np.int64) + np.repeat(lo - _starts(cnt)[:-1], cnt)
    slot = slot0 + rows[pos].astype(np.int64)
    same = np.all(sig_band[slot] == probe_band[pid], axis=1)
    return pid[same], slot[same]


def _pairs_to_lists(found_p, found_s, m: int, n: int):
    """(offsets int64[m + 1], slots int64[...]) of unique (probe, slot) pairs, ascending."""
    offsets = np.zeros(m + 1, dtype=np.int64)
    if not found_p:
        return offsets, np.empty(0, dtype=np.int64)
    code = np.unique(np.concatenate(found_p) * max(n, 1) + np.concatenate(found_s))
    np.cumsum(np.bincount(code // max(n, 1), minlength=m), out=offsets[1:])
    return offsets, code % max(n, 1)


def _is_dict_index(lsh) -> bool:
    """The reference's in-memory storage: ``keys`` a DictListStorage, every hashtable a DictSetStorage
    (ref: datasketch/storage.py:210-259), recognised by what they are made of."""
    import collections

    def plain(store, factory):
        d = getattr(store, "_dict", None)
        return isinstance(d, collections.defaultdict) and d.default_factory is factory

    return plain(lsh.keys, list) and all(plain(h, set) for h in lsh.hashtables)


def insert_bulk(lsh, keys: Iterable[Hashable], signatures, check_duplication: bool = True, gpu_mode: str = "detect",
                settle: str = "collect") -> None:
    """``for key, row in zip(keys, signatures): lsh.insert(key, MinHash(hashvalues=row))`` in bulk.

    ``lsh`` is a ``datasketch.MinHashLSH`` (or anything with its attributes ``h, b, r, keys,
    hashtables, prepickle, hashfunc``).  Validation, key pickling and the duplicate check are those of
    ref: datasketch/lsh.py:326-347; the ``b`` band keys per signature come from one pass over the matrix.
    With the in-memory storage the dictionaries are filled wholesale: ``keys`` by one ``dict.update`` of
    ``key -> [H_0 .. H_{b-1}]`` and every band's table by one ``dict.update`` of ``H -> {key}`` for the band
    keys that occur once and are new, plus a loop over the (few) band keys shared by several rows or already
    present -- the resulting state equals the per-key loop's.  Other storages take the per-key calls.

    ``settle`` says what happens to the ``N * (b + 1)`` new containers once the dictionaries are built (the
    cyclic collector is held off while they are): ``"collect"`` runs one full collection, which moves them
    into the oldest generation in a single walk (left young they would be walked three times, by whatever
    code allocates next -- 4.9 s landed on the first ``query_bulk`` after 300 000 keys); ``"freeze"`` calls
    ``gc.freeze()`` instead (no walk now or ever, process-wide effect); ``"leave"`` does neither."""
    if settle not in ("collect", "freeze", "leave"):
        raise ValueError("settle must be 'collect', 'freeze' or 'leave'")
    from datasketch_amd.lsh import MinHashLSH

    if isinstance(lsh, MinHashLSH):  # our own index: its bulk path (the index's gpu_mode decides where it lives)
        return lsh.insert_bulk(keys, signatures, check_duplication=check_duplication)
    sig, words = _matrix(signatures), _words(signatures)
    n, k = sig.shape
    if k != lsh.h * words:
        raise ValueError("Expecting minhash with length %d, got %d" % (lsh.h, k // words))
    keys = list(keys)
    if len(keys) != n:
        raise ValueError("keys and signatures must have the same length")
    if getattr(lsh, "_require_bytes_keys", False):
        for key in keys:
            if not isinstance(key, bytes):
                raise TypeError(
                    f"prepickle=False requires bytes keys for non-dict storage, got {type(key).__name__}. "
                    "Either pass bytes keys or use prepickle=True for automatic serialization."
                )
    if lsh.prepickle:
        keys = list(map(pickle.dumps, keys))
    dict_index = _is_dict_index(lsh)
    if check_duplication:
        if dict_index:
            if len(set(keys)) != n or not lsh.keys._dict.keys().isdisjoint(keys):
                raise ValueError("The given key already exists")
        else:
            seen = set()
            for key in keys:
                if key in seen or key in lsh.keys:
                    raise ValueError("The given key already exists")
                seen.add(key)
    columns = band_keys(sig, lsh.b, lsh.r * words, gpu_mode=gpu_mode).T.tolist()  # b lists of N bytes objects
    hashfunc = getattr(lsh, "hashfunc", None)
    if hashfunc is not None:
        columns = [list(map(hashfunc, col)) for col in columns]
    if not dict_index or (not check_duplication and len(set(keys)) != n):
        for i, key in enumerate(keys):
            lsh.keys.insert(key, *[col[i] for col in columns], buffer=False)
        for col, hashtable in zip(columns, lsh.hashtables):
            for h, key in zip(col, keys):
                hashtable.insert(h, key, buffer=False)
        return
    # ---- in-memory storage: whole dictionaries at a time (every iterator below runs in C).  The cyclic garbage
    # collector is held off meanwhile: N*(b+1) new containers, none of them part of a cycle, would otherwise trigger
    # full collections that walk everything built so far (17 s instead of 2.8 s for 200k keys x 25 bands)
    import gc

    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        _fill_dict_index(lsh, keys, columns, n)
    finally:
        if gc_was_on:
            gc.enable()
    if gc_was_on and n >= _SETTLE_MIN_KEYS:
        if settle == "collect":
            gc.collect()
        elif settle == "freeze":
            gc.freeze()


_SETTLE_MIN_KEYS = 20000  # below this the young containers cost a later collection milliseconds


def _fill_dict_index(lsh, keys, columns, n) -> None:
    kd = lsh.keys._dict
    fresh = kd.keys().isdisjoint(keys)
    rows = map(list, zip(*columns))
    if fresh:
        kd.update(zip(keys, rows))  # DictListStorage.insert: _dict[key].extend(Hs) on an absent key
    else:  # re-inserting existing keys without the duplicate check extends their lists, as the reference does
        for key, hs in zip(keys, rows):
            kd[key].extend(hs)
    for col, hashtable in zip(columns, lsh.hashtables):
        d = hashtable._dict
        first = dict(zip(col, keys))  # band key -> LAST row holding it
        if len(first) == n and d.keys().isdisjoint(first):
            d.update(zip(col, map(set, zip(keys))))  # every bucket is new and holds one key
            continue
        # some band keys are shared (near-duplicate rows) or present already: those few go one by one
        counts: dict = {}
        for h in col:
            counts[h] = counts.get(h, 0) + 1
        shared = {h for h, c in counts.items() if c > 1}
        shared.update(d.keys() & counts.keys())
        if shared:
            single_h, single_k = [], []
            for h, key in zip(col, keys):
                if h in shared:
                    d[h].add(key)
                else:
                    single_h.append(h)
                    single_k.append(key)
            d.update(zip(single_h, map(set, zip(single_k))))
        else:
            d.update(zip(col, map(set, zip(keys))))


def query_bulk(lsh, signatures, gpu_mode: str = "detect") -> List[list]:
    """``[lsh.query(MinHash(hashvalues=row)) for row in signatures]`` (ref: datasketch/lsh.py:370-431) with the band
    keys of all probes taken in one pass and, for the in-memory storage, the ``b`` dictionary probes per
    signature done by C-level ``map(dict.get, ...)``.  Returns one list of keys per row (order within a list
    is unspecified, as in the reference)."""
    from datasketch_amd.lsh import MinHashLSH

    if isinstance(lsh, MinHashLSH):
        return lsh.query_bulk(signatures)
    sig, words = _matrix(signatures), _words(signatures)
    n, k = sig.shape
    if k != lsh.h * words:
        raise ValueError("Expecting minhash with length %d, got %d" % (lsh.h, k // words))
    columns = band_keys(sig, lsh.b, lsh.r * words, gpu_mode=gpu_mode).T.tolist()
    hashfunc = getattr(lsh, "hashfunc", None)
    if hashfunc is not None:
        columns = [list(map(hashfunc, col)) for col in columns]
    if _is_dict_index(lsh):
        # (no cyclic garbage is made here, and a full collection would walk the whole index: 32 million sets at 10^6
        # keys -- with the collector left on, 20 000 probes against such an index took 3.9 s)
        import gc

        gc_was_on = gc.isenabled()
        gc.disable()
        try:
            empty = frozenset()
            found = [list(map(ht._dict.get, col, [empty] * n)) for col, ht in zip(columns, lsh.hashtables)]  # b lists of N buckets
            results = [set().union(*buckets) for buckets in zip(*found)] if n else []
            if lsh.prepickle:
                return [[pickle.loads(key) for key in cand] for cand in results]
            return [list(cand) for cand in results]
        finally:
            if gc_was_on:
                gc.enable()
    else:
        results = []
        for i in range(n):
            cand = set()
            for col, hashtable in zip(columns, lsh.hashtables):
                cand.update(hashtable.get(col[i]))
            results.append(cand)
    if lsh.prepickle:
        return [[pickle.loads(key) for key in cand] for cand in results]
    return [list(cand) for cand in results]


class SortedBandsIndex:
    """An LSH index over a signature matrix (grown in batches with :meth:`extend`), resident on the GPU as sorted bands: per band the FNV-1a-64
    digests of the band keys in ascending order with their rows (``mhx_lsh_sort_bands``) -- every bucket of
    the reference's per-band dictionary (ref: datasketch/lsh.py:326-347) is a run of equal digests.

    :meth:`query` answers what ``MinHashLSH.query`` would for a whole matrix of probes: binary search of the
    ``M x b`` probe digests, candidates confirmed by comparing the band's ``r`` hash values themselves (so the
    answer is the reference's even under a 64-bit digest collision), sort + unique across bands.  Rows are
    numbers ``0 .. N-1`` of the indexed matrix; map them to keys with your own array.  uint32 signature
    matrices (the compact / all-gathered form) are taken as they are.  A WeightedMinHash matrix ``[N, S, 2]`` int64 makes a
    weighted index: it is held as ``[N, 2 S]`` words, a band is ``r`` ``(k, t)`` pairs, probes are ``[M, S, 2]`` too, and
    :meth:`nearest` / :meth:`clusters` rank and filter by ``WeightedMinHash.jaccard``."""

    def __init__(self, signatures, b: int, r: int, device: Optional[int] = None):
        sig = np.asarray(signatures)
        self.words = 2 if sig.ndim == 3 and sig.shape[2] == 2 else 1
        if self.words == 2:
            sig = _matrix(sig)
        elif sig.ndim != 2:
            raise ValueError("signatures must be an [N, K] matrix")
        elif sig.dtype != np.uint32:
            sig = np.ascontiguousarray(sig, dtype=np.uint64)
        sig = np.ascontiguousarray(sig)
        _check_params(sig.shape[1], b, r * self.words)
        if not _native.gpu_available():
            raise RuntimeError("SortedBandsIndex needs an MI355X / libmhx.so")
        self.ctx = _native.context(device)
        self.k = sig.shape[1]                              # words per row
        self.b, self.r = int(b), int(r) * self.words       # r: words per band
        self.dtype = sig.dtype
        self._rows = DeviceRows(self.ctx, self.k, sig.dtype)
        self._rows.upload(sig)
        self._sort()

    @property
    def n(self) -> int:
        return self._rows.n

    def _sort(self) -> None:
        self._d_dig = self.ctx.alloc(max(1, self.n * self.b * 8))
        self._d_rows = self.ctx.alloc(max(1, self.n * self.b * 4))
        if self.n:
            self.ctx.lsh_sort_bands_dev(self._rows.d_sig.ptr, self._rows.code, self.n, self.k, self.b, self.r, self._d_dig.ptr,
                                        self._d_rows.ptr)

    def _rows_arg(self, signatures) -> np.ndarray:
        """Probes or further rows as a matrix of the index's words: ``[M, K]``, or ``[M, S, 2]`` for a weighted index."""
        q = np.asarray(signatures)
        if (q.ndim == 3) != (self.words == 2):
            raise ValueError("Cannot compare MinHash and WeightedMinHash signatures: this index holds %s rows"
                             % ("WeightedMinHash [N, S, 2]" if self.words == 2 else "MinHash [N, K]"))
        if self.words == 2:
            if q.shape[2] != 2 or 2 * q.shape[1] != self.k:
                raise ValueError("Expecting minhash with length %d, got %d" % (self.k // 2, q.shape[1]))
            return _matrix(q)
        if q.ndim != 2 or q.shape[1] != self.k:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.k, q.shape[-1]))
        return self._as_index_dtype(q)

    def _as_index_dtype(self, sig: np.ndarray) -> np.ndarray:
        """``sig`` in the index's signature type; a wider matrix must fit (a wrapped value would match band keys the
        reference's byte-keyed dictionaries keep apart)."""
        if sig.dtype.kind not in "ui":
            raise ValueError("signatures are unsigned integers (hashvalues), not %s" % sig.dtype)
        if sig.size and sig.dtype.kind == "i" and int(sig.min()) < 0:
            raise ValueError("negative signature values")
        if self.dtype == np.uint32 and sig.dtype.itemsize > 4 and sig.size and int(sig.max()) > 0xFFFFFFFF:
            raise ValueError("signature values >= 2**32 do not fit this uint32 index")
        return np.ascontiguousarray(sig, dtype=self.dtype)

    def extend(self, signatures) -> range:
        """Add rows (what ``MinHashLSH.insert`` does key by key, ref: datasketch/lsh.py:326-347) and return their row
        numbers ``range(old N, new N)``.  The matrix grows on the device (the rows already there are not uploaded
        again; the first build allocates room for its own rows, 1024 at least, and the capacity at least doubles whenever it runs
        out, so most calls copy nothing) and the bands are sorted afresh -- 40 ms per 10^6 rows, so add in batches."""
        more = self._rows_arg(signatures)
        first, m = self.n, more.shape[0]
        if m == 0:
            return range(first, first)
        self._rows.upload(more)
        self.ctx.synchronize()
        self._sort()
        return range(first, first + m)

    def query(self, signatures, capacity: Optional[int] = None):
        """``(offsets int64[M+1], rows int64[...])``: the index rows sharing at least one band key with probe
        ``i`` are ``rows[offsets[i]:offsets[i+1]]``, ascending."""
        q = self._rows_arg(signatures)
        if q.shape[0] == 0 or self.n == 0:
            return np.zeros(q.shape[0] + 1, dtype=np.int64), np.empty(0, dtype=np.int64)
        return self.ctx.lsh_query_dev(self._d_dig.ptr, self._d_rows.ptr, self.n, self.b, self.r, self._rows.d_sig.ptr, self._rows.code,
                                      self.k, q, capacity)

    def nearest(self, signatures, k: int, threshold: Optional[float] = None):
        """``(rows int64 [M, k], jaccard float64 [M, k])``: the ``k`` indexed rows nearest to every probe by ``MinHash.jaccard``,
        as :func:`nearest_neighbors` -- an exact scan of the resident matrix, only the probes are uploaded.  (A weighted index:
        by ``WeightedMinHash.jaccard``, as :func:`weighted_nearest_neighbors`.)"""
        q = self._rows_arg(signatures)
        k = _check_topk(k)
        rows, counts = rows_nearest(self._rows, q, k, threshold, words=self.words)
        return rows, _jaccard_of(rows, counts, self.k // self.words)

    def clusters(self, threshold: Optional[float] = None) -> np.ndarray:
        """``labels int64 [N]`` as :func:`duplicate_clusters` gives them, over the resident matrix and bands: nothing is
        uploaded, only the labels come down."""
        return rows_clusters(self._rows, self._d_dig.ptr, self._d_rows.ptr, self.b, self.k, threshold, words=self.words)


def sorted_bands(signatures, b: int, r: int, gpu_mode: str = "detect"):
    """``(digests [b, N] uint64 ascending per band, rows [b, N] uint32 in the same order)``: every LSH
    bucket of band ``j`` is a run of equal values in ``digests[j]``.  On the device this is one digest
    pass plus ``b`` radix sorts (mhx_lsh_sort_bands); the numpy fallback is ``argsort`` per band."""
    sig, r = _matrix(signatures), r * _words(signatures)
    n, k = sig.shape
    _check_params(k, b, r)
    if _use_gpu(gpu_mode) and n:
        return _native.context().lsh_sort_bands(sig, b, r)
    dig = band_digests(sig, b, r, gpu_mode="disable").T
    order = np.argsort(dig, axis=1, kind="stable")
    return np.take_along_axis(dig, order, axis=1), order.astype(np.uint32)


def candidate_pairs(signatures, b: int, r: int, gpu_mode: str = "detect") -> np.ndarray:
    """``[M, 2]`` int64, sorted, unique pairs ``i < j`` of rows that share the key of at least one band
    -- the pairs ``MinHashLSH(params=(b, r))`` would report for each other.  On the device: digests,
    per-band sort, run detection, pair emission, sort + unique in one call (mhx_lsh_candidate_pairs)."""
    sig, r = _matrix(signatures), r * _words(signatures)
    _check_params(sig.shape[1], b, r)
    if _use_gpu(gpu_mode) and sig.shape[0]:
        return _native.context().lsh_candidate_pairs(sig, b, r)[0]
    return _pairs_of_bands(*sorted_bands(sig, b, r, gpu_mode=gpu_mode))


def _pairs_of_bands(dig: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """The numpy form of mhx_lsh_candidate_pairs_dev: the unique pairs ``i < j`` of rows inside one run of equal digests."""
    b, n = dig.shape
    found: List[np.ndarray] = []
    for j in range(b):
        s, order = dig[j], rows[j].astype(np.int64)
        starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]])) if n else np.empty(0, np.int64)
        ends = np.concatenate([starts[1:], [n]]) if n else starts
        size = ends - starts
        two = starts[size == 2]  # the common bucket: exactly two rows
        if two.size:
            pair = np.stack([order[two], order[two + 1]], axis=1)
            found.append(np.sort(pair, axis=1))
        for a, e in zip(starts[size > 2], ends[size > 2]):
            members = np.sort(order[a:e])
            ii, jj = np.triu_indices(members.size, k=1)
            found.append(np.stack([members[ii], members[jj]], axis=1))
    if not found:
        return np.empty((0, 2), dtype=np.int64)
    return np.unique(np.concatenate(found).astype(np.int64), axis=0)


def jaccard_pairs(signatures, pairs, gpu_mode: str = "detect") -> np.ndarray:
    """``MinHash.jaccard`` of rows ``pairs[:, 0]`` and ``pairs[:, 1]``: float64, equal positions / K.
    (For a WeightedMinHash matrix use :func:`weighted_jaccard_pairs`: a position is a ``(k, t)`` pair.)"""
    if np.ndim(signatures) == 3:
        raise ValueError("jaccard_pairs takes an [N, K] matrix; use weighted_jaccard_pairs for [N, S, 2]")
    sig = _matrix(signatures)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= sig.shape[0]):
        raise ValueError("pair index out of range")
    if _use_gpu(gpu_mode):
        counts = _native.context().jaccard_pairs(sig, pairs)
    else:
        counts = np.count_nonzero(sig[pairs[:, 0]] == sig[pairs[:, 1]], axis=1)
    return counts.astype(np.float64) / float(sig.shape[1])


def weighted_jaccard_pairs(signatures, pairs, gpu_mode: str = "detect") -> np.ndarray:
    """``WeightedMinHash.jaccard`` (ref: weighted_minhash.py:41-60) of rows ``pairs[:, 0]`` and ``pairs[:, 1]`` of an
    ``[N, S, 2]`` matrix: the fraction of samples whose ``(k, t)`` pairs are equal (on the device: mhx_weighted_jaccard_pairs)."""
    _check_gpu_mode(gpu_mode)
    sig = np.asarray(signatures, dtype=np.int64)
    if sig.ndim != 3 or sig.shape[2] != 2:
        raise ValueError("signatures must be [N, S, 2]")
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= sig.shape[0]):
        raise ValueError("pair index out of range")
    if _use_gpu(gpu_mode) and pairs.size and sig.shape[1]:
        counts = _native.context().weighted_jaccard_pairs(sig, pairs)
    else:
        counts = _equal_samples(sig[pairs[:, 0]], sig[pairs[:, 1]])
    return counts.astype(np.float64) / float(sig.shape[1])


# ---- WeightedMinHash.jaccard of every pair: the weighted twins of jaccard_matrix, similar_pairs, nearest_neighbors and
# duplicate_clusters.  One definition throughout: count(x, y) = the samples s with x[s, 0] == y[s, 0] and x[s, 1] == y[s, 1], the
# estimate float(count) / float(S) (ref: weighted_minhash.py:45-60).  The numpy forms below are that definition.
def _equal_samples(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """Samples at which rows ``x[..., S, 2]`` and ``y[..., S, 2]`` (broadcast against each other) hold the same ``(k, t)``."""
    return np.count_nonzero(np.all(x == y, axis=-1), axis=-1)


def _weighted_rows(x, name: str):
    """(int64 [N, S, 2] matrix, seed or None) of a WeightedMinHash matrix or a sequence of WeightedMinHash objects."""
    if isinstance(x, np.ndarray) or (not hasattr(x, "__len__") or not len(x) or not hasattr(x[0], "hashvalues")):
        sig = np.asarray(x)
    else:
        seed, s = x[0].seed, len(x[0])
        for m in x:
            if m.seed != seed:
                raise ValueError("Cannot compute Jaccard given WeightedMinHash objects with different seeds")
            if len(m) != s:
                raise ValueError("Cannot compute Jaccard given WeightedMinHash objects with different numbers of hash values")
        sig = np.stack([np.asarray(m.hashvalues) for m in x])
        if sig.ndim == 3 and sig.shape[2] == 2:
            return np.ascontiguousarray(sig, dtype=np.int64), seed
    if sig.ndim != 3 or sig.shape[2] != 2:
        raise ValueError("%s must be an [N, S, 2] WeightedMinHash matrix or a sequence of WeightedMinHash, not MinHash [N, K] rows" % name)
    return np.ascontiguousarray(sig, dtype=np.int64), None


def _weighted_inputs(a, b):
    sa, seed_a = _weighted_rows(a, "a")
    if b is None:
        return sa, None
    sb, seed_b = _weighted_rows(b, "b")
    if seed_a is not None and seed_b is not None and seed_a != seed_b:
        raise ValueError("Cannot compute Jaccard given WeightedMinHash objects with different seeds")
    if sa.shape[1] != sb.shape[1]:
        raise ValueError("Cannot compute Jaccard given WeightedMinHash objects with different numbers of hash values")
    return sa, sb


def _equal_samples_blocks(va: np.ndarray, vb: Optional[np.ndarray]):
    """The weighted :func:`_equal_counts_blocks`: yields (first row, int64 [rows, n_b]) over ``[n, S, 2]`` matrices."""
    other = va if vb is None else vb
    n_b, s = other.shape[:2]
    step = max(1, _FALLBACK_ELEMS // max(1, 2 * n_b * s))
    for i0 in range(0, va.shape[0], step):
        yield i0, _equal_samples(va[i0 : i0 + step, None], other[None])


def weighted_jaccard_matrix(a, b=None, gpu_mode: str = "detect") -> np.ndarray:
    """``WeightedMinHash.jaccard`` of every row of ``a`` against every row of ``b``: float64 ``[M, N]``, equal samples / S.
    ``a`` / ``b``: ``[N, S, 2]`` int64 matrices (``WeightedMinHashGenerator.minhash_many_arrays``) or sequences of
    WeightedMinHash (seeds and lengths must agree, as ``WeightedMinHash.jaccard`` requires).  ``b=None``: ``a`` against itself."""
    _check_gpu_mode(gpu_mode)
    sa, sb = _weighted_inputs(a, b)
    s = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    if sa.shape[0] == 0 or n_b == 0 or s == 0:
        return np.zeros((sa.shape[0], n_b), dtype=np.float64)
    if _use_gpu(gpu_mode):
        counts = _native.context().weighted_jaccard_matrix(sa, sb)
    else:
        counts = _matrix_from_blocks(_equal_samples_blocks(sa, sb), sa.shape[0], n_b)
    return counts.astype(np.float64) / float(s)


def weighted_similar_pairs(a, b=None, threshold: float = 0.5, gpu_mode: str = "detect"):
    """Every pair whose ``WeightedMinHash.jaccard`` is ``>= threshold``: ``(pairs int64 [P, 2], jaccard float64 [P])`` as
    :func:`similar_pairs` gives them -- ascending by ``(i, j)``, with ``b=None`` the pairs ``i < j`` of ``a``; the threshold
    becomes the smallest count ``c`` with ``float(c) / float(S) >= threshold``."""
    _check_gpu_mode(gpu_mode)
    sa, sb = _weighted_inputs(a, b)
    s = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    if sa.shape[0] == 0 or n_b == 0 or s == 0:
        return np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float64)
    c = _threshold_count(s, threshold)
    if c > s:
        return np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float64)
    if _use_gpu(gpu_mode):
        pairs, counts = _native.context().weighted_jaccard_threshold_pairs(sa, sb, c)
    else:
        pairs, counts = _pairs_from_blocks(_equal_samples_blocks(sa, sb), c, sb is None)
    return pairs, counts.astype(np.float64) / float(s)


def weighted_nearest_neighbors(a, b=None, k: int = 10, threshold: Optional[float] = None, gpu_mode: str = "detect"):
    """The ``k`` nearest rows of ``b`` for every row of ``a`` by ``WeightedMinHash.jaccard``: ``(rows int64 [M, k], jaccard
    float64 [M, k])`` as :func:`nearest_neighbors` gives them -- best first, ties by the smaller row, padded with ``-1`` /
    ``nan``; ``b=None``: the rows of ``a`` among themselves, never a row itself; ``1 <= k <= 64``."""
    _check_gpu_mode(gpu_mode)
    sa, sb = _weighted_inputs(a, b)
    k = _check_topk(k)
    s = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    c = 0 if threshold is None else _threshold_count(max(s, 1), threshold)
    if sa.shape[0] == 0 or n_b == 0 or s == 0 or c > s:
        rows = counts = np.full((sa.shape[0], k), -1, dtype=np.int64)
    elif _use_gpu(gpu_mode):
        rows, counts = _native.context().weighted_jaccard_topk(sa, sb, k, c)
    else:
        rows, counts = _topk_from_blocks(_equal_samples_blocks(sa, sb), sa.shape[0], k, c, sb is None)
    return rows, _jaccard_of(rows, counts, max(s, 1))


def weighted_duplicate_clusters(signatures, b: int, r: int, threshold: Optional[float], gpu_mode: str = "detect") -> np.ndarray:
    """:func:`duplicate_clusters` of a WeightedMinHash matrix ``[N, S, 2]`` (or a sequence of WeightedMinHash) with a
    ``threshold``: ``labels int64 [N]`` of ``connected_components(pairs[weighted_jaccard_pairs(signatures, pairs) >= threshold],
    N)`` with ``pairs = candidate_pairs(signatures, b, r)``.  On the device the candidate pairs, their counts
    (mhx_weighted_jaccard_pairs_dev) and the union-find stay there and only the labels come down.  ``threshold=None``: the
    components of the candidate graph, as :func:`duplicate_clusters` gives them."""
    _check_gpu_mode(gpu_mode)
    sig, _ = _weighted_rows(signatures, "signatures")
    mat = _matrix(sig)
    n, k = mat.shape
    _check_params(k, b, 2 * r)
    if n == 0:
        return np.empty(0, dtype=np.int64)
    if not _use_gpu(gpu_mode):
        dig, rows = sorted_bands(mat, b, 2 * r, gpu_mode="disable")
        return bands_clusters_host(mat, dig, rows, threshold, words=2)
    ctx = _native.context()
    store = DeviceRows(ctx, k, mat.dtype)
    store.upload(mat)
    d_dig, d_rows = ctx.alloc(n * b * 8), ctx.alloc(n * b * 4)
    ctx.lsh_sort_bands_dev(store.d_sig.ptr, store.code, n, k, b, 2 * r, d_dig.ptr, d_rows.ptr)
    return rows_clusters(store, d_dig.ptr, d_rows.ptr, b, k, threshold, words=2)


# rows of A per numpy block of the all-pairs fallback: about 2^24 compared elements at a time
_FALLBACK_ELEMS = 1 << 24


def _hashvalue_rows(x, name: str):
    """(uint64 [N, K] matrix, seed or None) of a signature matrix or a sequence of MinHash / LeanMinHash objects."""
    if isinstance(x, np.ndarray) or (not hasattr(x, "__len__") or not len(x) or not hasattr(x[0], "hashvalues")):
        sig = np.asarray(x)
        if sig.ndim == 3:
            raise ValueError("%s: all-pairs Jaccard takes [N, K] matrices, not WeightedMinHash [N, S, 2] ones" % name)
        if sig.ndim != 2:
            raise ValueError("%s must be an [N, K] matrix or a sequence of MinHash" % name)
        return np.ascontiguousarray(sig, dtype=np.uint64), None
    seed, k = x[0].seed, len(x[0].hashvalues)
    for m in x:
        if m.seed != seed:
            raise ValueError("Cannot compute Jaccard given MinHash with different seeds")
        if len(m.hashvalues) != k:
            raise ValueError("Cannot compute Jaccard given MinHash with different numbers of permutation functions")
    return np.ascontiguousarray(np.stack([np.asarray(m.hashvalues) for m in x]), dtype=np.uint64), seed


def _all_pairs_inputs(a, b):
    sa, seed_a = _hashvalue_rows(a, "a")
    if b is None:
        return sa, None
    sb, seed_b = _hashvalue_rows(b, "b")
    if seed_a is not None and seed_b is not None and seed_a != seed_b:
        raise ValueError("Cannot compute Jaccard given MinHash with different seeds")
    if sa.shape[1] != sb.shape[1]:
        raise ValueError("Cannot compute Jaccard given MinHash with different numbers of permutation functions")
    return sa, sb


def _equal_counts_blocks(va: np.ndarray, vb: Optional[np.ndarray]):
    """numpy all-pairs equal-position counts, block of A rows by block: yields (first row, int64 [rows, n_b])."""
    other = va if vb is None else vb
    n_b, k = other.shape
    step = max(1, _FALLBACK_ELEMS // max(1, n_b * k))
    for i0 in range(0, va.shape[0], step):
        yield i0, np.count_nonzero(va[i0 : i0 + step, None, :] == other[None, :, :], axis=2)


def _matrix_from_blocks(blocks, n_a: int, n_b: int) -> np.ndarray:
    out = np.empty((n_a, n_b), dtype=np.int64)
    for i0, c in blocks:
        out[i0 : i0 + c.shape[0]] = c
    return out


def _pairs_from_blocks(blocks, min_count: int, self_join: bool):
    found, counts = [], []
    for i0, c in blocks:
        keep = c >= min_count
        if self_join:
            keep &= np.arange(c.shape[1])[None, :] > (i0 + np.arange(c.shape[0]))[:, None]
        ij = np.argwhere(keep)
        counts.append(c[ij[:, 0], ij[:, 1]])
        ij[:, 0] += i0
        found.append(ij)
    if not found:
        return np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.int64)
    return np.concatenate(found).astype(np.int64), np.concatenate(counts)


def _min_count(estimates: np.ndarray, threshold: float) -> int:
    """The smallest count whose estimate (estimates[c], c = 0..K, monotone in c) is >= threshold; K + 1 when none is."""
    hit = np.flatnonzero(estimates >= threshold)
    return int(hit[0]) if hit.size else len(estimates)


def jaccard_matrix(a, b=None, gpu_mode: str = "detect") -> np.ndarray:
    """``MinHash.jaccard`` (ref: datasketch/minhash.py:299-324) of every row of ``a`` against every row of ``b``: float64
    ``[M, N]``, equal positions / K.  ``a`` / ``b``: ``[N, K]`` uint32 or uint64 signature matrices or sequences of MinHash /
    LeanMinHash (seeds and ``num_perm`` must agree, as the reference requires).  ``b=None``: ``a`` against itself."""
    sa, sb = _all_pairs_inputs(a, b)
    k = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    if sa.shape[0] == 0 or n_b == 0 or k == 0:
        return np.zeros((sa.shape[0], n_b), dtype=np.float64)
    if _use_gpu(gpu_mode):
        counts = _native.context().jaccard_matrix(sa, sb)
    else:
        counts = _matrix_from_blocks(_equal_counts_blocks(sa, sb), sa.shape[0], n_b)
    return counts.astype(np.float64) / float(k)


def similar_pairs(a, b=None, threshold: float = 0.5, gpu_mode: str = "detect"):
    """Every pair whose ``MinHash.jaccard`` is ``>= threshold``: ``(pairs int64 [P, 2], jaccard float64 [P])``, ascending by
    ``(i, j)`` -- row ``i`` of ``a``, row ``j`` of ``b``; with ``b=None`` the pairs ``i < j`` of ``a``.  Exhaustive: every
    pair is compared (on the device, all-pairs tiles; no LSH banding, so no false negatives).  The threshold becomes the
    smallest count ``c`` with ``float(c) / float(K) >= threshold``, the reference's own float comparison."""
    sa, sb = _all_pairs_inputs(a, b)
    k = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    if sa.shape[0] == 0 or n_b == 0 or k == 0:
        return np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float64)
    c = _min_count(np.arange(k + 1, dtype=np.float64) / float(k), float(threshold))
    if c > k:
        return np.empty((0, 2), dtype=np.int64), np.empty(0, dtype=np.float64)
    if _use_gpu(gpu_mode):
        pairs, counts = _native.context().jaccard_threshold_pairs(sa, sb, c)
    else:
        pairs, counts = _pairs_from_blocks(_equal_counts_blocks(sa, sb), c, sb is None)
    return pairs, counts.astype(np.float64) / float(k)


def _check_topk(k) -> int:
    k = int(k)
    if k < 1 or k > _native.MHX_TOPK_MAX:
        raise ValueError("k must be in [1, %d]" % _native.MHX_TOPK_MAX)
    return k


def _topk_from_blocks(blocks, n_a: int, k: int, min_count: int, self_join: bool, live: Optional[np.ndarray] = None):
    """numpy top-k of all-pairs counts, block of A rows by block: ``(rows int64 [n_a, k], counts int64 [n_a, k])``, the best
    ``k`` columns of every row by (count descending, column ascending) -- the sort of the keys ``count << 32 | 0xFFFFFFFF - j``
    the device kernels keep -- padded with -1.  ``live``: bool per column, dead columns are no candidates."""
    rows = np.full((n_a, k), -1, dtype=np.int64)
    counts = np.full((n_a, k), -1, dtype=np.int64)
    low = np.uint64(0xFFFFFFFF)
    for i0, c in blocks:
        m, n_b = c.shape
        key = (c.astype(np.uint64) << np.uint64(32)) | (low - np.arange(n_b, dtype=np.uint64))[None, :]
        ok = c >= min_count
        if live is not None:
            ok &= live[None, :]
        if self_join:
            ok[np.arange(m), i0 + np.arange(m)] = False
        key[~ok] = 0
        kk = min(k, n_b)
        if kk < n_b:
            key = np.partition(key, n_b - kk, axis=1)[:, n_b - kk :]
        top = np.sort(key, axis=1)[:, ::-1]
        have = top != 0
        rows[i0 : i0 + m, :kk] = np.where(have, (low - (top & low)).astype(np.int64), -1)
        counts[i0 : i0 + m, :kk] = np.where(have, (top >> np.uint64(32)).astype(np.int64), -1)
    return rows, counts


def _jaccard_of(rows: np.ndarray, counts: np.ndarray, k: int) -> np.ndarray:
    return np.where(rows >= 0, counts.astype(np.float64) / float(k), np.nan)


def _topk_matrix(sa: np.ndarray, sb: Optional[np.ndarray], k: int, threshold, use_gpu: bool, live: Optional[np.ndarray] = None):
    """(rows, counts) of the best ``k`` rows of ``sb`` (``None``: ``sa`` itself, never a row itself) per row of ``sa``."""
    num_perm = sa.shape[1]
    n_b = sa.shape[0] if sb is None else sb.shape[0]
    c = 0 if threshold is None else _min_count(np.arange(num_perm + 1, dtype=np.float64) / float(max(num_perm, 1)), float(threshold))
    if sa.shape[0] == 0 or n_b == 0 or num_perm == 0 or c > num_perm:
        return np.full((sa.shape[0], k), -1, dtype=np.int64), np.full((sa.shape[0], k), -1, dtype=np.int64)
    if use_gpu and live is None:
        return _native.context().jaccard_topk(sa, sb, k, c)
    return _topk_from_blocks(_equal_counts_blocks(sa, sb), sa.shape[0], k, c, sb is None, live)


def nearest_neighbors(a, b=None, k: int = 10, threshold: Optional[float] = None, gpu_mode: str = "detect"):
    """The ``k`` nearest rows of ``b`` for every row of ``a`` by ``MinHash.jaccard`` (ref: datasketch/minhash.py:299-324):
    ``(rows int64 [M, k], jaccard float64 [M, k])``, best first, ties by the smaller row; a row with fewer than ``k``
    candidates is padded with ``-1`` / ``nan``.  Exact: every pair is compared (on the device without forming the ``M x N``
    matrix), which is this package's answer to the reference's HNSW use case.  ``b=None``: the rows of ``a`` among themselves,
    a row is never its own neighbour.  ``threshold``: only rows whose Jaccard is ``>= threshold`` (as :func:`similar_pairs`
    takes it).  Inputs as :func:`jaccard_matrix`; ``1 <= k <= 64``."""
    sa, sb = _all_pairs_inputs(a, b)
    k = _check_topk(k)
    rows, counts = _topk_matrix(sa, sb, k, threshold, _use_gpu(gpu_mode))
    return rows, _jaccard_of(rows, counts, sa.shape[1])


def live_bits(live: np.ndarray) -> np.ndarray:
    """The live-bit map the device entry points take: bit ``row & 31`` of uint32 word ``row >> 5``, ``ceil(n / 32)`` words."""
    words = np.zeros((live.size + 31) // 32 * 4, dtype=np.uint8)
    packed = np.packbits(live, bitorder="little")
    words[: packed.size] = packed
    return words.view(np.uint32)


def rows_nearest(store, probes: np.ndarray, k: int, threshold, live: Optional[np.ndarray] = None, words: int = 1):
    """(rows, counts) of the ``k`` best rows of an index's signature matrix (``DeviceRows`` / ``HostRows``) per probe (of the
    store's dtype); ``live``: bool per row, dead rows are no candidates.  ``words=2``: the rows are WeightedMinHash signatures as
    :func:`_matrix` views them, ``[n, 2 S]`` words, and a position is a ``(k, t)`` sample."""
    m, num_perm, n = probes.shape[0], store.kw // words, store.n
    c = 0 if threshold is None else _min_count(np.arange(num_perm + 1, dtype=np.float64) / float(num_perm), float(threshold))
    if isinstance(store, HostRows):
        if m == 0 or n == 0 or c > num_perm:
            return np.full((m, k), -1, dtype=np.int64), np.full((m, k), -1, dtype=np.int64)
        if words == 2:
            blocks = _equal_samples_blocks(probes.reshape(m, num_perm, 2), store.sig.reshape(n, num_perm, 2))
        else:
            blocks = _equal_counts_blocks(probes, store.sig)
        return _topk_from_blocks(blocks, m, k, c, False, live)
    if m == 0:
        return np.empty((0, k), dtype=np.int64), np.empty((0, k), dtype=np.int64)
    ctx = store.ctx
    d_q = ctx.to_device(probes)
    d_bits = None if live is None or n == 0 else ctx.to_device(live_bits(live))
    d_rows, d_counts = ctx.alloc(8 * m * k), ctx.alloc(4 * m * k)
    if words == 2:
        ctx.weighted_jaccard_topk_dev(d_q.ptr, m, store.d_sig.ptr if n else d_q.ptr, n, num_perm, None if d_bits is None else d_bits.ptr,
                                      c, k, d_rows.ptr, d_counts.ptr)
    else:
        ctx.jaccard_topk_dev(d_q.ptr, m, store.d_sig.ptr if n else d_q.ptr, n, store.code, num_perm, None if d_bits is None else d_bits.ptr,
                             c, k, d_rows.ptr, d_counts.ptr)
    return d_rows.download((m, k), np.int64), d_counts.download((m, k), np.int32).astype(np.int64)


# ---- near-duplicate clusters: the connected components of a pair graph ------------------------------------------------------
def _components_host(u: np.ndarray, v: np.ndarray, n: int) -> np.ndarray:
    """int64 [n]: the smallest row of every row's component under the edges ``(u[i], v[i])`` (all inside ``[0, n)``)."""
    if n == 0:
        return np.empty(0, dtype=np.int64)
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components as graph_components

    graph = coo_matrix((np.ones(u.size, dtype=np.bool_), (u, v)), shape=(n, n))
    count, comp = graph_components(graph, directed=False)
    smallest = np.full(count, n, dtype=np.int64)
    np.minimum.at(smallest, comp, np.arange(n, dtype=np.int64))
    return smallest[comp]


def _run_edges(dig: np.ndarray, rows: np.ndarray):
    """Every row of sorted bands with its predecessor where their digests are equal: what mhx_cc_link_bands_dev links."""
    same = dig[:, 1:] == dig[:, :-1]
    return rows[:, :-1][same].astype(np.int64), rows[:, 1:][same].astype(np.int64)


def _check_rows(n) -> int:
    n = int(n)
    if n < 0 or n >> 32:
        raise ValueError("n must be in [0, 2^32 - 1]")
    return n


def connected_components(pairs, n: int, keep=None, gpu_mode: str = "detect") -> np.ndarray:
    """``labels int64 [n]``: ``labels[i]`` is the smallest row of the connected component of row ``i`` in the graph whose edges
    are ``pairs`` (``[M, 2]``, any order; duplicates, ``i > j`` and ``i == j`` are fine) -- the near-duplicate clusters of the
    pairs :func:`candidate_pairs`, :func:`similar_pairs` or a thresholded :func:`jaccard_pairs` report.  ``keep``: optional bool
    mask ``[M]``, only those pairs are edges.  ``labels == np.arange(n)`` marks the one row to keep per cluster;
    ``np.unique(labels, return_inverse=True)`` gives dense cluster ids.  An edge with an end outside ``[0, n)`` raises
    ``ValueError``.  On the device: a lock-free union-find (mhx_cc_pairs); on the host scipy's ``connected_components``."""
    _check_gpu_mode(gpu_mode)
    n = _check_rows(n)
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    if keep is not None:
        keep = np.ascontiguousarray(keep, dtype=np.bool_)
        if keep.shape != (pairs.shape[0],):
            raise ValueError("keep must have one entry per pair")
    if _use_gpu(gpu_mode):
        labels, invalid = _native.context().cc_pairs(pairs, n, None if keep is None else keep.astype(np.int32), 1)
        if invalid:
            raise ValueError("%d pairs have an index out of range [0, %d)" % (invalid, n))
        return labels.astype(np.int64)
    if keep is not None:
        pairs = pairs[keep]
    if pairs.size and (pairs.min() < 0 or pairs.max() >= n):
        raise ValueError("%d pairs have an index out of range [0, %d)" % (int(np.count_nonzero(((pairs < 0) | (pairs >= n)).any(axis=1))), n))
    return _components_host(pairs[:, 0], pairs[:, 1], n)


def _threshold_count(num_perm: int, threshold: float) -> int:
    """The smallest count ``c`` with ``float(c) / float(num_perm) >= threshold`` (:func:`jaccard_pairs`' own quotient)."""
    return _min_count(np.arange(num_perm + 1, dtype=np.float64) / float(num_perm), float(threshold))


def bands_clusters_host(sig: np.ndarray, dig: np.ndarray, rows: np.ndarray, threshold, extra=None, words: int = 1) -> np.ndarray:
    """The numpy twin of :func:`rows_clusters`: ``sig`` the ``[n, K]`` matrix, ``dig`` / ``rows`` its sorted bands."""
    n = sig.shape[0]
    if threshold is None:
        u, v = _run_edges(dig, rows)
    else:
        pairs = _pairs_of_bands(dig, rows)
        if words == 2:
            samples = sig.reshape(n, -1, 2)
            counts = _equal_samples(samples[pairs[:, 0]], samples[pairs[:, 1]])
        else:
            counts = np.count_nonzero(sig[pairs[:, 0]] == sig[pairs[:, 1]], axis=1)
        pairs = pairs[counts >= _threshold_count(sig.shape[1] // words, threshold)]
        u, v = pairs[:, 0], pairs[:, 1]
    if extra is not None and len(extra):
        extra = np.asarray(extra, dtype=np.int64).reshape(-1, 2)
        u, v = np.concatenate([u, extra[:, 0]]), np.concatenate([v, extra[:, 1]])
    return _components_host(u, v, n)


def rows_clusters(store, d_dig: int, d_rows: int, b: int, num_perm: int, threshold, extra=None, words: int = 1) -> np.ndarray:
    """``labels int64 [n]`` of a resident signature matrix (``DeviceRows``) and its resident sorted bands.  ``threshold=None``:
    init, link bands, finish -- no pair is formed.  Else: candidate pairs on the device, their counts, link pairs with the
    threshold's count, finish.  ``extra``: further edges ``[E, 2]`` from the host, linked by one more call.  Only the labels
    come down.  ``words=2``: weighted rows of ``num_perm`` words, ``num_perm / 2`` samples, counted sample by sample."""
    ctx, n = store.ctx, store.n
    if n == 0:
        return np.empty(0, dtype=np.int64)
    d_labels = ctx.alloc(4 * n)
    d_bad = ctx.to_device(np.zeros(1, dtype=np.int64))
    ctx.cc_init_dev(d_labels.ptr, n)
    if threshold is None:
        ctx.cc_link_bands_dev(d_labels.ptr, n, d_dig, d_rows, n, b, d_bad.ptr)
    else:
        d_pairs, found = ctx.lsh_candidate_pairs_dev(d_dig, d_rows, n, b)
        if found:
            d_counts = ctx.alloc(4 * found)
            if words == 2:
                ctx.weighted_jaccard_pairs_dev(store.d_sig.ptr, store.d_sig.ptr, num_perm // 2, d_pairs.ptr, found, d_counts.ptr)
            else:
                ctx.jaccard_pairs_dev(store.d_sig.ptr, store.d_sig.ptr, store.code, num_perm, d_pairs.ptr, found, d_counts.ptr)
            ctx.cc_link_pairs_dev(d_labels.ptr, n, d_pairs.ptr, found, d_counts.ptr, _threshold_count(num_perm // words, threshold), d_bad.ptr)
    if extra is not None and len(extra):
        extra = np.ascontiguousarray(extra, dtype=np.int64).reshape(-1, 2)
        d_extra = ctx.to_device(extra)
        ctx.cc_link_pairs_dev(d_labels.ptr, n, d_extra.ptr, extra.shape[0], None, 0, d_bad.ptr)
    ctx.cc_finish_dev(d_labels.ptr, n)
    labels = d_labels.download((n,), np.uint32)  # (blocking: everything enqueued above is done)
    invalid = int(d_bad.download((1,), np.int64)[0])
    if invalid:
        raise _native.MhxError("%d edges name rows outside [0, %d): the bands do not belong to this matrix" % (invalid, n))
    return labels.astype(np.int64)


def duplicate_clusters(signatures, b: int, r: int, threshold: Optional[float] = None, gpu_mode: str = "detect") -> np.ndarray:
    """Near-duplicate clusters of a signature matrix: ``labels int64 [N]``, ``labels[i]`` the smallest row of the cluster of row
    ``i``.  ``labels == np.arange(N)`` marks the one row to keep per cluster; ``np.unique(labels, return_inverse=True)`` gives
    dense cluster ids.

    ``threshold=None``: the connected components of the candidate graph, ``connected_components(candidate_pairs(signatures, b,
    r), N)`` -- rows are one cluster when a chain of shared band keys joins them.  On the device no pair is ever formed: inside
    a band's sorted run of equal digests every row is linked to its predecessor, ``b * N`` implicit edges at most, so a bucket
    of 10^5 identical rows costs 10^5 links and not 5 * 10^9 pairs.  WeightedMinHash matrices ``[N, S, 2]`` are taken too.

    With a ``threshold`` only the candidate pairs whose ``MinHash.jaccard`` estimate reaches it are edges:
    ``connected_components(pairs[jaccard_pairs(signatures, pairs) >= threshold], N)`` with ``pairs = candidate_pairs(...)``;
    on the device the pairs and their counts stay there and only the labels come down.  (WeightedMinHash matrices: ``ValueError``.)"""
    _check_gpu_mode(gpu_mode)
    if threshold is not None and np.ndim(signatures) == 3:
        raise ValueError("a threshold is defined for MinHash signatures, not WeightedMinHash ones")
    mat, words = _words_matrix(signatures)
    n, k = mat.shape
    _check_params(k, b, r * words)
    if n == 0:
        return np.empty(0, dtype=np.int64)
    if not _use_gpu(gpu_mode):
        dig, rows = sorted_bands(mat, b, r * words, gpu_mode="disable")
        return bands_clusters_host(mat, dig, rows, threshold)
    ctx = _native.context()
    store = DeviceRows(ctx, k, mat.dtype)
    store.upload(mat)
    d_dig, d_rows = ctx.alloc(n * b * 8), ctx.alloc(n * b * 4)
    ctx.lsh_sort_bands_dev(store.d_sig.ptr, store.code, n, k, b, r * words, d_dig.ptr, d_rows.ptr)
    return rows_clusters(store, d_dig.ptr, d_rows.ptr, b, k, threshold)
