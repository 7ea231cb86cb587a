"""MinHashLSHBloom with the reference's API (ekzhu/datasketch ``datasketch.lsh_bloom``) over device-resident Bloom filters.

Mirror of datasketch/lsh_bloom.py:55-377: ``MinHashLSHBloom`` has the reference's constructor checks, messages, warnings and
attributes (``h``, ``b``, ``r``, ``hashranges``, ``hashtables``), ``insert``, ``query -> bool`` and ``sync``; ``BloomTable`` has
``insert``, ``query``, ``sync`` and ``assert_size``.  A band's key is the reference's (ref :105, :117): the sum of the band's
``r`` hash values, taken in uint64, modulo ``2**61 - 1``.

The filter itself is this project's own -- the reference hands the key to ``pybloomfilter``, and **the files that library writes
are not readable here** (nor ours there).  Every band has one cache-line-blocked Bloom filter: ``n_blocks`` blocks of 512 bits
(16 little-endian uint32 words), all ``k`` bits of a key in one block chosen by the first output of a splitmix64 stream seeded
with the key, the bit positions taken nine bits at a time from the following outputs (include/mhx.h has the exact recipe).
The whole index is one array ``uint32 [b, n_blocks, 16]``; ``(k, n_blocks)`` come from the user's ``(n, fp)`` by
:func:`bloom_size`, which evaluates the false-positive rate of a *blocked* filter (:func:`fp_blocked`), not the classic formula.

Beyond the reference, under the names ``MinHashLSH`` uses here: ``insert_bulk``, ``query_bulk``, ``query_insert_bulk`` (the
streaming near-duplicate step: answers against the index as it was before the call, then every row inserted), ``merge`` and
``flush``.  Single ``insert`` calls are staged and flushed when ``buffer_size`` rows are pending and before any query, sync,
merge or pickle.

``gpu_mode`` is the seam of ``MinHash``: ``'always'`` keeps the filter on an MI355X, ``'disable'`` in numpy, ``'detect'``
starts in numpy and moves the filter to the device (for good) with the first bulk call of at least ``DETECT_DEVICE_KEYS``
(row, band) keys when there is a device.  Both back ends produce identical filter words: OR does not depend on the order.

Persistence: ``save_dir/band-{i}.bf`` holds a 32-byte header (magic, version, ``k``, ``n_blocks``, ``band_size``) and the band's
words; ``sync()`` writes them, a constructor that finds them loads them and raises ``ValueError`` when their geometry is not
the one its arguments ask for.  Pickling carries the words.
"""
from __future__ import annotations

import logging
import math
import os
import struct
import warnings
from typing import Optional, Tuple

import numpy as np
from scipy.special import gammaln

from datasketch_amd import _native, lsh_bulk
from datasketch_amd.lsh import _optimal_param

__all__ = ["MinHashLSHBloom", "BloomTable", "bloom_size", "fp_blocked"]

logger = logging.getLogger(__name__)

_mersenne_prime = np.uint64((1 << 61) - 1)
_GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BLOCK_BITS = 512
BLOCK_WORDS = 16
MAX_K = 32
MAX_BLOCKS = (1 << 32) - 1
# 'detect': a bulk call with at least this many (row, band) keys moves the filter to the device.  Measured (both curves:
# DESIGN.md section 5, "The Bloom index"): the device path wins from the smallest batch on once the filter is there; the
# threshold is where one batch also pays for the filter's upload (between 2 304 and 9 216 keys for a 25 MB filter)
DETECT_DEVICE_KEYS = 1 << 12
_MAGIC = b"MHXBLOOM"
_VERSION = 1
_HEADER = struct.Struct("<8sIIQI4x")  # magic, version, k, n_blocks, band_size -> 32 bytes
# rows per device call / per pass of the twin (bounds the staging buffers and the temporaries)
_CHUNK_KEYS = 1 << 22


# ---------------------------------------------------------------------------------------------------------- sizing
def fp_blocked(n: int, n_blocks: int, k: int) -> float:
    """The false-positive rate of a blocked filter of ``n_blocks`` 512-bit blocks after ``n`` inserts of ``k`` bits each: a
    block receives Poisson(n / n_blocks) keys, and a block that holds ``j`` keys answers a fresh key with
    ``(1 - (1 - 1/512)**(j * k))**k``.  The sum runs to mean + 12 sqrt(mean) + 30 terms (and, for a mean in the thousands, from as
    far below it): what lies outside is below 1e-30."""
    lam = n / n_blocks
    spread = 12.0 * math.sqrt(lam) + 30.0
    j = np.arange(max(0, int(lam - spread)), int(lam + spread) + 1, dtype=np.float64)
    p = np.exp(j * math.log(lam) - lam - gammaln(j + 1.0))
    return float((p * (1.0 - (1.0 - 1.0 / BLOCK_BITS) ** (j * k)) ** k).sum())


def bloom_size(n: int, fp: float) -> Tuple[int, int]:
    """``(k, n_blocks)``: for every ``k`` in 1..32 the smallest ``n_blocks`` with ``fp_blocked(n, n_blocks, k) <= fp`` (the rate
    falls as blocks are added), of those the pair with the fewest blocks, the smaller ``k`` on a tie."""
    n = int(n)
    best = None
    for k in range(1, MAX_K + 1):
        lo, hi = 1, max(1, n >> 12)  # 4096 keys per block leave it full for every k: the search starts no lower
        if hi > 1 and fp_blocked(n, hi, k) <= fp:
            hi = 1  # (an fp within 1e-3 of 1)
        while hi <= MAX_BLOCKS and fp_blocked(n, hi, k) > fp:
            lo, hi = hi + 1, hi * 2
        if hi > MAX_BLOCKS:
            if fp_blocked(n, MAX_BLOCKS, k) > fp:
                continue
            hi = MAX_BLOCKS
        while lo < hi:
            mid = (lo + hi) // 2
            if fp_blocked(n, mid, k) <= fp:
                hi = mid
            else:
                lo = mid + 1
        if best is None or lo < best[1]:
            best = (k, lo)
    if best is None:
        raise ValueError("no Bloom filter of at most 2^32-1 blocks per band reaches fp=%g for n=%d" % (fp, n))
    return best


# ---------------------------------------------------------------------------------------------------------- the numpy twin
def _splitmix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def band_keys(sig: np.ndarray, b: int, r: int) -> np.ndarray:
    """uint64 [n, b]: ``sum(hashvalues[j*r:(j+1)*r]) % (2**61 - 1)``, the sum wrapping mod 2**64 (ref :105)."""
    n = sig.shape[0]
    s = sig[:, : b * r].reshape(n, b, r).sum(axis=2, dtype=np.uint64)
    x = (s & _mersenne_prime) + (s >> np.uint64(61))
    return np.where(x >= _mersenne_prime, x - _mersenne_prime, x)


def block_masks(keys: np.ndarray, n_blocks: int, k: int):
    """(int64 [m] block of every key, uint32 [m, 16] the words its ``k`` bits set)."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    with np.errstate(over="ignore"):
        state = keys + _GOLDEN
        block = ((_splitmix(state) >> np.uint64(32)) * np.uint64(n_blocks)) >> np.uint64(32)
        mask = np.zeros((keys.size, BLOCK_WORDS), dtype=np.uint32)
        rows = np.arange(keys.size)
        for i in range(k):
            if i % 7 == 0:
                state = state + _GOLDEN
                out = _splitmix(state)
            pos = (out >> np.uint64(9 * (i % 7))) & np.uint64(511)
            # one position of every key: no (row, word) pair repeats within this statement
            mask[rows, (pos >> np.uint64(5)).astype(np.int64)] |= np.uint32(1) << (pos & np.uint64(31)).astype(np.uint32)
    return block.astype(np.int64), mask


def _flat_blocks(sig: np.ndarray, b: int, r: int, n_blocks: int, k: int):
    block, mask = block_masks(band_keys(sig, b, r), n_blocks, k)
    block += np.tile(np.arange(b, dtype=np.int64) * n_blocks, sig.shape[0])
    return block, mask


def insert_host(words: np.ndarray, sig: np.ndarray, r: int, k: int) -> None:
    """The twin of mhx_bloom_insert_dev on ``words`` uint32 [b, n_blocks, 16], in place."""
    b, n_blocks, _ = words.shape
    step = max(1, _CHUNK_KEYS // b)
    for s in range(0, sig.shape[0], step):
        block, mask = _flat_blocks(sig[s: s + step], b, r, n_blocks, k)
        np.bitwise_or.at(words.reshape(-1, BLOCK_WORDS), block, mask)


def query_host(words: np.ndarray, sig: np.ndarray, r: int, k: int) -> np.ndarray:
    """The twin of mhx_bloom_query_dev: bool [n]."""
    b, n_blocks, _ = words.shape
    out = np.zeros(sig.shape[0], dtype=np.bool_)
    step = max(1, _CHUNK_KEYS // b)
    lines = words.reshape(-1, BLOCK_WORDS)
    for s in range(0, sig.shape[0], step):
        block, mask = _flat_blocks(sig[s: s + step], b, r, n_blocks, k)
        out[s: s + step] = ((lines[block] & mask) == mask).all(axis=1).reshape(-1, b).any(axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------- the filter
class _DevView:
    """What Context.bloom_* needs of a device buffer: the address (a band of a shared filter)."""

    def __init__(self, ptr: int):
        self.ptr = ptr


class _Filter:
    """``bands`` filters of one geometry, in numpy (``words``) or on a device (``buf``)."""

    def __init__(self, bands: int, n_blocks: int, k: int, ctx=None, words: Optional[np.ndarray] = None):
        self.bands, self.n_blocks, self.k, self.ctx = bands, n_blocks, k, ctx
        self.words, self.buf = None, None
        if ctx is None:
            self.words = np.zeros((bands, n_blocks, BLOCK_WORDS), dtype=np.uint32) if words is None else words
        else:
            self.buf = ctx.alloc(self.nbytes)
            if words is None:
                _native.check(ctx.lib.mhx_memset_dev(ctx.handle, self.buf.ptr, 0, self.nbytes))
            else:
                self.buf.upload(words)

    @property
    def nbytes(self) -> int:
        return self.bands * self.n_blocks * BLOCK_WORDS * 4

    def _view(self, band: Optional[int]):
        if band is None:
            return self.buf, self.bands
        return _DevView(self.buf.ptr + band * self.n_blocks * BLOCK_WORDS * 4), 1

    def insert(self, sig: np.ndarray, r: int, band: Optional[int] = None) -> None:
        if self.ctx is None:
            insert_host(self.words if band is None else self.words[band: band + 1], sig, r, self.k)
            return
        d_filter, bands = self._view(band)
        step = max(1, _CHUNK_KEYS // bands)
        for s in range(0, sig.shape[0], step):
            self.ctx.bloom_insert(sig[s: s + step], d_filter, bands, r, self.k, self.n_blocks)

    def query(self, sig: np.ndarray, r: int, then_insert: bool = False, band: Optional[int] = None) -> np.ndarray:
        if self.ctx is None:
            words = self.words if band is None else self.words[band: band + 1]
            hit = query_host(words, sig, r, self.k)
            if then_insert:
                insert_host(words, sig, r, self.k)
            return hit
        d_filter, bands = self._view(band)
        step = max(1, _CHUNK_KEYS // bands)
        if not then_insert or sig.shape[0] <= step:
            parts = [self.ctx.bloom_query(sig[s: s + step], d_filter, bands, r, self.k, self.n_blocks, then_insert)
                     for s in range(0, sig.shape[0], step)]
        else:  # the answers of every piece refer to the filter before the call: all the queries, then all the inserts
            parts = [self.ctx.bloom_query(sig[s: s + step], d_filter, bands, r, self.k, self.n_blocks) for s in range(0, sig.shape[0], step)]
            self.insert(sig, r, band)
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.bool_)

    def to_host(self, band: Optional[int] = None) -> np.ndarray:
        """A copy of the words: [bands, n_blocks, 16], or [n_blocks, 16] of one band."""
        if self.ctx is None:
            return (self.words if band is None else self.words[band]).copy()
        if band is None:
            return self.buf.download((self.bands, self.n_blocks, BLOCK_WORDS), np.uint32)
        return self.buf.download((self.n_blocks, BLOCK_WORDS), np.uint32, offset=band * self.n_blocks * BLOCK_WORDS * 4)

    def load_band(self, band: int, words: np.ndarray) -> None:
        if self.ctx is None:
            self.words[band] = words
        else:
            self.buf.upload(words, offset=band * self.n_blocks * BLOCK_WORDS * 4)

    def union(self, other: "_Filter") -> None:
        if self.ctx is None:
            self.words |= other.to_host()
        elif other.ctx is self.ctx:
            self.ctx.bloom_union(self.buf, other.buf, self.bands, self.n_blocks)
            self.ctx.synchronize()
        else:  # a host filter, or one on another device: through the host
            d_src = self.ctx.to_device(other.to_host())
            self.ctx.bloom_union(self.buf, d_src, self.bands, self.n_blocks)
            self.ctx.synchronize()
            d_src.free()

    def free(self) -> None:
        if self.buf is not None:
            self.buf.free()
            self.buf = None


def _as_signatures(signatures, h: int) -> np.ndarray:
    """[n, h] uint32 or uint64."""
    sig = np.asarray(signatures)
    if sig.ndim != 2:
        raise ValueError("signatures must be an [N, num_perm] matrix of MinHash values")
    if sig.dtype.kind not in "ui":
        raise ValueError("signatures must be integers")
    if sig.shape[1] != h:
        raise ValueError("Expecting minhash with length %d, got %d" % (h, sig.shape[1]))
    if sig.dtype != np.uint32:
        sig = sig.astype(np.uint64, copy=False)
    return np.ascontiguousarray(sig)


def _band_values(hashvalues) -> np.ndarray:
    """The hash values of one band as a 1-D uint64 array (``sum()`` over anything else has no defined meaning)."""
    hv = np.asarray(hashvalues)
    if hv.ndim != 1 or (hv.size and hv.dtype.kind not in "ui"):
        raise ValueError("hashvalues must be a 1-D array of integers (a WeightedMinHash cannot be indexed by a Bloom LSH)")
    return hv.astype(np.uint64, copy=False)


def _read_band(fname: str, k: int, n_blocks: int, band_size: int) -> np.ndarray:
    with open(fname, "rb") as f:
        head = f.read(_HEADER.size)
        if len(head) != _HEADER.size or head[:8] != _MAGIC:
            raise ValueError(f"{fname} is not a datasketch_amd Bloom filter file (the reference's pybloomfilter files are not readable)")
        _, version, fk, fblocks, fr = _HEADER.unpack(head)
        if version != _VERSION:
            raise ValueError(f"{fname}: unknown file version {version}")
        if (fk, fblocks, fr) != (k, n_blocks, band_size):
            raise ValueError(f"{fname} holds a filter of k={fk}, n_blocks={fblocks}, band_size={fr}; "
                             f"the arguments ask for k={k}, n_blocks={n_blocks}, band_size={band_size}")
        words = np.fromfile(f, dtype="<u4", count=n_blocks * BLOCK_WORDS)
    if words.size != n_blocks * BLOCK_WORDS:
        raise ValueError(f"{fname} is truncated")
    return words.astype(np.uint32, copy=False).reshape(n_blocks, BLOCK_WORDS)


def _write_band(fname: str, words: np.ndarray, k: int, n_blocks: int, band_size: int) -> None:
    tmp = fname + ".tmp"
    with open(tmp, "wb") as f:
        f.write(_HEADER.pack(_MAGIC, _VERSION, k, n_blocks, band_size))
        np.ascontiguousarray(words, dtype="<u4").tofile(f)
    os.replace(tmp, fname)


class BloomTable:
    """The Bloom filter of one band (ref :55-118).  Built directly it owns a filter in numpy; the ``hashtables`` of a
    :class:`MinHashLSHBloom` are views of band ``i`` of the index's shared array, wherever that lives.

    ``fname``: where ``sync()`` saves the filter; if the file exists the filter is loaded from it (``ValueError`` when its
    geometry differs from what ``item_count``, ``fp`` and ``band_size`` give).  The file format is this package's own."""

    def __init__(self, item_count: int, fp: float, band_size: int, fname: Optional[str] = None, *, _index=None, _band: int = 0):
        self.r = band_size
        self.fname = fname
        self._index, self._band = _index, _band
        if _index is not None:
            self.k, self.n_blocks = _index.k, _index.n_blocks
            self._own = None
        else:
            self.k, self.n_blocks = bloom_size(item_count, fp)
            self._own = _Filter(1, self.n_blocks, self.k)
        if fname is not None and os.path.exists(fname):
            logger.info(f"Loading Bloom Filter at {fname}...")
            self._filter().load_band(self._band, _read_band(fname, self.k, self.n_blocks, self.r))

    def _filter(self) -> _Filter:
        if self._index is None:
            return self._own
        self._index.flush()
        return self._index._store

    @property
    def words(self) -> np.ndarray:
        """A copy of the band's words, uint32 [n_blocks, 16]."""
        return self._filter().to_host(self._band)

    def sync(self):
        if self.fname is not None:
            _write_band(self.fname, self.words, self.k, self.n_blocks, self.r)
        else:
            warnings.warn("Attempting to save in-memory Bloom filter, this is a no-op.", RuntimeWarning, stacklevel=2)

    def assert_size(self, hashvalues):
        if not len(hashvalues) == self.r:
            raise RuntimeError(f"Invalid length for indices, {len(hashvalues)}, expected {self.r} hashvalues in band")

    def insert(self, hashvalues) -> None:
        """Insert the hash values of one band of a MinHash (ref :94-106)."""
        self.assert_size(hashvalues)
        self._filter().insert(_band_values(hashvalues).reshape(1, -1), self.r, band=self._band)

    def query(self, hashvalues) -> bool:
        """Whether these hash values of one band were (probably) inserted before (ref :108-118)."""
        self.assert_size(hashvalues)
        return bool(self._filter().query(_band_values(hashvalues).reshape(1, -1), self.r, band=self._band)[0])


class MinHashLSHBloom:
    """The LSHBloom index (ref :126-377; https://arxiv.org/abs/2411.04257): MinHashLSH with a Bloom filter per band in place of
    the hash tables.  It cannot return keys; ``query`` tells whether some inserted set probably has a Jaccard similarity above
    the threshold with the query.

    Args:
        threshold, num_perm, weights, params: as for :class:`MinHashLSH`.
        n (int): the number of sets to be inserted (an estimate of the dataset size).
        fp (float): the false-positive rate of every band's Bloom filter, in (0, 1).
        save_dir (str): where ``sync()`` saves the filters (``band-{i}.bf``, this package's own format -- the reference's
            ``pybloomfilter`` files are not readable); filters found there are loaded.  ``None``: in memory only.
        gpu_mode, device: where the filters live (module docstring).
    """

    def __init__(self, threshold: float = 0.9, num_perm: int = 128, n: Optional[int] = None, fp: Optional[float] = None,
                 save_dir: Optional[str] = None, weights=(0.5, 0.5), params=None, gpu_mode: str = "detect",
                 device: Optional[int] = None) -> None:
        lsh_bulk._check_gpu_mode(gpu_mode)
        if threshold > 1.0 or threshold < 0.0:
            raise ValueError("threshold must be in [0.0, 1.0]")
        if num_perm < 2:
            raise ValueError("Too few permutation functions")
        if n is None or n <= 0:
            raise ValueError("n for LSHBloom must be >= 0")
        if fp is None or fp >= 1.0 or fp <= 0.0:
            raise ValueError("fp must be in (0.0, 1.0)")
        if save_dir is None:
            warnings.warn("Creating LSHBloom index without save directory, this index will not be persisted.", RuntimeWarning,
                          stacklevel=2)
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
        self.n, self.fp, self.save_dir = n, fp, save_dir
        self.gpu_mode, self.device = gpu_mode, device
        self.buffer_size = 50000
        self.k, self.n_blocks = bloom_size(n, fp)
        self._pending = []
        self._store = _Filter(self.b, self.n_blocks, self.k, self._context() if gpu_mode == "always" else None)
        if save_dir is not None:
            os.makedirs(save_dir, exist_ok=True)
        self.hashtables = [
            BloomTable(n, fp, self.r, os.path.join(save_dir, f"band-{i}.bf") if save_dir is not None else None, _index=self, _band=i)
            for i in range(self.b)
        ]
        self.hashranges = [(i * self.r, (i + 1) * self.r) for i in range(self.b)]

    # ---------------------------------------------------------------- where the filter lives
    def _context(self):
        if not lsh_bulk._use_gpu("always"):
            raise RuntimeError("GPU mode 'always' requested but no MI355X / libmhx.so is available.")
        return _native.context(self.device)

    @property
    def on_device(self) -> bool:
        return self._store.ctx is not None

    def _place(self, rows: int) -> None:
        """'detect': the first bulk call that is large enough moves the filter to the device, where it stays."""
        if self.gpu_mode == "detect" and not self.on_device and rows * self.b >= DETECT_DEVICE_KEYS and lsh_bulk._use_gpu("detect"):
            self._store = _Filter(self.b, self.n_blocks, self.k, _native.context(self.device), words=self._store.words)

    # ---------------------------------------------------------------- staging
    def flush(self) -> None:
        """Insert the rows staged by :meth:`insert`."""
        if self._pending:
            rows, self._pending = np.vstack(self._pending), []
            self._place(rows.shape[0])
            self._store.insert(rows, self.r)

    def _row(self, minhash) -> np.ndarray:
        if len(minhash) != self.h:
            raise ValueError("Expecting minhash with length %d, got %d" % (self.h, len(minhash)))
        return _band_values(minhash.hashvalues)

    # ---------------------------------------------------------------- the reference's methods
    def insert(self, minhash) -> None:
        """Insert the MinHash of a set (ref :298-315).  Staged: visible to the next query."""
        self._insert(minhash)

    def _insert(self, minhash) -> None:
        self._pending.append(np.array(self._row(minhash)))
        if len(self._pending) >= self.buffer_size:
            self.flush()

    def query(self, minhash) -> bool:
        """Whether some inserted set collides with the query in some band (ref :317-372)."""
        row = self._row(minhash)
        self.flush()
        return bool(self._store.query(row.reshape(1, -1), self.r)[0])

    def sync(self) -> None:
        """Write every band to ``save_dir`` (ref :374-377); in memory a warning per band and nothing else."""
        logger.info("Saving Bloom Index...")
        self.flush()
        if self.save_dir is None:
            for _ in self.hashtables:
                warnings.warn("Attempting to save in-memory Bloom filter, this is a no-op.", RuntimeWarning, stacklevel=2)
            return
        words = self._store.to_host()
        for i, table in enumerate(self.hashtables):
            _write_band(table.fname, words[i], self.k, self.n_blocks, self.r)

    # ---------------------------------------------------------------- beyond the reference
    def insert_bulk(self, signatures) -> None:
        """Insert every row of a signature matrix ``[N, num_perm]`` (uint32 or uint64)."""
        sig = _as_signatures(signatures, self.h)
        self.flush()
        self._place(sig.shape[0])
        self._store.insert(sig, self.r)

    def query_bulk(self, signatures) -> np.ndarray:
        """``[query(m) for m in rows]`` as a bool array."""
        sig = _as_signatures(signatures, self.h)
        self.flush()
        self._place(sig.shape[0])
        return self._store.query(sig, self.r)

    def query_insert_bulk(self, signatures) -> np.ndarray:
        """The streaming near-duplicate step: the answers of :meth:`query_bulk` against the index as it is before the call,
        then every row inserted.  Rows of one call do not see each other."""
        sig = _as_signatures(signatures, self.h)
        self.flush()
        self._place(sig.shape[0])
        return self._store.query(sig, self.r, then_insert=True)

    def _geometry(self):
        return (self.h, self.b, self.r, self.k, self.n_blocks)

    def merge(self, other: "MinHashLSHBloom") -> None:
        """OR another index of the same geometry into this one (shards of one corpus)."""
        if not isinstance(other, MinHashLSHBloom):
            raise ValueError("Cannot merge type MinHashLSHBloom and %s" % type(other).__name__)
        if other._geometry() != self._geometry():
            raise ValueError("Cannot merge MinHashLSHBloom indexes of different geometry: (num_perm, b, r, k, n_blocks) = "
                             f"{self._geometry()} and {other._geometry()}")
        self.flush()
        other.flush()
        self._store.union(other._store)

    def words(self) -> np.ndarray:
        """A copy of the whole index, uint32 [b, n_blocks, 16]."""
        self.flush()
        return self._store.to_host()

    # ---------------------------------------------------------------- pickling
    def __getstate__(self):
        state = {k: v for k, v in self.__dict__.items() if k not in ("_store", "_pending", "hashtables")}
        state["words"] = self.words()
        return state

    def __setstate__(self, state) -> None:
        words = state.pop("words")
        self.__dict__.update(state)
        self._pending = []
        self._store = _Filter(self.b, self.n_blocks, self.k, self._context() if self.gpu_mode == "always" else None, words=words)
        self.hashtables = [
            BloomTable.__new__(BloomTable) for _ in range(self.b)
        ]
        for i, table in enumerate(self.hashtables):
            table.r, table._index, table._band, table._own = self.r, self, i, None
            table.k, table.n_blocks = self.k, self.n_blocks
            table.fname = os.path.join(self.save_dir, f"band-{i}.bf") if self.save_dir is not None else None
