"""HyperLogLog with the reference's API (ekzhu/datasketch ``datasketch.HyperLogLog``) and a HIP back end.

Mirror of datasketch/hyperloglog.py:25-320: same constructor, attributes, methods, exceptions and quirks, so an object of
this class stands in for the reference's.  What the reference lacks is added under the names ``MinHash`` uses here:

* ``update_batch`` folds a whole batch of tokens into one sketch, ``bulk`` / ``bulk_registers`` build one sketch per set of
  a corpus -- one kernel launch per chunk instead of one Python call per token (ref :136-142);
* ``count_many``, ``merge_many`` and ``union_groups`` estimate, merge and union whole register matrices.

``gpu_mode`` is the seam of ``MinHash``: ``'always'`` runs on the MI355X and raises ``RuntimeError`` without one,
``'detect'`` uses the device when there is one and the work is large enough to pay for the copies, ``'disable'`` is numpy.
Every device path has a vectorised numpy twin below; both give the reference's registers bit for bit, and ``count_many``
gives the reference's ``count()`` bit for bit for 32-bit hashes.

``HyperLogLogPlusPlus`` is not here: its estimator needs the bias and threshold tables of the reference's
``hyperloglog_const.py``.  Its *registers* are: ``bulk_registers(..., hash_bits=64)`` yields exactly what
``HyperLogLogPlusPlus.update`` leaves, and a row can be handed to ``datasketch.HyperLogLogPlusPlus(reg=row)``.
"""
from __future__ import annotations

import copy
import struct
import warnings
from typing import Callable, Iterable, List, Optional

import numpy as np

from datasketch_amd import _native
from datasketch_amd import shingle as _shingle
from datasketch_amd.hashfunc import device_hash, prehashed, sha1_hash32, sha1_hash64
from datasketch_amd.minhash import _no_device_error

# update_batch: below this many tokens the batch stays on the host whatever ``gpu_mode='detect'`` finds -- the vectorised numpy
# path costs less than one upload + launch + download (both curves: DESIGN.md section 5, "HyperLogLog")
UPDATE_BATCH_HOST_TOKENS = 32768
# count_many / merge_many / union_groups under 'detect': register matrices smaller than this stay on the host
_HOST_MATRIX_BYTES = 1 << 20
# tokens / output bytes per device call of bulk_registers (bounds the staging buffers)
_BULK_CHUNK_TOKENS = 1 << 25
_BULK_CHUNK_BYTES = 1 << 28


def _use_gpu(mode: str) -> bool:
    """The seam of ``MinHash._use_gpu`` (ref: datasketch/minhash.py:268-279)."""
    if mode == "always":
        try:
            ok = _native.gpu_available()
        except _native.MhxError as e:
            raise _no_device_error() from e
        if not ok:
            raise _no_device_error()
        return True
    if mode == "detect":
        return _native.gpu_detected()
    return False


def _overflow_error(hash_bits: int, p: int) -> ValueError:
    # ref :240-245 (the reference's message carries the run of blanks of its line continuation)
    return ValueError("Hash value overflow, maximum size is %d bits" % (hash_bits - p))


def _check_p(p: int) -> None:
    if not (4 <= p <= 16):
        raise ValueError("p=%d should be in range [4 : 16]" % p)


def _as_hashes(values, hash_bits: int, p: int) -> np.ndarray:
    """Token hashes as a flat uint64 (or, unchanged, uint32) array; what no unsigned 64-bit integer holds overflows every
    hash range (ref :238-246)."""
    if isinstance(values, np.ndarray) and values.dtype in (np.dtype(np.uint32), np.dtype(np.uint64)):
        return values.reshape(-1)
    try:
        return np.array(values, dtype=np.uint64).reshape(-1)
    except OverflowError:
        raise _overflow_error(hash_bits, p) from None


def _bit_length(x: np.ndarray) -> np.ndarray:
    """``int.bit_length`` of every element of a uint64 array: the exponent frexp reports, taken of the two 32-bit halves
    (a float64 holds those exactly; a whole 64-bit value could round up to the next power of two)."""
    hi, lo = (x >> np.uint64(32)).astype(np.float64), (x & np.uint64(0xFFFFFFFF)).astype(np.float64)
    return np.where(hi > 0, 32 + np.frexp(hi)[1], np.frexp(lo)[1]).astype(np.int64)


def _registers_host(hv: np.ndarray, offsets: Optional[np.ndarray], fixed_len: int, n_sets: int, p: int, hash_bits: int,
                    init: Optional[np.ndarray]) -> np.ndarray:
    """The numpy twin of mhx_hll_bulk_dev: uint8 [n_sets, m]."""
    m = 1 << p
    if offsets is not None:
        hv = hv[int(offsets[0]): int(offsets[n_sets])]
        lens = np.diff(offsets)
    else:
        hv = hv[: n_sets * fixed_len]
        lens = np.full(n_sets, fixed_len, dtype=np.int64)
    hv = hv.astype(np.uint64, copy=False)
    if hash_bits == 32 and hv.size and int(hv.max()) >> 32:
        raise _overflow_error(hash_bits, p)
    reg = np.zeros((n_sets, m), dtype=np.uint8)
    if init is not None:
        reg[:] = np.asarray(init).view(np.uint8)
    if hv.size:
        rank = (hash_bits - p + 1 - _bit_length(hv >> np.uint64(p))).astype(np.uint8)  # ref :239
        slot = np.repeat(np.arange(n_sets, dtype=np.int64) * m, lens) + (hv & np.uint64(m - 1)).astype(np.int64)  # ref :138
        np.maximum.at(reg.reshape(-1), slot, rank)
    return reg


def _histogram_host(reg: np.ndarray) -> np.ndarray:
    """The numpy twin of mhx_hll_histogram_dev: np.bincount of every row, uint32 [n, 64]; ValueError for a register above 63."""
    n, m = reg.shape
    hist = np.empty((n, 64), dtype=np.uint32)
    step = max(1, (1 << 22) // m)
    for s in range(0, n, step):
        blk = reg[s: s + step].astype(np.int64)
        if blk.size and int(blk.max()) > 63:
            raise ValueError("register values above 63 are no HyperLogLog ranks")
        blk += np.arange(blk.shape[0], dtype=np.int64)[:, None] * 64
        hist[s: s + step] = np.bincount(blk.reshape(-1), minlength=blk.shape[0] * 64).reshape(-1, 64)
    return hist


def _as_matrix(reg) -> np.ndarray:
    reg = np.asarray(reg)
    if reg.dtype not in (np.dtype(np.int8), np.dtype(np.uint8)) or reg.ndim != 2:
        raise ValueError("a register matrix is a 2-D int8 or uint8 array")
    m = reg.shape[1]
    if m < 16 or m > 65536 or m & (m - 1):
        raise ValueError("a register matrix has 2**p columns, p in [4 : 16]")
    return np.ascontiguousarray(reg).view(np.uint8)


def _on_device(gpu_mode: str, nbytes: int) -> bool:
    return gpu_mode == "always" and _use_gpu(gpu_mode) or (gpu_mode == "detect" and nbytes >= _HOST_MATRIX_BYTES and _use_gpu(gpu_mode))


def count_many(reg, hash_bits: int = 32, gpu_mode: str = "detect") -> np.ndarray:
    """``[HyperLogLog(reg=r).count() for r in reg]`` as a float64 array, without the objects and without warnings.

    Everything the estimator needs is the histogram of a row's register values (mhx_hll_histogram_dev, or np.bincount):
    the zero count of the linear counting, and ``sum(2.0 ** -reg) = sum_v hist[v] * 2**-v``.  For ``hash_bits=32`` every
    term of that sum is a multiple of 2**-29 and there are at most 2**16 of them, so it is exact in float64 in any order
    and the result equals the reference's ``count()`` (ref :144-168) bit for bit, ``nan`` of a saturated row included.
    A row with no zero register in the linear-counting range raises ``ZeroDivisionError``, as the reference's
    ``m / float(0)`` does (ref :249), naming the first such row.

    ``hash_bits=64``: the same formula with 2**64 as the hash range in the large-range correction (the reference's
    HyperLogLog++ estimator needs tables this package does not have).  Ranks then reach 61, the sum is not
    order-independent in float64, and the result is not pinned to any reference value."""
    if hash_bits not in (32, 64):
        raise ValueError("hash_bits must be 32 or 64")
    reg = _as_matrix(reg)
    n, m = reg.shape
    p = m.bit_length() - 1
    if n and _on_device(gpu_mode, reg.size):
        hist, invalid = _native.context().hll_histogram(reg)
        if invalid:
            raise ValueError("register values above 63 are no HyperLogLog ranks")
    else:
        hist = _histogram_host(reg)
    alpha = HyperLogLog._get_alpha(None, p)
    harmonic = np.zeros(n, dtype=np.float64)
    for v in range(64):
        harmonic += hist[:, v] * 2.0 ** (-v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = alpha * float(m ** 2) / harmonic  # ref :152
        out = e.copy()
        small = e <= (5.0 / 2.0) * m  # ref :154,161
        zeros = hist[:, 0]
        if np.any(small & (zeros == 0)):
            raise ZeroDivisionError("float division by zero: row %d has no zero register" % int(np.flatnonzero(small & (zeros == 0))[0]))
        if np.any(small):
            out[small] = m * np.log(m / zeros[small].astype(np.float64))  # ref :249
        space = float(1 << hash_bits)
        large = ~small & ~(e <= (1.0 / 30.0) * space)  # ref :165
        if np.any(large):
            out[large] = -space * np.log(1.0 - e[large] / space)  # ref :252
    return out


def merge_many(a, b, gpu_mode: str = "detect") -> np.ndarray:
    """Row-wise ``HyperLogLog.merge`` (ref :170-183): ``np.maximum(a, b)`` of two equally shaped register matrices, int8."""
    a, b = _as_matrix(a), _as_matrix(b)
    if a.shape != b.shape:
        raise ValueError("Cannot merge HyperLogLog with different precisions.")
    if a.size and _on_device(gpu_mode, a.size):
        return _native.context().hll_merge(a, b).view(np.int8)
    return np.maximum(a, b).view(np.int8)


def union_groups(reg, group_offsets, gpu_mode: str = "detect") -> np.ndarray:
    """``HyperLogLog.union`` per group (ref :254-268): row g of the result is ``np.maximum.reduce`` of the rows
    ``group_offsets[g] .. group_offsets[g + 1]`` of ``reg``; an empty group gives zeros.  int8 [len(group_offsets) - 1, m]."""
    reg = _as_matrix(reg)
    group_offsets = np.ascontiguousarray(group_offsets, dtype=np.int64).reshape(-1)
    if group_offsets.size < 1 or group_offsets[0] < 0 or group_offsets[-1] > reg.shape[0] or np.any(np.diff(group_offsets) < 0):
        raise ValueError("group_offsets must never decrease and stay inside the rows of reg")
    n_groups = group_offsets.size - 1
    if n_groups and reg.size and _on_device(gpu_mode, reg.size):
        return _native.context().hll_union_groups(reg, group_offsets).view(np.int8)
    out = np.zeros((n_groups, reg.shape[1]), dtype=np.uint8)
    starts, ends = group_offsets[:-1], group_offsets[1:]
    full = starts < ends
    if np.any(full):  # reduceat runs each segment to the next start: with the empty groups taken out that is the group's end
        out[full] = np.maximum.reduceat(reg[: int(group_offsets[-1])], starts[full], axis=0)
    return out.view(np.int8)


class HyperLogLog:
    """HyperLogLog sketch for cardinality estimation; drop-in for ``datasketch.HyperLogLog``.

    Args:
        p: precision, 4..16; ``m = 2**p`` registers (ignored when ``reg`` is given).
        reg: optional initial registers (a numpy array of a power-of-two size).
        hashfunc: callable mapping a token to an unsigned integer of at most 32 bits.
        hashobj: deprecated, as in the reference.
        gpu_mode: ``'disable'`` | ``'detect'`` | ``'always'`` for ``update_batch`` (see the module docstring).
    """

    __slots__ = ("alpha", "hashfunc", "m", "max_rank", "p", "reg", "_gpu_mode")

    _hash_range_bit = 32  # ref :52-53
    _hash_range_byte = 4

    def _get_alpha(self, p):
        _check_p(p)
        if p <= 6:
            return {4: 0.673, 5: 0.697, 6: 0.709}[p]
        return 0.7213 / (1.0 + 1.079 / (1 << p))

    def __init__(self, p: int = 8, reg: Optional[np.ndarray] = None, hashfunc: Callable = sha1_hash32, hashobj: Optional[object] = None,
                 gpu_mode: str = "detect"):
        if reg is None:
            self.p = p
            self.m = 1 << p
            self.reg = np.zeros((self.m,), dtype=np.int8)
        else:
            if not isinstance(reg, np.ndarray):
                raise ValueError("The imported register must be a numpy.ndarray.")
            self.m = reg.size
            self.p = int(self.m).bit_length() - 1
            if 1 << self.p != self.m:
                raise ValueError("The imported register has incorrect size. Expect a power of 2.")
            self.reg = reg  # (trusted as it is, ref :89-91)
        if not callable(hashfunc):
            raise ValueError("The hashfunc must be a callable.")
        if hashobj is not None:
            warnings.warn("hashobj is deprecated, use hashfunc instead.", DeprecationWarning, stacklevel=2)
        self.hashfunc = hashfunc
        self.alpha = self._get_alpha(self.p)
        self.max_rank = self._hash_range_bit - self.p
        self._gpu_mode = gpu_mode

    # ------------------------------------------------------------------ updates
    def update(self, b) -> None:
        """Add one token: on the host, as in the reference (ref :136-142)."""
        hv = self.hashfunc(b)
        reg_index = hv & (self.m - 1)
        bits = hv >> self.p
        self.reg[reg_index] = max(self.reg[reg_index], self._get_rank(bits))

    def _get_rank(self, bits):
        rank = self.max_rank - int(bits).bit_length() + 1
        if rank <= 0:
            raise _overflow_error(self._hash_range_bit, self.p)
        return rank

    def update_batch(self, b: Iterable) -> None:
        """Add many tokens with one max-update of the registers (not in the reference).  With ``hashfunc=prehashed`` a numpy
        integer array goes in as it is; byte tokens under the default ``sha1_hash32`` (or ``xxh32_hash32`` / ``xxh64_hash64`` at their width) are hashed on the device when the batch
        goes there; any other ``hashfunc`` is applied per token on the host.  Batches below ``UPDATE_BATCH_HOST_TOKENS`` stay on
        the host under ``'detect'``."""
        bits, p = self._hash_range_bit, self.p
        if not (self.hashfunc is prehashed and isinstance(b, np.ndarray)):
            b = b if isinstance(b, (list, tuple)) else list(b)
        n = b.size if isinstance(b, np.ndarray) else len(b)
        if n == 0:
            return
        device = self._gpu_mode == "always" and _use_gpu("always") or (self._gpu_mode == "detect" and n >= UPDATE_BATCH_HOST_TOKENS and _use_gpu("detect"))
        init = np.ascontiguousarray(self.reg).astype(np.int8, copy=False).view(np.uint8).reshape(-1)
        known = device_hash(self.hashfunc)
        if device and known and known[1] == bits and not isinstance(b, np.ndarray):
            buf, offs = _native.Context.pack_tokens(b)
            reg = _native.context().hll_bulk_bytes(buf, offs, np.array([0, n], dtype=np.int64), p, bits, init, kind=known[0])
        else:
            hv = _as_hashes(b if self.hashfunc is prehashed else [self.hashfunc(t) for t in b], bits, p)
            if device:
                reg, overflow = _native.context().hll_bulk(hv, None, hv.size, 1, p, bits, init)
                if overflow:
                    raise _overflow_error(bits, p)
            else:
                reg = _registers_host(hv, None, hv.size, 1, p, bits, init)
        self.reg = reg[0].view(np.int8)

    # ------------------------------------------------------------------ estimator
    def count(self) -> float:
        """The estimated cardinality (ref :144-168), warning near the small-range threshold as the reference does."""
        e = self.alpha * float(self.m ** 2) / np.sum(2.0 ** (-self.reg))
        threshold = (5.0 / 2.0) * self.m
        if abs(e - threshold) / threshold < 0.15:
            warnings.warn("Warning: estimate is close to error correction threshold. "
                          "Output may not satisfy HyperLogLog accuracy guarantee.", stacklevel=2)
        if e <= threshold:
            return self._linearcounting(self.m - np.count_nonzero(self.reg))
        if e <= (1.0 / 30.0) * (1 << 32):
            return e
        return self._largerange_correction(e)

    def _linearcounting(self, num_zero):
        return self.m * np.log(self.m / float(num_zero))

    def _largerange_correction(self, e):
        return -(1 << 32) * np.log(1.0 - e / (1 << 32))

    # ------------------------------------------------------------------ set operations / state
    def merge(self, other: "HyperLogLog") -> None:
        if self.m != other.m or self.p != other.p:
            raise ValueError("Cannot merge HyperLogLog with different precisions.")
        self.reg = np.maximum(self.reg, other.reg)

    def digest(self) -> np.ndarray:
        return copy.copy(self.reg)

    def copy(self) -> "HyperLogLog":
        return self.__class__(reg=self.digest(), hashfunc=self.hashfunc, gpu_mode=self._gpu_mode)

    def is_empty(self) -> bool:
        return not np.any(self.reg)

    def clear(self) -> None:
        self.reg = np.zeros((self.m,), dtype=np.int8)

    def __len__(self) -> int:
        return len(self.reg)

    def __eq__(self, other) -> bool:
        return type(self) is type(other) and self.p == other.p and self.m == other.m and np.array_equal(self.reg, other.reg)

    __hash__ = None  # (as for any class that defines __eq__ alone)

    @classmethod
    def union(cls, *hyperloglogs: "HyperLogLog") -> "HyperLogLog":
        if len(hyperloglogs) < 2:
            raise ValueError("Cannot union less than 2 HyperLogLog sketches")
        m = hyperloglogs[0].m
        if not all(h.m == m for h in hyperloglogs):
            raise ValueError("Cannot union HyperLogLog sketches with different precisions")
        reg = np.maximum.reduce([h.reg for h in hyperloglogs])
        return cls(reg=reg, hashfunc=hyperloglogs[0].hashfunc, gpu_mode=getattr(hyperloglogs[0], "_gpu_mode", "detect"))

    def bytesize(self) -> int:
        return struct.calcsize("B") * (1 + self.m)  # p, then one byte per register (ref :270-278)

    def serialize(self, buf) -> None:
        if len(buf) < self.bytesize():
            raise ValueError("The buffer does not have enough space for holding this HyperLogLog.")
        struct.pack_into("B%dB" % self.m, buf, 0, self.p, *self.reg)

    @classmethod
    def deserialize(cls, buf) -> "HyperLogLog":
        h = cls(cls._read_p(buf))
        h.reg = cls._read_reg(buf, h.m)
        return h

    @staticmethod
    def _read_p(buf) -> int:
        try:
            return struct.unpack_from("B", buf, 0)[0]
        except TypeError:
            return struct.unpack_from("B", memoryview(buf), 0)[0]

    @staticmethod
    def _read_reg(buf, m: int) -> np.ndarray:
        try:
            return np.array(struct.unpack_from("%dB" % m, buf, 1), dtype=np.int8)
        except TypeError:
            return np.array(struct.unpack_from("%dB" % m, memoryview(buf), 1), dtype=np.int8)

    def __getstate__(self):
        buf = bytearray(self.bytesize())
        self.serialize(buf)
        return buf

    def __setstate__(self, buf):
        # as in the reference (ref :309-320) the state is p and the registers: hashfunc (and gpu_mode) come back as the defaults
        self.__init__(p=self._read_p(buf))
        self.reg = self._read_reg(buf, self.m)

    # ------------------------------------------------------------------ bulk construction (not in the reference)
    @classmethod
    def bulk(cls, b: Iterable, **kwargs) -> List["HyperLogLog"]:
        """One sketch per element of ``b`` (what ``MinHash.bulk`` is to ``MinHash``); ``kwargs`` are the constructor's
        (``p``, ``hashfunc``, ``gpu_mode``)."""
        proto = cls(**kwargs)
        rows = cls.bulk_registers(b, p=proto.p, hashfunc=proto.hashfunc, hash_bits=cls._hash_range_bit, gpu_mode=proto._gpu_mode)
        out = []
        for row in rows:
            h = object.__new__(cls)
            h.p, h.m, h.alpha, h.max_rank, h.hashfunc, h._gpu_mode, h.reg = proto.p, proto.m, proto.alpha, proto.max_rank, proto.hashfunc, proto._gpu_mode, row
            out.append(h)
        return out

    @staticmethod
    def bulk_registers(b=None, packed=None, p: int = 8, hashfunc: Callable = sha1_hash32, hash_bits: int = 32,
                       gpu_mode: str = "detect", documents=None, shingle=None, words=None) -> np.ndarray:
        """The int8 ``[N, 2**p]`` register matrix of a corpus of N sets, without creating N objects.

        ``b``: any iterable of token iterables; with ``hashfunc=prehashed`` also a 2-D integer array (fixed-length sets; uint32
        and uint64 travel as they are) or a ``(values, offsets)`` CSR pair of hashes.  ``packed=(buf, byte_offsets,
        set_offsets)`` instead: byte tokens packed back to back, as for ``MinHash.bulk_signatures``.  Byte tokens are hashed on
        the device when ``hashfunc is sha1_hash32`` or ``xxh32_hash32`` with ``hash_bits=32``, or ``sha1_hash64`` or ``xxh64_hash64``
        with ``hash_bits=64``; any other callable, or any other pairing, is applied per token on the host and the integers go to the device.  ``hash_bits=64`` gives the registers of
        the reference's ``HyperLogLogPlusPlus``.  A hash that does not fit ``hash_bits`` raises ``ValueError``, as the
        reference's ``update`` does.

        Text: ``documents=`` with ``shingle=k`` (a ``(buf, doc_offsets)`` pair or a list of ``bytes`` / ``str``; a ``str`` is shingled
        over its UTF-8 bytes) counts the distinct ``k``-byte shingles of every document, ``packed=`` with ``shingle=w`` its distinct
        shingles of ``w`` consecutive tokens -- the rules of ``MinHash.bulk_signatures`` and :mod:`datasketch_amd.shingle`.  On the
        device the windows are hashed where they lie; ``hyperloglog.count_many`` turns the registers into counts.

        Words: ``documents=`` with ``shingle=w`` and ``words=True`` (or a uint8[256] translate table) counts the distinct shingles of
        ``w`` consecutive words of the normalised text (:func:`datasketch_amd.shingle.word_shingles`); on the device the raw text is
        tokenised, normalised, windowed and hashed in one call."""
        _check_p(p)
        if hash_bits not in (32, 64):
            raise ValueError("hash_bits must be 32 or 64")
        if not callable(hashfunc):
            raise ValueError("The hashfunc must be a callable.")
        if (b is not None) + (packed is not None) + (documents is not None) != 1:
            raise ValueError("give the corpus as exactly one of b, packed=(buf, byte_offsets, set_offsets) and documents=")
        if shingle is not None and b is not None:
            raise ValueError("shingle= goes with documents= (bytes) or packed= (tokens), not with b")
        if documents is not None and shingle is None:
            raise ValueError("documents= needs shingle=k, the number of bytes per shingle")
        table = _shingle.words_argument(words)
        if table is not None and documents is None:
            raise ValueError("words= goes with documents= and shingle=w, the number of words per shingle")
        device = _use_gpu(gpu_mode)
        known = device_hash(hashfunc)  # (hash_kind, bits): on the device where the function's width is hash_bits
        hash_on_device = device and known is not None and known[1] == hash_bits
        kind = known[0] if hash_on_device else 0
        m = 1 << p
        max_sets = max(1, _BULK_CHUNK_BYTES // m)

        def from_hashes(hv, offsets, fixed_len, n):
            if not device:
                return _registers_host(hv, offsets, fixed_len, n, p, hash_bits, None)
            reg, overflow = _native.context().hll_bulk(hv, offsets, fixed_len, n, p, hash_bits)
            if overflow:
                raise _overflow_error(hash_bits, p)
            return reg

        blocks = []
        if b is None:
            for piece in _shingle.text_corpus(packed, documents, shingle, table).chunks(max_sets, _BULK_CHUNK_TOKENS):
                if hash_on_device:
                    blocks.append(getattr(_native.context(), "hll_bulk_" + piece.native)(p=p, hash_bits=hash_bits, kind=kind, **piece.arrays()))
                    continue
                flat, offsets = _shingle.flatten(piece.host_sets())
                blocks.append(from_hashes(_as_hashes([hashfunc(t) for t in flat], hash_bits, p), offsets, 0, offsets.size - 1))
        elif hashfunc is prehashed and isinstance(b, np.ndarray) and b.ndim == 2:
            n, t = b.shape
            step = max(1, min(max_sets, _BULK_CHUNK_TOKENS // max(t, 1)))
            for s in range(0, n, step):
                blk = b[s: s + step]
                blocks.append(from_hashes(_as_hashes(np.ascontiguousarray(blk), hash_bits, p), None, t, blk.shape[0]))
        elif hashfunc is prehashed and isinstance(b, tuple) and len(b) == 2:
            values, offsets = _as_hashes(b[0], hash_bits, p), np.ascontiguousarray(b[1], dtype=np.int64).reshape(-1)
            if offsets.size < 1 or offsets[0] < 0 or offsets[-1] > values.size or np.any(np.diff(offsets) < 0):
                raise ValueError("offsets must never decrease and stay inside values")
            for s, e in _shingle.window_chunks(offsets, max_sets, _BULK_CHUNK_TOKENS):
                blocks.append(from_hashes(values[int(offsets[s]): int(offsets[e])], offsets[s: e + 1] - offsets[s], 0, e - s))
        else:
            chunk, tokens = [], 0

            def flush():
                if hash_on_device:
                    blocks.append(_native.context().hll_bulk_bytes(*_native.Context.pack_sets(chunk), p, hash_bits, kind=kind))
                    return
                lens = np.fromiter(map(len, chunk), dtype=np.int64, count=len(chunk))
                offsets = np.zeros(len(chunk) + 1, dtype=np.int64)
                np.cumsum(lens, out=offsets[1:])
                flat = [t if hashfunc is prehashed else hashfunc(t) for s in chunk for t in s]
                blocks.append(from_hashes(_as_hashes(flat, hash_bits, p), offsets, 0, len(chunk)))

            for s in b:
                s = s if isinstance(s, (list, tuple)) or (isinstance(s, np.ndarray) and s.ndim == 1) else list(s)
                chunk.append(s)
                tokens += len(s)
                if len(chunk) >= max_sets or tokens >= _BULK_CHUNK_TOKENS:
                    flush()
                    chunk, tokens = [], 0
            if chunk:
                flush()
        if not blocks:
            return np.empty((0, m), dtype=np.int8)
        return (blocks[0] if len(blocks) == 1 else np.concatenate(blocks, axis=0)).view(np.int8)
