"""The signature matrix of an index, one row per *slot*: what ``lsh.MinHashLSH``, ``lshforest.MinHashLSHForest`` and
``lsh_bulk.SortedBandsIndex`` keep their bands and trees beside.  :class:`DeviceRows` holds it on one MI355X, :class:`HostRows`
is the same surface over a numpy array.  Rows are uint32 while every value fits and uint64 after one :meth:`widen`."""
from __future__ import annotations

import numpy as np

from datasketch_amd import _native


class DeviceRows:
    """A ``[capacity, kw]`` device matrix whose first ``n`` rows are used; it grows by doubling."""

    def __init__(self, ctx, kw: int, dtype):
        self.ctx, self.kw = ctx, kw
        self.dtype = np.dtype(dtype)
        self.n = 0
        self.capacity = 0
        self.d_sig = None

    @property
    def code(self) -> int:
        return _native.MHX_U32 if self.dtype == np.uint32 else _native.MHX_U64

    @property
    def row_bytes(self) -> int:
        return self.kw * self.dtype.itemsize

    def reserve(self, need: int) -> None:
        """Room for ``need`` rows: at least twice the capacity (1024 rows to begin with) when there is less."""
        if need >> 32:
            raise ValueError("an index holds fewer than 2^32 rows")
        if need <= self.capacity:
            return
        cap = max(need, 2 * self.capacity, 1024)
        grown = self.ctx.alloc(cap * self.row_bytes)
        if self.n:
            self.ctx.copy_dev(grown.ptr, self.d_sig.ptr, self.n * self.row_bytes)
        self.ctx.synchronize()
        self.d_sig, self.capacity = grown, cap

    def upload(self, rows: np.ndarray) -> None:
        """Append host rows (of this matrix's dtype) after the last used one."""
        m = rows.shape[0]
        self.reserve(self.n + m)
        if m:
            self.d_sig.upload(rows, offset=self.n * self.row_bytes)
        self.n += m

    def copy_from(self, other: "DeviceRows") -> None:
        """Append the other matrix's rows (same context, width and dtype), device to device; enqueued."""
        self.reserve(self.n + other.n)
        if other.n:
            self.ctx.copy_dev(self.d_sig.ptr + self.n * self.row_bytes, other.d_sig.ptr, other.n * self.row_bytes)
        self.n += other.n

    def widen(self) -> None:
        """uint32 -> uint64 once.  Whatever is ordered by the rows' values (band digests, tree orders) stays valid: widening does
        not change how rows compare.  The wider matrix is allocated and filled before anything is reassigned, so a failure
        leaves the uint32 matrix as it was."""
        host = self.matrix().astype(np.uint64)
        grown = self.ctx.alloc(max(self.capacity, 1) * self.kw * 8)
        if self.n:
            grown.upload(host)
        self.ctx.synchronize()
        self.d_sig, self.dtype = grown, np.dtype(np.uint64)

    def matrix(self) -> np.ndarray:
        if self.n == 0:
            return np.empty((0, self.kw), dtype=self.dtype)
        return self.d_sig.download((self.n, self.kw), self.dtype)

    def row(self, slot: int) -> np.ndarray:
        return self.d_sig.download((self.kw,), self.dtype, offset=slot * self.row_bytes)


class HostRows:
    """The numpy twin: ``sig`` is the ``[n, kw]`` matrix itself."""

    def __init__(self, kw: int, dtype):
        self.kw = kw
        self.dtype = np.dtype(dtype)
        self.sig = np.empty((0, kw), dtype=self.dtype)

    @property
    def n(self) -> int:
        return self.sig.shape[0]

    def upload(self, rows: np.ndarray) -> None:
        self.sig = np.concatenate([self.sig, rows])

    def copy_from(self, other: "HostRows") -> None:
        self.upload(other.sig.astype(self.dtype))

    def widen(self) -> None:
        self.sig, self.dtype = self.sig.astype(np.uint64), np.dtype(np.uint64)

    def matrix(self) -> np.ndarray:
        return self.sig

    def row(self, slot: int) -> np.ndarray:
        return self.sig[slot]
