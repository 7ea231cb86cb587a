"""Cases that put the data of a device entry point past 2^31 / 2^32 elements or 4 GiB (host only: no device is touched and
libmhx is not loaded; the C oracle is the one oracle/ compiles with the host compiler).

A kernel that forms ``row * k``, ``offsets[i] + lane`` or a byte offset in 32 bits still returns a well-formed answer at these
sizes -- the answer of whatever lies at the wrapped address.  Every builder below therefore describes one large, mostly empty
device buffer as a sparse model (:class:`Big`): a fill byte, a few planted stretches of real data around a mark, and DECOYS,
different valid data planted where a 32-bit wrap of the planted indices would land.  From the model alone it computes

    * the expected result, by the existing definitions (oracle.oracle, the numpy twins behind gpu_mode="disable", hashlib,
      overlap.py) on the compact data, and
    * for every way of wrapping (``WRAPS``) the result a kernel would give that read through the wrapped indices,

so that tests/test_gpu_index_width.py can say "equals the decoy at index mod 2^32" and tests/test_index_width_host.py can check,
without a device, that every case still tests something: the touched indices pass the mark, one item straddles it, and no decoy
answers like the real data.

A mark M is measured in the unit the kernel indexes (``MARKS``); ``ACROSS`` is the distance of the straddling item's first
element below M, odd so that 16-byte loads straddle too.
"""
import hashlib
import os
import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import b_bit_minhash, hyperloglog, lsh_bulk, overlap  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.weighted_dispatch import MI355X_CUS, MI355X_LDS_PER_BLOCK  # noqa: E402

GiB = 1 << 30
MAX_LIVE_BYTES = 64 * GiB  # the most any one case may have allocated at a time
MAX_DOWNLOAD_BYTES = 64 << 20
ACROSS = 37
MARKS = {"byte": 1 << 32, "signed": 1 << 31, "unsigned": 1 << 32}  # unit -> M
BELOW, ACROSS_ROLE, ABOVE = "below", "across", "above"


def wraps(elem_bytes: int) -> Dict[str, Callable[[int], int]]:
    """What 32-bit arithmetic can make of an element index: the name is what a failure report says."""
    return {
        "index mod 2^32": lambda i: i % (1 << 32),
        "index mod 2^31": lambda i: i % (1 << 31),
        "byte offset mod 2^32": lambda i: (i * elem_bytes) % (1 << 32) // elem_bytes,
    }


def mark_elems(unit: str, elem_bytes: int) -> int:
    """The mark as an element index: byte 2^32 is element 2^30 of a uint32 array, 2^29 of a uint64 array."""
    return MARKS[unit] // elem_bytes if unit == "byte" else MARKS[unit]


class Big:
    """A large device buffer as a sparse model: ``n`` elements of ``dtype``, all bytes ``fill`` except the planted stretches."""

    def __init__(self, name: str, dtype, n: int, fill: int, fill_value=None):
        self.name, self.dtype, self.n, self.fill = name, np.dtype(dtype), int(n), int(fill)
        self.fill_value = fill_value  # an element no byte fill can write (-inf): the buffer is filled by copies of it instead
        self.plants: List[tuple] = []  # (first element, array), disjoint

    @property
    def nbytes(self) -> int:
        return self.n * self.dtype.itemsize

    @property
    def fill_elem(self):
        if self.fill_value is not None:
            return self.dtype.type(self.fill_value)
        return np.frombuffer(bytes([self.fill]) * self.dtype.itemsize, dtype=self.dtype)[0]

    def _free(self, start: int, count: int):
        """The sub-ranges of [start, start + count) that nothing is planted on."""
        free = [(start, start + count)]
        for s, d in self.plants:
            e, nxt = s + d.size, []
            for lo, hi in free:
                if e <= lo or hi <= s:
                    nxt.append((lo, hi))
                    continue
                if lo < s:
                    nxt.append((lo, s))
                if e < hi:
                    nxt.append((e, hi))
            free = nxt
        return free

    def plant(self, start: int, data: np.ndarray, where_free: bool = False) -> None:
        data = np.ascontiguousarray(data, dtype=self.dtype).reshape(-1)
        if data.size == 0:
            return
        assert 0 <= start and start + data.size <= self.n, f"{self.name}: plant [{start}, {start + data.size}) outside [0, {self.n})"
        free = self._free(start, data.size)
        if not where_free:
            assert free == [(start, start + data.size)], f"{self.name}: plant at {start} overlaps another"
        for lo, hi in free:
            self.plants.append((lo, data[lo - start: hi - start].copy()))

    def read(self, start: int, count: int) -> np.ndarray:
        """What the device buffer holds at [start, start + count), from the model."""
        assert 0 <= start and start + count <= self.n, f"{self.name}: read [{start}, {start + count}) outside [0, {self.n})"
        out = np.full(count, self.fill_elem, dtype=self.dtype)
        for s, d in self.plants:
            lo, hi = max(s, start), min(s + d.size, start + count)
            if lo < hi:
                out[lo - start: hi - start] = d[lo - s: hi - s]
        return out

    def pieces(self, start: int, count: int):
        """[start, start + count) cut wherever a wrap changes its translation: at multiples of 2^31 bytes and elements."""
        step = (1 << 31) // self.dtype.itemsize
        cuts = [start] + [c for c in range((start // step + 1) * step, start + count, step)] + [start + count]
        return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]

    def read_wrapped(self, start: int, count: int, wrap) -> np.ndarray:
        return np.concatenate([self.read(wrap(a), n) for a, n in self.pieces(start, count)] or [np.empty(0, self.dtype)])

    def moved(self, start: int, count: int, wrap) -> bool:
        return any(wrap(a) != a for a, n in self.pieces(start, count))

    def plant_decoys(self, start: int, count: int, make: Callable[[np.ndarray], np.ndarray]) -> None:
        """Different valid data wherever a wrap of [start, start + count) lands (and nothing is planted yet): make(the real data
        of the piece) returns as many elements."""
        for wrap in wraps(self.dtype.itemsize).values():
            for a, n in self.pieces(start, count):
                if wrap(a) != a:
                    self.plant(wrap(a), make(self.read(a, n)), where_free=True)


@dataclass
class Item:
    """One set / row / token of a case, in the unit of its mark: what the host test measures."""
    role: str
    first: int  # first and last touched index, in the case's unit
    last: int


@dataclass
class Check:
    """``expected`` is what a buffer must hold from byte ``offset`` on after the call; ``decoys[name]`` what it would hold had the
    kernel read through wrap ``name``, and ``moved[name][row]`` whether that wrap moves anything row ``row`` reads."""
    buffer: str
    offset: int
    expected: np.ndarray
    what: str
    roles: List[str] = field(default_factory=list)  # per row of expected (first axis)
    decoys: Dict[str, np.ndarray] = field(default_factory=dict)
    moved: Dict[str, np.ndarray] = field(default_factory=dict)


def describe_mismatch(got: np.ndarray, chk: Check) -> str:
    """"" when ``got`` is what the check expects; else which rows differ and, for each, the decoy it equals (the CPU side of
    the comparison in tests/test_gpu_index_width.py; tests/test_index_width_host.py holds its wording)."""
    rows = max(len(chk.roles), 1)
    g, w = got.reshape(rows, -1), chk.expected.reshape(rows, -1)
    bad = np.flatnonzero((g != w).any(axis=1))
    if bad.size == 0:
        return ""
    lines = [f"{chk.what}: {bad.size} of {rows} rows differ"]
    for r in bad[:6].tolist():
        role = chk.roles[r] if chk.roles else "-"
        named = [f"equals the decoy at {name}" for name, d in chk.decoys.items()
                 if np.asarray(chk.moved[name]).reshape(-1)[r] and np.array_equal(d.reshape(rows, -1)[r], g[r])]
        at = np.flatnonzero(g[r] != w[r])
        lines.append(f"  row {r} ({role}): {'; '.join(named) or 'equals no decoy'}; first differing element {at[0]}: got {g[r][at[0]]}, want {w[r][at[0]]}")
    return "\n".join(lines)


@dataclass
class Call:
    args: dict
    checks: List[Check]
    what: str = ""
    bigs: Dict[str, Big] = field(default_factory=dict)  # models whose plants go up before this call and are erased after it
    refill: Dict[str, int] = field(default_factory=dict)  # output buffers set to a byte before the call


@dataclass
class Case:
    id: str
    entry: str  # the C entry point(s)
    unit: str  # "byte", "signed", "unsigned"
    mark: int  # in that unit
    items: List[Item]
    calls: List[Call]
    bigs: Dict[str, Big] = field(default_factory=dict)  # filled and planted once
    arrays: Dict[str, np.ndarray] = field(default_factory=dict)  # small inputs, uploaded whole
    outputs: Dict[str, int] = field(default_factory=dict)  # name -> bytes
    across_first_elem: Optional[int] = None  # where the layout is free: mark_elems - ACROSS
    elem_bytes: int = 1
    definition: Optional[Callable[[], None]] = None  # compact data through two host definitions; raises on disagreement
    no_decoys: str = ""  # why a case has none (nothing is read or written at the index that passes the mark)
    scratch_bytes: int = 0  # what the library allocates for the call beside the caller's buffers, where that is large

    def live_bytes(self) -> int:
        per_call = max([sum(b.nbytes for name, b in c.bigs.items() if name not in self.bigs) for c in self.calls] or [0])  # (a call's model of a shared buffer is no allocation)
        return sum(b.nbytes for b in self.bigs.values()) + sum(a.nbytes for a in self.arrays.values()) + sum(self.outputs.values()) + per_call + self.scratch_bytes


def _roles_of(first: np.ndarray, last: np.ndarray, mark: int) -> List[str]:
    """first / last touched ELEMENT index of every row (last < first: touches nothing)."""
    return ["empty" if l < f else BELOW if l < mark else ABOVE if f >= mark else ACROSS_ROLE for f, l in zip(first.tolist(), last.tolist())]


def _items(roles, first, last, scale: int) -> List[Item]:
    return [Item(r, int(f) * scale, int(l) * scale + scale - 1) for r, f, l in zip(roles, first.tolist(), last.tolist()) if r != "empty"]


def _rand(rng, count: int, dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    if dtype == np.uint8:
        return rng.randint(0, 256, size=count).astype(np.uint8)
    if dtype == np.uint32:
        return rng.randint(0, 1 << 32, size=count, dtype=np.uint64).astype(np.uint32)
    v = rng.randint(0, 1 << 63, size=count, dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, size=count).astype(np.uint64)
    v[::3] >>= np.uint64(33)  # a third of the values in the range of sha1_hash32
    return v


# ---- CSR corpora: mhx_minhash_bulk_dev, mhx_hll_bulk_dev -------------------------------------------------------------------------
CSR_SHAPES = ("long", "tiny")


def csr_corpus(dtype, unit: str, shape: str, seed: int):
    """(Big, offsets int64[n + 1] with offsets[across] == M - ACROSS, compact tokens, roles, items, mark in elements).
    "long": 12 sets of 300 .. 5000 tokens, which the MinHash launcher splits over waves; "tiny": 16 x CUs + 37 sets of 0 .. 40
    tokens with repeats, one wave (or less) per set."""
    rng = np.random.RandomState(seed)
    z = np.dtype(dtype).itemsize
    m = mark_elems(unit, z)
    if shape == "long":
        lens = rng.randint(300, 5001, size=12)
        across = 5
    else:
        lens = rng.randint(0, 41, size=16 * MI355X_CUS + 37)
        lens[::11] = 0
        across = lens.size // 2
        lens[across] = 40
    assert lens[across] > ACROSS
    offsets = np.zeros(lens.size + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    offsets += m - ACROSS - offsets[across]
    tokens = _rand(rng, int(lens.sum()), dtype)
    if shape == "tiny":  # repeated tokens inside a set: every third set draws from four values
        for i in range(0, lens.size, 3):
            s, e = offsets[i] - offsets[0], offsets[i + 1] - offsets[0]
            if e - s > 4:
                tokens[s:e] = tokens[s: s + 4][rng.randint(0, 4, size=e - s)]
    big = Big("hv", dtype, int(offsets[-1]), 0x5A)
    big.plant(int(offsets[0]), tokens)
    # a decoy token keeps 14 bits of the real one: another register (bit 0 flipped) with a rank no random hash reaches, another minimum
    big.plant_decoys(int(offsets[0]), tokens.size, lambda src: (src & np.dtype(dtype).type(0x3FFF)) ^ np.dtype(dtype).type(1))
    roles = _roles_of(offsets[:-1], offsets[1:] - 1, m)
    scale = z if unit == "byte" else 1
    return big, offsets, tokens, roles, _items(roles, offsets[:-1], offsets[1:] - 1, scale), m


def _csr_views(big: Big, offsets: np.ndarray, tokens: np.ndarray):
    """name -> (tokens as a kernel reading through that wrap would see them, which sets the wrap moves)."""
    views = {}
    for name, wrap in wraps(big.dtype.itemsize).items():
        seen = [big.read_wrapped(int(s), int(e - s), wrap) for s, e in zip(offsets[:-1], offsets[1:])]
        moved = np.array([e > s and big.moved(int(s), int(e - s), wrap) for s, e in zip(offsets[:-1], offsets[1:])])
        if moved.any():
            views[name] = (np.concatenate(seen), moved)
    return views


MINHASH_VARIANTS = [(64, np.uint32, False), (64, np.uint64, False), (128, np.uint32, False), (128, np.uint64, True), (256, np.uint32, False),
                    (256, np.uint64, False)]  # (num_perm, out dtype, with d_init): the three launch_typed families, both outputs


def minhash_cases() -> List[Case]:
    cases = []
    for dtype in (np.uint32, np.uint64):
        for unit in ("byte", "signed", "unsigned"):
            for shape in CSR_SHAPES:
                big, offsets, tokens, roles, items, m = csr_corpus(dtype, unit, shape, seed=len(cases) + 1)
                compact = offsets - offsets[0]
                views = _csr_views(big, offsets, tokens)
                n = offsets.size - 1
                calls = []
                for k, out_dtype, with_init in MINHASH_VARIANTS:
                    a, b = O.np_init_permutations(k, 3)
                    init = None
                    if with_init:  # a state per set, some of it below what the tokens reach
                        init = np.random.RandomState(k).randint(0, 1 << 32, size=(n, k), dtype=np.uint64)
                        init[:, ::2] >>= np.uint64(12)
                    want = O.c_minhash_bulk(tokens.astype(np.uint64), compact, a, b, init).astype(out_dtype)
                    decoys = {name: O.c_minhash_bulk(v.astype(np.uint64), compact, a, b, init).astype(out_dtype) for name, (v, _) in views.items()}
                    calls.append(Call(dict(num_perm=k, seed=3, out_dtype=np.dtype(out_dtype), init=init),
                                      [Check("out", 0, want, "signatures", roles, decoys, {name: mv for name, (_, mv) in views.items()})],
                                      what=f"num_perm={k} out={np.dtype(out_dtype).name}" + (" d_init" if with_init else ""), refill={"out": 0xEE}))

                def definition(tokens=tokens, compact=compact):
                    a, b = O.np_init_permutations(64, 3)
                    sets = [tokens[s:e] for s, e in zip(compact[:-1], compact[1:])]
                    np.testing.assert_array_equal(O.c_minhash_bulk(tokens.astype(np.uint64), compact, a, b), O.np_minhash_bulk(sets, a, b))

                cases.append(Case(f"mhx_minhash_bulk_dev-{np.dtype(dtype).name}-{unit}-{shape}", "mhx_minhash_bulk_dev", unit, MARKS[unit], items, calls,
                                  bigs={"hv": big}, arrays={"offsets": offsets}, outputs={"out": n * 256 * 8, "init": n * 256 * 8},
                                  across_first_elem=int(offsets[roles.index(ACROSS_ROLE)]),
                                  elem_bytes=np.dtype(dtype).itemsize, definition=definition))
    return cases


class _HyperLogLog64(hyperloglog.HyperLogLog):
    """The reference's update with the 64-bit hash range of its HyperLogLogPlusPlus (ref: hyperloglog.py:348)."""
    __slots__ = ()
    _hash_range_bit = 64


HLL_VARIANTS = [(np.uint32, 4, 32), (np.uint32, 14, 64), (np.uint64, 4, 64), (np.uint64, 14, 64)]  # (token dtype, p, hash_bits)


def hll_bulk_cases() -> List[Case]:
    cases = []
    for dtype in (np.uint32, np.uint64):
        for unit in ("byte", "signed", "unsigned"):
            for shape in CSR_SHAPES:
                big, offsets, tokens, roles, items, m = csr_corpus(dtype, unit, shape, seed=100 + len(cases))
                compact = offsets - offsets[0]
                views = _csr_views(big, offsets, tokens)
                n = offsets.size - 1
                calls = []
                for tok, p, bits in HLL_VARIANTS:
                    if np.dtype(tok) != np.dtype(dtype):
                        continue
                    want = hyperloglog._registers_host(tokens, compact, 0, n, p, bits, None)
                    decoys = {name: hyperloglog._registers_host(v, compact, 0, n, p, bits, None) for name, (v, _) in views.items()}
                    checks = []
                    pieces = [(lo, min(n, lo + (MAX_DOWNLOAD_BYTES >> p))) for lo in range(0, n, MAX_DOWNLOAD_BYTES >> p)]  # every row, at most 64 MB at a time
                    if shape == "tiny" and p == 14 and unit != "unsigned":  # 68 MB of registers: all of them at one mark per token type,
                        mid = roles.index(ACROSS_ROLE)                        # at the others the first, the last and the 1200 sets around the mark
                        pieces = [(0, 200), (mid - 600, mid + 600), (n - 200, n)]
                    for lo, hi in pieces:
                        moved = {nm: mv[lo:hi] for nm, (_, mv) in views.items() if mv[lo:hi].any()}
                        checks.append(Check("out", lo << p, want[lo:hi], f"registers of sets {lo} .. {hi - 1}", roles[lo:hi],
                                            {nm: decoys[nm][lo:hi] for nm in moved}, moved))
                    calls.append(Call(dict(p=p, hash_bits=bits), checks, what=f"p={p} hash_bits={bits}", refill={"out": 0xEE}))

                def definition(tokens=tokens, compact=compact, dtype=dtype):
                    bits = 32 if np.dtype(dtype) == np.uint32 else 64
                    got = hyperloglog._registers_host(tokens, compact, 0, compact.size - 1, 8, bits, None)
                    for i in (0, compact.size // 2, compact.size - 2):  # the reference's object, one update per token
                        h = (hyperloglog.HyperLogLog if bits == 32 else _HyperLogLog64)(p=8, hashfunc=lambda x: x, gpu_mode="disable")
                        for t in tokens[compact[i]: compact[i + 1]].tolist():
                            h.update(t)
                        np.testing.assert_array_equal(np.asarray(h.reg).view(np.uint8), got[i])

                cases.append(Case(f"mhx_hll_bulk_dev-{np.dtype(dtype).name}-{unit}-{shape}", "mhx_hll_bulk_dev", unit, MARKS[unit], items, calls,
                                  bigs={"hv": big}, arrays={"offsets": offsets}, outputs={"out": n << 14, "overflow": 8},
                                  across_first_elem=int(offsets[roles.index(ACROSS_ROLE)]), elem_bytes=np.dtype(dtype).itemsize,
                                  definition=definition))
    return cases


# ---- mhx_sha1_tokens_dev: byte offsets around 2^32 -----------------------------------------------------------------------------
SHA1_LENGTHS = (0, 1, 55, 56, 64, 119)  # empty, one byte, the last one-block message, the first two-block one, a full block, the last two-block one


def _sha1(data: bytes, dtype) -> int:
    digest = hashlib.sha1(data).digest()
    return int.from_bytes(digest[: np.dtype(dtype).itemsize], "little")


def sha1_tokens_cases() -> List[Case]:
    rng = np.random.RandomState(11)
    group = list(SHA1_LENGTHS) + [2]  # 297 bytes: every group starts one byte further into its dword than the one before
    before = group * 4
    lens = before + [3] + [119] + group * 4  # the 119-byte token starts at M - ACROSS
    across = len(before) + 1
    offsets = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    offsets += MARKS["byte"] - ACROSS - offsets[across]
    seen = {(n, int(s) % 4, s >= MARKS["byte"]) for n, s in zip(lens, offsets[:-1])}
    assert all((n, al, side) in seen for n in SHA1_LENGTHS for al in range(4) for side in (False, True))
    data = _rand(rng, int(offsets[-1] - offsets[0]), np.uint8)
    big = Big("bytes", np.uint8, int(offsets[-1]), 0x20)
    big.plant(int(offsets[0]), data)
    big.plant_decoys(int(offsets[0]), data.size, lambda src: src ^ np.uint8(0xA5))
    roles = _roles_of(offsets[:-1], offsets[1:] - 1, MARKS["byte"])
    spans = list(zip(offsets[:-1].tolist(), offsets[1:].tolist()))
    calls = []
    for out_dtype in (np.uint32, np.uint64):
        want = np.array([_sha1(big.read(s, e - s).tobytes(), out_dtype) for s, e in spans], dtype=out_dtype)
        decoys, moved = {}, {}
        for name, wrap in wraps(1).items():
            mv = np.array([e > s and big.moved(s, e - s, wrap) for s, e in spans])
            if mv.any():
                decoys[name] = np.array([_sha1(big.read_wrapped(s, e - s, wrap).tobytes(), out_dtype) for s, e in spans], dtype=out_dtype)
                moved[name] = mv
        calls.append(Call(dict(out_dtype=np.dtype(out_dtype)), [Check("out", 0, want, "hashes", roles, decoys, moved)],
                          what=f"out={np.dtype(out_dtype).name}", refill={"out": 0xEE}))

    def definition():
        from datasketch_amd.hashfunc import sha1_hash32, sha1_hash64
        for s, e in spans:
            tok = big.read(s, e - s).tobytes()
            assert sha1_hash32(tok) == _sha1(tok, np.uint32) and sha1_hash64(tok) == _sha1(tok, np.uint64)

    items = [Item(r, s, e - 1) for r, (s, e) in zip(roles, spans) if r != "empty"]
    return [Case("mhx_sha1_tokens_dev-byte", "mhx_sha1_tokens_dev", "byte", MARKS["byte"], items, calls, bigs={"bytes": big},
                 arrays={"offsets": offsets}, outputs={"out": len(lens) * 8}, across_first_elem=int(offsets[across]), definition=definition)]


# ---- listed pairs of sets: mhx_overlap_pairs_dev -------------------------------------------------------------------------------
def overlap_lds_max_items(key_bytes: int, lds_per_block: int) -> int:
    """mhx_overlap_limits (include/mhx.h) restated, so that building the cases loads no library: the most items of a pair whose
    table -- a 64-byte header, the power of two >= max(64, 2 items) of keys, two bits per slot -- fits lds_per_block bytes."""
    slots = 64
    while 64 + 2 * slots * key_bytes + 2 * slots // 4 <= lds_per_block:
        slots *= 2
    return slots // 2 if 64 + slots * key_bytes + slots // 4 <= lds_per_block else 0


def overlap_cases() -> List[Case]:
    """One call per key width: clusters of sets at the byte mark, at 2^31 and at 2^32 elements, giant unlisted gap sets between
    them, and listed pairs of every class -- a wave pair, an LDS workgroup pair, a scratch pair -- that name sets at every mark."""
    cases = []
    for dtype in (np.uint32, np.uint64):
        rng = np.random.RandomState(29 + np.dtype(dtype).itemsize)
        z = np.dtype(dtype).itemsize
        bits = 8 * z
        limit = overlap_lds_max_items(z, MI355X_LDS_PER_BLOCK)
        marks = sorted({mark_elems(u, z) for u in MARKS})
        top = np.iinfo(dtype).max
        pool = _rand(rng, 4 * limit, dtype)
        # per mark: [below small, below LDS, across (starts at M - ACROSS), above small, above LDS, above with the all-ones key, above scratch]
        sizes = [200, 3000, 260, 240, 2500, 64, limit + 500]
        lens, starts, cluster_of = [], [], []
        cursor = 0
        for c, m in enumerate(marks):
            first = m - ACROSS - sizes[0] - sizes[1]
            assert first > cursor
            lens.append(first - cursor)  # the gap set: never listed, never followed
            starts.append(cursor)
            cluster_of.append(-1)
            cursor = first
            for s in sizes:
                lens.append(s)
                starts.append(cursor)
                cluster_of.append(c)
                cursor += s
        offsets = np.array(starts + [cursor], dtype=np.int64)
        big = Big("hv", dtype, cursor, 0x5A)
        sets = {}
        for i, (s, n, c) in enumerate(zip(starts, lens, cluster_of)):
            if c < 0:
                continue
            at = rng.randint(0, pool.size - n)
            vals = pool[at: at + n].copy()  # stretches of one pool: the sets overlap
            vals[rng.randint(0, n, n // 5)] = vals[0]  # and repeat values
            if n == 64:
                vals[7] = top  # the all-ones key: the empty value of the hash table
            sets[i] = vals
            big.plant(s, vals)
        for i, vals in sets.items():
            big.plant_decoys(starts[i], vals.size, lambda src: _rand(rng, src.size, dtype))
        per = len(sizes) + 1
        idx = lambda c, j: c * per + 1 + j  # noqa: E731  set j of cluster c
        last = len(marks) - 1
        pairs = []
        for c in range(len(marks)):
            pairs += [[idx(c, 0), idx(c, 3)], [idx(c, 3), idx(c, 2)], [idx(c, 3), idx(c, 5)],  # wave pairs: (below, above), (above, across), (above, above)
                      [idx(c, 1), idx(c, 4)], [idx(c, 4), idx(c, 2)],  # LDS workgroup pairs
                      [idx(c, 5), idx(c, 5)], [idx(c, 2), idx(c, 2)]]  # i == j
        pairs += [[idx(last, 6), idx(0, 4)], [idx(0, 0), idx(last, 3)], [idx(0, 6), idx(last, 6)]]  # scratch pairs; below the lowest with above the highest
        pairs = np.array(pairs, dtype=np.int64)
        used = np.unique(pairs)
        totals = np.array([lens[i] + lens[j] for i, j in pairs])
        assert (totals <= 512).any() and ((totals > 512) & (totals <= limit)).any() and (totals > limit).any()

        def counts_of(read):
            got = {i: set(read(starts[i], lens[i]).tolist()) for i in used.tolist()}
            return np.array([(len(got[i] & got[j]), len(got[i]), len(got[j])) for i, j in pairs.tolist()], dtype=np.int32)

        want = counts_of(big.read)
        decoys, moved = {}, {}
        for name, wrap in wraps(z).items():
            mv = np.array([big.moved(starts[i], lens[i], wrap) or big.moved(starts[j], lens[j], wrap) for i, j in pairs.tolist()])
            if mv.any():
                decoys[name] = counts_of(lambda s, n, wrap=wrap: big.read_wrapped(s, n, wrap))
                moved[name] = mv
        first = np.array(starts)[used]
        lastx = first + np.array(lens)[used] - 1
        # a pair is as high as its highest set, and straddles if one of its sets does
        set_role = dict(zip(used.tolist(), _roles_of(first, lastx, marks[-1])))
        roles = [ACROSS_ROLE if ACROSS_ROLE in (set_role[i], set_role[j]) else ABOVE if ABOVE in (set_role[i], set_role[j]) else BELOW for i, j in pairs.tolist()]
        items = _items([set_role[i] for i in used.tolist()], first, lastx, 1)

        def definition(used=used, big=big, starts=starts, lens=lens, pairs=pairs, want=want):
            remap = {i: r for r, i in enumerate(used.tolist())}
            flat = [big.read(starts[i], lens[i]) for i in used.tolist()]
            off = np.zeros(len(flat) + 1, dtype=np.int64)
            np.cumsum([f.size for f in flat], out=off[1:])
            local = np.array([[remap[i], remap[j]] for i, j in pairs.tolist()], dtype=np.int64)
            np.testing.assert_array_equal(overlap.overlap_counts_host(np.concatenate(flat), off, local), want)

        cases.append(Case(f"mhx_overlap_pairs_dev-{np.dtype(dtype).name}", "mhx_overlap_pairs_dev", "unsigned", marks[-1], items,
                          [Call(dict(max_set_items=max(sizes)), [Check("counts", 0, want, "counts", roles, decoys, moved),
                                                                 Check("invalid", 0, np.zeros(1, dtype=np.int64), "invalid pairs")], refill={"counts": 0xEE})],
                          bigs={"hv": big}, arrays={"offsets": offsets, "pairs": pairs, "invalid": np.zeros(1, dtype=np.int64)},
                          outputs={"counts": pairs.shape[0] * 12}, across_first_elem=starts[idx(last, 2)], elem_bytes=z, definition=definition))
    return cases


# ---- listed pairs of rows: mhx_jaccard_pairs_dev_typed, mhx_bbit_jaccard_pairs_dev ------------------------------------------------
def _rows_around(marks, width: int):
    """Per mark the rows -2 .. +2 around the row that holds element M (for widths that divide M, that row starts at M)."""
    return sorted({m // width + d for m in marks for d in (-2, -1, 0, 1, 2)})


def _row_pairs(rows, marks, width):
    out = []
    for m in marks:
        r = m // width
        out += [[r - 2, r + 1], [r + 1, r if r * width < m else r - 1], [r + 1, r + 2], [r + 2, r - 1]]  # (below, above), (above, across or the last below), (above, above), (above, below)
    out.append([marks[0] // width - 2, marks[-1] // width + 2])
    return np.array(out, dtype=np.int64)


def _pair_case(case_id, entry, dtype, widths_and_args, count, what, clean=lambda row, args: row):
    """A matrix of rows of ``width`` elements (several widths over one buffer, one call each); count(rows_a, rows_b, args);
    clean(random row, args) makes it a valid row of the entry."""
    z = np.dtype(dtype).itemsize
    marks = sorted({mark_elems(u, z) for u in MARKS})
    calls, items, n_max = [], [], 0
    for width, args in widths_and_args:
        rng = np.random.RandomState(width + 7 * len(calls))
        rows = _rows_around(marks, width)
        n_rows = rows[-1] + 1
        n_max = max(n_max, n_rows * width)
        big = Big("sig", dtype, n_rows * width, 0x5A)
        base = _rand(rng, width, dtype)
        for r in rows:  # near-copies of one row, so that counts are neither 0 nor width
            row = base.copy()
            flip = rng.random_sample(width) < 0.4
            row[flip] = _rand(rng, int(flip.sum()), dtype)
            big.plant(r * width, clean(row, args))

        def decoy(src):
            """Half of a whole row kept, half redrawn, made a valid row again; a piece of a row cut at a wrap boundary redrawn."""
            if src.size != width:
                return _rand(rng, src.size, dtype)
            mixed = np.where(rng.random_sample(width) < 0.5, src, _rand(rng, width, dtype)).astype(dtype)
            return clean(mixed, args)

        for r in rows:
            big.plant_decoys(r * width, width, decoy)
        pairs = _row_pairs(rows, marks, width)
        want = count(np.stack([big.read(i * width, width) for i in pairs[:, 0]]), np.stack([big.read(j * width, width) for j in pairs[:, 1]]), args)
        decoys, moved = {}, {}
        for name, wrap in wraps(z).items():
            mv = np.array([big.moved(i * width, width, wrap) or big.moved(j * width, width, wrap) for i, j in pairs.tolist()])
            if mv.any():
                decoys[name] = count(np.stack([big.read_wrapped(i * width, width, wrap) for i in pairs[:, 0]]),
                                     np.stack([big.read_wrapped(j * width, width, wrap) for j in pairs[:, 1]]), args).astype(np.int32)
                moved[name] = mv
        first = np.array(rows) * width
        row_role = dict(zip(rows, _roles_of(first, first + width - 1, marks[-1])))
        roles = [ACROSS_ROLE if ACROSS_ROLE in (row_role[i], row_role[j]) else ABOVE if ABOVE in (row_role[i], row_role[j]) else BELOW for i, j in pairs.tolist()]
        items += _items([row_role[r] for r in rows], first, first + width - 1, 1)
        calls.append(Call(dict(args, width=width, pairs=pairs), [Check("counts", 0, want.astype(np.int32), "counts", roles, decoys, moved)],
                          what=f"{what(args)} rows of {width} elements", bigs={"sig": big}, refill={"counts": 0xEE}))
    shell = Big("sig", dtype, n_max, 0x5A)  # allocated and filled once; every call plants its own rows and erases them

    def definition():
        for call in calls:
            big, width, pairs = call.bigs["sig"], call.args["width"], call.args["pairs"]
            a = np.stack([big.read(i * width, width) for i in pairs[:, 0]])
            b = np.stack([big.read(j * width, width) for j in pairs[:, 1]])
            np.testing.assert_array_equal(call.checks[0].expected, np.array([int(np.count_nonzero(x == y)) for x, y in zip(
                *(_positions(a, call.args), _positions(b, call.args)))], dtype=np.int32))

    return Case(case_id, entry, "unsigned", marks[-1], items, calls, bigs={"sig": shell}, outputs={"counts": 64 * 4, "pairs": 64 * 16}, elem_bytes=z,
                definition=definition)


def _positions(rows: np.ndarray, args: dict) -> np.ndarray:
    """The values MinHash.jaccard / bBitMinHash.jaccard compare position by position."""
    if "b" not in args:
        return rows
    return b_bit_minhash._unpack_rows(rows, b_bit_minhash._slot_size(args["b"]), args["num_perm"])


def jaccard_pairs_cases() -> List[Case]:
    plain = lambda a, b, args: np.count_nonzero(a == b, axis=1)  # noqa: E731  (lsh_bulk.jaccard_pairs, gpu_mode="disable")
    return [_pair_case(f"mhx_jaccard_pairs_dev_typed-{np.dtype(dt).name}", "mhx_jaccard_pairs_dev_typed", dt,
                       [(256, dict(num_perm=256)), (100, dict(num_perm=100))], plain, lambda args: f"k={args['num_perm']}") for dt in (np.uint32, np.uint64)]


def bbit_jaccard_pairs_cases() -> List[Case]:
    def agree(a, b, args):  # (b_bit_minhash.jaccard_pairs, gpu_mode="disable": unpack and compare)
        slot = b_bit_minhash._slot_size(args["b"])
        return np.count_nonzero(b_bit_minhash._unpack_rows(a, slot, args["num_perm"]) == b_bit_minhash._unpack_rows(b, slot, args["num_perm"]), axis=1)

    shapes = []
    for k in (256, 100):
        for b in (1, 4, 32):
            slot = b_bit_minhash._slot_size(b)
            shapes.append((-(-k // (64 // slot)), dict(num_perm=k, b=b)))
    def packed(row, args):  # what mhx_bbit_pack* writes: values of b bits in their slots, the slots past num_perm zero
        slot = b_bit_minhash._slot_size(args["b"])
        vals = b_bit_minhash._unpack_rows(row[None, :], slot, args["num_perm"]) & np.uint64((1 << args["b"]) - 1)
        return b_bit_minhash._pack_rows(vals, slot)[0]

    return [_pair_case("mhx_bbit_jaccard_pairs_dev", "mhx_bbit_jaccard_pairs_dev", np.uint64, shapes, agree, lambda args: f"k={args['num_perm']} b={args['b']}", packed)]


# ---- mhx_rows_compact_dev ------------------------------------------------------------------------------------------------------
def rows_compact_cases() -> List[Case]:
    """n_rows x row_bytes just past 2^32 bytes; five live rows around the mark, so dst is a few KB and n_kept exact.  (With 48-byte
    rows the 16-byte UNIT index passes 2^32 only at 64 GiB of source: beyond the budget of a case, left out.)"""
    cases = []
    m = MARKS["byte"]
    for row_bytes in (1024, 48):
        rng = np.random.RandomState(row_bytes)
        r = m // row_bytes
        rows = [r - 2, r - 1, r, r + 1, r + 2]
        n_rows = r + 5
        big = Big("src", np.uint8, n_rows * row_bytes, 0x5A)
        for x in rows:
            big.plant(x * row_bytes, _rand(rng, row_bytes, np.uint8))
        for x in rows:
            big.plant_decoys(x * row_bytes, row_bytes, lambda src: _rand(rng, src.size, np.uint8))
        live = np.zeros(-(-n_rows // 32), dtype=np.uint32)
        for x in rows:
            live[x >> 5] |= np.uint32(1 << (x & 31))
        want = np.stack([big.read(x * row_bytes, row_bytes) for x in rows])
        decoys = {name: np.stack([big.read_wrapped(x * row_bytes, row_bytes, wrap) for x in rows]) for name, wrap in wraps(1).items()}
        moved = {name: np.array([big.moved(x * row_bytes, row_bytes, wrap) for x in rows]) for name, wrap in wraps(1).items()}
        first = np.array(rows) * row_bytes
        roles = _roles_of(first, first + row_bytes - 1, m)

        def definition(live=live, rows=rows, n_rows=n_rows):
            bits = np.unpackbits(live.view(np.uint8), bitorder="little")[:n_rows]
            assert np.flatnonzero(bits).tolist() == rows and np.array_equal(lsh_bulk.live_bits(bits.astype(bool)), live)

        cases.append(Case(f"mhx_rows_compact_dev-row_bytes{row_bytes}", "mhx_rows_compact_dev", "byte", m, _items(roles, first, first + row_bytes - 1, 1),
                          [Call(dict(row_bytes=row_bytes, n_rows=n_rows, n_kept=len(rows)), [Check("dst", 0, want, "kept rows", roles, decoys, moved)],
                                refill={"dst": 0xEE})], bigs={"src": big}, arrays={"live": live}, outputs={"dst": len(rows) * row_bytes},
                          definition=definition))
    return cases


# ---- connected components over 2^32 - 1 rows -----------------------------------------------------------------------------------------
def cc_cases() -> List[Case]:
    """mhx_cc_init_dev, mhx_cc_link_pairs_dev, mhx_cc_finish_dev on the largest label array the entries accept.  200 edges among rows
    within 64 of 0, of 2^31 and of 2^32 - 2.  The rows used near 0 are below 24 and the high rows used are at least 24 past a multiple
    of 2^31, so a row number cut to 31 bits lands on a label near 0 that nothing else touches: that slice is the wrapped location."""
    rng = np.random.RandomState(5)
    n = (1 << 32) - 1
    low = np.arange(0, 24)
    mid = np.concatenate([(1 << 31) - 64 + np.arange(0, 40), (1 << 31) + 24 + np.arange(0, 40)])
    high = (1 << 31) + (1 << 31) - 2 - np.arange(0, 36)  # 2^32 - 2 downwards: 2^31 + (2^31 - 38 .. 2^31 - 2)
    pools = [low, mid, high]
    edges = []
    for p in pools:
        for _ in range(60):
            edges.append([rng.choice(p), rng.choice(p)])
    edges += [[3, (1 << 31) + 30], [(1 << 31) + 30, (1 << 32) - 2], [(1 << 31) - 1, (1 << 31) + 24], [(1 << 32) - 2, (1 << 32) - 3], [5, 5],
              [(1 << 31) + 63, (1 << 31) - 64]]  # a path that joins a low and a high row, a pair across 2^31, the last row, i == j, i > j
    edges += [[rng.choice(mid), rng.choice(mid)] for _ in range(200 - len(edges))]
    edges = np.array(edges, dtype=np.int64)
    assert edges.shape == (200, 2)

    def labels_of(e):
        touched = np.unique(e)
        local = np.searchsorted(touched, e)  # monotone, so the smallest row of a component stays the smallest
        comp = lsh_bulk.connected_components(local, touched.size, gpu_mode="disable")
        return dict(zip(touched.tolist(), touched[comp].tolist()))

    def slices_of(lab):
        out = []
        for start, count in ((0, 128), ((1 << 31) - 64, 128), (n - 128, 128), ((1 << 30) + 12345, 1 << 20), (3 << 30, 1 << 20)):
            want = np.arange(start, start + count, dtype=np.uint32)
            for row, label in lab.items():
                if start <= row < start + count:
                    want[row - start] = label
            out.append((start, want))
        return out

    real = labels_of(edges)
    cut = labels_of(edges % (1 << 31))  # row numbers cut to 31 bits
    checks = []
    for (start, want), (_, other) in zip(slices_of(real), slices_of(cut)):
        roles = [BELOW if start + want.size <= (1 << 31) else ABOVE if start >= (1 << 31) else ACROSS_ROLE]
        chk = Check("labels", start * 4, want, f"labels[{start} .. {start + want.size})", roles)
        if start == 0:
            chk.decoys, chk.moved = {"index mod 2^31": other}, {"index mod 2^31": np.array([True])}
        checks.append(chk)
    touched = np.unique(edges)
    items = [Item(BELOW if r < (1 << 31) else ABOVE, int(r), int(r)) for r in touched.tolist()]
    items.append(Item(ACROSS_ROLE, (1 << 31) - 1, (1 << 31) + 24))  # the edge whose ends lie on both sides

    def definition():
        parent = {r: r for r in touched.tolist()}

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x
        for u, v in edges.tolist():
            ru, rv = find(u), find(v)
            parent[max(ru, rv)] = min(ru, rv)
        assert {r: find(r) for r in parent} == real

    return [Case("mhx_cc_init_dev-mhx_cc_link_pairs_dev-mhx_cc_finish_dev", "mhx_cc", "signed", MARKS["signed"], items,
                 [Call(dict(n=n), checks)], arrays={"pairs": edges, "invalid": np.zeros(1, dtype=np.int64)}, outputs={"labels": n * 4}, elem_bytes=4,
                 definition=definition)]


# ---- streaming: mhx_hll_merge_dev ------------------------------------------------------------------------------------------------
def hll_merge_cases() -> List[Case]:
    """count = 2^32 + 4099 bytes: a is 3 and b is 5 everywhere but on planted stretches where a is larger or random, at 0, across the
    mark, above it and on the ragged tail.  The result is 5 wherever nothing is planted: slices on each side of the mark say so, and
    the wrapped images of the planted stretches must hold 5 too."""
    rng = np.random.RandomState(17)
    m = MARKS["byte"]
    count = m + 4099
    a, b = Big("a", np.uint8, count, 3), Big("b", np.uint8, count, 5)
    spans = [(0, 300), (m - ACROSS, 301), (m + 1024 + 13, 299), (count - 67, 67)]
    for s, n in spans:
        a.plant(s, rng.randint(0, 64, size=n).astype(np.uint8))
        b.plant(s, rng.randint(0, 64, size=n).astype(np.uint8))
    checks = []
    for start, n in [(0, 1 << 16), (m - (1 << 16), (1 << 16) + 4099), (1 << 31, 1 << 16)]:
        want = np.maximum(a.read(start, n), b.read(start, n))
        roles = _roles_of(np.array([start]), np.array([start + n - 1]), m)
        checks.append(Check("a", start, want, f"a[{start} .. {start + n})", roles))
    # a kernel that wrapped would write (or read) the stretch across the mark at byte 0 ..: the first check covers that image too
    items = [Item(_roles_of(np.array([s]), np.array([s + n - 1]), m)[0], s, s + n - 1) for s, n in spans]

    def definition():
        for s, n in spans:
            x, y = a.read(s, 64).reshape(4, 16), b.read(s, 64).reshape(4, 16)  # four sketches of p = 4
            np.testing.assert_array_equal(hyperloglog.merge_many(x, y, gpu_mode="disable").view(np.uint8), np.maximum(a.read(s, 64), b.read(s, 64)).reshape(4, 16))

    first = checks[0]
    seen = a.read(0, first.expected.size).copy()
    seen[: 301 - ACROSS] = np.maximum(a.read(m, 301 - ACROSS), b.read(m, 301 - ACROSS))
    first.decoys = {"index mod 2^32": np.maximum(seen, b.read(0, seen.size))}
    first.moved = {"index mod 2^32": np.array([True])}
    return [Case("mhx_hll_merge_dev-byte", "mhx_hll_merge_dev", "byte", m, items, [Call(dict(count=count), checks)], bigs={"a": a, "b": b},
                 across_first_elem=m - ACROSS, definition=definition)]


# ---- streaming over a signature matrix uint32 [2^24 + 3, 256]: the pack / digest / serialize family and its inverses ---------------
STREAM_K, STREAM_N = 256, (1 << 24) + 3
ROW_MAJOR, BAND_MAJOR = 0, 1


@dataclass
class Out:
    """One output of a streaming call: ``f(signature rows [m, 256])`` gives its rows [m, w] -- a row-wise function, so the
    result for a filler row comes from one filler row.  BAND_MAJOR: stored as [w, n]."""
    name: str
    dtype: type
    w: int
    f: Callable[[np.ndarray], np.ndarray]
    layout: int = ROW_MAJOR
    decoys: bool = True  # the call reads the signature matrix itself (a later stage reads an earlier output)


def _merge(windows, n):
    out = []
    for lo, hi in sorted((max(lo, 0), min(hi, n)) for lo, hi in windows):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        elif lo < hi:
            out.append([lo, hi])
    return [tuple(w) for w in out]


def _stream_case(case_id, entry, stages, seed, definition):
    """stages: [(C entry, args, [Out, ...])] run in order on one signature matrix.  Rows are planted at 0, around the row of every
    mark of the input and of every output (the row that holds M - 1, the one that holds M, the next) and at the end; everything
    else is the fill.  Every planted row is checked with two filler rows on each side, and so is every place where a 32-bit wrap
    of an output index of a planted row would land."""
    rng = np.random.RandomState(seed)
    k, n = STREAM_K, STREAM_N
    sig = Big("sig", np.uint32, n * k, 0x5A)
    rows = {0, 1, n - 1}
    for u in MARKS:
        r = mark_elems(u, 4) // k
        rows |= {r - 1, r, r + 1}
    outs = [o for _, _, os_ in stages for o in os_]
    for o in outs:
        z = np.dtype(o.dtype).itemsize
        for u in MARKS:
            m = mark_elems(u, z)
            r = m // o.w if o.layout == ROW_MAJOR else m % n if m // n < o.w else n
            rows |= {x for x in (r - 1, r, r + 1) if 0 <= x < n}
    rows = sorted(rows)
    for r in rows:
        sig.plant(r * k, _rand(rng, k, np.uint32))
    for r in rows:
        sig.plant_decoys(r * k, k, lambda src: src ^ np.uint32(0x9E3779B1))
    windows = [(r - 2, r + 3) for r in rows]
    for o in outs:  # where a wrapped write of a planted row's output would land
        if o.layout == ROW_MAJOR:
            for r in rows:
                for wrap in wraps(np.dtype(o.dtype).itemsize).values():
                    r2 = wrap(r * o.w) // o.w
                    if r2 != r:
                        windows.append((r2 - 1, r2 + 2))
    windows = _merge(windows, n)
    top = mark_elems("unsigned", 4)

    def model(r0, r1, wrap=None):
        return np.stack([sig.read(r * k, k) if wrap is None else sig.read_wrapped(r * k, k, wrap) for r in range(r0, r1)])

    calls = []
    for fn, args, os_ in stages:
        checks = []
        for o in os_:
            z = np.dtype(o.dtype).itemsize
            for r0, r1 in windows:
                want = np.ascontiguousarray(o.f(model(r0, r1))).astype(o.dtype, copy=False).reshape(r1 - r0, o.w)
                first = np.arange(r0, r1) * k
                roles = [role if r in rows else "filler" for r, role in zip(range(r0, r1), _roles_of(first, first + k - 1, top))]
                if o.layout == BAND_MAJOR:  # band j of the rows r0 .. r1 lies at j * n + r0: the first band, the last, those at a mark
                    bands = {0, o.w - 1} | {mark_elems(u, z) // n for u in MARKS if mark_elems(u, z) // n < o.w}
                    for j in sorted(bands):
                        checks.append(Check(o.name, (j * n + r0) * z, np.ascontiguousarray(want[:, j]), f"{o.name} band {j} rows {r0} .. {r1 - 1}"))
                    continue
                decoys, moved = {}, {}
                if o.decoys:
                    for name, wrap in wraps(4).items():
                        mv = np.array([not np.array_equal(sig.read_wrapped(r * k, k, wrap), sig.read(r * k, k)) for r in range(r0, r1)])  # (a filler row's image is mostly filler)
                        if mv.any():
                            decoys[name] = np.ascontiguousarray(o.f(model(r0, r1, wrap))).astype(o.dtype, copy=False).reshape(r1 - r0, o.w)
                            moved[name] = mv
                checks.append(Check(o.name, r0 * o.w * z, want, f"{o.name} rows {r0} .. {r1 - 1}", roles, decoys, moved))
        calls.append(Call(dict(args, fn=fn, n=n, k=k), checks, what=fn + "".join(f" {a}={v}" for a, v in args.items()), refill={o.name: 0xEE for o in os_}))
    first = np.array(rows) * k
    roles = _roles_of(first, first + k - 1, top)
    outputs = {}
    for o in outs:
        outputs[o.name] = max(outputs.get(o.name, 0), n * o.w * np.dtype(o.dtype).itemsize)
    return Case(case_id, entry, "unsigned", MARKS["unsigned"], _items(roles, first, first + k - 1, 1), calls, bigs={"sig": sig}, outputs=outputs, elem_bytes=4,
                definition=lambda: definition(np.stack([sig.read(r * k, k) for r in rows[:6]])))


def _pack8(rows):
    return b_bit_minhash.pack_matrix(rows, 8, gpu_mode="disable")


def _digests(rows):
    return lsh_bulk.band_digests(rows.astype(np.uint64), 32, 8, gpu_mode="disable")


def _lean(rows, seed, big_endian):
    from datasketch_amd import lean_minhash
    if not big_endian:
        return lean_minhash.serialize_matrix(rows, seed, gpu_mode="disable")
    import struct
    out = np.empty((rows.shape[0], 12 + 4 * rows.shape[1]), dtype=np.uint8)
    out[:, :12] = np.frombuffer(struct.pack(">qi", seed, rows.shape[1]), dtype=np.uint8)
    out[:, 12:] = rows.astype(">u4").view(np.uint8).reshape(rows.shape[0], -1)
    return out


LEAN_SEED = 0x0123456789ABCDEF


def stream_cases() -> List[Case]:
    def pack_definition(rows):
        np.testing.assert_array_equal(_pack8(rows), O.np_bbit_pack(rows.astype(np.uint64), 8))
        np.testing.assert_array_equal(b_bit_minhash.unpack_matrix(_pack8(rows), STREAM_K, 8, gpu_mode="disable"), rows & np.uint32(0xFF))

    def digest_definition(rows):
        keys = lsh_bulk.band_keys(rows.astype(np.uint64), 32, 8, gpu_mode="disable")
        want = np.array([[lsh_bulk.fnv1a_64(bytes(keys[i, j])) for j in range(32)] for i in range(rows.shape[0])], dtype=np.uint64)
        np.testing.assert_array_equal(_digests(rows), want)

    def lean_definition(rows):
        from datasketch_amd import lean_minhash
        for order, big_endian in (("<", False), (">", True)):
            recs = _lean(rows, LEAN_SEED, big_endian)
            for row, rec in zip(rows, recs):
                assert rec.tobytes() == O.np_lean_serialize(row, LEAN_SEED, order)
            seeds, back = lean_minhash.deserialize_matrix(recs, STREAM_K, order, gpu_mode="disable")
            assert (seeds == LEAN_SEED).all() and np.array_equal(back, rows)

    unpacked = lambda rows: rows & np.uint32(0xFF)  # noqa: E731
    fused = [("mhx_bbit_pack_band_digests_dev", dict(b=8, bands=32, r=8, layout=layout),
              [Out("blocks", np.uint64, 32, _pack8), Out("digests", np.uint64, 32, _digests, layout)]) for layout in (ROW_MAJOR, BAND_MAJOR)]
    lean = []
    for order in (0, 1):
        lean += [("mhx_lean_serialize_dev_typed", dict(seed=LEAN_SEED, byteorder=order), [Out("records", np.uint8, 12 + 4 * STREAM_K, lambda rows, order=order: _lean(rows, LEAN_SEED, order))]),
                 ("mhx_lean_deserialize_dev", dict(byteorder=order), [Out("sig2", np.uint32, STREAM_K, lambda rows: rows, decoys=False),
                                                                       Out("seeds", np.int64, 1, lambda rows: np.full((rows.shape[0], 1), LEAN_SEED, dtype=np.int64), decoys=False)])]
    return [
        _stream_case("mhx_bbit_pack_dev_typed-mhx_bbit_unpack_dev", "stream",
                     [("mhx_bbit_pack_dev_typed", dict(b=8), [Out("blocks", np.uint64, 32, _pack8)]),
                      ("mhx_bbit_unpack_dev", dict(b=8), [Out("unpacked", np.uint32, STREAM_K, unpacked, decoys=False)])], 41, pack_definition),
        _stream_case("mhx_band_digests_dev_typed-mhx_band_digests_layout_dev", "stream",
                     [("mhx_band_digests_dev_typed", dict(bands=32, r=8), [Out("digests", np.uint64, 32, _digests)]),
                      ("mhx_band_digests_layout_dev", dict(bands=32, r=8, layout=BAND_MAJOR), [Out("digests", np.uint64, 32, _digests, BAND_MAJOR)])], 42, digest_definition),
        _stream_case("mhx_bbit_pack_band_digests_dev", "stream", fused, 43, lambda rows: (pack_definition(rows), digest_definition(rows))),
        _stream_case("mhx_lean_serialize_dev_typed-mhx_lean_deserialize_dev", "stream", lean, 44, lean_definition),
    ]


# ---- mhx_jaccard_topk_dev: 3 probes against 2^24 + 3 rows ------------------------------------------------------------------------
def topk_cases() -> List[Case]:
    """The filler rows of B match nothing; rows around every mark (and the decoys at their wrapped images, which are rows of B like
    any other) are near-copies of a probe.  topk = 4, min_count = 1: the lists are exactly the best planted rows, in order."""
    rng = np.random.RandomState(61)
    k, n = STREAM_K, STREAM_N
    big = Big("b", np.uint32, n * k, 0x5A)
    probes = _rand(rng, 3 * k, np.uint32).reshape(3, k)
    probes[probes == big.fill_elem] ^= np.uint32(1)
    rows = {0, n - 1}
    for u in MARKS:
        r = mark_elems(u, 4) // k
        rows |= {r - 1, r, r + 1}
    rows = sorted(rows)

    def near(i, keep):
        row = _rand(rng, k, np.uint32)
        row[row == big.fill_elem] ^= np.uint32(1)
        at = rng.permutation(k)[:keep]
        row[at] = probes[i % 3][at]
        return row

    for x, r in enumerate(rows):
        big.plant(r * k, near(x, 40 + 11 * x))  # every row agrees with its probe in another number of positions
    for x, r in enumerate(rows):
        big.plant_decoys(r * k, k, lambda src, x=x: near(x, 5 + x) if src.size == k else _rand(rng, src.size, np.uint32))  # a decoy agrees less: it is a row of B too
    planted = sorted({s // k for s, _ in big.plants})

    def lists(wrap=None):
        cand = set(planted)
        if wrap is not None:  # the rows whose image is planted read planted data too
            for step in ((1 << 30) // k, (1 << 31) // k, (1 << 32) // k):
                cand |= {q + j * step for q in planted for j in range(1, 5) if q + j * step < n}
        cand = np.array(sorted(cand), dtype=np.int64)
        data = np.stack([big.read(r * k, k) if wrap is None else big.read_wrapped(r * k, k, wrap) for r in cand.tolist()])
        local, counts = lsh_bulk._topk_from_blocks(lsh_bulk._equal_counts_blocks(probes, data), 3, 4, 1, False)
        return np.where(local >= 0, cand[np.maximum(local, 0)], -1).astype(np.int64), counts.astype(np.int32)

    want_rows, want_counts = lists()
    checks = [Check("rows", 0, want_rows, "rows", [ABOVE] * 3), Check("counts", 0, want_counts, "counts", [ABOVE] * 3)]
    for name, wrap in wraps(4).items():
        r2, c2 = lists(wrap)
        for chk, other in zip(checks, (r2, c2)):
            chk.decoys[name], chk.moved[name] = other, np.ones(3, dtype=bool)
    assert (want_rows >= (1 << 24)).any(axis=1).all() and (want_rows < 0).any()  # every list reaches past the mark; one is padded
    first = np.array(rows) * k

    def definition():
        data = np.stack([big.read(r * k, k) for r in planted])
        counts = np.array([[int(np.count_nonzero(p == d)) for d in data] for p in probes])
        for i in range(3):
            order = sorted((j for j in range(len(planted)) if counts[i, j] >= 1), key=lambda j: (-counts[i, j], planted[j]))[:4]
            pad = [-1] * (4 - len(order))
            assert [planted[j] for j in order] + pad == want_rows[i].tolist() and [counts[i, j] for j in order] + pad == want_counts[i].tolist()

    return [Case("mhx_jaccard_topk_dev", "mhx_jaccard_topk_dev", "unsigned", MARKS["unsigned"], _items(_roles_of(first, first + k - 1, 1 << 32), first, first + k - 1, 1),
                 [Call(dict(n_b=n, k=k, topk=4, min_count=1), checks, refill={"rows": 0xEE, "counts": 0xEE})], bigs={"b": big}, arrays={"probes": probes},
                 outputs={"rows": 3 * 4 * 8, "counts": 3 * 4 * 4}, elem_bytes=4, definition=definition)]


# ---- mhx_jaccard_matrix_dev, mhx_jaccard_threshold_pairs_dev: 65 537 x 65 537 rows of 4 ----------------------------------------------
MATRIX_N, MATRIX_K = 65537, 4
MATRIX_PLANTED = (0, 32767, 32768, 65535, 65536)


def jaccard_matrix_cases() -> List[Case]:
    """The OUTPUT passes the marks: 2^32 + 131 073 counts with ldc = n_b.  The filler rows of A and B are all equal (count 4); planted
    rows differ.  Output rows are downloaded whole: the planted ones, those around output elements 2^30, 2^31 and 2^32, and rows 1
    and 2, where the counts of the last rows would land if their index were cut to 32 bits."""
    rng = np.random.RandomState(71)
    n, k = MATRIX_N, MATRIX_K
    a = np.full((n, k), 7, dtype=np.uint32)
    b = np.full((n, k), 7, dtype=np.uint32)
    for r in MATRIX_PLANTED:
        a[r] = rng.randint(0, 3, size=k) + 6  # values 6 .. 8: every count from 0 to 4 occurs
        b[r] = rng.randint(0, 3, size=k) + 6
    out_rows = sorted(set(MATRIX_PLANTED) | {1, 2, 16383, 16384, 32766, 32769, 65534})

    def row_of(i):
        return np.count_nonzero(a[i][None, :] == b, axis=1).astype(np.int32)

    checks = []
    for i in out_rows:
        first, last = i * n, i * n + n - 1
        checks.append(Check("counts", first * 4, row_of(i), f"counts[{i}, :]", _roles_of(np.array([first]), np.array([last]), 1 << 32)))
    # a write of row 65536 through an index cut to 32 bits lands one element before row 1
    chk = next(c for c in checks if c.what == "counts[1, :]")
    seen = chk.expected.copy()
    seen[: n - 1] = row_of(65536)[1:]
    chk.decoys, chk.moved = {"index mod 2^32": seen}, {"index mod 2^32": np.array([True])}
    items = [Item(_roles_of(np.array([i * n]), np.array([i * n + n - 1]), 1 << 32)[0], i * n, i * n + n - 1) for i in out_rows]
    assert {it.role for it in items} == {BELOW, ACROSS_ROLE, ABOVE}

    def definition():
        sel = list(MATRIX_PLANTED)
        got = lsh_bulk.jaccard_matrix(a[sel].astype(np.uint64), b[sel].astype(np.uint64), gpu_mode="disable") * k
        np.testing.assert_array_equal(got.astype(np.int32), np.stack([row_of(i)[sel] for i in sel]))

    return [Case("mhx_jaccard_matrix_dev", "mhx_jaccard_matrix_dev", "unsigned", MARKS["unsigned"], items, [Call(dict(n=n, k=k), checks, refill={"counts": 0xEE})],
                 arrays={"a": a, "b": b}, outputs={"counts": n * n * 4}, elem_bytes=4, definition=definition)]


def jaccard_threshold_cases() -> List[Case]:
    """The same shape with filler rows that are all different, so that only planted pairs reach min_count = 2: the pair NUMBER
    i * n_b + j passes 2^32 inside the call, the list that comes out is short and must be exact."""
    rng = np.random.RandomState(73)
    n, k = MATRIX_N, MATRIX_K
    a = (np.arange(n * k, dtype=np.uint32)).reshape(n, k)
    b = (np.arange(n * k, dtype=np.uint32) + np.uint32(1 << 20)).reshape(n, k)
    base = np.arange(k, dtype=np.uint32) + np.uint32(1 << 24)
    for r in MATRIX_PLANTED:
        a[r] = base + (rng.randint(0, 2, size=k) << 8).astype(np.uint32)
        b[r] = base + (rng.randint(0, 2, size=k) << 8).astype(np.uint32)
    sel = np.array(MATRIX_PLANTED)
    c = np.count_nonzero(a[sel][:, None, :] == b[sel][None, :, :], axis=2)
    ij = np.argwhere(c >= 2)
    pairs = sel[ij].astype(np.int64)
    counts = c[ij[:, 0], ij[:, 1]].astype(np.int32)
    assert 5 <= pairs.shape[0] < 25 and (pairs[:, 0] == 65536).any() and (pairs[:, 0] == 0).any()
    cap = 32
    roles = [ABOVE if i * n + j >= (1 << 32) else BELOW for i, j in pairs.tolist()]
    items = [Item(r, i * n + j, i * n + j) for r, (i, j) in zip(roles, pairs.tolist())] + [Item(ACROSS_ROLE, 65535 * n, 65535 * n + n - 1)]

    def definition():
        got_pairs, got_j = lsh_bulk.similar_pairs(a[sel].astype(np.uint64), b[sel].astype(np.uint64), threshold=0.5, gpu_mode="disable")
        np.testing.assert_array_equal(sel[got_pairs], pairs)
        np.testing.assert_array_equal((got_j * k).astype(np.int32), counts)

    return [Case("mhx_jaccard_threshold_pairs_dev", "mhx_jaccard_threshold_pairs_dev", "unsigned", MARKS["unsigned"], items,
                 [Call(dict(n=n, k=k, min_count=2, capacity=cap, n_pairs=pairs.shape[0]),
                       [Check("pairs", 0, pairs, "pairs", roles), Check("pair_counts", 0, counts, "counts of the pairs", roles)])],
                 arrays={"a": a, "b": b}, outputs={"pairs": cap * 16, "pair_counts": cap * 4}, elem_bytes=4, definition=definition,
                 no_decoys="the index that passes 2^32 is the number of a pair inside the call; nothing is stored at it")]


# ---- mhx_hll_histogram_dev, mhx_hll_union_groups_dev: 65 539 sketches of 2^16 registers ----------------------------------------------
def hll_rows_cases() -> List[Case]:
    rng = np.random.RandomState(83)
    m, n = 1 << 16, 65537 + 2
    big = Big("reg", np.uint8, n * m, 5)
    rows = [0, 65535, 65536, 65537, n - 1]
    for r in rows:
        big.plant(r * m, rng.randint(0, 64, size=m).astype(np.uint8))
    for r in rows:
        big.plant_decoys(r * m, m, lambda src: (63 - src).astype(np.uint8))
    planted = sorted({s // m for s, _ in big.plants})
    filler_hist = np.zeros(64, dtype=np.uint32)
    filler_hist[5] = m

    def hist(wrap=None):
        out = np.tile(filler_hist, (n, 1))
        cand = set(planted)
        if wrap is not None:
            cand |= {q + j * 32768 for q in planted for j in (1, 2) if q + j * 32768 < n}
        for r in cand:
            row = big.read(r * m, m) if wrap is None else big.read_wrapped(r * m, m, wrap)
            out[r] = hyperloglog._histogram_host(row[None, :])[0]
        return out

    first = np.arange(n, dtype=np.int64) * m
    roles = [role if r in rows else "filler" for r, role in enumerate(_roles_of(first, first + m - 1, 1 << 32))]
    want = hist()
    chk = Check("hist", 0, want, "histograms", roles)
    for name, wrap in wraps(1).items():
        other = hist(wrap)
        chk.decoys[name], chk.moved[name] = other, (other != want).any(axis=1)
    offsets = np.array([0, 2, 65535, 65536, 65537, n], dtype=np.int64)  # groups that end on both sides of the mark; one is 65 533 rows

    def union(wrap=None):
        out = np.zeros((offsets.size - 1, m), dtype=np.uint8)
        for g, (s, e) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist())):
            cand = set(planted)
            if wrap is not None:
                cand |= {q + j * 32768 for q in planted for j in (1, 2)}
            inside = [r for r in sorted(cand) if s <= r < e]
            if len(inside) < e - s:
                out[g] = big.fill
            for r in inside:
                out[g] = np.maximum(out[g], big.read(r * m, m) if wrap is None else big.read_wrapped(r * m, m, wrap))
        return out

    want_u = union()
    g_roles = _roles_of(offsets[:-1] * m, offsets[1:] * m - 1, 1 << 32)
    chk_u = Check("union", 0, want_u, "unions", g_roles)
    for name, wrap in wraps(1).items():
        other = union(wrap)
        chk_u.decoys[name], chk_u.moved[name] = other, (other != want_u).any(axis=1)
    items = _items([roles[r] for r in rows], first[rows], first[rows] + m - 1, 1)

    def definition():
        reg = np.stack([big.read(r * m, m) for r in rows])
        np.testing.assert_array_equal(np.stack([np.bincount(x, minlength=64) for x in reg]).astype(np.uint32), want[rows])
        np.testing.assert_array_equal(hyperloglog.union_groups(reg, np.array([0, 1, 3, 5]), gpu_mode="disable").view(np.uint8),
                                      np.stack([reg[0], np.maximum(reg[1], reg[2]), np.maximum(reg[3], reg[4])]))

    return [Case("mhx_hll_histogram_dev-mhx_hll_union_groups_dev", "mhx_hll_rows", "byte", MARKS["byte"], items,
                 [Call(dict(fn="mhx_hll_histogram_dev", n=n, p=16), [chk], what="mhx_hll_histogram_dev", refill={"hist": 0xEE}),
                  Call(dict(fn="mhx_hll_union_groups_dev", n=n, p=16, n_groups=offsets.size - 1), [chk_u], what="mhx_hll_union_groups_dev", refill={"union": 0xEE})],
                 bigs={"reg": big}, arrays={"group_offsets": offsets}, outputs={"hist": n * 64 * 4, "union": (offsets.size - 1) * m, "invalid": 8}, definition=definition)]


# ---- mhx_bloom_insert_dev, mhx_bloom_query_dev, mhx_bloom_union_dev: 32 bands x (2^23 + 8) blocks -------------------------------------
def bloom_cases() -> List[Case]:
    """The filter's word index passes 2^32 in the last 256 blocks of band 31 and its byte offset 2^34.  64 rows are inserted into a
    zeroed filter; half of them were searched for a band-31 key that falls into those last blocks.  Only the 64-byte lines the
    host twin names are downloaded, with their wrapped twins, which must stay zero."""
    from datasketch_amd import lsh_bloom
    rng = np.random.RandomState(91)
    bands, r, kbits, n_blocks = 32, 8, 7, (1 << 23) + 8
    k = bands * r
    lines_total = bands * n_blocks
    assert lines_total * 16 > (1 << 32)
    trial = _rand(rng, (1 << 21) * r, np.uint32).reshape(-1, r)  # band-31 values whose block lies past word 2^32
    keys = lsh_bloom.band_keys(trial.astype(np.uint64), 1, r)
    block, _ = lsh_bloom.block_masks(keys, n_blocks, kbits)
    high = np.flatnonzero(31 * n_blocks + block >= (1 << 28))
    assert high.size >= 32, high.size
    sig = _rand(rng, 128 * k, np.uint32).reshape(128, k)
    sig[:32, 31 * r:] = trial[high[:32]]
    sig[64:80, 31 * r:] = trial[high[:16]]  # rows that are NOT inserted but share a band-31 line with an inserted row
    inserted, others = sig[:64], sig[64:]
    flat, mask = lsh_bloom._flat_blocks(inserted.astype(np.uint64), bands, r, n_blocks, kbits)
    lines = {}
    for f, mk in zip(flat.tolist(), mask):
        lines[f] = lines.get(f, np.zeros(16, dtype=np.uint32)) | mk
    assert sum(f >= (1 << 28) for f in lines) >= 16

    def query(rows):
        f2, m2 = lsh_bloom._flat_blocks(rows.astype(np.uint64), bands, r, n_blocks, kbits)
        hit = np.array([((lines.get(f, np.zeros(16, dtype=np.uint32)) & mk) == mk).all() for f, mk in zip(f2.tolist(), m2)])
        return hit.reshape(-1, bands).any(axis=1).astype(np.uint8)

    want_hits = query(sig)
    assert want_hits[:64].all() and want_hits[64:80].all() and not want_hits[80:].all()
    checks, items = [], []
    for f in sorted(lines):
        role = ABOVE if f * 16 >= (1 << 32) else BELOW
        items.append(Item(role, f * 16, f * 16 + 15))
        checks.append(Check("filter", f * 64, lines[f], f"line {f}", [role]))
        for name, wrap in wraps(4).items():  # the line where a 32-bit word index or byte offset of this one lands stays zero
            f2 = wrap(f * 16) // 16
            if f2 != f and f2 not in lines:
                checks.append(Check("filter", f2 * 64, np.zeros(16, dtype=np.uint32), f"line {f2}, the image of line {f} at {name}", [role],
                                    {name: lines[f]}, {name: np.array([True])}))
    hits = Check("hit", 0, want_hits, "hits", [BELOW] * 128)

    def definition():
        small = np.zeros((bands, 64, 16), dtype=np.uint32)  # the twin's own insert and query at a size a host can hold
        lsh_bloom.insert_host(small, inserted.astype(np.uint64), r, kbits)
        f3, m3 = lsh_bloom._flat_blocks(inserted.astype(np.uint64), bands, r, 64, kbits)
        acc = np.zeros((bands * 64, 16), dtype=np.uint32)
        for f, mk in zip(f3.tolist(), m3):
            acc[f] |= mk
        np.testing.assert_array_equal(small.reshape(-1, 16), acc)
        assert lsh_bloom.query_host(small, inserted.astype(np.uint64), r, kbits).all()

    a = dict(bands=bands, r=r, kbits=kbits, n_blocks=n_blocks, k=k)
    return [Case("mhx_bloom_insert_dev-mhx_bloom_query_dev-mhx_bloom_union_dev", "mhx_bloom", "unsigned", MARKS["unsigned"], items,
                 [Call(dict(a, fn="mhx_bloom_insert_dev"), checks, what="mhx_bloom_insert_dev", refill={"filter": 0}),
                  Call(dict(a, fn="mhx_bloom_query_dev"), [hits] + checks, what="mhx_bloom_query_dev", refill={"hit": 0xEE}),
                  Call(dict(a, fn="mhx_bloom_union_dev"), [Check("filter2", c.offset, c.expected, c.what, c.roles, c.decoys, c.moved) for c in checks],
                       what="mhx_bloom_union_dev", refill={"filter2": 0})],
                 arrays={"sig": sig}, outputs={"filter": lines_total * 64, "filter2": lines_total * 64, "hit": 128}, elem_bytes=4, definition=definition)]


# ---- mhx_sha1_windows_dev: windows of documents that lie around byte 2^32 ---------------------------------------------------------
def sha1_windows_cases() -> List[Case]:
    """include/mhx.h trusts the device arrays, so the corpus starts high instead of behind a filler document: in byte mode
    doc_offsets[0] = M - a (an item is a byte), in token mode item_offsets[0] = M - a (documents count items from 0).  Widths 5
    (the one-block kernel of short byte shingles) and 12; empty documents, documents shorter than a window, and one document that
    starts at M - 37."""
    from datasketch_amd import shingle
    m = MARKS["byte"]
    cases = []
    for mode in ("byte", "token"):
        rng = np.random.RandomState(101 + len(cases))
        counts = [0, 3, 30, 100, 0, 50, 12, 5, 4, 64]  # items per document; document 3 starts at M - ACROSS
        if mode == "byte":
            item_lens = np.ones(sum(counts), dtype=np.int64)
        else:
            item_lens = rng.randint(1, 10, size=sum(counts)).astype(np.int64)
        doc_items = np.zeros(len(counts) + 1, dtype=np.int64)
        np.cumsum(counts, out=doc_items[1:])
        item_offsets = np.zeros(item_lens.size + 1, dtype=np.int64)
        np.cumsum(item_lens, out=item_offsets[1:])
        item_offsets += m - ACROSS - item_offsets[doc_items[3]]
        data = _rand(rng, int(item_offsets[-1] - item_offsets[0]), np.uint8)
        big = Big("bytes", np.uint8, int(item_offsets[-1]), 0x20)
        big.plant(int(item_offsets[0]), data)
        big.plant_decoys(int(item_offsets[0]), data.size, lambda src: src ^ np.uint8(0xA5))
        doc_offsets = item_offsets[doc_items] if mode == "byte" else doc_items  # byte mode: a document owns bytes; token mode: items
        calls, items = [], []
        for width, out_dtype in ((5, np.uint32), (12, np.uint64)):
            set_offsets = shingle.window_offsets(doc_offsets, width)
            spans = []
            for d, c in enumerate(counts):
                for i in range(0 if c == 0 else 1 if c < width else c - width + 1):
                    first = int(doc_items[d]) + i
                    spans.append((int(item_offsets[first]), int(item_offsets[first + min(width, c)])))
            assert len(spans) == set_offsets[-1]
            want = np.array([_sha1(big.read(s, e - s).tobytes(), out_dtype) for s, e in spans], dtype=out_dtype)
            beg, end = np.array([s for s, _ in spans]), np.array([e for _, e in spans])
            roles = _roles_of(beg, end - 1, m)
            decoys, moved = {}, {}
            for name, wrap in wraps(1).items():
                mv = np.array([big.moved(s, e - s, wrap) for s, e in spans])
                if mv.any():
                    decoys[name] = np.array([_sha1(big.read_wrapped(s, e - s, wrap).tobytes(), out_dtype) for s, e in spans], dtype=out_dtype)
                    moved[name] = mv
            calls.append(Call(dict(width=width, out_dtype=np.dtype(out_dtype), set_offsets=set_offsets, n_windows=len(spans), token_mode=mode == "token"),
                              [Check("out", 0, want, "window hashes", roles, decoys, moved)], what=f"width={width} out={np.dtype(out_dtype).name}",
                              refill={"out": 0xEE}))
            items += _items(roles, beg, end - 1, 1)

        def definition(big=big, item_offsets=item_offsets, doc_offsets=doc_offsets, mode=mode, calls=calls):
            base = int(item_offsets[0])
            buf = big.read(base, big.n - base)
            for call in calls:  # the package's own host shingler on the compact corpus
                sh = shingle.host_shingles(buf, item_offsets - base if mode == "token" else None, doc_offsets - (base if mode == "byte" else 0), call.args["width"])
                flat = [w for doc in sh for w in doc]
                got = np.array([_sha1(bytes(w), call.args["out_dtype"]) for w in flat], dtype=call.args["out_dtype"])
                np.testing.assert_array_equal(got, call.checks[0].expected)

        arrays = {"doc_offsets": doc_offsets, "set_offsets": np.zeros(len(counts) + 1, dtype=np.int64)}
        if mode == "token":
            arrays["item_offsets"] = item_offsets
        cases.append(Case(f"mhx_sha1_windows_dev-{mode}-mode", "mhx_sha1_windows_dev", "byte", m, items, calls, bigs={"bytes": big}, arrays=arrays,
                          outputs={"out": 8 * (sum(counts) + len(counts))}, across_first_elem=int(item_offsets[doc_items[3]]), definition=definition))
    return cases


# ---- mhx_words_normalize_dev: 2^32 + 9001 bytes of text and spaces -----------------------------------------------------------------
def words_cases() -> List[Case]:
    """doc_offsets runs from 0 to n_bytes, as the host form requires.  Five documents: text at 0, a filler of spaces up to M - 37,
    text across the mark, a filler, text on the last bytes.  The normal form does not say where its words stood, so the expected
    triple is shingle.normalize_words of the same documents with the fillers cut short."""
    from datasketch_amd import shingle
    rng = np.random.RandomState(131)
    m = MARKS["byte"]
    n_bytes = m + 9001
    table = shingle.word_table()

    def text(n):  # words of 1 .. 9 letters in both cases, runs of separators between them; ends inside a word
        out = bytearray()
        while len(out) < n:
            out += bytes(rng.choice(list(b"abcdefgXYZ019"), size=rng.randint(1, 10)).tolist()) + bytes(rng.choice(list(b" ,.\n\t"), size=rng.randint(1, 4)).tolist())
        return np.frombuffer(bytes(out[: n - 1]) + b"q", dtype=np.uint8)

    spans = [(0, 400), (m - ACROSS, 333), (n_bytes - 211, 211)]
    doc_offsets = np.array([0, 400, m - ACROSS, m - ACROSS + 333, n_bytes - 211, n_bytes], dtype=np.int64)
    big = Big("bytes", np.uint8, n_bytes, 0x20)
    for s, n in spans:
        big.plant(s, text(n))

    def triple(wrap=None):
        docs = []
        for d in range(5):
            s, e = int(doc_offsets[d]), int(doc_offsets[d + 1])
            if d in (1, 3):
                docs.append(np.full(7, 0x20, dtype=np.uint8))  # a filler holds no word however long it is
            else:
                docs.append(big.read(s, e - s) if wrap is None else big.read_wrapped(s, e - s, wrap))
        off = np.zeros(6, dtype=np.int64)
        np.cumsum([d.size for d in docs], out=off[1:])
        return shingle.normalize_words(np.concatenate(docs), off, table, gpu_mode="disable")

    out_bytes, item_offsets, word_doc_offsets = triple()
    checks = [Check("out_bytes", 0, out_bytes, "normal form", []), Check("item_offsets", 0, item_offsets, "item_offsets", []),
              Check("word_doc_offsets", 0, word_doc_offsets, "word_doc_offsets", [])]
    wrap = wraps(1)["index mod 2^32"]  # the documents across and past the mark read from byte 0 on, where document 0 lies
    other = triple(wrap)[0]
    size = min(other.size, out_bytes.size)
    assert not np.array_equal(other[:size], out_bytes[:size])
    seen = out_bytes.copy()
    seen[:size] = other[:size]
    checks[0].decoys, checks[0].moved = {"index mod 2^32": seen}, {"index mod 2^32": np.array([True])}
    roles = _roles_of(np.array([s for s, _ in spans]), np.array([s + n - 1 for s, n in spans]), m)
    items = _items(roles, np.array([s for s, _ in spans]), np.array([s + n - 1 for s, n in spans]), 1)

    def definition():
        words = [w for d in (0, 2, 4) for w in shingle.words(big.read(int(doc_offsets[d]), int(doc_offsets[d + 1] - doc_offsets[d])).tobytes(), table)]
        assert out_bytes.tobytes() == b"".join(w + b" " for w in words) and item_offsets.size == len(words) + 1

    return [Case("mhx_words_normalize_dev", "mhx_words_normalize_dev", "byte", m, items,
                 [Call(dict(n_bytes=n_bytes, n_docs=5, table=table, n_words=item_offsets.size - 1, n_out_bytes=out_bytes.size), checks,
                       refill={"out_bytes": 0xEE, "item_offsets": 0xEE, "word_doc_offsets": 0xEE})],
                 bigs={"bytes": big}, arrays={"doc_offsets": doc_offsets},
                 outputs={"out_bytes": out_bytes.size, "item_offsets": item_offsets.nbytes, "word_doc_offsets": word_doc_offsets.nbytes},
                 across_first_elem=m - ACROSS, definition=definition)]


# ---- weighted MinHash: mhx_weighted_minhash_many_dev (CSR), mhx_weighted_minhash_many_dense_dev ------------------------------------
def csr_row_is_walked(nnz: int, dim: int, chunks: int) -> bool:
    """weighted_kernels.hip csr_row_is_walked, mode 0: the cost rule between the walk and the entry-by-entry evaluation."""
    return 683 * chunks * nnz * nnz > (39000 + 11 * dim + 20000 * chunks) * nnz + (3000 + 13700 * chunks + 3 * dim) * dim


def _weighted_logs(rng, n: int) -> np.ndarray:
    return rng.normal(0.0, 2.0, size=n).astype(np.float32)


def _device_logs(values: np.ndarray) -> np.ndarray:
    """The logarithm the device takes in values-in mode: numpy's float32 log as oracle/np_logf.c restates it, which
    tests/test_gpu_round4.py pins to the device for every float32."""
    return O.c_np_logf(values)


WEIGHTED_SEED = 9


def weighted_csr_cases() -> List[Case]:
    """indptr[0] = M - a at M = 2^31 and 2^32 elements of d_indices / d_values; rows on both sides of the walk / entry-by-entry
    crossover below and above the mark, empty rows, one row from M - 37.  d_values is filled with byte 0x3F (0.747, a sane value
    and a sane log): values-in mode takes the log of all nnz entries into scratch and the plan samples them.  Logs in: the
    planted floats are the logs; values in: they are exp(logs) and the oracle is fed the device's logarithm of them."""
    cases = []
    for dim, s_count in ((1024, 64), (4096, 128)):
        chunks = (s_count + 63) // 64
        rs, ln_cs, betas = O.np_weighted_params(dim, s_count, WEIGHTED_SEED)
        for unit in ("signed", "unsigned"):
            rng = np.random.RandomState(dim + len(cases))
            m = MARKS[unit]
            lens = np.array([3, 0, 60, dim // 8, dim, dim // 2, dim, 1, dim // 16, 200, 0, ACROSS + 5, dim // 3], dtype=np.int64)
            across = 5
            indptr = np.zeros(lens.size + 1, dtype=np.int64)
            np.cumsum(lens, out=indptr[1:])
            indptr += m - ACROSS - indptr[across]
            roles = _roles_of(indptr[:-1], indptr[1:] - 1, m)
            walked = [csr_row_is_walked(int(n), dim, chunks) for n in lens]
            for side in (BELOW, ABOVE):  # both evaluations on both sides of the mark
                assert {w for w, r, n in zip(walked, roles, lens) if r == side and n} == {False, True}, (dim, unit, side)
            n_rows, base, total = lens.size, int(indptr[0]), int(indptr[-1])
            cols = np.concatenate([np.sort(rng.permutation(dim)[:n]) for n in lens]).astype(np.int32)
            logs = _weighted_logs(rng, cols.size)
            indices = Big("indices", np.int32, total, 0)
            indices.plant(base, cols)
            indices.plant_decoys(base, cols.size, lambda src: (dim - 1 - src).astype(np.int32))
            spans = list(zip(indptr[:-1].tolist(), indptr[1:].tolist()))
            calls = []
            for values_are_logs in (True, False):
                planted = logs if values_are_logs else np.exp(logs).astype(np.float32)
                values = Big("values", np.float32, total, 0x3F)
                values.plant(base, planted)
                values.plant_decoys(base, planted.size, lambda src: (src * np.float32(0.5) + np.float32(0.25)).astype(np.float32))

                def sketch(wrap=None, values=values, values_are_logs=values_are_logs):
                    read = (lambda b, st, n: b.read(st, n)) if wrap is None else (lambda b, st, n: b.read_wrapped(st, n, wrap))
                    c = np.concatenate([read(indices, st, e - st) for st, e in spans])
                    v = np.concatenate([read(values, st, e - st) for st, e in spans])
                    out, ne = O.c_weighted_minhash_many(indptr - base, c, None, rs, ln_cs, betas, logs=v if values_are_logs else _device_logs(v))
                    return out, ne.astype(np.uint8)

                want, want_ne = sketch()
                decoys, moved = {}, {}
                for name, wrap in wraps(4).items():
                    mv = np.array([e > st and indices.moved(st, e - st, wrap) for st, e in spans])
                    if mv.any():
                        decoys[name], moved[name] = sketch(wrap)[0], mv
                calls.append(Call(dict(dim=dim, sample_size=s_count, values_are_logs=values_are_logs, n_rows=n_rows, nnz=total),
                                  [Check("out", 0, want, "(k, t) pairs", roles, decoys, moved), Check("nonempty", 0, want_ne, "nonempty")],
                                  what="logs in" if values_are_logs else "values in", bigs={"values": values}, refill={"out": 0xEE, "nonempty": 0xEE}))

            def definition(indptr=indptr, cols=cols, logs=logs, base=base, calls=calls, rs=rs, ln_cs=ln_cs, betas=betas):
                got, ne = O.np_weighted_minhash_many(indptr - base, cols, np.exp(logs.astype(np.float64)), rs, ln_cs, betas)  # the reference's numpy steps
                want = calls[0].checks[0].expected
                same = (got == want).all(axis=(1, 2))  # np.log(exp(.)) is not the planted log to the last bit: most rows agree, all winners nearly
                assert np.array_equal(ne.astype(np.uint8), calls[0].checks[1].expected) and same.mean() >= 0.5
                assert (got[..., 0] == want[..., 0]).mean() > 0.99

            cases.append(Case(f"mhx_weighted_minhash_many_dev-dim{dim}-S{s_count}-{unit}", "mhx_weighted_minhash_many_dev", unit, m,
                              _items(roles, indptr[:-1], indptr[1:] - 1, 1), calls, bigs={"indices": indices, "values": Big("values", np.float32, total, 0x3F)},
                              arrays={"indptr": indptr}, outputs={"out": n_rows * s_count * 16, "nonempty": n_rows}, across_first_elem=int(indptr[across]),
                              elem_bytes=4, definition=definition, scratch_bytes=total * 4))
    return cases


DENSE_DIM, DENSE_N = 4096, (1 << 20) + 3


def weighted_dense_cases() -> List[Case]:
    """dim = 4096, 2^20 + 3 rows that hold nothing -- zeros with values in, -inf with logs in (no byte fill writes -inf: the
    buffer is filled by copies of the element) -- and planted rows around float index 2^30 (byte 2^32), 2^31 and 2^32, at 0 and at
    the end.  S = 1 takes the one-wave-per-row kernel, S = 128 its fetcher / walker form (tests/weighted_dispatch.py)."""
    from tests.weighted_dispatch import dense_walk_launch
    dim, n = DENSE_DIM, DENSE_N
    cases = []
    for values_are_logs in (False, True):
        rng = np.random.RandomState(211 + values_are_logs)
        absent = np.float32(-np.inf) if values_are_logs else np.float32(0)
        big = Big("x", np.float32, n * dim, 0, fill_value=absent)
        rows = {0, n - 1}
        for u in MARKS:
            r = mark_elems(u, 4) // dim
            rows |= {r - 1, r, r + 1}
        rows = sorted(rows)

        def row(density, cls):
            """Stored entries only in the columns = cls mod 5: rows of different classes never name the same winning column, so
            a row and what lies at its wrapped image differ even in one sample."""
            logs = _weighted_logs(rng, dim)
            x = logs if values_are_logs else np.exp(logs).astype(np.float32)
            x[(rng.random_sample(dim) >= density) | (np.arange(dim) % 5 != cls)] = absent
            return x

        for i, r in enumerate(rows):  # the class is the 2^18-row block: every wrap lands in a lower block
            big.plant(r * dim, row((1.0, 0.6, 0.05, 0.3)[i % 4], (r >> 18) % 5))
        for r in rows:
            big.plant_decoys(r * dim, dim, lambda src, r=r: row(0.5, ((r >> 18) + 2) % 5))
        stored_rows = sorted({st // dim for st, _ in big.plants})
        first = np.array(rows) * dim
        roles = _roles_of(first, first + dim - 1, 1 << 32)
        calls = []
        for s_count in (1, 128):
            rs, ln_cs, betas = O.np_weighted_params(dim, s_count, WEIGHTED_SEED)
            name = dense_walk_launch(dim, s_count, values_are_logs).name

            def sketch(which, wrap=None, rs=rs, ln_cs=ln_cs, betas=betas):
                data = np.stack([big.read(r * dim, dim) if wrap is None else big.read_wrapped(r * dim, dim, wrap) for r in which])
                keep = data != absent
                indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int64)
                cols = np.nonzero(keep)[1].astype(np.int32)
                v = data[keep]
                return O.c_weighted_minhash_many(indptr, cols, None, rs, ln_cs, betas, logs=v if values_are_logs else _device_logs(v))[0]

            want = sketch(rows)
            decoys, moved = {}, {}
            for wname, wrap in wraps(4).items():
                mv = np.array([big.moved(r * dim, dim, wrap) for r in rows])
                if mv.any():
                    decoys[wname], moved[wname] = sketch(rows, wrap), mv
            checks = []
            for i, r in enumerate(rows):  # every planted row on its own, and the filler row behind it: zeros
                checks.append(Check("out", r * s_count * 16, want[i: i + 1], f"(k, t) pairs of row {r}", [roles[i]], {k_: d[i: i + 1] for k_, d in decoys.items() if moved[k_][i]},
                                    {k_: mv[i: i + 1] for k_, mv in moved.items() if mv[i]}))
                if r + 1 < n and r + 1 not in stored_rows:
                    checks.append(Check("out", (r + 1) * s_count * 16, np.zeros((1, s_count, 2), dtype=np.int64), f"(k, t) pairs of the empty row {r + 1}"))
            nonempty = np.zeros(n, dtype=np.uint8)
            nonempty[stored_rows] = 1
            checks.append(Check("nonempty", 0, nonempty, "nonempty"))
            calls.append(Call(dict(dim=dim, sample_size=s_count, values_are_logs=values_are_logs, n_rows=n, kernel=name), checks,
                              what=f"S={s_count} {name}", refill={"out": 0xEE, "nonempty": 0xEE}))
        assert [c.args["kernel"].rsplit("_", 1)[1] for c in calls] == ["SPLIT0", "SPLIT2"]  # one wave per row; fetchers and walkers

        def definition(big=big, rows=rows, values_are_logs=values_are_logs, absent=absent):
            import scipy.sparse as sp
            rs, ln_cs, betas = O.np_weighted_params(dim, 4, WEIGHTED_SEED)
            data = np.stack([big.read(r * dim, dim) for r in rows[:4]])
            x = np.exp(data.astype(np.float64)).astype(np.float32) if values_are_logs else data
            csr = sp.csr_matrix(x)
            csr.sort_indices()
            assert np.array_equal(csr.indptr, np.concatenate([[0], np.cumsum((data != absent).sum(axis=1))]))  # stored = not absent
            a = O.c_weighted_minhash_many(csr.indptr, csr.indices, csr.data, rs, ln_cs, betas)
            b = O.np_weighted_minhash_many(csr.indptr, csr.indices, csr.data, rs, ln_cs, betas)
            assert np.array_equal(a[1], b[1]) and (a[0][..., 0] == b[0][..., 0]).mean() > 0.99

        cases.append(Case(f"mhx_weighted_minhash_many_dense_dev-{'logs' if values_are_logs else 'values'}-in", "mhx_weighted_minhash_many_dense_dev", "unsigned",
                          MARKS["unsigned"], _items(roles, first, first + dim - 1, 1), calls, bigs={"x": big}, outputs={"out": n * 128 * 16, "nonempty": n},
                          elem_bytes=4, definition=definition))
    return cases


BUILDERS = {
    "mhx_minhash_bulk_dev": minhash_cases,
    "mhx_hll_bulk_dev": hll_bulk_cases,
    "mhx_sha1_tokens_dev": sha1_tokens_cases,
    "mhx_overlap_pairs_dev": overlap_cases,
    "mhx_jaccard_pairs_dev_typed": jaccard_pairs_cases,
    "mhx_bbit_jaccard_pairs_dev": bbit_jaccard_pairs_cases,
    "mhx_rows_compact_dev": rows_compact_cases,
    "mhx_cc": cc_cases,
    "mhx_hll_merge_dev": hll_merge_cases,
    "stream": stream_cases,
    "mhx_jaccard_topk_dev": topk_cases,
    "mhx_jaccard_matrix_dev": jaccard_matrix_cases,
    "mhx_jaccard_threshold_pairs_dev": jaccard_threshold_cases,
    "mhx_hll_rows": hll_rows_cases,
    "mhx_bloom": bloom_cases,
    "mhx_sha1_windows_dev": sha1_windows_cases,
    "mhx_words_normalize_dev": words_cases,
    "mhx_weighted_minhash_many_dev": weighted_csr_cases,
    "mhx_weighted_minhash_many_dense_dev": weighted_dense_cases,
}
_BUILT: Dict[str, List[Case]] = {}


def cases_of(entry: str) -> List[Case]:
    """The cases of one entry, built once per process (the expected values are shared by every test and never changed)."""
    if entry not in _BUILT:
        _BUILT[entry] = BUILDERS[entry]()
    return _BUILT[entry]


_CSR_IDS = [f"{t}-{u}-{s}" for t in ("uint32", "uint64") for u in ("byte", "signed", "unsigned") for s in CSR_SHAPES]
CASE_IDS = {  # written out, so that collecting the GPU tests builds nothing (tests/test_index_width_host.py holds the builders to it)
    "mhx_minhash_bulk_dev": [f"mhx_minhash_bulk_dev-{i}" for i in _CSR_IDS],
    "mhx_hll_bulk_dev": [f"mhx_hll_bulk_dev-{i}" for i in _CSR_IDS],
    "mhx_sha1_tokens_dev": ["mhx_sha1_tokens_dev-byte"],
    "mhx_overlap_pairs_dev": ["mhx_overlap_pairs_dev-uint32", "mhx_overlap_pairs_dev-uint64"],
    "mhx_jaccard_pairs_dev_typed": ["mhx_jaccard_pairs_dev_typed-uint32", "mhx_jaccard_pairs_dev_typed-uint64"],
    "mhx_bbit_jaccard_pairs_dev": ["mhx_bbit_jaccard_pairs_dev"],
    "mhx_rows_compact_dev": ["mhx_rows_compact_dev-row_bytes1024", "mhx_rows_compact_dev-row_bytes48"],
    "mhx_cc": ["mhx_cc_init_dev-mhx_cc_link_pairs_dev-mhx_cc_finish_dev"],
    "mhx_hll_merge_dev": ["mhx_hll_merge_dev-byte"],
    "stream": ["mhx_bbit_pack_dev_typed-mhx_bbit_unpack_dev", "mhx_band_digests_dev_typed-mhx_band_digests_layout_dev", "mhx_bbit_pack_band_digests_dev",
               "mhx_lean_serialize_dev_typed-mhx_lean_deserialize_dev"],
    "mhx_jaccard_topk_dev": ["mhx_jaccard_topk_dev"],
    "mhx_jaccard_matrix_dev": ["mhx_jaccard_matrix_dev"],
    "mhx_jaccard_threshold_pairs_dev": ["mhx_jaccard_threshold_pairs_dev"],
    "mhx_hll_rows": ["mhx_hll_histogram_dev-mhx_hll_union_groups_dev"],
    "mhx_bloom": ["mhx_bloom_insert_dev-mhx_bloom_query_dev-mhx_bloom_union_dev"],
    "mhx_sha1_windows_dev": ["mhx_sha1_windows_dev-byte-mode", "mhx_sha1_windows_dev-token-mode"],
    "mhx_words_normalize_dev": ["mhx_words_normalize_dev"],
    "mhx_weighted_minhash_many_dev": [f"mhx_weighted_minhash_many_dev-dim{d}-S{s}-{u}" for d, s in ((1024, 64), (4096, 128)) for u in ("signed", "unsigned")],
    "mhx_weighted_minhash_many_dense_dev": ["mhx_weighted_minhash_many_dense_dev-values-in", "mhx_weighted_minhash_many_dense_dev-logs-in"],
}


def case(case_id: str) -> Case:
    for entry, ids in CASE_IDS.items():
        if case_id in ids:
            return next(c for c in cases_of(entry) if c.id == case_id)
    raise KeyError(case_id)


def all_cases() -> List[Case]:
    return [c for entry in BUILDERS for c in cases_of(entry)]
