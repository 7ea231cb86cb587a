"""Every value of every mhx_ctx_set_option key at a shape whose launcher reads it: the cases of tests/test_gpu_options.py and the
ledger of tests/test_option_ledger.py.  include/mhx.h promises for nearly every key "timings depend on it, results never"; a case
holds one (key, value) to that promise: the operation, the smallest input that makes the launcher look at the option, the
reference the result must equal byte for byte, the places in datasketch_amd/csrc that read the option (`reads`) and the launcher's
own condition restated in Python (`applies`, in the manner of tests/weighted_dispatch.py).  Nothing here needs a GPU: the inputs
and references are numpy, the C oracle and the gpu_mode="disable" twins, built on first use and computed once.

DOMAIN    key -> the values mhx_ctx_set_option accepts: a tuple where the header lists them, a Range where the value is a count
CASES     one Case per (key, non-default value of a finite domain), per (key, both ends and one inner value of a range), per shape
EXCLUDED  key or (key, value) -> why no reference can hold it; the GPU test sets such a value and sets it back, launching nothing
SITE_EXEMPT  (field, file, function) of a read no case claims -> why
"""
from dataclasses import dataclass, field
from typing import Callable, Dict, Mapping, Optional, Tuple

import numpy as np

from tests.weighted_dispatch import MI355X_CUS, MI355X_LDS_PER_BLOCK, dense_walk_launch

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
KWAVE = 64


@dataclass(frozen=True)
class Range:
    """lo .. hi, both included; step > 0: 0 or a multiple of step in the range.  inner: the value between the ends that has a case."""
    lo: int
    hi: int
    inner: int
    step: int = 0

    def __contains__(self, v):
        return self.lo <= v <= self.hi and (self.step == 0 or v % self.step == 0)

    def representatives(self):
        return (self.lo, self.inner, self.hi)

    def outside(self):
        """Values the library must refuse: one beyond each end, a non-multiple of the step, and -- where the range is open on one side --
        the far end of the other."""
        out = [v for v in (self.lo - 1, self.hi + 1) if I64_MIN <= v <= I64_MAX]
        if self.step:
            out.append(self.lo + self.step + 2)
        if len(out) == 1:
            out.append(I64_MAX if self.lo == I64_MIN else I64_MIN)
        return tuple(out)


# the value a fresh context holds
DEFAULTS = {
    "minhash.path": 0, "minhash.split": 0, "minhash.packed": 0, "minhash.ties": 0, "minhash.p3": 0, "minhash.share": 0, "minhash.adapt": 0,
    "blocks_per_cu": 0, "minhash.alias": -1, "minhash.prefetch": 1, "weighted.path": 0, "weighted.direct": 0, "weighted.split": 0,
    "weighted.tail": 0, "weighted.debug": 0, "weighted.kernel": 0, "weighted.plan": 0, "weighted.rescue": 0, "weighted.min_dim": 0,
    "host.chunk_bytes": 0, "lsh.sort_bits": 0, "lsh.gather": 0, "lsh.sort": 0, "lsh.levels": 0, "lsh.chunk": 0, "lsh.team": 0, "lsh.bigbins": 0,
    "pack.fused": 0, "weighted.refill": 0, "lsh.prehash": 0, "lsh.merge_items": 0, "hll.split_tokens": 0, "bloom.lanes": 0,
    "jaccard.topk_path": 0, "jaccard.topk_segments": 0, "debug.cus": 0, "overlap.bins": 0,
}

# blocks_per_cu: (2^32 - 1) // (512 threads * CUs) -- see max_blocks_per_cu in mhx_api.hip and the comment in include/mhx.h
MAX_BLOCKS_PER_CU = 0xFFFFFFFF // (512 * MI355X_CUS)

DOMAIN = {
    "minhash.path": (0, 1, 2), "minhash.split": (0, 1, 2), "minhash.packed": (0, 1, 2), "minhash.ties": (0, 1), "minhash.p3": (0, 1),
    "minhash.share": (0, 1), "minhash.adapt": (0, 1), "minhash.prefetch": (0, 1, 2),
    "blocks_per_cu": Range(0, MAX_BLOCKS_PER_CU, 4),
    "minhash.alias": Range(-1, I64_MAX, 4095),
    "weighted.path": (0, 1, 2), "weighted.direct": Range(0, 1000, 500), "weighted.split": (0, 1), "weighted.tail": Range(0, 5, 3),
    "weighted.debug": (0, 1, 2, 4, 8), "weighted.kernel": (0, 1, 2), "weighted.plan": (0, 1),
    "weighted.rescue": Range(I64_MIN, 64, 1), "weighted.min_dim": Range(0, 4096, 64, step=4),
    "weighted.refill": (0, 1, 2, 3, 5, 6, 8, 9, 13),
    "host.chunk_bytes": Range(I64_MIN, I64_MAX, 4096),
    "lsh.sort_bits": Range(0, 64, 20), "lsh.gather": (0, 1), "lsh.sort": (0, 1), "lsh.levels": (0, 2), "lsh.chunk": (0, 8),
    "lsh.team": (0, 256, 1024), "lsh.bigbins": (0, 1, 2), "lsh.prehash": (0, 1), "lsh.merge_items": (0, 8, 16),
    "pack.fused": (0, 1), "hll.split_tokens": Range(0, I64_MAX, 64), "bloom.lanes": (0, 1, 16),
    "jaccard.topk_path": (0, 1, 2), "jaccard.topk_segments": Range(0, I64_MAX, 3),
    "debug.cus": Range(0, MI355X_CUS, 3),  # (the upper end is the device's own count: the GPU test takes it from mhx_ctx_device_info)
    "overlap.bins": (0, 1, 2),
}

EXCLUDED = {
    ("weighted.debug", 1): "profiling only: the rows are staged and scanned, not walked -- the results are meaningless by design",
    ("weighted.debug", 2): "profiling only: the scan is skipped as well -- the results are meaningless by design",
    ("weighted.debug", 4): "profiling only: every stripe keeps its first row (the walkers alone) -- the results are meaningless by design",
    ("weighted.debug", 8): "turns a hand-over wait that outlasts 2^24 polls into a trap: must never be run",
    "minhash.alias": ">= 0 makes set i read the tokens of set i & mask: it changes what is read, so no reference of the input holds it "
                     "(-1, the default, is what every other case runs with)",
}

SITE_EXEMPT = {
    ("weighted_debug", "weighted_kernels.hip", "launch_weighted_dense_walk"): "weighted.debug is excluded: every non-zero value is profiling only or a trap",
    ("minhash_alias", "minhash_kernels.hip", "launch_minhash_bulk"): "minhash.alias is excluded: >= 0 changes what is read",
    ("host_chunk_bytes", "mhx_api.hip", "weighted_dense"): "read only from 2 x max(4096, 64 MiB / row) dense rows on -- 128 MiB of rows or of samples at the "
                                                            "least; tests/test_gpu_weighted_small_dims.py runs its large shapes with host.chunk_bytes -1",
}


def value_needs_case(key):
    """The values of DOMAIN[key] that need a case or an exclusion: every non-default one of a finite domain, both ends and the
    inner value of a range (the default among them stands for itself: every case runs it first)."""
    dom = DOMAIN[key]
    values = dom.representatives() if isinstance(dom, Range) else dom
    return tuple(v for v in values if v != DEFAULTS[key])


def outside(key):
    """Two values outside DOMAIN[key] (fewer where the domain is every int64)."""
    dom = DOMAIN[key]
    if isinstance(dom, Range):
        return dom.outside()
    return (min(dom) - 1, max(dom) + 1) if key != "lsh.merge_items" else (12, 32)


# ------------------------------------------------------------------------------------------------------------------ the launchers, restated
def _cus(shape):
    return shape.get("cus") or MI355X_CUS


def minhash_total(shape):
    return int(shape["n_sets"]) * int(shape["fixed_len"]) if shape["layout"] == "fixed" else int(minhash_lengths(shape).sum())


def minhash_lengths(shape):
    if shape["layout"] == "fixed":
        return np.full(shape["n_sets"], shape["fixed_len"], dtype=np.int64)
    return np.asarray([(0, 1, 5, 63, 64, 65, 100, 200, 257)[i % 9] for i in range(shape["n_sets"])], dtype=np.int64)


def minhash_split(shape, opts=None):
    """launch_minhash_bulk: few sets with long token lists are split over waves."""
    opts = opts or {}
    n, total = shape["n_sets"], minhash_total(shape)
    split = n < _cus(shape) * 16 and total > n * 128 and total >= 1024
    if opts.get("minhash.split") == 1:
        split = False
    if opts.get("minhash.split") == 2:
        split = total > 0
    return split


def minhash_per_lane(shape, opts=None):
    """launch_p: permutations per lane of the sieve launch (beyond 64 permutations)."""
    opts = opts or {}
    k, split = shape["num_perm"], minhash_split(shape, opts)
    slots = lambda p: (k + KWAVE * p - 1) // (KWAVE * p) * p  # noqa: E731
    best = 2
    if not split and opts.get("minhash.p3") != 1 and slots(3) <= slots(best):
        best = 3
    if not split and shape["tok"] == "u64" and slots(4) <= slots(best):
        best = 4
    return best


def minhash_shares_last_slot(shape, opts=None):
    """launch_typed: lane groups share the rows of a last slot of at most 32 permutations."""
    opts = opts or {}
    p, k = minhash_per_lane(shape, opts), shape["num_perm"]
    kchunks = (k + KWAVE * p - 1) // (KWAVE * p)
    last = k - (p - 1) * KWAVE
    return k > 64 and not minhash_split(shape, opts) and p >= 3 and kchunks == 1 and opts.get("minhash.share") != 1 and 0 < last <= 32


def minhash_packed(shape, opts=None):
    """launch_typed: several sets per wave (the sieve launch of path 0, one or two permutations per lane)."""
    opts = opts or {}
    k = shape["num_perm"]
    two = k <= 64 or minhash_per_lane(shape, opts) <= 2
    return (not minhash_split(shape, opts) and not opts.get("minhash.path") and opts.get("minhash.packed") != 1 and two
            and (k <= 96 or (opts.get("minhash.packed") == 2 and k <= 128)))


def minhash_prefetch(shape, opts=None):
    v = (opts or {}).get("minhash.prefetch", 1)
    return v == 2 or (v == 1 and (shape["layout"] == "csr" or shape["fixed_len"] < 256))


def minhash_grid(shape, opts=None):
    """launch_typed, wave per set: min(ceil(n / 4), CUs * blocks_per_cu) workgroups."""
    opts = opts or {}
    per_cu = opts.get("blocks_per_cu") or (128 if minhash_per_lane(shape, opts) >= 3 and shape["num_perm"] > 64 else 64)
    return max(1, min((shape["n_sets"] + 3) // 4, _cus(shape) * per_cu))


def _differs(f):
    return lambda shape, key, value: f(shape, {key: value}) != f(shape, {})


def weighted_launch(shape, opts=None):
    return dense_walk_launch(shape["dim"], shape["samples"], True, options=opts or {}, cus=_cus(shape))


def weighted_stored_permille(shape):
    """Stored entries per 1000 columns of the row kinds of a weighted shape."""
    return tuple(int(round(1000 * d)) for d in shape["densities"])


def _direct_set(shape, value):
    limit = value if value > 0 else 100
    return tuple(p <= limit for p in weighted_stored_permille(shape))


def lsh_bin_bits(n):
    bits = 0
    while bits < 14 and (n >> bits) > 2500:
        bits += 1
    return bits


def lsh_bucketing(shape, opts):
    """launch_lsh_sort_bands: the options of the radix path select it."""
    return opts.get("lsh.sort", 0) != 1 and not opts.get("lsh.sort_bits") and not opts.get("lsh.gather") and shape["n"] > 0


def lsh_unit_stride(shape, opts):
    """The bucketing's first pass reads a unit-stride source: band-major digests, or digests / signatures it has turned band-major first."""
    bands = shape["bands"]
    pow2 = 2 <= bands <= 64 and bands & (bands - 1) == 0
    if shape["source"] == "band_major":
        return True
    if shape["source"] == "row_major":
        return pow2
    return pow2 and opts.get("lsh.prehash") != 1


def lsh_one_team_of_1024(shape, opts):
    """launch_scatter_rows<., 16>: one team of 1024 threads x 8 rows per workgroup."""
    if not (lsh_bucketing(shape, opts) and lsh_unit_stride(shape, opts)) or opts.get("lsh.chunk") == 8 or opts.get("lsh.team") == 256:
        return False
    items2 = (shape["n"] + 8191) // 8192 * shape["bands"]
    return items2 >= 8 * _cus(shape) or opts.get("lsh.team") == 1024


def lsh_big_bins(shape, opts):
    bits = lsh_bin_bits(shape["n"])
    return (lsh_bucketing(shape, opts) and opts.get("lsh.bigbins") != 1 and opts.get("lsh.levels") != 2
            and (opts.get("lsh.bigbins") == 2 and bits >= 2))  # (the automatic rule starts at 2.56M rows: no test shape)


def lsh_two_levels(shape, opts):
    return lsh_bucketing(shape, opts) and opts.get("lsh.levels") == 2 and lsh_bin_bits(shape["n"]) >= 2


def pack_fused_takes(shape):
    """The shapes bbit_digest_fused_kernel takes (tests/test_gpu_round5.py): bands * r == num_perm, bands a power of two, r in 4 / 8 / 16,
    and whole groups of bands per 64-bit block."""
    b, bands, r = shape["b"], shape["bands"], shape["r"]
    slot = 1 if b == 1 else 2 if b == 2 else 4 if b <= 4 else 8 if b <= 8 else 16 if b <= 16 else 32
    g = max(1, (64 // slot) // r)
    return bands * r == shape["num_perm"] and bands & (bands - 1) == 0 and r in (4, 8, 16) and bands % g == 0


def hll_lengths(shape):
    base = (0, 1, 63, 64, 65, 257, 1025, 5000)
    lengths = [base[i % len(base)] for i in range(shape["n_sets"])]
    lengths[shape["n_sets"] // 2] = shape["long"]
    return np.asarray(lengths, dtype=np.int64)


def hll_split_sets(shape, value):
    limit = value if value > 0 else 32768  # kHllSplitTokens
    return tuple(np.flatnonzero(hll_lengths(shape) > limit).tolist())


def topk_stream(shape, opts):
    """launch_jaccard_topk: the stream kernel exists for dense and weighted rows; auto takes it for up to 16 probes."""
    path = opts.get("jaccard.topk_path", 0)
    return shape["rows"] != "bbit" and (path == 2 or (path == 0 and shape["m"] <= 16))


def overlap_slots(items):
    s = 64
    while s < 2 * items:
        s <<= 1
    return s


def overlap_bins(shape):
    """The LDS bins (caps 1024 and 4096 slots, then the rest) that the pairs of an overlap shape fall into."""
    sizes = {2 * shape["tiny"], 2 * shape["mid"], 2 * shape["top"]}
    return {0 if overlap_slots(s) <= 1024 else 1 if overlap_slots(s) <= 4096 else 2 for s in sizes}


def host_pieces(shape, value):
    """mhx_minhash_bulk_typed: pieces of `value` bytes of tokens and signatures (fixed-length sets); the host top-k: row blocks of B."""
    if value <= 0:
        return 1
    if shape.get("rows"):
        return -(-shape["n"] // max(1, min(shape["n"], value // (8 * (shape["k_perm"] // 2)))))
    per_set = 8 * shape["fixed_len"] + 8 * shape["num_perm"]
    return -(-shape["n_sets"] // max(1, value // per_set))


APPLIES: Dict[str, Callable] = {
    # MinHash bulk (minhash_kernels.hip)
    "minhash.path": lambda s, k, v: True,
    "minhash.split": _differs(minhash_split),
    "minhash.packed": _differs(minhash_packed),
    "minhash.ties": lambda s, k, v: not minhash_split(s) and s["corpus"] == "repeats",      # the second launch has flagged sets to do
    "minhash.adapt": lambda s, k, v: not minhash_split(s) and not minhash_packed(s),        # the first launch reads the mode word
    "minhash.p3": _differs(minhash_per_lane),
    "minhash.share": _differs(minhash_shares_last_slot),
    "minhash.prefetch": _differs(minhash_prefetch),
    "debug.cus": lambda s, k, v: True,
    # weighted MinHash (weighted_kernels.hip)
    "weighted.path": lambda s, k, v: True,
    "weighted.direct": lambda s, k, v: _direct_set(s, v) != _direct_set(s, 0),
    "weighted.split": lambda s, k, v: s["layout"] == "dense" and weighted_launch(s).kernel == "walk_dense" and any(_direct_set(s, 0)),
    "weighted.tail": lambda s, k, v: s["layout"] == "dense",
    "weighted.plan": lambda s, k, v: s["layout"] == "dense",
    "weighted.kernel": lambda s, k, v: s["layout"] == "dense" and weighted_launch(s, {k: v}).name != weighted_launch(s).name,
    "weighted.refill": lambda s, k, v: s["layout"] == "dense" and weighted_launch(s, {k: v}) != weighted_launch(s) and (v not in (1, 2, 3) or s["dim"] > 2048),
    "weighted.rescue": lambda s, k, v: s["layout"] == "dense" and weighted_launch(s).kernel == "walk_wave" and weighted_launch(s).split == 0,
    "weighted.min_dim": lambda s, k, v: s["layout"] == "dense" and s["dim"] % 4 == 0 and (v == 4 or weighted_launch(s, {k: v}) != weighted_launch(s)),
    # the LSH sort (lsh_kernels.hip)
    "lsh.sort": lambda s, k, v: lsh_bucketing(s, {}),
    "lsh.sort_bits": lambda s, k, v: lsh_bucketing(s, {}),
    "lsh.gather": lambda s, k, v: lsh_bucketing(s, {}),
    "lsh.levels": lambda s, k, v: lsh_two_levels(s, {k: v}),
    "lsh.bigbins": lambda s, k, v: lsh_big_bins(s, {"lsh.bigbins": 2}) and lsh_bin_bits(s["n"]) >= 2,
    "lsh.chunk": lambda s, k, v: lsh_bucketing(s, {}) and lsh_unit_stride(s, {}),
    "lsh.team": _differs(lsh_one_team_of_1024),
    "lsh.prehash": lambda s, k, v: s["source"] == "signatures" and lsh_unit_stride(s, {}) and not lsh_unit_stride(s, {k: v}),
    "lsh.merge_items": lambda s, k, v: s["n_a"] + s["n_b"] > 256 * (v or 8),
    "pack.fused": lambda s, k, v: pack_fused_takes(s),
    "hll.split_tokens": lambda s, k, v: hll_split_sets(s, v) != hll_split_sets(s, 0),
    "bloom.lanes": lambda s, k, v: True,  # auto is 16 lanes for the insert and 1 for the query: either value changes one of the two
    "jaccard.topk_path": _differs(topk_stream),
    "jaccard.topk_segments": lambda s, k, v: s["n"] > 128,
    "overlap.bins": lambda s, k, v: len(overlap_bins(s)) >= 2,
    "host.chunk_bytes": lambda s, k, v: host_pieces(s, v) >= 3 or host_pieces(s, v) == 1 and (v <= 0 or v >= 1 << 40),
}


def _blocks_per_cu_applies(shape, key, value):
    if shape["op"] == "minhash":
        return minhash_grid(shape, {key: value}) != minhash_grid(shape)
    if shape["layout"] == "csr":
        return True  # launch_weighted_csr_walk: min(ceil(n / 4), CUs * n / chunks) groups; the rows of one CU and 16 blocks never fill it
    a, b = weighted_launch(shape, {key: value}), weighted_launch(shape)
    return a.kernel == shape["kernel"] and min(a.rows_per_turn, shape["n_rows"]) != min(b.rows_per_turn, shape["n_rows"])


APPLIES["blocks_per_cu"] = _blocks_per_cu_applies


# ------------------------------------------------------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    key: str
    value: int
    op: str                              # the operation: a runner of tests/test_gpu_options.py and a builder below
    shape: Mapping                       # what the builder makes the input from, and what applies() judges
    reference: str                       # what the result must equal
    reads: Tuple[Tuple[str, str], ...]   # (file of datasketch_amd/csrc, enclosing function) where the option is read on this case's way
    with_options: Mapping = field(default_factory=dict)  # other options the shape needs (debug.cus: a small device)

    @property
    def id(self):
        tail = "_".join(f"{k}{v}" for k, v in self.shape.items() if k not in ("op",) and not isinstance(v, tuple))
        return f"{self.key}={self.value}-{self.op}-{tail}"

    def applies(self, shape: Optional[Mapping] = None, value: Optional[int] = None) -> bool:
        shape = dict(self.shape if shape is None else shape, op=self.op)
        return bool(APPLIES[self.key](shape, self.key, self.value if value is None else value))


CASES = []

ORACLE = "the C oracle (oracle/mh_oracle.c through oracle.oracle)"
TWIN = "the numpy twin"


def _add(key, values, op, shape, reference, reads, cus=0):
    shape = dict(shape, cus=cus)
    for v in values:
        CASES.append(Case(key, v, op, shape, reference, tuple(reads), {"debug.cus": cus} if cus else {}))


MH, WK, LK, API = "minhash_kernels.hip", "weighted_kernels.hip", "lsh_kernels.hip", "mhx_api.hip"


def _mh(num_perm, tok="u64", layout="csr", fixed_len=0, n_sets=300, corpus="random"):
    return dict(num_perm=num_perm, tok=tok, layout=layout, fixed_len=fixed_len, n_sets=n_sets, corpus=corpus)


# --- MinHash bulk: a few hundred ragged sets (mean length below 128, so that the launcher keeps a wave per set)
_add("minhash.path", (1, 2), "minhash", _mh(128, corpus="near_zero"), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.path", (1, 2), "minhash", _mh(144, tok="u32", corpus="repeats"), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.split", (1,), "minhash", _mh(128, layout="fixed", fixed_len=5000, n_sets=3), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.split", (2,), "minhash", _mh(128, corpus="repeats"), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.split", (2,), "minhash", _mh(208, tok="u32"), ORACLE, [(MH, "launch_minhash_bulk")])
for _k in (64, 96):
    _add("minhash.packed", (1,), "minhash", _mh(_k, tok="u32" if _k == 64 else "u64"), ORACLE, [(MH, "launch_typed")])
_add("minhash.packed", (2,), "minhash", _mh(128), ORACLE, [(MH, "launch_typed")])
_add("minhash.packed", (2,), "minhash", _mh(128, tok="u32", layout="fixed", fixed_len=100), ORACLE, [(MH, "launch_typed")])
_add("minhash.ties", (1,), "minhash", _mh(128, corpus="repeats"), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.ties", (1,), "minhash", _mh(300, tok="u32", corpus="repeats"), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.adapt", (1,), "minhash", _mh(128, corpus="repeats"), ORACLE, [(MH, "launch_typed")])
_add("minhash.adapt", (1,), "minhash", _mh(208, tok="u32", corpus="repeats"), ORACLE, [(MH, "launch_typed")])
for _k, _tok in ((144, "u64"), (144, "u32"), (300, "u64")):
    _add("minhash.p3", (1,), "minhash", _mh(_k, tok=_tok), ORACLE, [(MH, "launch_p")])
for _k, _tok in ((144, "u64"), (144, "u32"), (208, "u64")):
    _add("minhash.share", (1,), "minhash", _mh(_k, tok=_tok), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.prefetch", (0,), "minhash", _mh(128), ORACLE, [(MH, "launch_minhash_bulk")])
_add("minhash.prefetch", (0,), "minhash", _mh(144, tok="u32", layout="fixed", fixed_len=255), ORACLE, [(MH, "launch_minhash_bulk")])
# (fixed lengths of 256 and more with a wave per set: a device of one CU, or 300 sets of 256 tokens would be split over waves)
_add("minhash.prefetch", (2,), "minhash", _mh(128, layout="fixed", fixed_len=256, n_sets=67), ORACLE, [(MH, "launch_minhash_bulk")], cus=1)
_add("minhash.prefetch", (2,), "minhash", _mh(96, tok="u32", layout="fixed", fixed_len=300, n_sets=67), ORACLE, [(MH, "launch_minhash_bulk")], cus=1)
_add("blocks_per_cu", DOMAIN["blocks_per_cu"].representatives()[1:] + (1,), "minhash", _mh(128, corpus="repeats"), ORACLE, [(MH, "launch_typed")], cus=1)
_add("debug.cus", (1, 3, MI355X_CUS), "minhash", _mh(128, n_sets=1103, corpus="repeats"), ORACLE, [])
_add("host.chunk_bytes", (I64_MIN, 4096, I64_MAX), "minhash_host", _mh(128, layout="fixed", fixed_len=100), ORACLE, [(API, "mhx_minhash_bulk_typed")])
_add("host.chunk_bytes", (I64_MIN, 4096, I64_MAX), "topk_host", dict(rows="dense", m=3, n=300, k_perm=64, k=10), TWIN, [(API, "all_pairs_topk")])


# --- weighted MinHash: dense rows of mixed density (entry-by-entry rows, walked rows, two empty rows), logs in and values in
def _wm(dim, samples, n_rows=40, densities=(0.02, 0.09, 0.3, 1.0), layout="dense", kernel=None):
    shape = dict(dim=dim, samples=samples, n_rows=n_rows, densities=densities, layout=layout)
    if kernel:
        shape["kernel"] = kernel
    return shape


_DENSE_WALK, _DENSE, _CSR = (WK, "launch_weighted_dense_walk"), (WK, "launch_weighted_dense"), (WK, "launch_weighted")
_add("weighted.path", (1, 2), "weighted", _wm(64, 64), ORACLE, [_DENSE])
_add("weighted.path", (1, 2), "weighted", _wm(64, 64, layout="csr"), ORACLE, [_CSR])
_add("weighted.direct", (1, 500, 1000), "weighted", _wm(200, 64, densities=(0.02, 0.09, 0.3, 0.6, 1.0)), ORACLE, [_DENSE_WALK])
_add("weighted.direct", (1, 500, 1000), "weighted", _wm(1022, 128, densities=(0.02, 0.09, 0.3, 0.6, 1.0)), ORACLE, [_DENSE_WALK])
_add("weighted.direct", (1, 500, 1000), "weighted", _wm(200, 64, densities=(0.02, 0.09, 0.3, 0.6, 1.0), layout="csr"), ORACLE, [(WK, "launch_weighted_csr_walk")])
_add("weighted.split", (1,), "weighted", _wm(1022, 128, densities=(0.02, 0.05, 0.09, 1.0)), ORACLE, [_DENSE_WALK])
_add("weighted.tail", (3, 5), "weighted", _wm(64, 64), ORACLE, [(WK, "launch_walk_plan")])
_add("weighted.tail", (3, 5), "weighted", _wm(1022, 128), ORACLE, [(WK, "launch_walk_plan")])
_add("weighted.plan", (1,), "weighted", _wm(64, 64), ORACLE, [(WK, "launch_walk_plan")])
_add("weighted.plan", (1,), "weighted", _wm(1024, 128), ORACLE, [(WK, "launch_walk_plan")])
_add("weighted.kernel", (1, 2), "weighted", _wm(64, 64), ORACLE, [_DENSE_WALK])
_add("weighted.kernel", (1, 2), "weighted", _wm(1024, 200), ORACLE, [_DENSE_WALK])
_add("weighted.refill", (5, 6, 8, 9, 13), "weighted", _wm(64, 128), ORACLE, [_DENSE_WALK])
_add("weighted.refill", (1, 2, 3, 13), "weighted", _wm(4096, 128, n_rows=24), ORACLE, [_DENSE_WALK])
_add("weighted.rescue", (I64_MIN, 1, 64), "weighted", _wm(64, 64, densities=(0.3, 0.6, 1.0)), ORACLE, [_DENSE_WALK])
_add("weighted.rescue", (I64_MIN, 1, 64), "weighted", _wm(1024, 64, densities=(0.3, 0.6, 1.0)), ORACLE, [_DENSE_WALK])
_add("weighted.min_dim", (4, 64, 4096), "weighted", _wm(32, 64), ORACLE, [_DENSE_WALK])
_add("weighted.min_dim", (4096,), "weighted", _wm(1024, 128), ORACLE, [_DENSE_WALK])
# (one CU: a turn of the grid is 1 .. a few rows, so that blocks_per_cu changes how many turns the rows take)
_add("blocks_per_cu", (1, 4, MAX_BLOCKS_PER_CU), "weighted", _wm(64, 64, n_rows=131, kernel="walk_wave"), ORACLE, [_DENSE_WALK], cus=1)
_add("blocks_per_cu", (1, 2, MAX_BLOCKS_PER_CU), "weighted", _wm(62, 64, n_rows=67, kernel="walk_dense"), ORACLE, [_DENSE_WALK], cus=1)
_add("blocks_per_cu", (1, 4, MAX_BLOCKS_PER_CU), "weighted", _wm(64, 64, n_rows=67, layout="csr"), ORACLE, [(WK, "launch_weighted_csr_walk")], cus=1)


# --- the LSH sort: a few thousand rows (5 003: four bins per band), digests with runs of equal values
def _ls(source, n=5003, bands=4, **more):
    return dict(source=source, n=n, bands=bands, **more)


_SORT, _BUCKET, _SCATTER = (LK, "launch_lsh_sort_bands"), (LK, "launch_lsh_bucket_bands"), (LK, "launch_scatter_rows")
for _src in ("row_major", "band_major"):
    _add("lsh.sort", (1,), "lsh_sort", _ls(_src), TWIN, [_SORT])
    _add("lsh.sort_bits", (1, 20, 64), "lsh_sort", _ls(_src), TWIN, [_SORT])
    _add("lsh.gather", (1,), "lsh_sort", _ls(_src), TWIN, [_SORT])
    _add("lsh.levels", (2,), "lsh_sort", _ls(_src), TWIN, [_BUCKET])
    _add("lsh.bigbins", (1, 2), "lsh_sort", _ls(_src), TWIN, [_BUCKET])
    _add("lsh.chunk", (8,), "lsh_sort", _ls(_src), TWIN, [(LK, "scatter_rows")])
    _add("lsh.team", (1024,), "lsh_sort", _ls(_src), TWIN, [_SCATTER])
    _add("lsh.team", (256,), "lsh_sort", _ls(_src, bands=8), TWIN, [_SCATTER], cus=1)  # one CU: 8 items are "eight per CU", auto takes the one team
_add("lsh.prehash", (1,), "lsh_sort", _ls("signatures", num_perm=64, r=16, dtype="u32"), TWIN, [_SORT])
_add("lsh.prehash", (1,), "lsh_sort", _ls("signatures", num_perm=128, r=8, bands=16, dtype="u64"), TWIN, [_SORT])
_add("lsh.merge_items", (8, 16), "lsh_merge", dict(bands=3, n_a=3000, n_b=2501), TWIN, [("lsh_index_kernels.hip", "launch_lsh_bands_merge")])

# --- packers, HyperLogLog, Bloom filters, top-k, overlaps
for _tok in ("u32", "u64"):
    _add("pack.fused", (1,), "pack_digests", dict(n=517, num_perm=128, bands=32, r=4, b=4, dtype=_tok), ORACLE + " and " + TWIN, [(API, "mhx_bbit_pack_band_digests_dev")])
for _p, _tok in ((4, "u32"), (10, "u64"), (14, "u32")):
    _add("hll.split_tokens", (1, 64, I64_MAX), "hll", dict(p=_p, n_sets=67, long=40000, dtype=_tok), TWIN, [("hll_kernels.hip", "launch_hll_bulk")])
for _tok in ("u32", "u64"):
    _add("bloom.lanes", (1, 16), "bloom", dict(n=321, num_perm=64, bands=9, r=7, k=14, n_blocks=97, dtype=_tok), TWIN, [("bloom_kernels.hip", "launch_lanes")])
_TOPK = ("jaccard_topk_kernels.hip", "launch_jaccard_topk")
for _rows in ("dense", "weighted"):
    _add("jaccard.topk_path", (1,), "topk", dict(rows=_rows, m=3, n=300, k_perm=64, k=10), TWIN, [_TOPK])
    _add("jaccard.topk_path", (2,), "topk", dict(rows=_rows, m=130, n=300, k_perm=64, k=10), TWIN, [_TOPK])
for _rows, _m in (("dense", 3), ("dense", 130), ("bbit", 130), ("weighted", 3), ("weighted", 130)):
    _add("jaccard.topk_segments", (1, 3, I64_MAX), "topk", dict(rows=_rows, m=_m, n=300, k_perm=64, k=10), TWIN, [_TOPK])
for _tok in ("u32", "u64"):
    _add("overlap.bins", (1, 2), "overlap", dict(tiny=8, mid=750, top=1500, n_pairs=400, dtype=_tok), TWIN, [("overlap_kernels.hip", "launch_typed")])


# ------------------------------------------------------------------------------------------------------------------ inputs and references
_BUILT = {}


def build(case):
    """The input and the reference of a case's (op, shape), made once and frozen."""
    key = (case.op, tuple(sorted((k, v) for k, v in case.shape.items() if k != "cus")))
    if key not in _BUILT:
        made = _BUILDERS[case.op](dict(case.shape))
        for v in made.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _BUILT[key] = made
    return _BUILT[key]


def _tokens(rng, count, tok):
    hi = rng.randint(0, 2**29, size=count, dtype=np.uint64) << np.uint64(32) if tok == "u64" else np.uint64(0)
    return rng.randint(0, 2**32, size=count, dtype=np.uint64) | hi


def _build_minhash(shape):
    from oracle import oracle as O
    k, n = shape["num_perm"], shape["n_sets"]
    a, b = O.np_init_permutations(k, 1)
    rng = np.random.RandomState(k + n)
    lengths = minhash_lengths(shape)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    hv = _tokens(rng, int(offsets[-1]), shape["tok"])
    planted = 0
    if shape["corpus"] == "repeats":  # every third set repeats its own tokens: equal tokens at the minimum defeat the first proof
        for i in range(0, n, 3):
            lo, hi = int(offsets[i]), int(offsets[i + 1])
            half = (hi - lo) // 2
            if half:
                hv[lo + half: hi] = hv[lo: lo + half][rng.randint(0, half, size=hi - lo - half)]
    if shape["corpus"] == "near_zero":
        # a token whose hash under permutation pi has a low word of 0 .. 6: the fast fold of minhash.path 2 cannot tell such a
        # minimum from a wrapped one and redoes the set with the exact fold (tests/test_gpu_parity.py, near minima)
        long_sets = np.flatnonzero(lengths >= 63)
        for j, i in enumerate(long_sets[:48]):
            pi = j % 24
            a_lo, b_lo = int(a[pi]) & 0xFFFFFFFF, int(b[pi]) & 0xFFFFFFFF
            if a_lo % 2 == 0:
                continue
            low = ((j % 7) - b_lo) * pow(a_lo, -1, 1 << 32) % 2**32
            hv[int(offsets[i]) + j % 60] = low
            planted += 1
    want = O.c_minhash_bulk(hv, offsets, a, b)
    return dict(a=a, b=b, hv=hv.astype(np.uint32 if shape["tok"] == "u32" else np.uint64), offsets=offsets, want=want, planted=np.int64(planted))


def _build_weighted(shape):
    import scipy.sparse as sp

    from datasketch_amd.weighted_minhash import WeightedMinHashGenerator
    from oracle import oracle as O
    dim, s, n = shape["dim"], shape["samples"], shape["n_rows"]
    g = WeightedMinHashGenerator(dim, s, seed=11, gpu_mode="disable")
    rng = np.random.RandomState(dim + s + n)
    x = rng.lognormal(0, 2.0, (n, dim)).astype(np.float32)
    dens = np.asarray(shape["densities"])
    for i in range(n):  # exactly round(density * dim) stored entries per row: the stored share is what weighted.direct compares
        keep = int(round(dens[i % len(dens)] * dim))
        x[i, rng.permutation(dim)[keep:]] = 0
    x[7] = 0
    x[n - 2] = 0
    csr = sp.csr_matrix(x)
    csr.sort_indices()
    with np.errstate(invalid="ignore", divide="ignore"):
        want, wn = O.c_weighted_minhash_many(csr.indptr, csr.indices, csr.data, g.rs, g.ln_cs, g.betas)
        logs = np.log(x)
        want_v, wn_v = O.c_weighted_minhash_many(csr.indptr, csr.indices, csr.data, g.rs, g.ln_cs, g.betas, logs=O.c_np_logf(csr.data))
        csr_logs = np.log(csr.data)
    assert np.array_equal(wn_v, wn)
    return dict(rs=g.rs, ln_cs=g.ln_cs, betas=g.betas, x=x, logs=logs, indptr=csr.indptr.astype(np.int64), indices=csr.indices.astype(np.int32),
                data=csr.data.astype(np.float32), data_logs=csr_logs.astype(np.float32), want=want, want_values=want_v, nonempty=wn.astype(bool))


def _build_lsh_sort(shape):
    from datasketch_amd import lsh_bulk
    n, bands = shape["n"], shape["bands"]
    rng = np.random.RandomState(n + bands)
    made = {}
    if shape["source"] == "signatures":
        k, r = shape["num_perm"], shape["r"]
        hi = 2**32 if shape["dtype"] == "u32" else 2**63
        sig = rng.randint(0, hi, (n, k), dtype=np.uint64)
        dup = rng.randint(0, n, n // 3)
        sig[dup, : 2 * r] = sig[(dup * 7) % n, : 2 * r]  # rows that share their first two bands with another row
        dig = lsh_bulk.band_digests(sig, bands, r, gpu_mode="disable")
        made["sig"] = sig.astype(np.uint32 if shape["dtype"] == "u32" else np.uint64)
    else:
        dig = rng.randint(0, 2**63, (n, bands), dtype=np.uint64) * np.uint64(2) + rng.randint(0, 2, (n, bands)).astype(np.uint64)
        dig[rng.randint(0, n, 600), 1] = dig[0, 1]     # a long run of one digest
        dup = rng.randint(0, n, n // 3)
        dig[dup, 2] = dig[(dup * 7) % n, 2]            # many short runs
        # (the top bits of every band stay spread over the bins: a bin of more than 3072 entries would send the call to the radix sort)
    order = np.stack([np.lexsort((np.arange(n), dig[:, j])) for j in range(bands)])
    made.update(dig=dig, dig_bm=np.ascontiguousarray(dig.T), want_rows=order.astype(np.uint32), want_dig=np.take_along_axis(dig.T, order, axis=1))
    return made


def _build_lsh_merge(shape):
    bands, n_a, n_b = shape["bands"], shape["n_a"], shape["n_b"]
    rng = np.random.RandomState(n_a + n_b)
    dig_a, dig_b = (np.sort(rng.randint(0, 700, size=(bands, n)).astype(np.uint64) << np.uint64(40), axis=1) for n in (n_a, n_b))
    rows_a, rows_b = (np.stack([rng.permutation(n) for _ in range(bands)]).astype(np.uint32) for n in (n_a, n_b))
    dig = np.concatenate([dig_a, dig_b], axis=1)
    order = np.argsort(dig, axis=1, kind="stable")  # A's entries first among equal digests
    return dict(dig_a=dig_a, rows_a=rows_a, dig_b=dig_b, rows_b=rows_b, offset=np.int64(100000), want_dig=np.take_along_axis(dig, order, axis=1),
                want_rows=np.take_along_axis(np.concatenate([rows_a, rows_b + np.uint32(100000)], axis=1), order, axis=1))


def _build_pack_digests(shape):
    from datasketch_amd import lsh_bulk
    from oracle import oracle as O
    rng = np.random.RandomState(shape["n"])
    hi = 2**32 if shape["dtype"] == "u32" else 2**63
    sig = rng.randint(0, hi, (shape["n"], shape["num_perm"]), dtype=np.uint64)
    return dict(sig=sig.astype(np.uint32 if shape["dtype"] == "u32" else np.uint64), want_blocks=O.c_bbit_pack(sig, shape["b"]),
                want_dig=lsh_bulk.band_digests(sig, shape["bands"], shape["r"], gpu_mode="disable"))


def _build_hll(shape):
    from datasketch_amd import hyperloglog as H
    wide = shape["dtype"] == "u64"
    bits, dtype = (64, np.uint64) if wide else (32, np.uint32)
    lengths = hll_lengths(shape)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    rng = np.random.RandomState(shape["p"])
    count = int(offsets[-1])
    hv = rng.randint(0, 2**32, size=count, dtype=np.uint64)
    if wide:
        hv = (hv << np.uint64(32)) | rng.randint(0, 2**32, size=count, dtype=np.uint64)
    hv >>= rng.randint(0, bits, size=count).astype(np.uint64)  # long runs of leading zeros: high ranks
    hv = hv.astype(dtype)
    init = rng.randint(0, 9, size=(shape["n_sets"], 1 << shape["p"])).astype(np.uint8)
    return dict(hv=hv, offsets=offsets, init=init, bits=np.int64(bits), want=H._registers_host(hv, offsets, 0, shape["n_sets"], shape["p"], bits, None),
                want_init=H._registers_host(hv, offsets, 0, shape["n_sets"], shape["p"], bits, init))


def _build_bloom(shape):
    from datasketch_amd import lsh_bloom as B
    n, k_perm, b, r, k, nb = (shape[x] for x in ("n", "num_perm", "bands", "r", "k", "n_blocks"))
    dtype = np.uint32 if shape["dtype"] == "u32" else np.uint64
    rng = np.random.RandomState(n + nb)
    draw = lambda: rng.randint(0, 2**32 if dtype == np.uint32 else 2**63, size=(n, k_perm), dtype=np.uint64).astype(dtype)  # noqa: E731
    old = rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01010101)
    sig, shared = draw(), draw()
    shared[:, (b - 1) * r: b * r] = sig[:, (b - 1) * r: b * r]
    probes = np.vstack([sig, shared, draw()])
    want = old.copy()
    B.insert_host(want, sig, r, k)
    return dict(old=old, sig=sig, probes=probes, want=want, want_hit=B.query_host(want, probes, r, k))


def topk_want(counts, k):
    """(rows int64 [m, k], counts int32 [m, k]): the best k by (count descending, row ascending), padded with -1."""
    low = np.uint64(0xFFFFFFFF)
    m, n = counts.shape
    key = (counts.astype(np.uint64) << np.uint64(32)) | (low - np.arange(n, dtype=np.uint64))[None, :]
    top = np.sort(key, axis=1)[:, ::-1][:, :k]
    rows, cnt = np.full((m, k), -1, dtype=np.int64), np.full((m, k), -1, dtype=np.int32)
    rows[:, : top.shape[1]] = (low - (top & low)).astype(np.int64)
    cnt[:, : top.shape[1]] = (top >> np.uint64(32)).astype(np.int32)
    return rows, cnt


def _build_topk(shape):
    m, n, kp, k = shape["m"], shape["n"], shape["k_perm"], shape["k"]
    rng = np.random.RandomState(m + n)
    if shape["rows"] == "weighted":
        from tests.weighted_jaccard_guard_cases import planted_weighted, want_matrix
        a, b = planted_weighted(rng, m, n, kp)
        counts = want_matrix(a, b)
        made = dict(a=a, b=b)
    else:
        base = rng.randint(0, 2**32, size=(12, kp), dtype=np.uint64)  # families of rows: many equal counts, ties at the k-th place

        def family(count):
            rows = base[rng.randint(0, 12, size=count)]
            redraw = rng.random_sample(rows.shape) < rng.choice([0.0, 0.25, 0.5], size=(count, 1))
            rows[redraw] = rng.randint(0, 2**32, size=int(redraw.sum()), dtype=np.uint64)
            return rows
        a, b = family(m), family(n)
        if shape["rows"] == "bbit":
            from oracle import oracle as O
            a, b = a & np.uint64(15), b & np.uint64(15)
            made = dict(a=O.c_bbit_pack(a, 4), b=O.c_bbit_pack(b, 4))
        else:
            made = dict(a=a.astype(np.uint32), b=b.astype(np.uint32))
        counts = np.count_nonzero(a[:, None, :] == b[None, :, :], axis=2).astype(np.int32)
    s = np.sort(counts, axis=1)[:, ::-1]
    assert np.any(s[:, k - 1] == s[:, k]), "no tie at the k-th place"
    rows, cnt = topk_want(counts, k)
    made.update(want_rows=rows, want_counts=cnt)
    return made


def _build_overlap(shape):
    from datasketch_amd import overlap
    dtype = np.uint32 if shape["dtype"] == "u32" else np.uint64
    rng = np.random.RandomState(shape["n_pairs"])
    top = 2**32 if dtype == np.uint32 else 2**63
    sets = [rng.randint(0, 12, rng.randint(0, shape["tiny"] + 1)).astype(dtype) for _ in range(50)]
    for size, groups in ((shape["mid"], 4), (shape["top"], 4)):  # sets of one group draw from one pool of values: they overlap
        pool = rng.randint(0, top, size=size + size // 8, dtype=np.uint64).astype(dtype)
        sets += [pool[rng.randint(0, pool.size, size)] for _ in range(groups)]
    offsets = np.zeros(len(sets) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in sets], out=offsets[1:])
    hashes = np.concatenate(sets).astype(dtype)
    pairs = np.concatenate([rng.randint(0, 50, size=(shape["n_pairs"] - 40, 2)), 50 + rng.randint(0, 4, size=(20, 2)), 54 + rng.randint(0, 4, size=(20, 2))])
    pairs = pairs[rng.permutation(len(pairs))].astype(np.int64)
    return dict(hashes=hashes, offsets=offsets, pairs=pairs, want=overlap.overlap_counts_host(hashes, offsets, pairs))


_BUILDERS = {"minhash": _build_minhash, "minhash_host": _build_minhash, "weighted": _build_weighted, "lsh_sort": _build_lsh_sort,
             "lsh_merge": _build_lsh_merge, "pack_digests": _build_pack_digests, "hll": _build_hll, "bloom": _build_bloom, "topk": _build_topk,
             "topk_host": _build_topk, "overlap": _build_overlap}
