"""What launch_weighted_dense_walk (datasketch_amd/csrc/weighted_kernels.hip) launches for dense rows: the kernel, its
template arguments and the rows one turn of its grid takes.  A plain restatement of that function for the tests, line by
line (the numbers in the comments are that file's lines); it reads nothing from a device.  That function runs for dense
rows when the generator has walk tables and option weighted.path is 0 (launch_weighted_dense, line 2241).

The weighted GPU tests name their cases and size their row counts by it, so a change of the launcher's rules is made here
as well; tests/test_weighted_dispatch.py pins it on worked cases.
"""
from dataclasses import dataclass
from typing import Mapping, Optional

KWAVE = 64
K_WALK_CACHED = 8        # kWalkCached
K_CACHED_CHUNKS = 4      # kCachedChunks
K_SPLIT_HAND_WORDS2 = 128  # kSplitHandWords2
K_PRE = 4                # kPre
MI355X_CUS = 256
MI355X_LDS_PER_BLOCK = 160 << 10  # hipDeviceProp_t::sharedMemPerBlock on gfx950


def _div(a: int, b: int) -> int:
    """C++ integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


@dataclass(frozen=True)
class DenseLaunch:
    kernel: str                    # "walk_wave" (weighted_walk_wave_kernel) or "walk_dense" (weighted_walk_dense_kernel)
    nv: Optional[int] = None       # walk_wave: <LOGS, NV, PAIRS, FETCH, SPLIT>
    pairs: Optional[bool] = None
    fetch: Optional[int] = None
    split: Optional[int] = None
    ahead: Optional[bool] = None   # walk_dense: <LOGS, AHEAD>
    rows_per_turn: int = 0         # rows a full grid takes at once: one per workgroup, per wave, or per stripe / fetcher (SPLIT 2)

    @property
    def name(self) -> str:
        """The instantiation without LOGS (the tests run both): walk_wave_NV4_PAIRS_true_FETCH0_SPLIT0, walk_dense_AHEAD_false."""
        if self.kernel == "walk_wave":
            return f"walk_wave_NV{self.nv}_PAIRS_{str(self.pairs).lower()}_FETCH{self.fetch}_SPLIT{self.split}"
        return f"walk_dense_AHEAD_{str(self.ahead).lower()}"


def dense_walk_launch(dim: int, sample_size: int, values_are_logs: bool, aligned: bool = True, options: Optional[Mapping[str, int]] = None,
                      cus: int = MI355X_CUS, lds_per_block: int = MI355X_LDS_PER_BLOCK) -> DenseLaunch:
    """The launch of launch_weighted_dense_walk for a generator of (dim, sample_size) with the context options `options`
    (mhx_ctx_set_option keys; absent = 0) on a device of `cus` CUs.  aligned: the matrix starts on a 16-byte boundary.
    rows_per_turn: workgroups of a full grid (n_rows large) times the rows each holds at once."""
    opts = dict(options or {})
    opt = lambda key: int(opts.get(key, 0))  # noqa: E731
    s_pad = (sample_size + KWAVE - 1) // KWAVE * KWAVE
    list_cap = max(64, _div(dim, 4))                                                                         # 2140
    # the one-wave-per-row kernel                                                                            # 2144-2212
    n_cc_w = min(s_pad // KWAVE, K_CACHED_CHUNKS)                                                             # 2145
    cache_bytes = 20 * n_cc_w * K_WALK_CACHED * KWAVE                                                         # 2146
    list_cap_w = max(64, _div(dim, 8))                                                                       # 2147
    stripe_bytes = (4 * ((dim + 3) & ~3) + 2 * ((list_cap_w + 7) & ~7) + 15) & ~15                            # 2148
    fit = _div(lds_per_block - cache_bytes - 64, stripe_bytes)                                               # 2149
    waves = min(8, fit)                                                                                      # 2150
    min_dim_w = opt("weighted.min_dim") if opt("weighted.min_dim") > 0 else 4                                # 2151
    shape_ok = (dim & 3) == 0 and aligned and dim >= min_dim_w and dim <= 4096                                # 2152
    if shape_ok and waves >= 4 and opt("weighted.kernel") != 1:                                              # 2153
        lds = cache_bytes + stripe_bytes * waves                                                             # 2154
        per_cu = opt("blocks_per_cu") if opt("blocks_per_cu") > 0 else max(1, _div(lds_per_block, lds + 64))  # 2156
        nv = 4 if dim <= 1024 else 8 if dim <= 2048 else 16                                                  # 2158
        rf = opt("weighted.refill")                                                                          # 2182
        chunks_w = s_pad // KWAVE                                                                            # 2185
        chunks_ok = chunks_w in (2, 3, 4, 6)                                                                 # 2186
        groups2 = _div(12, chunks_w) if chunks_ok else 1                                                     # 2187
        n_stripes2 = groups2 + 1 if chunks_w != 2 else 5 if rf == 6 else 8 if rf == 8 else 6 if rf in (5, 9) else 7  # 2188
        cached2 = K_WALK_CACHED if rf in (5, 8) else 16 if rf in (6, 9) else 12                               # 2189
        n_fetch2 = 6 if rf == 6 and chunks_w == 2 else 4                                                     # 2190
        lds2 = 20 * n_cc_w * cached2 * KWAVE + 4 * K_SPLIT_HAND_WORDS2 + stripe_bytes * n_stripes2            # 2192
        split = 2 if (rf == 0 or 5 <= rf <= 9) and opt("weighted.kernel") == 0 and chunks_ok and lds2 <= lds_per_block else 0  # 2193
        auto_fetch = rf in (0, 13)                                                                           # 2195
        fetch_mode = (2 if values_are_logs else 3) if auto_fetch else 0 if rf == 1 else rf & 3               # 2196
        if opt("weighted.kernel") == 0:                                                                      # 2199
            pairs = not (nv == 16 and not values_are_logs and auto_fetch)
        else:
            pairs = opt("weighted.kernel") != 2
        if split == 2:  # MHX_WALK_WAVE_NV, 2165-2167: <LOGS, NV, false, 2, 2>; one workgroup per CU (2194), a row per stripe or per fetcher (1736-1758)
            return DenseLaunch("walk_wave", nv=nv, pairs=False, fetch=2, split=2, rows_per_turn=cus * max(n_stripes2, n_fetch2))
        fetch = fetch_mode if nv == 16 and fetch_mode in (2, 3) else 0                                       # 2168-2172
        return DenseLaunch("walk_wave", nv=nv, pairs=pairs, fetch=fetch, split=0, rows_per_turn=per_cu * cus * waves)  # 2157, 1546: one row per wave
    # the workgroup-per-row kernel                                                                           # 2213-2231
    threads = 256
    n_cc = min(s_pad // KWAVE, K_CACHED_CHUNKS)                                                               # 2215
    lds = 4 * ((dim + 3) & ~3) + 2 * ((list_cap + 7) & ~7) + 20 * n_cc * K_WALK_CACHED * KWAVE                # 2216
    per_cu = opt("blocks_per_cu") if opt("blocks_per_cu") > 0 else max(1, min(4, _div(160 << 10, lds + 64)))  # 2217-2218
    ahead = (dim & 3) == 0 and aligned and 4 <= dim <= K_PRE * 4 * threads                                    # 2220
    return DenseLaunch("walk_dense", ahead=ahead, rows_per_turn=per_cu * cus)                                # 2219: one row per workgroup
