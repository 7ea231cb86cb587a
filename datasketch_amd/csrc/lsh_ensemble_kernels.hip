// lsh_ensemble_kernels.hip -- the containment query of datasketch_amd.MinHashLSHEnsemble (mhx_lsh_ensemble_query_dev).
//
// Reference: MinHashLSHEnsemble.query (datasketch/lshensemble.py:230-249) walks num_part partitions; in each it picks (b, r) from
// upper bound / probe size and asks the partition's MinHashLSH of r rows per band for the buckets of its first b bands
// (lsh.py:545-557).  Here the partitions are slot ranges of one size-sorted signature matrix and every distinct r is a *level*: per
// partition a block of sorted bands, laid out as mhx_lsh_sort_bands_dev_typed writes them for the partition's rows (include/mhx.h).
// One call answers all probes in all partitions: the work items are (probe q, partition p, band j < b(q, p)) -- the sum of the
// chosen b, not probes x partitions x bands -- and each item is the search of launch_lsh_query's query_ranges_kernel in the block
// the item's (level, partition) selects.  The candidates then take the tail launch_lsh_query takes (lsh_raw_pairs_*).
//
//   1. band digests of the probes, once per level that the table uses (launch_band_digests, the level's largest b bands only);
//   2. b(q, p) per (probe, partition) pair -> exclusive scan = the pair's first item; the total T comes back to the host;
//   3. every pair names itself in its b items (ensemble_items_kernel), so that an item finds (q, p, j) with two loads;
//   4. ensemble_ranges_kernel: one thread per item, lower bound + galloping upper bound in the band of n_p digests;
//   5. exclusive scan of the run lengths; ensemble_emit_kernel compares the band's r words and writes (q << 32) | (start[p] + row);
//   6. sort, unique, unpack (lsh_raw_pairs_finish).
// The search is a chain of ~log2(n_p) dependent loads into cold memory per item; one thread per item keeps as many chains in
// flight as there are lanes, which is what hides them.
#include "device_scan.h"
#include "mhx_internal.h"

namespace mhx {
namespace {

struct EnsLevel {
    const uint64_t *dig;   // [bands * n]: partition p's block from bands * start[p], band j of it from j * n_p
    const uint32_t *rows;  // the same positions: rows local to the partition
    const uint64_t *qdig;  // [m][qbands]: the probes' digests of this level's first qbands bands
    int32_t r, bands, qbands, pad;
};
struct EnsTable {  // lives in device memory for the call (scratch[2]): indexed by data, so not a kernel argument
    EnsLevel level[MHX_ENSEMBLE_MAX_LEVELS];
    int32_t p_level[MHX_ENSEMBLE_MAX_PARAMS], p_b[MHX_ENSEMBLE_MAX_PARAMS];
    int32_t n_params, pad;
};

struct PairBandsIn {  // value = b of the table row the pair's choice byte names; 0 for a byte that names none (255: unused partition)
    const uint8_t *choice;
    const EnsTable *tab;
    __device__ __forceinline__ uint32_t get(int64_t i) const {
        const int c = choice[i];
        return c < tab->n_params ? (uint32_t)tab->p_b[c] : 0u;
    }
};

// item_pair[item_off[i] + j] = i for the b items of pair i
__global__ __launch_bounds__(256) void ensemble_items_kernel(const uint8_t *__restrict__ choice, const EnsTable *__restrict__ tab,
                                                             const uint64_t *__restrict__ item_off, int64_t n_pairs, int64_t n_items,
                                                             uint32_t *__restrict__ item_pair) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_pairs; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t b = PairBandsIn{choice, tab}.get(i);
        const int64_t at = (int64_t)item_off[i];
        for (uint32_t j = 0; j < b && at + j < n_items; ++j) item_pair[at + j] = (uint32_t)i;
    }
}

struct Item {  // what item t searches: band j of partition p's block of one level, for probe q
    int64_t q, s0, n_p, band_at;  // band_at: where the band starts in the level's buffers
    int32_t j, r;
    const EnsLevel *lv;
};
__device__ __forceinline__ Item item_of(int64_t t, const uint32_t *item_pair, const uint64_t *item_off, const uint8_t *choice,
                                        const EnsTable *tab, const int64_t *start, int32_t n_parts) {
    const int64_t pair = item_pair[t];
    Item it;
    it.j = (int32_t)(t - (int64_t)item_off[pair]);
    it.q = pair / n_parts;
    const int64_t p = pair - it.q * n_parts;
    it.lv = &tab->level[tab->p_level[choice[pair]]];  // (an item exists only where the byte names a row of the table)
    it.r = it.lv->r;
    it.s0 = start[p];
    it.n_p = start[p + 1] - it.s0;
    it.band_at = (int64_t)it.lv->bands * it.s0 + (int64_t)it.j * it.n_p;
    return it;
}

// per item: first = position of the first equal digest in its band, count = the run's length
__global__ __launch_bounds__(256) void ensemble_ranges_kernel(const uint32_t *__restrict__ item_pair, const uint64_t *__restrict__ item_off,
                                                              const uint8_t *__restrict__ choice, const EnsTable *__restrict__ tab,
                                                              const int64_t *__restrict__ start, int32_t n_parts, int64_t n_items,
                                                              uint32_t *__restrict__ first, uint32_t *__restrict__ count) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_items; t += (int64_t)gridDim.x * blockDim.x) {
        const Item it = item_of(t, item_pair, item_off, choice, tab, start, n_parts);
        const uint64_t d = it.lv->qdig[it.q * it.lv->qbands + it.j];
        const uint64_t *col = it.lv->dig + it.band_at;
        const int64_t n = it.n_p;
        int64_t lo = 0, hi = n;  // lower bound
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (col[mid] < d) lo = mid + 1; else hi = mid;
        }
        int64_t end = lo;
        if (lo < n && col[lo] == d) {  // upper bound by galloping: buckets are short
            int64_t step = 1;
            end = lo + 1;
            while (end < n && col[end] == d) {
                end = std::min<int64_t>(n, end + step);
                step <<= 1;
            }
            int64_t a = std::max<int64_t>(lo, end - step / 2 - 1), b = end;  // last equal is in [a, b)
            while (a < b) {
                const int64_t mid = (a + b) >> 1;
                if (col[mid] <= d) a = mid + 1; else b = mid;
            }
            end = a;
        }
        first[t] = (uint32_t)lo;
        count[t] = (uint32_t)(end - lo);
    }
}

// raw[where[t] + i] = (q << 32) | (start[p] + row) for the rows of item t's bucket whose band words equal the probe's, ~0 otherwise
template <typename SigT>
__global__ __launch_bounds__(256) void ensemble_emit_kernel(const uint32_t *__restrict__ item_pair, const uint64_t *__restrict__ item_off,
                                                            const uint8_t *__restrict__ choice, const EnsTable *__restrict__ tab,
                                                            const int64_t *__restrict__ start, int32_t n_parts, int64_t n_items,
                                                            const uint32_t *__restrict__ first, const uint32_t *__restrict__ count,
                                                            const uint64_t *__restrict__ where, const SigT *__restrict__ q_sig,
                                                            const SigT *__restrict__ idx_sig, int32_t k, uint64_t *__restrict__ raw) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n_items; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = count[t];
        if (c == 0) continue;
        const Item it = item_of(t, item_pair, item_off, choice, tab, start, n_parts);
        const uint32_t *rows = it.lv->rows + it.band_at + first[t];
        const SigT *x = q_sig + it.q * k + (int64_t)it.j * it.r;
        uint64_t *dst = raw + where[t];
        for (uint32_t i = 0; i < c; ++i) {
            const int64_t row = rows[i];
            bool same = row < it.n_p;  // (a band holds rows of its partition: anything else is never dereferenced)
            if (same) {
                const SigT *y = idx_sig + (it.s0 + row) * k + (int64_t)it.j * it.r;
                for (int w = 0; w < it.r; ++w) same &= x[w] == y[w];
            }
            dst[i] = same ? (((uint64_t)it.q << 32) | (uint64_t)(it.s0 + row)) : ~0ull;
        }
    }
}

unsigned grid_for(const mhx_ctx *ctx, int64_t items) {
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, (int64_t)ctx->num_cus * 16));
}

size_t pad256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

int read_total(mhx_ctx *ctx, const uint64_t *d_total, int64_t *total) {
    uint64_t v = 0;
    MHX_HIP_CHECK(hipMemcpyAsync(&v, d_total, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *total = (int64_t)v;
    return MHX_OK;
}

}  // namespace

// The arguments are checked by the caller (mhx_api.hip): n_levels and n_params within their maxima, every level's r * bands <= k,
// every table row's level in range and 0 <= b <= that level's bands, start ascending from 0 to fewer than 2^32 rows, m < 2^32.
int launch_lsh_ensemble_query(mhx_ctx *ctx, const mhx_ensemble_level *levels, int32_t n_levels, const int64_t *start, int32_t n_parts,
                              const void *d_idx_sig, int sig_dtype, int32_t k, const void *d_q_sig, int64_t m, const uint8_t *d_choice,
                              const int32_t *params, int32_t n_params, int64_t *d_pairs, int64_t capacity, int64_t *n_pairs) {
    *n_pairs = 0;
    const int64_t n_pp = m * (int64_t)n_parts;  // (probe, partition) pairs
    if (n_pp == 0 || start[n_parts] == 0) return MHX_OK;
    if (n_pp >= (int64_t)1 << 32) return fail(MHX_ERR_UNSUPPORTED, "more than 2^32-1 (probe, partition) pairs per call");
    EnsTable tab{};
    tab.n_params = n_params;
    for (int c = 0; c < n_params; ++c) {
        tab.p_level[c] = params[2 * c];
        tab.p_b[c] = params[2 * c + 1];
        EnsLevel &lv = tab.level[params[2 * c]];
        lv.qbands = std::max(lv.qbands, params[2 * c + 1]);
    }
    // scratch[2]: table | start i64[n_parts + 1] | per level the probes' digests u64[m][qbands] | item_off u64[n_pp] | scan temporary
    const size_t start_bytes = pad256(sizeof(int64_t) * (size_t)(n_parts + 1));
    size_t qdig_at[MHX_ENSEMBLE_MAX_LEVELS], at = pad256(sizeof(EnsTable)) + start_bytes;
    for (int l = 0; l < n_levels; ++l) {
        qdig_at[l] = at;
        at += pad256(sizeof(uint64_t) * (size_t)m * (size_t)tab.level[l].qbands);
    }
    const size_t off_at = at, off_bytes = pad256(sizeof(uint64_t) * (size_t)n_pp);
    if (int rc = ctx->ensure_scratch(2, off_at + off_bytes + scan_tmp_bytes(n_pp))) return rc;
    char *base = (char *)ctx->scratch[2];
    for (int l = 0; l < n_levels; ++l) {
        EnsLevel &lv = tab.level[l];
        lv.dig = levels[l].d_digests;
        lv.rows = levels[l].d_rows;
        lv.r = levels[l].r;
        lv.bands = levels[l].bands;
        lv.qdig = (const uint64_t *)(base + qdig_at[l]);
    }
    const EnsTable *d_tab = (const EnsTable *)base;
    const int64_t *d_start = (const int64_t *)(base + pad256(sizeof(EnsTable)));
    uint64_t *d_item_off = (uint64_t *)(base + off_at);
    void *d_scan_a = base + off_at + off_bytes;
    // the table and the bounds are host memory of this call: they are on the device before anything else is enqueued
    MHX_HIP_CHECK(hipMemcpyAsync(base, &tab, sizeof(EnsTable), hipMemcpyHostToDevice, ctx->stream));
    MHX_HIP_CHECK(hipMemcpyAsync(base + pad256(sizeof(EnsTable)), start, sizeof(int64_t) * (size_t)(n_parts + 1), hipMemcpyHostToDevice,
                                 ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int l = 0; l < n_levels; ++l)
        if (tab.level[l].qbands > 0)
            if (int rc = launch_band_digests(ctx, d_q_sig, sig_dtype, m, k, tab.level[l].qbands, tab.level[l].r,
                                             (uint64_t *)(base + qdig_at[l])))
                return rc;
    uint64_t *d_total = nullptr;
    if (int rc = device_exclusive_scan(ctx, PairBandsIn{d_choice, d_tab}, WhereOut{d_item_off}, n_pp, d_scan_a, &d_total)) return rc;
    int64_t n_items = 0;
    if (int rc = read_total(ctx, d_total, &n_items)) return rc;
    if (n_items == 0) return MHX_OK;
    if ((size_t)n_items * 20 > (size_t)ctx->hbm_bytes / 2)
        return fail(MHX_ERR_OOM, "%lld band searches in one call do not fit in device memory", (long long)n_items);
    // scratch[4]: item_pair u32[T] | first u32[T] | count u32[T] | where u64[T] | scan temporary
    const size_t u32_bytes = pad256(sizeof(uint32_t) * (size_t)n_items), u64_bytes = pad256(sizeof(uint64_t) * (size_t)n_items);
    if (int rc = ctx->ensure_scratch(4, 3 * u32_bytes + u64_bytes + scan_tmp_bytes(n_items))) return rc;
    char *items = (char *)ctx->scratch[4];
    uint32_t *d_item_pair = (uint32_t *)items, *d_first = (uint32_t *)(items + u32_bytes), *d_count = (uint32_t *)(items + 2 * u32_bytes);
    uint64_t *d_where = (uint64_t *)(items + 3 * u32_bytes);
    void *d_scan_b = items + 3 * u32_bytes + u64_bytes;
    hipLaunchKernelGGL(ensemble_items_kernel, dim3(grid_for(ctx, n_pp)), dim3(256), 0, ctx->stream, d_choice, d_tab, d_item_off, n_pp, n_items,
                       d_item_pair);
    const dim3 grid(grid_for(ctx, n_items));
    hipLaunchKernelGGL(ensemble_ranges_kernel, grid, dim3(256), 0, ctx->stream, d_item_pair, d_item_off, d_choice, d_tab, d_start, n_parts,
                       n_items, d_first, d_count);
    MHX_HIP_CHECK(hipGetLastError());
    if (int rc = device_exclusive_scan(ctx, CountsIn{d_count}, WhereOut{d_where}, n_items, d_scan_b, &d_total)) return rc;
    int64_t raw = 0;
    if (int rc = read_total(ctx, d_total, &raw)) return rc;
    if (raw == 0) return MHX_OK;
    uint64_t *d_raw = nullptr;
    if (int rc = lsh_raw_pairs_reserve(ctx, raw, &d_raw)) return rc;
    if (sig_dtype == MHX_U32)
        hipLaunchKernelGGL(ensemble_emit_kernel<uint32_t>, grid, dim3(256), 0, ctx->stream, d_item_pair, d_item_off, d_choice, d_tab, d_start,
                           n_parts, n_items, d_first, d_count, d_where, (const uint32_t *)d_q_sig, (const uint32_t *)d_idx_sig, k, d_raw);
    else
        hipLaunchKernelGGL(ensemble_emit_kernel<uint64_t>, grid, dim3(256), 0, ctx->stream, d_item_pair, d_item_off, d_choice, d_tab, d_start,
                           n_parts, n_items, d_first, d_count, d_where, (const uint64_t *)d_q_sig, (const uint64_t *)d_idx_sig, k, d_raw);
    MHX_HIP_CHECK(hipGetLastError());
    return lsh_raw_pairs_finish(ctx, raw, d_pairs, capacity, n_pairs);
}

}  // namespace mhx
