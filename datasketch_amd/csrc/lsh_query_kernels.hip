// lsh_query_kernels.hip -- everything that READS sorted bands (lsh_kernels.hip builds them): the candidate pairs of an index
// (mhx_lsh_candidate_pairs*), MinHashLSH's bulk query (mhx_lsh_query_dev*) and MinHashLSHEnsemble's containment query
// (mhx_lsh_ensemble_query_dev).  All three find a bucket -- the run of equal digests -- in a band's ascending digests with one
// search (band_lower_bound / band_run), the two queries verify the band's r words with one comparison (band_words_equal), and all
// three hand their raw 64-bit candidates to one tail (lsh_raw_pairs_reserve / _finish: radix sort, unique, unpack).
//
// The ensemble.  Reference: MinHashLSHEnsemble.query (datasketch/lshensemble.py:230-249) walks num_part partitions; in each it
// picks (b, r) from upper bound / probe size and asks the partition's MinHashLSH of r rows per band for the buckets of its first b
// bands (lsh.py:545-557).  Here the partitions are slot ranges of one size-sorted signature matrix and every distinct r is a
// *level*: per partition a block of sorted bands, laid out as mhx_lsh_sort_bands_dev_typed writes them for the partition's rows
// (include/mhx.h).  One call answers all probes in all partitions: the work items are (probe q, partition p, band j < b(q, p)) --
// the sum of the chosen b, not probes x partitions x bands -- and each item is the plain query's search in the block the item's
// (level, partition) selects.
//
//   1. band digests of the probes, once per level that the table uses (launch_band_digests, the level's largest b bands only);
//   2. b(q, p) per (probe, partition) pair -> exclusive scan = the pair's first item; the total T comes back to the host;
//   3. every pair names itself in its b items (ensemble_items_kernel), so that an item finds (q, p, j) with two loads;
//   4. ensemble_ranges_kernel: one thread per item, band_run in the band of n_p digests;
//   5. exclusive scan of the run lengths; ensemble_emit_kernel compares the band's r words and writes (q << 32) | (start[p] + row);
//   6. sort, unique, unpack (lsh_raw_pairs_finish).
// The search is a chain of ~log2(n_p) dependent loads into cold memory per item; one thread per item keeps as many chains in
// flight as there are lanes, which is what hides them.  The plain kernels find their item (probe, band) by index arithmetic and
// stay separate __global__ functions: going through the item list would put two more dependent loads in front of every chain.
#include <rocprim/device/device_radix_sort.hpp>

#include "device_scan.h"
#include "mhx_internal.h"

namespace mhx {
namespace {

// ---- the one search and the one verification ----------------------------------------------------------------
// first position in col[0, n) whose digest is not below d (n when there is none)
__device__ __forceinline__ int64_t band_lower_bound(const uint64_t *__restrict__ col, int64_t n, uint64_t d) {
    int64_t lo = 0, hi = n;  // lower bound
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (col[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the bucket of digest d in the ascending col[0, n): *first = band_lower_bound, *count = the length of the run of d there
__device__ __forceinline__ void band_run(const uint64_t *__restrict__ col, int64_t n, uint64_t d, uint32_t *first, uint32_t *count) {
    const int64_t lo = band_lower_bound(col, n, d);
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
    *first = (uint32_t)lo;
    *count = (uint32_t)(end - lo);
}

// the r words of a band, probe against index row: a 64-bit digest collision between different band keys is no candidate
template <typename SigT>
__device__ __forceinline__ bool band_words_equal(const SigT *x, const SigT *y, int32_t r) {
    bool same = true;
    for (int w = 0; w < r; ++w) same &= x[w] == y[w];
    return same;
}

// ---- candidate pairs from the sorted bands --------------------------------------------------------
// A bucket is a run of equal digests inside one band.  Element p of a run that starts at s pairs with
// the p - s elements in front of it, so the run of length L yields L(L-1)/2 pairs, each exactly once.
// Most elements are alone in their bucket: only an element that equals its predecessor looks for the
// start of its run (binary search in the sorted band, ~log2 n reads).

// ahead[p] = number of earlier elements of p's run (0 for a run's first element)
__global__ __launch_bounds__(256) void run_position_kernel(const uint64_t *__restrict__ digests, int64_t n, int64_t total,
                                                           uint32_t *__restrict__ ahead) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t band_start = p / n * n;
        uint32_t c = 0;
        if (p > band_start && digests[p] == digests[p - 1]) {
            // the run's first element: p - 1 holds d, so the search is over [band_start, p - 1)
            c = (uint32_t)(p - band_start - band_lower_bound(digests + band_start, p - 1 - band_start, digests[p]));
        }
        ahead[p] = c;
    }
}

// raw[where[p] + q] = (min(row_p, row_q) << 32) | max(row_p, row_q) for the ahead[p] elements q in front of p
__global__ __launch_bounds__(256) void emit_pairs_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ ahead,
                                                         const uint64_t *__restrict__ where, int64_t total,
                                                         uint64_t *__restrict__ raw) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = ahead[p];
        if (c == 0) continue;
        const uint32_t me = rows[p];
        uint64_t *dst = raw + where[p];
        for (uint32_t q = 0; q < c; ++q) {
            const uint32_t other = rows[p - c + q];
            const uint32_t lo = me < other ? me : other, hi = me < other ? other : me;
            dst[q] = ((uint64_t)lo << 32) | hi;
        }
    }
}

__global__ __launch_bounds__(256) void unpack_pairs_kernel(const uint64_t *__restrict__ keys, int64_t count,
                                                           int64_t *__restrict__ pairs) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        longlong2 v;
        v.x = (long long)(key >> 32);
        v.y = (long long)(key & 0xFFFFFFFFu);
        reinterpret_cast<longlong2 *>(pairs)[i] = v;
    }
}

// ---- bulk query against sorted bands ---------------------------------------------------------------
// What MinHashLSH.query does per probe (ref: datasketch/lsh.py:423-431: for every band, look the band key up
// in that band's dictionary and union the buckets), for M probes at once against an index of n rows held as
// sorted bands: the probe's band digest is located by binary search in the band's ascending digests; the
// matching run is its bucket.

// per (probe q, band j): first[idx] = position of the first equal digest in the band, count[idx] = run length
__global__ __launch_bounds__(256) void query_ranges_kernel(const uint64_t *__restrict__ q_digests, int64_t m, int32_t bands,
                                                           const uint64_t *__restrict__ sorted_digests, int64_t n,
                                                           uint32_t *__restrict__ first, uint32_t *__restrict__ count) {
    const int64_t total = m * (int64_t)bands;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int band = (int)(idx % bands);
        band_run(sorted_digests + (int64_t)band * n, n, q_digests[idx], &first[idx], &count[idx]);
    }
}

// raw[where[idx] + i] = (q << 32) | row for the rows of the probe's bucket in band j.  With VERIFY the r words of
// the band are compared (probe signature against index signature): a 64-bit digest collision between different
// band keys then yields no candidate -- exactly the reference's dictionary semantics -- and the slot gets ~0.
template <typename SigT, bool VERIFY>
__global__ __launch_bounds__(256) void query_emit_kernel(const uint32_t *__restrict__ first, const uint32_t *__restrict__ count,
                                                         const uint64_t *__restrict__ where, int64_t m, int32_t bands, int64_t n,
                                                         const uint32_t *__restrict__ sorted_rows,
                                                         const SigT *__restrict__ q_sig, const SigT *__restrict__ idx_sig,
                                                         int32_t k, int32_t r, uint64_t *__restrict__ raw) {
    const int64_t total = m * (int64_t)bands;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t c = count[idx];
        if (c == 0) continue;
        const int64_t q = idx / bands;
        const int band = (int)(idx - q * bands);
        const uint32_t *rows = sorted_rows + (int64_t)band * n + first[idx];
        uint64_t *dst = raw + where[idx];
        for (uint32_t i = 0; i < c; ++i) {
            const uint32_t row = rows[i];
            bool same = true;
            if (VERIFY) same = band_words_equal(q_sig + q * k + (int64_t)band * r, idx_sig + (int64_t)row * k + (int64_t)band * r, r);
            dst[i] = same ? (((uint64_t)q << 32) | row) : ~0ull;
        }
    }
}

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
        band_run(it.lv->dig + it.band_at, it.n_p, it.lv->qdig[it.q * it.lv->qbands + it.j], &first[t], &count[t]);
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
            // (a band holds rows of its partition: anything else is never dereferenced)
            const bool same = row < it.n_p && band_words_equal(x, idx_sig + (it.s0 + row) * k + (int64_t)it.j * it.r, it.r);
            dst[i] = same ? (((uint64_t)it.q << 32) | (uint64_t)(it.s0 + row)) : ~0ull;
        }
    }
}

// ---- the tail the three launchers share --------------------------------------------------------------------
// `raw` 64-bit candidates (high word << 32 | row; the queries leave ~0 where the band's words differed) -> unique pairs, ascending.
// scratch[3]: raw u64[raw] | sorted u64[raw] | count u64 | sort / select temporary.  lsh_raw_pairs_reserve sizes the slot and
// hands out the raw array for the caller's emit kernel; lsh_raw_pairs_finish sorts, keeps the run heads and unpacks them, and
// blocks (it reads the count).  What differs between the callers: end_bit, the bits the radix sort (the one library primitive
// here) orders by -- candidate pairs hold a row number < n in the high word and need 32 + ceil(log2 n), the queries all 64,
// because ~0 must sort last --; whether ~0 can be present at all (`dropped`: one more word read back); and what the candidates
// are called when they do not fit.
int raw_pair_tmp_bytes(mhx_ctx *ctx, int64_t raw, int end_bit, size_t *sort_tmp) {
    hipError_t e = rocprim::radix_sort_keys(nullptr, *sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)raw, 0, end_bit,
                                            ctx->stream);
    if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim size query failed: %s", hipGetErrorString(e));
    return MHX_OK;
}

int lsh_raw_pairs_reserve(mhx_ctx *ctx, int64_t raw, int end_bit, const char *what, uint64_t **d_raw) {
    if ((size_t)raw * 16 > (size_t)ctx->hbm_bytes / 2)
        return fail(MHX_ERR_OOM, "%lld %s do not fit in device memory", (long long)raw, what);
    size_t sort_tmp = 0;
    if (int rc = raw_pair_tmp_bytes(ctx, raw, end_bit, &sort_tmp)) return rc;
    if (int rc = ctx->ensure_scratch(3, 2 * pad256(sizeof(uint64_t) * (size_t)raw) + 256 + std::max(sort_tmp, scan_tmp_bytes(raw)))) return rc;
    *d_raw = (uint64_t *)ctx->scratch[3];
    return MHX_OK;
}

int lsh_raw_pairs_finish(mhx_ctx *ctx, int64_t raw, int end_bit, bool dropped, int64_t *d_pairs, int64_t capacity, int64_t *n_pairs) {
    const size_t raw_bytes = pad256(sizeof(uint64_t) * (size_t)raw);
    size_t sort_tmp = 0;
    if (int rc = raw_pair_tmp_bytes(ctx, raw, end_bit, &sort_tmp)) return rc;
    uint64_t *d_raw = (uint64_t *)ctx->scratch[3];
    uint64_t *d_sorted = (uint64_t *)((char *)ctx->scratch[3] + raw_bytes);
    void *d_tmp = (char *)ctx->scratch[3] + 2 * raw_bytes + 256;
    hipError_t e = rocprim::radix_sort_keys(d_tmp, sort_tmp, (const uint64_t *)d_raw, d_sorted, (size_t)raw, 0, end_bit, ctx->stream);
    if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim::radix_sort_keys failed: %s", hipGetErrorString(e));
    uint64_t *d_cnt = nullptr;  // unique: the run heads of the sorted candidates, packed
    if (int rc = device_exclusive_scan(ctx, HeadsIn{d_sorted}, CompactOut{d_sorted, d_raw}, raw, d_tmp, &d_cnt)) return rc;
    uint64_t unique_count = 0, last_key = 0;
    if (int rc = read_back_u64(ctx, d_cnt, &unique_count)) return rc;
    if (dropped && unique_count > 0) {  // a failed verification left ~0, which sorts last
        if (int rc = read_back_u64(ctx, d_raw + (unique_count - 1), &last_key)) return rc;
        if (last_key == ~0ull) --unique_count;
    }
    *n_pairs = (int64_t)unique_count;
    if ((int64_t)unique_count > capacity || unique_count == 0) return MHX_OK;  // caller sees n_pairs > capacity and calls again
    hipLaunchKernelGGL(unpack_pairs_kernel, dim3(grid_for(ctx, (int64_t)unique_count)), dim3(256), 0, ctx->stream, d_raw,
                       (int64_t)unique_count, d_pairs);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace

int launch_lsh_candidate_pairs(mhx_ctx *ctx, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows, int64_t n,
                               int32_t bands, int64_t *d_pairs, int64_t capacity, int64_t *n_pairs, int64_t *n_raw) {
    *n_pairs = 0;
    if (n_raw) *n_raw = 0;
    const int64_t total = n * (int64_t)bands;
    if (total == 0) return MHX_OK;
    // scratch[4], first part: ahead u32[total] | where u64[total] | tail u64[2] | scan temporary
    const size_t ahead_bytes = pad256(sizeof(uint32_t) * (size_t)total), where_bytes = pad256(sizeof(uint64_t) * (size_t)total);
    const size_t scan_tmp = scan_tmp_bytes(total);
    if (int rc = ctx->ensure_scratch(4, ahead_bytes + where_bytes + 256 + scan_tmp)) return rc;
    uint32_t *d_ahead = (uint32_t *)ctx->scratch[4];
    uint64_t *d_where = (uint64_t *)((char *)ctx->scratch[4] + ahead_bytes);
    void *d_scan_tmp = (char *)ctx->scratch[4] + ahead_bytes + where_bytes + 256;
    hipLaunchKernelGGL(run_position_kernel, dim3(grid_for(ctx, total)), dim3(256), 0, ctx->stream, d_sorted_digests, n, total,
                       d_ahead);
    MHX_HIP_CHECK(hipGetLastError());
    uint64_t *d_raw_total = nullptr;
    if (int rc = device_exclusive_scan(ctx, CountsIn{d_ahead}, WhereOut{d_where}, total, d_scan_tmp, &d_raw_total)) return rc;
    uint64_t raw_total = 0;
    if (int rc = read_back_u64(ctx, d_raw_total, &raw_total)) return rc;
    const int64_t raw = (int64_t)raw_total;  // pairs before deduplication across bands
    if (n_raw) *n_raw = raw;
    if (raw == 0) return MHX_OK;
    int end_bit = 33;  // the high word holds a row number < n
    while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < n) ++end_bit;
    uint64_t *d_raw = nullptr;
    if (int rc = lsh_raw_pairs_reserve(ctx, raw, end_bit, "candidate pairs before deduplication (large buckets of equal band keys)", &d_raw))
        return rc;
    hipLaunchKernelGGL(emit_pairs_kernel, dim3(grid_for(ctx, total)), dim3(256), 0, ctx->stream, d_sorted_rows, d_ahead, d_where,
                       total, d_raw);
    MHX_HIP_CHECK(hipGetLastError());
    return lsh_raw_pairs_finish(ctx, raw, end_bit, false, d_pairs, capacity, n_pairs);  // (every raw pair is a pair: no ~0 to look for)
}

int launch_lsh_query(mhx_ctx *ctx, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows, int64_t n, int32_t bands,
                     int32_t r, const void *d_q_sig, const void *d_idx_sig, int sig_dtype, int32_t k, int64_t m,
                     int64_t *d_pairs, int64_t capacity, int64_t *n_pairs) {
    *n_pairs = 0;
    const int64_t total = m * (int64_t)bands;
    if (total == 0 || n == 0) return MHX_OK;
    // scratch[4]: probe digests u64[total] | first u32[total] | count u32[total] | where u64[total] | scan temporary
    const size_t dig_bytes = pad256(sizeof(uint64_t) * (size_t)total), u32_bytes = pad256(sizeof(uint32_t) * (size_t)total);
    const size_t scan_tmp = scan_tmp_bytes(total);
    if (int rc = ctx->ensure_scratch(4, 2 * dig_bytes + 2 * u32_bytes + 256 + scan_tmp)) return rc;
    char *base = (char *)ctx->scratch[4];
    uint64_t *d_qdig = (uint64_t *)base;
    uint32_t *d_first = (uint32_t *)(base + dig_bytes);
    uint32_t *d_count = (uint32_t *)(base + dig_bytes + u32_bytes);
    uint64_t *d_where = (uint64_t *)(base + dig_bytes + 2 * u32_bytes);
    void *d_scan_tmp = base + 2 * dig_bytes + 2 * u32_bytes + 256;
    if (int rc = launch_band_digests(ctx, d_q_sig, sig_dtype, m, k, bands, r, d_qdig)) return rc;
    const dim3 grid(grid_for(ctx, total));
    hipLaunchKernelGGL(query_ranges_kernel, grid, dim3(256), 0, ctx->stream, d_qdig, m, bands, d_sorted_digests, n, d_first, d_count);
    MHX_HIP_CHECK(hipGetLastError());
    uint64_t *d_raw_total = nullptr;
    if (int rc = device_exclusive_scan(ctx, CountsIn{d_count}, WhereOut{d_where}, total, d_scan_tmp, &d_raw_total)) return rc;
    uint64_t raw_total = 0;
    if (int rc = read_back_u64(ctx, d_raw_total, &raw_total)) return rc;
    const int64_t raw = (int64_t)raw_total;
    if (raw == 0) return MHX_OK;
    uint64_t *d_raw = nullptr;
    if (int rc = lsh_raw_pairs_reserve(ctx, raw, 64, "candidates before deduplication", &d_raw)) return rc;
    const bool verify = d_idx_sig != nullptr;
    if (sig_dtype == MHX_U32) {
        if (verify)
            hipLaunchKernelGGL((query_emit_kernel<uint32_t, true>), grid, dim3(256), 0, ctx->stream, d_first, d_count, d_where, m, bands, n,
                               d_sorted_rows, (const uint32_t *)d_q_sig, (const uint32_t *)d_idx_sig, k, r, d_raw);
        else
            hipLaunchKernelGGL((query_emit_kernel<uint32_t, false>), grid, dim3(256), 0, ctx->stream, d_first, d_count, d_where, m, bands, n,
                               d_sorted_rows, (const uint32_t *)d_q_sig, (const uint32_t *)d_idx_sig, k, r, d_raw);
    } else {
        if (verify)
            hipLaunchKernelGGL((query_emit_kernel<uint64_t, true>), grid, dim3(256), 0, ctx->stream, d_first, d_count, d_where, m, bands, n,
                               d_sorted_rows, (const uint64_t *)d_q_sig, (const uint64_t *)d_idx_sig, k, r, d_raw);
        else
            hipLaunchKernelGGL((query_emit_kernel<uint64_t, false>), grid, dim3(256), 0, ctx->stream, d_first, d_count, d_where, m, bands, n,
                               d_sorted_rows, (const uint64_t *)d_q_sig, (const uint64_t *)d_idx_sig, k, r, d_raw);
    }
    MHX_HIP_CHECK(hipGetLastError());
    return lsh_raw_pairs_finish(ctx, raw, 64, true, d_pairs, capacity, n_pairs);
}

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
    uint64_t total = 0;
    if (int rc = read_back_u64(ctx, d_total, &total)) return rc;
    const int64_t n_items = (int64_t)total;
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
    if (int rc = read_back_u64(ctx, d_total, &total)) return rc;
    const int64_t raw = (int64_t)total;
    if (raw == 0) return MHX_OK;
    uint64_t *d_raw = nullptr;
    if (int rc = lsh_raw_pairs_reserve(ctx, raw, 64, "candidates before deduplication", &d_raw)) return rc;
    if (sig_dtype == MHX_U32)
        hipLaunchKernelGGL(ensemble_emit_kernel<uint32_t>, grid, dim3(256), 0, ctx->stream, d_item_pair, d_item_off, d_choice, d_tab, d_start,
                           n_parts, n_items, d_first, d_count, d_where, (const uint32_t *)d_q_sig, (const uint32_t *)d_idx_sig, k, d_raw);
    else
        hipLaunchKernelGGL(ensemble_emit_kernel<uint64_t>, grid, dim3(256), 0, ctx->stream, d_item_pair, d_item_off, d_choice, d_tab, d_start,
                           n_parts, n_items, d_first, d_count, d_where, (const uint64_t *)d_q_sig, (const uint64_t *)d_idx_sig, k, d_raw);
    MHX_HIP_CHECK(hipGetLastError());
    return lsh_raw_pairs_finish(ctx, raw, 64, true, d_pairs, capacity, n_pairs);
}

}  // namespace mhx
