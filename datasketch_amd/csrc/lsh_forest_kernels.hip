// lsh_forest_kernels.hip -- the LSH Forest (datasketch_amd.MinHashLSHForest; ref: datasketch/lshforest.py) on the device.
//
// The reference keeps, per tree, the sorted list of the trees' keys (the big-endian bytes of D hash values) and binary-searches
// prefixes in it.  Here tree t is `order[t]`: the slots of the signature matrix ascending by (the tree's D*w words compared
// lexicographically as unsigned integers, slot).  The slots matching a probe on their first r hash values (level r) are one
// contiguous range of order[t], and the ranges nest as r falls.
//
// BUILD.  A least-significant-word-first radix sort: one stable pass (rocPRIM radix_sort_pairs) per 32-bit half-word of the
// tree's key, all trees in one pass with the tree number above the half-word, so equal keys keep slot order and runs of equal
// leading words -- up to every row identical -- cost what any other input costs: D*w (uint32) or 2*D*w (uint64) passes over
// l*n pairs.  The gather of the next half-word through the current order is ours.
//
// QUERY.  query(probe, k) of the reference walks r = D .. 1, t = 0 .. l-1, the positions of tree t's level-r range ascending,
// takes every slot not taken before and stops at k.  Two launches reproduce that walk exactly without a per-probe hash set:
//   1. one thread per (probe, tree): a lexicographic binary search for the insertion point, then the level ranges outwards
//      (the common prefix of the two neighbours names the next level at which the range grows; a galloping search finds how
//      far) until a range holds k slots.  That level r_t is the shallowest this tree can be walked at, so the tree's candidates
//      are its range at level r_t + 1 (fewer than k) and the first k positions the level r_t adds: a window of four positions.
//   2. one wave (or workgroup) per probe: every candidate (slot, tree t, level r = its match length in t) is the slot's first
//      discovery exactly when no other tree matches it deeper and no lower tree as deep -- decided from the slot's row and
//      the probe.  The first discoveries are sorted in LDS by (level descending, tree, position) and the first k go out.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "mhx_internal.h"

namespace mhx {
namespace {

// ---- build --------------------------------------------------------------------------------------------------------------
// keys[t * n + i] = (t << 32) | half-word `col32` of tree t's key of the slot at position i of tree t's current order (the slots
// in slot order when there is none yet: the first pass, which also writes that order for the sort to carry).
__global__ __launch_bounds__(256) void forest_keys_kernel(const uint32_t *__restrict__ sig32, int64_t row_stride32, int64_t n, int32_t l,
                                                          int64_t tree_stride32, int64_t col32, const uint32_t *__restrict__ order_in,
                                                          uint64_t *__restrict__ keys, uint32_t *__restrict__ iota_out) {
    const int64_t total = (int64_t)l * n;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = idx / n;
        const uint32_t slot = order_in ? order_in[idx] : (uint32_t)(idx - t * n);
        keys[idx] = ((uint64_t)t << 32) | sig32[(int64_t)slot * row_stride32 + t * tree_stride32 + col32];
        if (!order_in) iota_out[idx] = slot;
    }
}

// ---- query --------------------------------------------------------------------------------------------------------------
// leading words of a[0 .. nw) equal to b's
template <typename T>
__device__ __forceinline__ int lcp_words(const T *__restrict__ a, const T *__restrict__ b, int nw) {
    int i = 0;
    while (i < nw && a[i] == b[i]) ++i;
    return i;
}

// win[(p * l + t) * 4 ..]: {lo_out, lo_in, hi_in, hi_out} -- [lo_in, hi_in) is tree t's range one level above r_t, [lo_out, hi_out)
// its range at r_t (equal to the inner one when no level holds k slots: then everything is inside).
template <typename T>
__global__ __launch_bounds__(256) void forest_search_kernel(const T *__restrict__ sig, int64_t n, int32_t row_words, int32_t l, int32_t dw,
                                                            int32_t w, const uint32_t *__restrict__ order, const T *__restrict__ probes,
                                                            int64_t m, int64_t k, uint4 *__restrict__ win) {
    const int64_t total = m * l;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = idx / l;
        const int32_t t = (int32_t)(idx - p * l);
        const T *q = probes + p * row_words + (int64_t)t * dw;
        const uint32_t *ord = order + (int64_t)t * n;
        const T *base = sig + (int64_t)t * dw;
        auto row = [&](int64_t pos) { return base + (int64_t)ord[pos] * row_words; };
        auto matches = [&](int64_t pos, int nw) { return lcp_words(row(pos), q, nw) == nw; };
        int64_t lo = 0, hi = n;  // the insertion point of the probe's whole key
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            const T *r = row(mid);
            const int c = lcp_words(r, q, dw);
            if (c < dw && r[c] < q[c]) lo = mid + 1; else hi = mid;
        }
        int64_t a = lo, b = lo, oa = lo, ob = lo;
        for (;;) {
            const int cl = a > 0 ? lcp_words(row(a - 1), q, dw) / w : 0;
            const int cr = b < n ? lcp_words(row(b), q, dw) / w : 0;
            const int r = cl > cr ? cl : cr;  // the deepest level whose range is wider than [a, b)
            if (r == 0) { oa = a; ob = b; break; }
            const int nw = r * w;
            int64_t na = a, nb = b;
            if (cl == r) {  // position a - 1 matches: gallop left, then bisect between the last match and the first miss
                int64_t good = a - 1, bad = -1;
                for (int64_t step = 2;; step <<= 1) {
                    const int64_t pos = a - step;
                    if (pos < 0) break;
                    if (matches(pos, nw)) good = pos; else { bad = pos; break; }
                }
                while (good - bad > 1) {
                    const int64_t mid = bad + ((good - bad) >> 1);
                    if (matches(mid, nw)) good = mid; else bad = mid;
                }
                na = good;
            }
            if (cr == r) {
                int64_t good = b, bad = n;
                for (int64_t step = 2;; step <<= 1) {
                    const int64_t pos = b + step - 1;
                    if (pos >= n) break;
                    if (matches(pos, nw)) good = pos; else { bad = pos; break; }
                }
                while (bad - good > 1) {
                    const int64_t mid = good + ((bad - good) >> 1);
                    if (matches(mid, nw)) good = mid; else bad = mid;
                }
                nb = good + 1;
            }
            if (nb - na >= k) { oa = na; ob = nb; break; }
            a = na;
            b = nb;
        }
        win[idx] = make_uint4((uint32_t)oa, (uint32_t)a, (uint32_t)b, (uint32_t)ob);
    }
}

// TPP threads per probe (64: one wave, four probes per workgroup; 256: the workgroup).  LDS: sort_cap keys per probe.
template <typename T, int TPP>
__global__ __launch_bounds__(256) void forest_rank_kernel(const T *__restrict__ sig, int64_t n, int32_t row_words, int32_t l, int32_t dw,
                                                          int32_t w, const uint32_t *__restrict__ order, const T *__restrict__ probes,
                                                          int64_t m, int64_t k, const uint4 *__restrict__ win, int32_t cstride,
                                                          int32_t sort_cap, uint32_t *__restrict__ slots, int32_t *__restrict__ counts) {
    constexpr int kPerBlock = 256 / TPP;
    extern __shared__ uint64_t s_keys[];
    __shared__ int s_count[kPerBlock];
    const int g = threadIdx.x / TPP, lane = threadIdx.x % TPP;
    const int64_t p = (int64_t)blockIdx.x * kPerBlock + g;
    const bool valid = p < m;
    uint64_t *keys = s_keys + (size_t)g * sort_cap;
    const int depth = dw / w;
    if (lane == 0) s_count[g] = 0;
    for (int i = lane; i < sort_cap; i += TPP) keys[i] = ~(uint64_t)0;
    __syncthreads();
    if (valid) {
        const T *q = probes + p * row_words;
        const int total = l * cstride;
        for (int idx = lane; idx < total; idx += TPP) {
            const int t = idx / cstride;
            const int64_t i = idx - t * cstride;
            const uint4 x = win[p * l + t];
            const int64_t lo_out = x.x, lo_in = x.y, hi_in = x.z, hi_out = x.w;
            const int64_t left = std::min<int64_t>(k, lo_in - lo_out), inner = hi_in - lo_in;
            const int64_t right = std::min<int64_t>(k - left, hi_out - hi_in);
            if (i >= left + inner + right) continue;
            const int64_t pos = i < left ? lo_out + i : i < left + inner ? lo_in + (i - left) : hi_in + (i - left - inner);
            const T *row = sig + (int64_t)order[(int64_t)t * n + pos] * row_words;
            const int r = lcp_words(row + (int64_t)t * dw, q + (int64_t)t * dw, dw) / w;  // the level this tree finds the slot at
            bool first = r > 0;
            for (int t2 = 0; t2 < l && first; ++t2) {  // found earlier: deeper in any tree, or as deep in a lower one
                const int need = t2 < t ? r : r + 1;
                if (t2 == t || need > depth) continue;
                first = lcp_words(row + (int64_t)t2 * dw, q + (int64_t)t2 * dw, need * w) < need * w;
            }
            if (first) keys[atomicAdd(&s_count[g], 1)] = ((uint64_t)(depth - r) << 48) | ((uint64_t)t << 32) | (uint64_t)pos;
        }
    }
    __syncthreads();
    const int count = s_count[g];
    int sort_n = sort_cap;
    if (kPerBlock == 1) {  // the workgroup sorts one probe: no more than its keys
        sort_n = 1;
        while (sort_n < count) sort_n <<= 1;
    }
    for (int size = 2; size <= sort_n; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = lane; i < sort_n / 2; i += TPP) {
                const int at = 2 * i - (i & (stride - 1));
                const uint64_t x = keys[at], y = keys[at + stride];
                if ((x > y) == ((at & size) == 0)) {
                    keys[at] = y;
                    keys[at + stride] = x;
                }
            }
            __syncthreads();
        }
    if (valid) {
        const int n_out = (int)std::min<int64_t>(count, k);
        for (int j = lane; j < n_out; j += TPP) {
            const uint64_t key = keys[j];
            slots[p * k + j] = order[(int64_t)((key >> 32) & 0xFFFF) * n + (uint32_t)key];
        }
        if (lane == 0) counts[p] = n_out;
    }
}

}  // namespace

int launch_lsh_forest_build(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t row_words, int32_t l, int32_t tree_words,
                            uint32_t *d_order) {
    const int64_t total = (int64_t)l * n;
    if (total >= ((int64_t)1 << 32)) return fail(MHX_ERR_UNSUPPORTED, "l * n_sigs = %lld entries: a forest build sorts fewer than 2^32", (long long)total);
    const int halves = sig_dtype == MHX_U32 ? 1 : 2;  // 32-bit half-words per word
    const int passes = tree_words * halves;
    int end_bit = 32;
    while (((int64_t)1 << (end_bit - 32)) < l) ++end_bit;
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, tmp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (size_t)total, 0, end_bit, ctx->stream);
    if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim::radix_sort_pairs (size query) failed: %s", hipGetErrorString(e));
    // scratch[3]: keys u64[total] | sorted keys u64[total] | the other order buffer u32[total] | sort temporary
    const size_t key_bytes = pad256(sizeof(uint64_t) * (size_t)total), val_bytes = pad256(sizeof(uint32_t) * (size_t)total);
    if (int rc = ctx->ensure_scratch(3, 2 * key_bytes + val_bytes + tmp_bytes + 256)) return rc;
    char *base = (char *)ctx->scratch[3];
    uint64_t *d_keys = (uint64_t *)base, *d_keys_sorted = (uint64_t *)(base + key_bytes);
    uint32_t *d_other = (uint32_t *)(base + 2 * key_bytes);
    void *d_tmp = base + 2 * key_bytes + val_bytes;
    const dim3 grid(grid_for(ctx, total, 32));
    for (int p = 0; p < passes; ++p) {  // least significant half-word first; the last pass lands in d_order
        const int word = tree_words - 1 - p / halves;
        const int64_t col32 = (int64_t)word * halves + (halves == 2 ? p % 2 : 0);
        uint32_t *d_out = (passes - 1 - p) % 2 == 0 ? d_order : d_other;
        uint32_t *d_in = d_out == d_order ? d_other : d_order;
        hipLaunchKernelGGL(forest_keys_kernel, grid, dim3(256), 0, ctx->stream, (const uint32_t *)d_sig, (int64_t)row_words * halves, n, l,
                           (int64_t)tree_words * halves, col32, p == 0 ? (const uint32_t *)nullptr : (const uint32_t *)d_in, d_keys, p == 0 ? d_in : (uint32_t *)nullptr);
        MHX_HIP_CHECK(hipGetLastError());
        e = rocprim::radix_sort_pairs(d_tmp, tmp_bytes, (const uint64_t *)d_keys, d_keys_sorted, (const uint32_t *)d_in, d_out, (size_t)total, 0,
                                      end_bit, ctx->stream);
        if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim::radix_sort_pairs failed: %s", hipGetErrorString(e));
    }
    return MHX_OK;
}

int launch_lsh_forest_query(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t row_words, int32_t l, int32_t tree_words,
                            int32_t w, const uint32_t *d_order, const void *d_probes, int64_t m, int32_t k, uint32_t *d_slots,
                            int32_t *d_counts) {
    const int64_t cstride = std::min<int64_t>(2 * (int64_t)k - 1, n);  // candidates of one (probe, tree)
    const int64_t cand = cstride * l;
    if (cand > MHX_LSH_FOREST_MAX_CANDIDATES)
        return fail(MHX_ERR_INVALID, "k = %d: l * min(2k - 1, n) = %lld candidates per probe exceed MHX_LSH_FOREST_MAX_CANDIDATES (%d)", (int)k,
                    (long long)cand, (int)MHX_LSH_FOREST_MAX_CANDIDATES);
    int sort_cap = 2;
    while (sort_cap < cand) sort_cap <<= 1;
    const bool per_wave = sort_cap <= 1024;
    const size_t lds = sizeof(uint64_t) * (size_t)sort_cap * (per_wave ? 4 : 1);
    if (lds + 64 > (size_t)ctx->lds_per_block) return fail(MHX_ERR_UNSUPPORTED, "%zu bytes of LDS per workgroup are not available", lds);
    if (int rc = ctx->ensure_scratch(3, sizeof(uint4) * (size_t)m * (size_t)l)) return rc;
    uint4 *d_win = (uint4 *)ctx->scratch[3];
    const dim3 sgrid(grid_for(ctx, m * l, 32)), rgrid((unsigned)(per_wave ? (m + 3) / 4 : m));
#define MHX_FOREST_QUERY(T)                                                                                                              \
    do {                                                                                                                                 \
        hipLaunchKernelGGL(forest_search_kernel<T>, sgrid, dim3(256), 0, ctx->stream, (const T *)d_sig, n, row_words, l, tree_words, w,  \
                           d_order, (const T *)d_probes, m, (int64_t)k, d_win);                                                          \
        if (per_wave)                                                                                                                    \
            hipLaunchKernelGGL((forest_rank_kernel<T, 64>), rgrid, dim3(256), lds, ctx->stream, (const T *)d_sig, n, row_words, l,       \
                               tree_words, w, d_order, (const T *)d_probes, m, (int64_t)k, d_win, (int32_t)cstride, sort_cap, d_slots,   \
                               d_counts);                                                                                                \
        else                                                                                                                             \
            hipLaunchKernelGGL((forest_rank_kernel<T, 256>), rgrid, dim3(256), lds, ctx->stream, (const T *)d_sig, n, row_words, l,      \
                               tree_words, w, d_order, (const T *)d_probes, m, (int64_t)k, d_win, (int32_t)cstride, sort_cap, d_slots,   \
                               d_counts);                                                                                                \
    } while (0)
    if (sig_dtype == MHX_U32) MHX_FOREST_QUERY(uint32_t);
    else MHX_FOREST_QUERY(uint64_t);
#undef MHX_FOREST_QUERY
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
