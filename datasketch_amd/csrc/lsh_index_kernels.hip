// lsh_index_kernels.hip -- the update path of a live LSH index held as sorted bands (datasketch_amd.MinHashLSH).
//
// The index is the layout of mhx_lsh_sort_bands*: per band, the band digests of every slot in ascending (digest, row) order with
// their rows (slot numbers).  After the first build most work is a small batch against a big index, so nothing is sorted twice:
//   * a batch's bands (sorted on their own) are MERGED into the index's: a merge path in two launches (partition, merge);
//   * removed slots are dropped by COMPACTION: an order-preserving remap of the slot numbers (the exclusive popcount prefix of
//     the liveness bitmap) rewrites the bands without the dead entries, and a gather packs the live signature rows.
// Both keep the (digest, row) order: a merge of two sorted runs whose B rows are all above the A rows is the stable sort of
// A||B by digest, and a strictly increasing remap of the rows does not reorder a band.
#include <cstring>

#include "device_scan.h"
#include "mhx_internal.h"

namespace mhx {
namespace {

// ---- merge path ---------------------------------------------------------------------------------------------------------
// One workgroup per output tile of one band: 256 threads x ITEMS outputs.  The partition launch finds, for the first output
// of every tile, how many of the outputs before it come from A (binary search on digests: the co-rank).  The merge launch loads
// its A and B slices into LDS, every thread co-ranks its own ITEMS outputs inside LDS and merges them serially into registers,
// and the tile goes back out through LDS so that the global stores are contiguous.  ITEMS is 8 or 16 (option lsh.merge_items;
// the default is the measured faster one at 10k rows into 10M x 32 bands, DESIGN.md "The live index").
constexpr int kMergeThreads = 256;
constexpr int kMergeItemsDefault = 8;

// number of A elements among the first `diag` outputs of the stable merge of A and B (a tie goes to A)
template <typename DigA, typename DigB>
__device__ __forceinline__ int64_t co_rank(int64_t diag, int64_t na, int64_t nb, DigA a, DigB b) {
    int64_t lo = diag > nb ? diag - nb : 0, hi = diag < na ? diag : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a(mid) <= b(diag - mid - 1)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// part[band * (tiles + 1) + t] = A elements before output t * tile of the band (t = tiles: na)
__global__ __launch_bounds__(256) void bands_merge_partition_kernel(const uint64_t *__restrict__ dig_a, int64_t na,
                                                                    const uint64_t *__restrict__ dig_b, int64_t nb, int32_t bands,
                                                                    int64_t tiles, int32_t tile, int64_t *__restrict__ part) {
    const int64_t total = (int64_t)bands * (tiles + 1);
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t band = idx / (tiles + 1), t = idx - band * (tiles + 1);
        const int64_t diag = std::min<int64_t>(t * tile, na + nb);
        const uint64_t *a = dig_a + band * na, *b = dig_b + band * nb;
        part[idx] = co_rank(diag, na, nb, [a](int64_t i) { return a[i]; }, [b](int64_t i) { return b[i]; });
    }
}

// count elements of src (global) -> dst (LDS), each plus `add`; the 16-byte-aligned middle of the slice in 16-byte loads
template <typename T>
__device__ __forceinline__ void load_slice(const T *__restrict__ src, int count, T *dst, T add) {
    constexpr int kPer = 16 / sizeof(T);
    const int head = std::min(count, (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) / sizeof(T)));
    const int n_vec = (count - head) / kPer;
    for (int i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i] + add;
    const uint4 *vsrc = reinterpret_cast<const uint4 *>(src + head);
    for (int v = threadIdx.x; v < n_vec; v += blockDim.x) {
        const uint4 x = vsrc[v];
        T e[kPer];
        memcpy(e, &x, 16);
#pragma unroll
        for (int j = 0; j < kPer; ++j) dst[head + v * kPer + j] = e[j] + add;
    }
    for (int i = head + n_vec * kPer + threadIdx.x; i < count; i += blockDim.x) dst[i] = src[i] + add;
}

// count elements of src (LDS) -> dst (global); the 16-byte-aligned middle of the destination in 16-byte stores
template <typename T>
__device__ __forceinline__ void store_slice(T *__restrict__ dst, int count, const T *src) {
    constexpr int kPer = 16 / sizeof(T);
    const int head = std::min(count, (int)(((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / sizeof(T)));
    const int n_vec = (count - head) / kPer;
    for (int i = threadIdx.x; i < head; i += blockDim.x) dst[i] = src[i];
    uint4 *vdst = reinterpret_cast<uint4 *>(dst + head);
    for (int v = threadIdx.x; v < n_vec; v += blockDim.x) {
        T e[kPer];
#pragma unroll
        for (int j = 0; j < kPer; ++j) e[j] = src[head + v * kPer + j];
        uint4 x;
        memcpy(&x, e, 16);
        vdst[v] = x;
    }
    for (int i = head + n_vec * kPer + threadIdx.x; i < count; i += blockDim.x) dst[i] = src[i];
}

template <int ITEMS>
__global__ __launch_bounds__(kMergeThreads) void bands_merge_kernel(const uint64_t *__restrict__ dig_a, const uint32_t *__restrict__ rows_a,
                                                                    int64_t na, const uint64_t *__restrict__ dig_b,
                                                                    const uint32_t *__restrict__ rows_b, int64_t nb, uint32_t row_offset_b,
                                                                    int64_t tiles, const int64_t *__restrict__ part,
                                                                    uint64_t *__restrict__ dig_out, uint32_t *__restrict__ rows_out) {
    constexpr int kMergeTile = kMergeThreads * ITEMS;
    __shared__ uint64_t s_dig[kMergeTile];  // the A slice, then the B slice; afterwards the merged tile
    __shared__ uint32_t s_rows[kMergeTile];
    const int64_t band = blockIdx.x / tiles, t = blockIdx.x - band * tiles;
    const int64_t n_out = na + nb;
    const int64_t d0 = t * kMergeTile, d1 = std::min<int64_t>(d0 + kMergeTile, n_out);
    const int64_t a0 = part[band * (tiles + 1) + t], a1 = part[band * (tiles + 1) + t + 1];
    const int la = (int)(a1 - a0), lb = (int)((d1 - a1) - (d0 - a0)), n = la + lb;
    load_slice(dig_a + band * na + a0, la, s_dig, (uint64_t)0);
    load_slice(rows_a + band * na + a0, la, s_rows, 0u);
    load_slice(dig_b + band * nb + (d0 - a0), lb, s_dig + la, (uint64_t)0);
    load_slice(rows_b + band * nb + (d0 - a0), lb, s_rows + la, row_offset_b);
    __syncthreads();
    const int diag = std::min(n, (int)threadIdx.x * ITEMS);
    const uint64_t *sa = s_dig, *sb = s_dig + la;
    int ai = (int)co_rank(diag, la, lb, [sa](int64_t i) { return sa[i]; }, [sb](int64_t i) { return sb[i]; });
    int bi = diag - ai;
    uint64_t od[ITEMS];
    uint32_t orow[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const bool take_a = bi >= lb || (ai < la && sa[ai] <= sb[bi]);
        const int at = take_a ? ai : la + bi;
        if (diag + i < n) {
            od[i] = s_dig[at];
            orow[i] = s_rows[at];
        }
        ai += take_a ? 1 : 0;
        bi += take_a ? 0 : 1;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i)
        if (diag + i < n) {
            s_dig[diag + i] = od[i];
            s_rows[diag + i] = orow[i];
        }
    __syncthreads();
    store_slice(dig_out + band * n_out + d0, n, s_dig);
    store_slice(rows_out + band * n_out + d0, n, s_rows);
}

// ---- compaction ---------------------------------------------------------------------------------------------------------
// The liveness bitmap: bit (row & 31) of word row >> 5 is set when slot `row` is live.  remap[row] = live slots before it =
// prefix[row >> 5] + popcount(word & bits below row), with prefix the exclusive scan of the words' popcounts.
__device__ __forceinline__ bool slot_live(const uint32_t *bits, int64_t n, uint32_t row) {
    return (int64_t)row < n && ((bits[row >> 5] >> (row & 31)) & 1u);
}
__device__ __forceinline__ uint32_t slot_remap(const uint32_t *bits, const uint32_t *prefix, uint32_t row) {
    return prefix[row >> 5] + (uint32_t)__popc(bits[row >> 5] & ((1u << (row & 31)) - 1u));
}

struct WordPopcIn {  // value = live slots in word i (bits past n masked off)
    const uint32_t *bits;
    int64_t n;
    __device__ __forceinline__ uint32_t get(int64_t i) const {
        const int64_t left = n - i * 32;
        const uint32_t mask = left >= 32 ? ~0u : ((1u << left) - 1u);
        return (uint32_t)__popc(bits[i] & mask);
    }
};
struct WordPrefixOut {
    uint32_t *prefix;
    __device__ __forceinline__ void put(int64_t i, uint64_t p, uint32_t) const { prefix[i] = (uint32_t)p; }
};
struct LiveEntryIn {  // value = 1 where the band entry's row is live
    const uint32_t *rows, *bits;
    int64_t n;
    __device__ __forceinline__ uint32_t get(int64_t i) const { return slot_live(bits, n, rows[i]) ? 1u : 0u; }
};
struct BandEntryOut {  // the live entries, packed, with remapped rows; nothing at or past `limit`
    const uint64_t *dig;
    const uint32_t *rows, *bits, *prefix;
    int64_t limit;
    uint64_t *dig_out;
    uint32_t *rows_out;
    __device__ __forceinline__ void put(int64_t i, uint64_t p, uint32_t live) const {
        if (live && (int64_t)p < limit) {
            dig_out[p] = dig[i];
            rows_out[p] = slot_remap(bits, prefix, rows[i]);
        }
    }
};

// dst row remap[row] = src row `row` for every live row; V is the access unit (16, 8, 4 or 1 bytes)
template <typename V>
__global__ __launch_bounds__(256) void rows_compact_kernel(const V *__restrict__ src, int64_t units, int64_t n_rows,
                                                           const uint32_t *__restrict__ bits, const uint32_t *__restrict__ prefix,
                                                           V *__restrict__ dst) {
    const int64_t total = n_rows * units;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / units, u = idx - row * units;
        if (slot_live(bits, n_rows, (uint32_t)row)) dst[(int64_t)slot_remap(bits, prefix, (uint32_t)row) * units + u] = src[idx];
    }
}

// scratch[3]: prefix u32[n_words] | scan temporary; the popcount scan enqueued, its total in *d_total
int live_prefix(mhx_ctx *ctx, const uint32_t *d_bits, int64_t n, size_t extra_tmp, uint32_t **d_prefix, void **d_tmp,
                uint64_t **d_total) {
    const int64_t n_words = (n + 31) / 32;
    const size_t prefix_bytes = pad256(sizeof(uint32_t) * (size_t)n_words);
    const size_t tmp = std::max(scan_tmp_bytes(n_words), extra_tmp);
    if (int rc = ctx->ensure_scratch(3, prefix_bytes + tmp)) return rc;
    *d_prefix = (uint32_t *)ctx->scratch[3];
    *d_tmp = (char *)ctx->scratch[3] + prefix_bytes;
    return device_exclusive_scan(ctx, WordPopcIn{d_bits, n}, WordPrefixOut{*d_prefix}, n_words, *d_tmp, d_total);
}

}  // namespace

int launch_lsh_bands_merge(mhx_ctx *ctx, const uint64_t *d_dig_a, const uint32_t *d_rows_a, int64_t n_a, const uint64_t *d_dig_b,
                           const uint32_t *d_rows_b, int64_t n_b, uint32_t row_offset_b, int32_t bands, uint64_t *d_dig_out,
                           uint32_t *d_rows_out) {
    const int items = ctx->opt_lsh_merge_items == 16 ? 16 : ctx->opt_lsh_merge_items == 8 ? 8 : kMergeItemsDefault;
    const int tile = kMergeThreads * items;
    const int64_t n_out = n_a + n_b;
    const int64_t tiles = (n_out + tile - 1) / tile;
    // one workgroup per (band, tile): the grid's work-items (blocks x 256) must stay below 2^32
    if (tiles * bands * kMergeThreads >= ((int64_t)1 << 32)) return fail(MHX_ERR_UNSUPPORTED, "too many merge tiles for one launch");
    if (int rc = ctx->ensure_scratch(3, sizeof(int64_t) * (size_t)bands * (size_t)(tiles + 1))) return rc;
    int64_t *d_part = (int64_t *)ctx->scratch[3];
    hipLaunchKernelGGL(bands_merge_partition_kernel, dim3(grid_for(ctx, (int64_t)bands * (tiles + 1))), dim3(256), 0, ctx->stream,
                       d_dig_a, n_a, d_dig_b, n_b, bands, tiles, tile, d_part);
    if (items == 16)
        hipLaunchKernelGGL(bands_merge_kernel<16>, dim3((unsigned)(tiles * bands)), dim3(kMergeThreads), 0, ctx->stream, d_dig_a, d_rows_a,
                           n_a, d_dig_b, d_rows_b, n_b, row_offset_b, tiles, d_part, d_dig_out, d_rows_out);
    else
        hipLaunchKernelGGL(bands_merge_kernel<8>, dim3((unsigned)(tiles * bands)), dim3(kMergeThreads), 0, ctx->stream, d_dig_a, d_rows_a,
                           n_a, d_dig_b, d_rows_b, n_b, row_offset_b, tiles, d_part, d_dig_out, d_rows_out);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_lsh_bands_compact(mhx_ctx *ctx, const uint64_t *d_dig, const uint32_t *d_rows, int64_t n, int32_t bands,
                             const uint32_t *d_live_bits, int64_t n_live, uint64_t *d_dig_out, uint32_t *d_rows_out) {
    const int64_t total = n * (int64_t)bands;
    uint32_t *d_prefix = nullptr;
    void *d_tmp = nullptr;
    uint64_t *d_live_total = nullptr, *d_kept_total = nullptr;
    if (int rc = live_prefix(ctx, d_live_bits, n, scan_tmp_bytes(total) + 256, &d_prefix, &d_tmp, &d_live_total)) return rc;
    uint64_t live_total = 0;  // once it is read back, the flat scan below reuses the popcount scan's temporary
    if (int rc = read_back_u64(ctx, d_live_total, &live_total)) return rc;
    if ((int64_t)live_total != n_live)
        return fail(MHX_ERR_INVALID, "n_live %lld differs from the %llu live slots of the bitmap", (long long)n_live,
                    (unsigned long long)live_total);
    const int64_t limit = n_live * (int64_t)bands;
    if (int rc = device_exclusive_scan(ctx, LiveEntryIn{d_rows, d_live_bits, n},
                                       BandEntryOut{d_dig, d_rows, d_live_bits, d_prefix, limit, d_dig_out, d_rows_out}, total, d_tmp,
                                       &d_kept_total))
        return rc;
    uint64_t kept = 0;
    if (int rc = read_back_u64(ctx, d_kept_total, &kept)) return rc;
    if ((int64_t)kept != limit)
        return fail(MHX_ERR_INVALID, "the bands hold %llu live entries, not bands * n_live = %lld (is every band a permutation of the slots?)",
                    (unsigned long long)kept, (long long)limit);
    return MHX_OK;
}

int launch_rows_compact(mhx_ctx *ctx, const void *d_src, int64_t row_bytes, int64_t n_rows, const uint32_t *d_live_bits, void *d_dst,
                        int64_t *n_kept) {
    uint32_t *d_prefix = nullptr;
    void *d_tmp = nullptr;
    uint64_t *d_total = nullptr;
    if (int rc = live_prefix(ctx, d_live_bits, n_rows, 0, &d_prefix, &d_tmp, &d_total)) return rc;
    const uintptr_t align = reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_dst) | (uintptr_t)row_bytes;
    const int unit = align % 16 == 0 ? 16 : align % 8 == 0 ? 8 : align % 4 == 0 ? 4 : 1;
    const int64_t units = row_bytes / unit;
    const dim3 grid(grid_for(ctx, n_rows * units));
    if (unit == 16)
        hipLaunchKernelGGL(rows_compact_kernel<uint4>, grid, dim3(256), 0, ctx->stream, (const uint4 *)d_src, units, n_rows, d_live_bits,
                           d_prefix, (uint4 *)d_dst);
    else if (unit == 8)
        hipLaunchKernelGGL(rows_compact_kernel<uint2>, grid, dim3(256), 0, ctx->stream, (const uint2 *)d_src, units, n_rows, d_live_bits,
                           d_prefix, (uint2 *)d_dst);
    else if (unit == 4)
        hipLaunchKernelGGL(rows_compact_kernel<uint32_t>, grid, dim3(256), 0, ctx->stream, (const uint32_t *)d_src, units, n_rows,
                           d_live_bits, d_prefix, (uint32_t *)d_dst);
    else
        hipLaunchKernelGGL(rows_compact_kernel<uint8_t>, grid, dim3(256), 0, ctx->stream, (const uint8_t *)d_src, units, n_rows,
                           d_live_bits, d_prefix, (uint8_t *)d_dst);
    MHX_HIP_CHECK(hipGetLastError());
    uint64_t kept = 0;
    if (int rc = read_back_u64(ctx, d_total, &kept)) return rc;
    *n_kept = (int64_t)kept;
    return MHX_OK;
}

}  // namespace mhx
