// device_scan.h -- the hand-written device-wide exclusive scan, and the read-back of its total: lsh_query_kernels.hip and lsh_index_kernels.hip.
// Header-only: every kernel and helper is in an anonymous namespace, so each translation unit that includes it has its own copy.
#pragma once

#include <cstdint>

#include "mhx_internal.h"

namespace mhx {
namespace {

// ---- device-wide exclusive scan, hand-written (round 5: rocPRIM's exclusive_scan and unique are gone from this file) ------
// Three launches over tiles of 256 threads x 16 items: (1) every tile's sum, (2) one workgroup turns the tile sums into tile
// offsets (and the grand total), (3) every tile scans again from its offset and hands (index, exclusive prefix, value) to the
// output functor.  The input is a functor too, so that "unique" is the same three launches: value = 1 where a sorted key
// differs from its predecessor, output = the key written at its prefix.  The input is read twice (8 B + 8 B per element for
// 40M counts -> where: 0.5 GB, ~0.15 ms); a decoupled look-back would read it once and is not worth its spin loops here.
constexpr int kScanItems = 16, kScanTile = 256 * kScanItems;

struct CountsIn {  // value = counts[i]
    const uint32_t *counts;
    __device__ __forceinline__ uint32_t get(int64_t i) const { return counts[i]; }
};
struct WhereOut {  // where[i] = exclusive prefix
    uint64_t *where;
    __device__ __forceinline__ void put(int64_t i, uint64_t prefix, uint32_t) const { where[i] = prefix; }
};
struct HeadsIn {  // value = 1 at the first element of a run of equal sorted keys
    const uint64_t *keys;
    __device__ __forceinline__ uint32_t get(int64_t i) const { return i == 0 || keys[i] != keys[i - 1] ? 1u : 0u; }
};
struct CompactOut {  // the run heads, packed
    const uint64_t *keys;
    uint64_t *out;
    __device__ __forceinline__ void put(int64_t i, uint64_t prefix, uint32_t head) const {
        if (head) out[prefix] = keys[i];
    }
};

__device__ __forceinline__ uint64_t block_inclusive_scan64(uint64_t v, uint64_t *tmp4, int tid) {
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), o);
        if (lane >= o) v += ((uint64_t)hi << 32) | lo;
    }
    if (lane == 63) tmp4[wave] = v;
    __syncthreads();
    uint64_t add = 0;
    for (int w = 0; w < wave; ++w) add += tmp4[w];
    __syncthreads();
    return v + add;
}

template <typename In>
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(In in, int64_t n, uint64_t *__restrict__ tile_sums) {
    __shared__ uint64_t tmp[4];
    const int64_t first = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (first + j < n) sum += in.get(first + j);
    const uint64_t incl = block_inclusive_scan64(sum, tmp, threadIdx.x);
    if (threadIdx.x == 255) tile_sums[blockIdx.x] = incl;
}

// tile sums -> exclusive tile offsets in place; total[0] = the grand total.  One workgroup: a 10M-row index has 80 000 tiles.
__global__ __launch_bounds__(1024) void scan_tile_offsets_kernel(uint64_t *__restrict__ tiles, int64_t n_tiles, uint64_t *__restrict__ total) {
    __shared__ uint64_t tmp[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_tiles; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const uint64_t v = i < n_tiles ? tiles[i] : 0;
        // inclusive scan over the 1024 threads: 16 waves
        uint64_t x = v;
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)x, o), hi = (uint32_t)__shfl_up((int)(uint32_t)(x >> 32), o);
            if (lane >= o) x += ((uint64_t)hi << 32) | lo;
        }
        if (lane == 63) tmp[wave] = x;
        __syncthreads();
        uint64_t add = carry;
        for (int w = 0; w < wave; ++w) add += tmp[w];
        if (i < n_tiles) tiles[i] = add + x - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = add + x;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

template <typename In, typename Out>
__global__ __launch_bounds__(256) void scan_apply_kernel(In in, int64_t n, const uint64_t *__restrict__ tile_offsets, Out out) {
    __shared__ uint64_t tmp[4];
    const int64_t first = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    uint32_t v[kScanItems];
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        v[j] = first + j < n ? in.get(first + j) : 0u;
        sum += v[j];
    }
    uint64_t at = tile_offsets[blockIdx.x] + block_inclusive_scan64(sum, tmp, threadIdx.x) - sum;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (first + j < n) out.put(first + j, at, v[j]);
        at += v[j];
    }
}

// scratch words the scan needs for n elements: the tile sums and the total
inline size_t scan_tmp_bytes(int64_t n) { return ((sizeof(uint64_t) * (size_t)((n + kScanTile - 1) / kScanTile + 2)) + 255) & ~(size_t)255; }

// enqueues the three launches; the grand total lands in d_tmp[n_tiles] (device) -- the caller reads it back when it needs it
template <typename In, typename Out>
int device_exclusive_scan(mhx_ctx *ctx, In in, Out out, int64_t n, void *d_tmp, uint64_t **d_total) {
    const int64_t n_tiles = (n + kScanTile - 1) / kScanTile;
    uint64_t *tiles = static_cast<uint64_t *>(d_tmp);
    *d_total = tiles + n_tiles;
    if (n_tiles >= (int64_t)1 << 31) return fail(MHX_ERR_UNSUPPORTED, "scan of more than 2^43 elements");
    hipLaunchKernelGGL(scan_tile_sums_kernel<In>, dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, in, n, tiles);
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, tiles, n_tiles, *d_total);
    hipLaunchKernelGGL((scan_apply_kernel<In, Out>), dim3((unsigned)n_tiles), dim3(256), 0, ctx->stream, in, n, tiles, out);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

// one device word -- a scan's total -- back on the host: blocks until the stream has drained
inline int read_back_u64(mhx_ctx *ctx, const uint64_t *d_word, uint64_t *word) {
    MHX_HIP_CHECK(hipMemcpyAsync(word, d_word, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

}  // namespace
}  // namespace mhx
