// bloom_kernels.hip -- the per-band Bloom filters of MinHashLSHBloom (ref: datasketch/lsh_bloom.py).
//
// The index is one array uint32 [bands][n_blocks][16]: every band has a cache-line-blocked Bloom filter of n_blocks blocks of 512
// bits, and all the bits of a key fall into one block -- a query reads one 64-byte line per (row, band), an insert touches one.
// For row i and band j over the signature matrix [n, num_perm] (columns from bands * r on are ignored)
//     s   = sum of sig[i, j*r .. j*r + r) in uint64, wrapping mod 2^64        (ref :105, :117: sum(hashvalues) over np.uint64)
//     x   = s mod (2^61 - 1)                                                  (ref :105: % _mersenne_prime)
//     out_t = splitmix64 output t of the stream seeded with x (state x, += 0x9E3779B97F4A7C15 per draw)
//     block = ((out_0 >> 32) * n_blocks) >> 32
//     pos_i = (out_{1 + i / 7} >> 9 * (i % 7)) & 511   for i < k; word pos >> 5, bit pos & 31; positions may repeat
// The bit layout is this project's own (the reference leaves it to pybloomfilter); datasketch_amd/lsh_bloom.py holds the numpy
// twin, which produces the same words: OR does not depend on the order of the inserts.
//
// Two lane mappings, each kept for the operation it is faster at (measured: DESIGN.md section 5, "The Bloom index"); option
// "bloom.lanes" forces one of them for both operations:
//   16 lanes per (row, band), the insert: lane w owns word w of the block, so the atomics of one key are one contiguous
//      64-byte segment (they cost next to nothing that way); the r values of the band are summed 16 at a time and folded
//      with four shuffles; every lane of the group repeats the key's arithmetic;
//   1 lane per (row, band), the query: the lane builds the whole mask in LDS ([16][256] words, its column) and reads the line
//      as four 16-byte loads -- a sixteenth of the arithmetic; as an insert it issues up to 16 atomics to scattered lines.
// A workgroup owns tiles of kTileRows rows: the any-band answer of a row is OR-ed together in LDS and written as one byte per
// row by the workgroup that owns the row -- no workgroup waits for another.  Word indices are 64-bit throughout.
#include "mhx_internal.h"

namespace mhx {
namespace {

constexpr int kTileRows = 64;
constexpr uint64_t kM61 = ((uint64_t)1 << 61) - 1;
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t splitmix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint64_t mod_m61(uint64_t s) {
    const uint64_t x = (s & kM61) + (s >> 61);  // <= 2^61 - 1 + 7
    return x >= kM61 ? x - kM61 : x;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, mask, 16), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), mask, 16);
    return ((uint64_t)hi << 32) | lo;
}

enum { kInsert = 0, kQuery = 1 };

// LANES lanes per (row, band); MODE kInsert: filter |= masks; kQuery: hit[row] = any band whose mask is in the filter
template <class T, int LANES, int MODE>
__global__ __launch_bounds__(256) void bloom_kernel(const T *__restrict__ sig, int64_t n, int num_perm, int bands, int r, int k,
                                                    uint32_t n_blocks, uint32_t *filter, uint8_t *__restrict__ hit) {
    __shared__ uint32_t tile_hit[kTileRows];
    __shared__ uint32_t lane_mask[LANES == 1 ? 16 * 256 : 1];
    const int tid = (int)threadIdx.x;
    const int sub = LANES == 16 ? tid & 15 : 0;          // the word this lane owns (16 lanes per key)
    const int team = LANES == 16 ? tid >> 4 : tid;       // which key of a step this lane works on
    const int teams = 256 / LANES;
    const int64_t tiles = (n + kTileRows - 1) / kTileRows;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t row0 = tile * kTileRows;
        const int rows = (int)(n - row0 < kTileRows ? n - row0 : kTileRows);
        const int items = rows * bands;
        if (MODE == kQuery) {
            if (tid < kTileRows) tile_hit[tid] = 0;
            __syncthreads();
        }
        // every lane of the workgroup makes the same number of trips: the shuffles and the ballot below see whole waves
        for (int base = 0; base < items; base += teams) {
            const int item = base + team;
            const bool live = item < items;
            const int local = live ? item / bands : 0, band = live ? item - local * bands : 0;
            const T *src = sig + (row0 + local) * (int64_t)num_perm + (int64_t)band * r;
            uint64_t s = 0;
            if (LANES == 16) {
                if (live)
                    for (int c = sub; c < r; c += 16) s += (uint64_t)src[c];
                s += shfl_xor64(s, 8);
                s += shfl_xor64(s, 4);
                s += shfl_xor64(s, 2);
                s += shfl_xor64(s, 1);
            } else if (live) {
                for (int c = 0; c < r; ++c) s += (uint64_t)src[c];
            }
            uint64_t state = mod_m61(s) + kGolden;
            const uint64_t block = ((splitmix(state) >> 32) * (uint64_t)n_blocks) >> 32;
            uint32_t *line = filter + (((int64_t)band * n_blocks + (int64_t)block) << 4);
            if (LANES == 16) {
                uint32_t m = 0;
                for (int i = 0; i < k; i += 7) {
                    state += kGolden;
                    uint64_t out = splitmix(state);
                    const int here = k - i < 7 ? k - i : 7;
                    for (int t = 0; t < here; ++t, out >>= 9) {
                        const uint32_t pos = (uint32_t)out & 511u;
                        if ((int)(pos >> 5) == sub) m |= 1u << (pos & 31);
                    }
                }
                if (MODE == kInsert) {
                    // read first: a word whose bits are all there already costs no atomic (duplicate-heavy corpora)
                    if (live && m && (__atomic_load_n(line + sub, __ATOMIC_RELAXED) & m) != m) atomicOr(line + sub, m);
                } else {
                    const uint32_t have = live ? __atomic_load_n(line + sub, __ATOMIC_RELAXED) : 0u;
                    const unsigned long long ok = __ballot(live && (have & m) == m);
                    const int shift = (int)(threadIdx.x & 48);  // this key's 16 lanes within the wave
                    if (sub == 0 && live && ((ok >> shift) & 0xFFFFull) == 0xFFFFull) atomicOr(&tile_hit[local], 1u);
                }
            } else {
                uint32_t *mine = lane_mask + tid;  // word w of this lane's mask: mine[w * 256]
#pragma unroll
                for (int w = 0; w < 16; ++w) mine[w * 256] = 0;
                for (int i = 0; i < k; i += 7) {
                    state += kGolden;
                    uint64_t out = splitmix(state);
                    const int here = k - i < 7 ? k - i : 7;
                    for (int t = 0; t < here; ++t, out >>= 9) {
                        const uint32_t pos = (uint32_t)out & 511u;
                        mine[(pos >> 5) * 256] |= 1u << (pos & 31);
                    }
                }
                if (MODE == kInsert) {
                    if (live) {
#pragma unroll
                        for (int w = 0; w < 16; ++w) {
                            const uint32_t m = mine[w * 256];
                            if (m && (__atomic_load_n(line + w, __ATOMIC_RELAXED) & m) != m) atomicOr(line + w, m);
                        }
                    }
                } else if (live) {
                    bool ok = true;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint4 have = reinterpret_cast<const uint4 *>(line)[q];
                        const uint32_t m0 = mine[(4 * q) * 256], m1 = mine[(4 * q + 1) * 256], m2 = mine[(4 * q + 2) * 256],
                                       m3 = mine[(4 * q + 3) * 256];
                        ok = ok && (have.x & m0) == m0 && (have.y & m1) == m1 && (have.z & m2) == m2 && (have.w & m3) == m3;
                    }
                    if (ok) atomicOr(&tile_hit[local], 1u);
                }
            }
        }
        if (MODE == kQuery) {
            __syncthreads();
            if (tid < rows) hit[row0 + tid] = (uint8_t)tile_hit[tid];
            __syncthreads();
        }
    }
}

// dst |= src, 16 bytes per lane (a filter is whole 64-byte blocks)
// (no __restrict__: a filter may be merged into itself)
__global__ __launch_bounds__(256) void bloom_union_kernel(uint4 *dst, const uint4 *src, int64_t quads) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += stride) {
        uint4 x = dst[i];
        const uint4 y = src[i];
        x.x |= y.x;
        x.y |= y.y;
        x.z |= y.z;
        x.w |= y.w;
        dst[i] = x;
    }
}

template <class T, int LANES>
int launch_typed(mhx_ctx *ctx, const T *d_sig, int64_t n, int num_perm, int bands, int r, int k, uint32_t n_blocks, uint32_t *d_filter,
                 uint8_t *d_hit, bool query) {
    const int64_t tiles = (n + kTileRows - 1) / kTileRows;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)ctx->num_cus * 16));
    if (query)
        hipLaunchKernelGGL((bloom_kernel<T, LANES, kQuery>), dim3(grid), dim3(256), 0, ctx->stream, d_sig, n, num_perm, bands, r, k, n_blocks,
                           d_filter, d_hit);
    else
        hipLaunchKernelGGL((bloom_kernel<T, LANES, kInsert>), dim3(grid), dim3(256), 0, ctx->stream, d_sig, n, num_perm, bands, r, k, n_blocks,
                           d_filter, d_hit);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

template <class T>
int launch_lanes(mhx_ctx *ctx, const T *d_sig, int64_t n, int num_perm, int bands, int r, int k, uint32_t n_blocks, uint32_t *d_filter,
                 uint8_t *d_hit, bool query) {
    const bool one = ctx->opt_bloom_lanes == 0 ? query : ctx->opt_bloom_lanes == 1;  // auto: one lane queries, sixteen insert
    if (one) return launch_typed<T, 1>(ctx, d_sig, n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, query);
    return launch_typed<T, 16>(ctx, d_sig, n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, query);
}

int launch_one(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int num_perm, int bands, int r, int k, uint32_t n_blocks,
               uint32_t *d_filter, uint8_t *d_hit, bool query) {
    if (sig_dtype == MHX_U32)
        return launch_lanes(ctx, static_cast<const uint32_t *>(d_sig), n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, query);
    return launch_lanes(ctx, static_cast<const uint64_t *>(d_sig), n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, query);
}

}  // namespace

int launch_bloom_insert(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                        uint32_t n_blocks, uint32_t *d_filter) {
    if (n == 0) return MHX_OK;
    return launch_one(ctx, d_sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, nullptr, false);
}

int launch_bloom_query(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                       uint32_t n_blocks, uint32_t *d_filter, uint8_t *d_hit) {
    if (n == 0) return MHX_OK;
    return launch_one(ctx, d_sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, true);
}

int launch_bloom_union(mhx_ctx *ctx, uint32_t *d_dst, const uint32_t *d_src, int64_t words) {
    if (words == 0) return MHX_OK;
    hipLaunchKernelGGL(bloom_union_kernel, dim3(grid_for(ctx, words / 4, 32)), dim3(256), 0, ctx->stream, reinterpret_cast<uint4 *>(d_dst),
                       reinterpret_cast<const uint4 *>(d_src), words / 4);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
