// jaccard_kernels.hip -- all-pairs Jaccard numerators: counts[i][j] = positions where row i of A
// and row j of B agree, as a dense matrix or as the list of pairs whose count reaches a threshold.
//
// Dense signatures: the numerator of MinHash.jaccard (ref: datasketch/minhash.py:299-324), exact equality on the full element
// width.  b-bit rows (mhx_bbit_pack*: ref datasketch/b_bit_minhash.py:53-72, 82-101): num_perm minus the slots that differ,
// XOR + fold every slot to its lowest bit + popcount, on the packed words.
//
// One workgroup (256 threads) owns a 128 x 128 tile of pairs and walks the rows in chunks of 16 32-bit words staged through
// LDS ([word][row], k-major so that a thread's 4 consecutive rows are one 16-byte LDS read).  Thread (ty, tx) keeps an 8 x 8
// register sub-tile: rows ty*4 + {0..3} and 64 + ty*4 + {0..3}, columns likewise with tx -- the two halves keep every 16-byte
// LDS read of a wave on distinct banks.  The next chunk's global loads are issued before the current chunk is computed.
// Per (pair, 32-bit word): v_cmp_eq_u32 + v_addc_co_u32 for dense uint32, v_xor_b32 + v_bcnt_u32_b32 for b = 1.
//
// Thresholded emission: every thread counts its qualifying pairs, a wave takes its slots with one atomicAdd on a 64-bit
// counter and writes (i << 32 | j, count) at the slots below capacity -- into the caller's own pair / count buffers, which the
// sort then reads.  The total comes back to the host; when it fits, a radix sort of the packed keys (count riding along) puts
// the pairs in ascending (i, j) order and a last kernel unpacks them.  Emit + sort rather than count + scan + write: a scan
// needs the per-row counts of every pair row (n_a x n_b / 128 words, 31 GB at 10^6 rows) or a second full pass over the
// tiles to recompute them, while a threshold query's output is small next to its n^2 work.
#include <rocprim/device/device_radix_sort.hpp>

#include "jaccard_tile.h"

namespace mhx {
namespace {

using namespace jtile;  // the tile geometry, shared with the top-k strip kernel

struct TileSpace {
    int64_t tiles_m, tiles_n;
    bool triangle;  // self-join: only tiles with tj >= ti
    __device__ __forceinline__ int64_t count() const {
        return triangle ? tiles_m * (tiles_m + 1) / 2 : tiles_m * tiles_n;
    }
    __device__ __forceinline__ void locate(int64_t t, int64_t &ti, int64_t &tj) const {
        if (!triangle) {
            ti = t / tiles_n;
            tj = t - ti * tiles_n;
            return;
        }
        // row ti of the upper triangle starts at ti*T - ti*(ti-1)/2 and holds T - ti tiles
        const int64_t T = tiles_m;
        const double b = 2.0 * (double)T + 1.0;
        int64_t r = (int64_t)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
        r = r < 0 ? 0 : (r >= T ? T - 1 : r);
        auto start = [T](int64_t x) { return x * T - x * (x - 1) / 2; };
        while (r > 0 && start(r) > t) --r;
        while (r + 1 < T && start(r + 1) <= t) ++r;
        ti = r;
        tj = r + (t - start(r));
    }
};

struct EmitArgs {
    int32_t min_count;
    bool self;                       // keep i < j only
    unsigned long long *total;       // pairs found
    uint64_t *keys;                  // i << 32 | j, [capacity]
    int32_t *counts;                 // [capacity]
    int64_t capacity;
};

// SLOT 0: dense equality (WIDE: uint64 elements, else uint32).  SLOT > 0: b-bit blocks, counted as differing slots.  SLOT -1: weighted (k, t) samples.
// W: 32-bit words per row of A / B (dense uint64: elements per row).  k: num_perm.
template <int SLOT, bool WIDE, bool EMIT>
__global__ __launch_bounds__(kThreads, 2) void jaccard_tile_kernel(const uint32_t *__restrict__ a, int64_t n_a,
                                                                const uint32_t *__restrict__ b, int64_t n_b, int32_t W,
                                                                int32_t k, TileSpace space, int32_t *__restrict__ out,
                                                                int64_t ldc, int vec_store, EmitArgs em) {
    __shared__ __attribute__((aligned(16))) uint32_t As[kChunk][kLdsRow];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[kChunk][kLdsRow];
    __shared__ __attribute__((aligned(16))) uint32_t Ah[WIDE ? kChunk : 1][WIDE ? kLdsRow : 4];
    __shared__ __attribute__((aligned(16))) uint32_t Bh[WIDE ? kChunk : 1][WIDE ? kLdsRow : 4];
    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    // words past the end of a row: never equal in the dense kinds (A 0, B 1), equal (no differing slot) in the b-bit kind
    const uint32_t pad_b = SLOT <= 0 ? 1u : 0u;
    const int64_t n_tiles = space.count();
    const int chunks = (W + kChunk - 1) / kChunk;

    for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        int64_t ti, tj;
        space.locate(t, ti, tj);
        const int64_t i0 = ti * kTile, j0 = tj * kTile;

#include "jaccard_tile_count.inc"

        // sub-tile element (r, q) is pair (i0 + rowof(r), j0 + rowof(q))
        auto rowof = [](int t4, int r) { return (r < 4 ? 0 : 64) + t4 * 4 + (r & 3); };
        if (!EMIT) {
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const int64_t i = i0 + rowof(ty, r);
                if (i >= n_a) continue;
                int32_t *dst = out + i * ldc;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int64_t j = j0 + rowof(tx, 4 * h);
                    int32_t v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = SLOT <= 0 ? (int32_t)acc[r][4 * h + q] : k - (int32_t)acc[r][4 * h + q];
                    if (vec_store && j + 3 < n_b) {
                        *reinterpret_cast<int4 *>(dst + j) = make_int4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            if (j + q < n_b) dst[j + q] = v[q];
                    }
                }
            }
        } else {
            uint32_t hits = 0;
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int64_t i = i0 + rowof(ty, r), j = j0 + rowof(tx, q);
                    const int32_t cnt = SLOT <= 0 ? (int32_t)acc[r][q] : k - (int32_t)acc[r][q];
                    const bool ok = i < n_a && j < n_b && cnt >= em.min_count && (!em.self || i < j);
                    hits += ok ? 1u : 0u;
                }
            if (__ballot(hits != 0) != 0) {
                // wave-wide exclusive prefix of the hits, one atomic per wave
                const int lane = tid & 63;
                uint32_t incl = hits;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = (uint32_t)__shfl_up((int)incl, o);
                    if (lane >= o) incl += up;
                }
                unsigned long long base = 0;
                if (lane == 63) base = atomicAdd(em.total, (unsigned long long)incl);
                base = (unsigned long long)__shfl((long long)base, 63);
                int64_t slot = (int64_t)base + (int64_t)(incl - hits);
                if (hits) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int64_t i = i0 + rowof(ty, r), j = j0 + rowof(tx, q);
                            const int32_t cnt = SLOT <= 0 ? (int32_t)acc[r][q] : k - (int32_t)acc[r][q];
                            if (i < n_a && j < n_b && cnt >= em.min_count && (!em.self || i < j)) {
                                if (slot < em.capacity) {
                                    em.keys[slot] = ((uint64_t)i << 32) | (uint64_t)j;
                                    em.counts[slot] = cnt;
                                }
                                ++slot;
                            }
                        }
                }
            }
        }
        // the next tile's first LDS stores wait at the barrier at the top of its chunk loop
    }
}

__global__ __launch_bounds__(256) void unpack_threshold_pairs_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ vals,
                                                                     int64_t count, int64_t *__restrict__ pairs,
                                                                     int32_t *__restrict__ counts) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < count; p += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[p];
        pairs[2 * p] = (int64_t)(key >> 32);
        pairs[2 * p + 1] = (int64_t)(key & 0xFFFFFFFFull);
        counts[p] = vals[p];
    }
}

template <bool EMIT>
int launch_tiles(mhx_ctx *ctx, const Shape &s, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int32_t k,
                 TileSpace space, int32_t *d_out, int64_t ldc, int vec_store, const EmitArgs &em) {
    const int64_t tiles = space.triangle ? space.tiles_m * (space.tiles_m + 1) / 2 : space.tiles_m * space.tiles_n;
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)ctx->num_cus * 16)));
    const uint32_t *a = (const uint32_t *)d_a, *b = (const uint32_t *)d_b;
#define MHX_TILES(S, WD) \
    hipLaunchKernelGGL((jaccard_tile_kernel<S, WD, EMIT>), grid, dim3(kThreads), 0, ctx->stream, a, n_a, b, n_b, s.W, k, space, d_out, ldc, vec_store, em)
    switch (s.slot) {
        case -1: MHX_TILES(-1, false); break;
        case 0: if (s.wide) MHX_TILES(0, true); else MHX_TILES(0, false); break;
        case 1: MHX_TILES(1, false); break;
        case 2: MHX_TILES(2, false); break;
        case 4: MHX_TILES(4, false); break;
        case 8: MHX_TILES(8, false); break;
        case 16: MHX_TILES(16, false); break;
        default: MHX_TILES(32, false); break;
    }
#undef MHX_TILES
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace

int launch_jaccard_matrix(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t k,
                          int32_t b, int32_t *d_counts, int64_t ldc) {
    const Shape s = shape_of(sig_dtype, k, b);
    const TileSpace space{(n_a + kTile - 1) / kTile, (n_b + kTile - 1) / kTile, false};
    const int vec_store = (ldc % 4 == 0 && ((uintptr_t)d_counts & 15) == 0) ? 1 : 0;
    return launch_tiles<false>(ctx, s, d_a, n_a, d_b, n_b, k, space, d_counts, ldc, vec_store, EmitArgs{});
}

int launch_jaccard_threshold(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t k,
                             int32_t b, int32_t min_count, int64_t *d_pairs, int32_t *d_counts, int64_t capacity,
                             int64_t *n_pairs) {
    *n_pairs = 0;
    const bool self = d_b == nullptr;
    if (self) {
        d_b = d_a;
        n_b = n_a;
    }
    const Shape s = shape_of(sig_dtype, k, b);
    if (int rc = ctx->ensure_scratch(4, 256)) return rc;  // scratch[4]: the pair counter
    unsigned long long *d_total = (unsigned long long *)ctx->scratch[4];
    MHX_HIP_CHECK(hipMemsetAsync(d_total, 0, sizeof(unsigned long long), ctx->stream));
    const TileSpace space{(n_a + kTile - 1) / kTile, (n_b + kTile - 1) / kTile, self};
    const EmitArgs em{min_count, self, d_total, reinterpret_cast<uint64_t *>(d_pairs), d_counts, capacity};
    if (int rc = launch_tiles<true>(ctx, s, d_a, n_a, d_b, n_b, k, space, nullptr, 0, 0, em)) return rc;
    unsigned long long total = 0;
    MHX_HIP_CHECK(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n_pairs = (int64_t)total;
    if (total == 0 || (int64_t)total > capacity) return MHX_OK;  // caller sees n_pairs > capacity and calls again

    // the emitted (key, count) sit in the first `total` slots of the caller's buffers: sort them into scratch[3], unpack back
    const int64_t m = (int64_t)total;
    int end_bit = 33;  // the high word holds a row of A < n_a
    while (end_bit < 64 && ((int64_t)1 << (end_bit - 32)) < n_a) ++end_bit;
    size_t sort_tmp = 0;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, sort_tmp, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                             (const int32_t *)nullptr, (int32_t *)nullptr, (size_t)m, 0, end_bit, ctx->stream);
    if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim size query failed: %s", hipGetErrorString(e));
    const size_t key_bytes = ((sizeof(uint64_t) * (size_t)m) + 255) & ~(size_t)255;
    const size_t val_bytes = ((sizeof(int32_t) * (size_t)m) + 255) & ~(size_t)255;
    if (int rc = ctx->ensure_scratch(3, key_bytes + val_bytes + sort_tmp + 256)) return rc;
    uint64_t *d_keys = (uint64_t *)ctx->scratch[3];
    int32_t *d_vals = (int32_t *)((char *)ctx->scratch[3] + key_bytes);
    void *d_tmp = (char *)ctx->scratch[3] + key_bytes + val_bytes;
    e = rocprim::radix_sort_pairs(d_tmp, sort_tmp, (const uint64_t *)d_pairs, d_keys, (const int32_t *)d_counts, d_vals, (size_t)m, 0,
                                  end_bit, ctx->stream);
    if (e != hipSuccess) return fail(MHX_ERR_HIP, "rocprim::radix_sort_pairs failed: %s", hipGetErrorString(e));
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, (int64_t)ctx->num_cus * 16)));
    hipLaunchKernelGGL(unpack_threshold_pairs_kernel, grid, dim3(256), 0, ctx->stream, d_keys, d_vals, m, d_pairs, d_counts);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
