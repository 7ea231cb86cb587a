// weighted_jaccard_kernels.hip -- WeightedMinHash.jaccard numerators of listed pairs (mhx_weighted_jaccard_pairs*): counts[p] =
// the samples s at which rows pairs[p][0] of A and pairs[p][1] of B hold the same (k, t) -- both int64 values, all 64 bits of
// each (ref: datasketch/weighted_minhash.py:45-60).  Rows are [samples][2] int64, 16 bytes per sample.
//
// The all-pairs forms (matrix, threshold, top-k) are the SLOT -1 kind of the shared tile (jaccard_tile.h, jaccard_kernels.hip,
// jaccard_topk_kernels.hip); this file holds the twin of jaccard_pairs_kernel (pack_kernels.hip).  LPP lanes share a pair
// (the power of two >= samples, at most 64: one pair per wave from 64 samples on, 64 / LPP pairs per wave below), a lane
// reads one whole sample of either row per trip -- one 16-byte load where both matrices are 16-byte aligned, two 8-byte loads
// otherwise -- so a wave's loads of a row are contiguous; the lanes' counts are summed by __shfl_xor inside the group.
#include "mhx_internal.h"

namespace mhx {
namespace {

constexpr int kWave = 64;

template <bool VEC>
__global__ __launch_bounds__(256) void weighted_jaccard_pairs_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b,
                                                                     int32_t samples, int32_t lpp, const int64_t *__restrict__ pairs,
                                                                     int64_t m, int32_t *__restrict__ counts) {
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (lpp - 1);  // my position among the lanes of one pair
    const int pairs_per_wave = kWave / lpp;
    const int64_t wave_id = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t wave_stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t p0 = wave_id * pairs_per_wave; p0 < m; p0 += wave_stride * pairs_per_wave) {  // uniform: every lane reaches the shuffles
        const int64_t p = p0 + lane / lpp;
        int32_t same = 0;
        if (p < m) {
            const uint64_t *x = a + pairs[2 * p] * (2 * (int64_t)samples), *y = b + pairs[2 * p + 1] * (2 * (int64_t)samples);
            for (int c = sub; c < samples; c += lpp) {
                if (VEC) {
                    const uint4 u = reinterpret_cast<const uint4 *>(x)[c], v = reinterpret_cast<const uint4 *>(y)[c];
                    same += ((u.x ^ v.x) | (u.y ^ v.y) | (u.z ^ v.z) | (u.w ^ v.w)) == 0 ? 1 : 0;
                } else {
                    same += ((x[2 * c] ^ y[2 * c]) | (x[2 * c + 1] ^ y[2 * c + 1])) == 0 ? 1 : 0;
                }
            }
        }
        for (int d = 1; d < lpp; d <<= 1) same += __shfl_xor(same, d);
        if (p < m && sub == 0) counts[p] = same;
    }
}

}  // namespace

int launch_weighted_jaccard_pairs(mhx_ctx *ctx, const void *d_a, const void *d_b, int32_t samples, const int64_t *d_pairs, int64_t m,
                                  int32_t *d_counts) {
    int lpp = 1;
    while (lpp < samples && lpp < kWave) lpp <<= 1;
    const int64_t waves = (m + kWave / lpp - 1) / (kWave / lpp);
    const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((waves + 3) / 4, (int64_t)ctx->num_cus * 16)));
    const bool vec = (((uintptr_t)d_a | (uintptr_t)d_b) & 15) == 0;  // (a row is a multiple of 16 bytes)
    if (vec)
        hipLaunchKernelGGL(weighted_jaccard_pairs_kernel<true>, grid, dim3(256), 0, ctx->stream, (const uint64_t *)d_a, (const uint64_t *)d_b,
                           samples, lpp, d_pairs, m, d_counts);
    else
        hipLaunchKernelGGL(weighted_jaccard_pairs_kernel<false>, grid, dim3(256), 0, ctx->stream, (const uint64_t *)d_a, (const uint64_t *)d_b,
                           samples, lpp, d_pairs, m, d_counts);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
