// hll_kernels.hip -- HyperLogLog registers, histograms and unions (ref: datasketch/hyperloglog.py).
//
// hll_bulk: for every set i and every token hash hv of its CSR range
//     idx  = hv & (m - 1)                                   (ref :138)
//     rank = clz_W(hv >> p) - p + 1, clz_W(0) = W           (ref :140, :238-246: max_rank - bit_length(bits) + 1)
//     reg[i, idx] = max(reg[i, idx], rank)                  (ref :142)
// Registers are accumulated in LDS and written out as packed bytes.  LDS has a 32-bit max but no byte-wide one, so the
// layout depends on p (hll_layout): up to kWaveMaxP one wave per set over one word per register (four sets per workgroup),
// up to kWordMaxP one workgroup per set over one word per register (32 KiB at p = 13), beyond that one workgroup per set
// over packed bytes (64 KiB at p = 16) raised by a compare-and-swap on the word that holds the byte.  That loop does not
// wait for anybody: a failed swap means a byte of the word has risen, a byte rises at most 61 times, so a lane retries at
// most 4 * 61 times whatever the other lanes do.
//
// Sets longer than the split threshold are left out by the per-set kernel (it writes their init row) and done by the split
// kernel: the token array is cut into equal ranges, one workgroup each with private LDS registers, and what a workgroup found
// for a long set is folded into the set's output row by a byte-wise max under a compare-and-swap of the 32-bit word (bounded
// in the same way).  Max is commutative and idempotent: every path writes the same bytes, in whatever order workgroups run.
#include "mhx_internal.h"

namespace mhx {
namespace {

constexpr int kWaveMaxP = 8;   // one wave per set, words: 4 sets x 1 KiB per workgroup at p = 8
constexpr int kWordMaxP = 13;  // one workgroup per set, words: 32 KiB at p = 13 (five workgroups per CU of 160 KiB)
enum { kLayoutWave = 0, kLayoutWords = 1, kLayoutBytes = 2 };

// idx and rank of one hash; false: the hash does not fit hash_bits (ref :240-245, "Hash value overflow")
template <class T>
__device__ __forceinline__ bool hll_slot(T raw, int p, int hash_bits, uint32_t mask, uint32_t &idx, uint32_t &rank) {
    const uint64_t hv = (uint64_t)raw;
    idx = (uint32_t)hv & mask;
    if (hash_bits == 32) {
        if (hv >> 32) return false;
        const uint32_t bits = (uint32_t)hv >> p;
        rank = (uint32_t)((bits ? __clz((int)bits) : 32) - p + 1);
    } else {
        const uint64_t bits = hv >> p;
        rank = (uint32_t)((bits ? __clzll((long long)bits) : 64) - p + 1);
    }
    return true;
}

// raise byte (idx & 3) of LDS word idx >> 2 to rank
__device__ __forceinline__ void lds_byte_max(uint32_t *words, uint32_t idx, uint32_t rank) {
    uint32_t *w = words + (idx >> 2);
    const int sh = (int)(idx & 3) * 8;
    uint32_t old = *(volatile uint32_t *)w;
    while (((old >> sh) & 0xFFu) < rank) {
        const uint32_t want = (old & ~(0xFFu << sh)) | (rank << sh);
        const uint32_t seen = atomicCAS(w, old, want);
        if (seen == old) break;
        old = seen;
    }
}

__device__ __forceinline__ uint32_t byte_max4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const uint32_t x = (a >> k) & 0xFFu, y = (b >> k) & 0xFFu;
        r |= (x > y ? x : y) << k;
    }
    return r;
}

// fold four packed registers into a word of an output row that other workgroups fold into as well
__device__ __forceinline__ void global_byte_max4(uint32_t *g, uint32_t v) {
    uint32_t old = __atomic_load_n(g, __ATOMIC_RELAXED);
    for (;;) {
        const uint32_t want = byte_max4(old, v);
        if (want == old) break;
        const uint32_t seen = atomicCAS(g, old, want);
        if (seen == old) break;
        old = seen;
    }
}

template <int LAYOUT>
__device__ __forceinline__ void lds_update(uint32_t *slab, uint32_t idx, uint32_t rank) {
    if (LAYOUT == kLayoutBytes)
        lds_byte_max(slab, idx, rank);
    else
        atomicMax(slab + idx, rank);
}

// four packed registers q*4 .. q*4+3 of a slab
template <int LAYOUT>
__device__ __forceinline__ uint32_t lds_packed(const uint32_t *slab, int q) {
    if (LAYOUT == kLayoutBytes) return slab[q];
    const uint4 w = *reinterpret_cast<const uint4 *>(slab + 4 * q);
    return w.x | (w.y << 8) | (w.z << 16) | (w.w << 24);
}

// One wave (kLayoutWave) or one workgroup per set.  Every wave of a workgroup makes the same number of trips through the
// set loop, so the barriers are met by all of them; a set beyond n_sets, or longer than `split`, only skips its tokens.
// The first kPrefetch tokens per lane of the NEXT set are fetched before the current set is folded: a set of a few hundred
// tokens is otherwise one memory latency per set with nothing else in flight from its wave.
constexpr int kPrefetch = 4;

template <int LAYOUT, class T>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void hll_bulk_kernel(const T *__restrict__ hv, const int64_t *__restrict__ offsets, int64_t fixed_len,
                                                       int64_t n_sets, int p, int hash_bits, int64_t split,
                                                       const uint8_t *__restrict__ init, int64_t init_stride, uint8_t *__restrict__ out,
                                                       unsigned long long *overflow) {
    extern __shared__ __align__(16) uint32_t hll_lds[];
    const int m = 1 << p;
    const uint32_t mask = (uint32_t)m - 1;
    const int team = LAYOUT == kLayoutWave ? 64 : 256;
    const int lane = LAYOUT == kLayoutWave ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    const int wave = LAYOUT == kLayoutWave ? (int)(threadIdx.x >> 6) : 0;
    const int per_block = LAYOUT == kLayoutWave ? 4 : 1;
    const int words = LAYOUT == kLayoutBytes ? m / 4 : m;
    uint32_t *slab = hll_lds + (size_t)wave * words;
    unsigned long long bad = 0;
    // the tokens [beg, end) this kernel folds for the set of this wave in the trip that starts at `base` (none: no such set, or a split one)
    auto span = [&](int64_t base, int64_t &beg, int64_t &end) {
        const int64_t set = base + wave;
        beg = end = 0;
        if (base < n_sets && set < n_sets) {
            beg = offsets ? offsets[set] : set * fixed_len;
            end = offsets ? offsets[set + 1] : beg + fixed_len;
            if (split > 0 && end - beg > split) end = beg;
        }
    };
    auto fetch = [&](T (&tok)[kPrefetch], int64_t beg, int64_t end) {
#pragma unroll
        for (int u = 0; u < kPrefetch; ++u) {
            const int64_t t = beg + lane + (int64_t)u * team;
            tok[u] = t < end ? hv[t] : T(0);
        }
    };
    auto fold = [&](T raw) {
        uint32_t idx, rank;
        if (hll_slot(raw, p, hash_bits, mask, idx, rank))
            lds_update<LAYOUT>(slab, idx, rank);
        else
            ++bad;
    };
    const int64_t step = (int64_t)gridDim.x * per_block;
    int64_t beg, end;
    T cur[kPrefetch];
    span((int64_t)blockIdx.x * per_block, beg, end);
    fetch(cur, beg, end);
    for (int64_t base = (int64_t)blockIdx.x * per_block; base < n_sets; base += step) {
        const int64_t set = base + wave;
        const bool live = set < n_sets;
        int64_t next_beg, next_end;
        T next[kPrefetch];
        span(base + step, next_beg, next_end);
        fetch(next, next_beg, next_end);
        if (live) {
            const uint8_t *row = init ? init + set * init_stride : nullptr;
            for (int w = lane; w < words; w += team) {
                uint32_t v = 0;
                if (row) v = LAYOUT == kLayoutBytes ? reinterpret_cast<const uint32_t *>(row)[w] : (uint32_t)row[w];
                slab[w] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kPrefetch; ++u)
            if (beg + lane + (int64_t)u * team < end) fold(cur[u]);
#pragma unroll 4
        for (int64_t t = beg + lane + (int64_t)kPrefetch * team; t < end; t += team) fold(hv[t]);
        __syncthreads();
        if (live) {
            uint32_t *dst = reinterpret_cast<uint32_t *>(out + set * (int64_t)m);
            for (int q = lane; q < m / 4; q += team) dst[q] = lds_packed<LAYOUT>(slab, q);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kPrefetch; ++u) cur[u] = next[u];
        beg = next_beg;
        end = next_end;
    }
    if (bad) atomicAdd(overflow, bad);
}

// The split path: workgroup b owns the tokens [b * chunk, (b + 1) * chunk) of the array and folds, for every set longer than
// `split` that overlaps them, its part of the set into the set's row (which hll_bulk_kernel has written before).
template <int LAYOUT, class T>
__global__ __launch_bounds__(256) void hll_split_kernel(const T *__restrict__ hv, const int64_t *__restrict__ offsets, int64_t fixed_len,
                                                        int64_t n_sets, int64_t total, int64_t chunk, int p, int hash_bits, int64_t split,
                                                        uint8_t *out, unsigned long long *overflow) {
    extern __shared__ __align__(16) uint32_t hll_lds[];
    const int m = 1 << p;
    const uint32_t mask = (uint32_t)m - 1;
    const int tid = (int)threadIdx.x;
    const int words = LAYOUT == kLayoutBytes ? m / 4 : m;
    const int64_t t0 = (int64_t)blockIdx.x * chunk, t1 = t0 + chunk < total ? t0 + chunk : total;
    if (t0 >= t1) return;
    int64_t first = 0;  // the last set that begins at or before t0 (0 when none does)
    if (!offsets) {
        first = fixed_len > 0 ? t0 / fixed_len : n_sets;
    } else {
        int64_t lo = 0, hi = n_sets;  // the first set that begins after t0, in [0, n_sets]
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (offsets[mid] <= t0) lo = mid + 1; else hi = mid;
        }
        first = lo > 0 ? lo - 1 : 0;
    }
    unsigned long long bad = 0;
    for (int64_t tile = first; tile < n_sets; tile += 256) {
        const int64_t s = tile + tid;
        bool is_long = false, past = false;
        if (s < n_sets) {
            const int64_t b = offsets ? offsets[s] : s * fixed_len, e = offsets ? offsets[s + 1] : b + fixed_len;
            past = b >= t1;
            is_long = !past && e - b > split && e > t0;
        }
        // which of the tile's 256 sets are long: one ballot per wave, handed round through the first words of the LDS
        const unsigned long long mine = __ballot(is_long);
        if ((tid & 63) == 0) {
            hll_lds[2 * (tid >> 6)] = (uint32_t)mine;
            hll_lds[2 * (tid >> 6) + 1] = (uint32_t)(mine >> 32);
        }
        const int any_past = __syncthreads_or(past);
        unsigned long long longs[4];
#pragma unroll
        for (int w = 0; w < 4; ++w) longs[w] = (unsigned long long)hll_lds[2 * w] | ((unsigned long long)hll_lds[2 * w + 1] << 32);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned long long bits = longs[w];
            while (bits) {
                const int j = __ffsll((long long)bits) - 1;
                bits &= bits - 1;
                const int64_t set = tile + 64 * w + j;
                const int64_t b = offsets ? offsets[set] : set * fixed_len, e = offsets ? offsets[set + 1] : b + fixed_len;
                const int64_t lo = b > t0 ? b : t0, hi = e < t1 ? e : t1;
                for (int x = tid; x < words; x += 256) hll_lds[x] = 0;
                __syncthreads();
#pragma unroll 4
                for (int64_t t = lo + tid; t < hi; t += 256) {
                    uint32_t idx, rank;
                    if (hll_slot(hv[t], p, hash_bits, mask, idx, rank))
                        lds_update<LAYOUT>(hll_lds, idx, rank);
                    else
                        ++bad;
                }
                __syncthreads();
                uint32_t *dst = reinterpret_cast<uint32_t *>(out + set * (int64_t)m);
                for (int q = tid; q < m / 4; q += 256) {
                    const uint32_t v = lds_packed<LAYOUT>(hll_lds, q);
                    if (v) global_byte_max4(dst + q, v);
                }
                __syncthreads();
            }
        }
        if (any_past) break;
    }
    if (bad) atomicAdd(overflow, bad);
}

// hist[i, v] = number of registers of row i equal to v (v < 64); larger values are counted into *invalid.  One wave per row.
__global__ __launch_bounds__(256) void hll_histogram_kernel(const uint8_t *__restrict__ reg, int64_t n, int m, uint32_t *__restrict__ hist,
                                                            unsigned long long *invalid) {
    __shared__ uint32_t h[4][64];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    unsigned long long bad = 0;
    for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
        const int64_t row = base + wave;
        h[wave][lane] = 0;
        __syncthreads();
        if (row < n) {
            const uint32_t *r = reinterpret_cast<const uint32_t *>(reg + row * (int64_t)m);
#pragma unroll 4
            for (int w = lane; w < m / 4; w += 64) {
                const uint32_t x = r[w];
#pragma unroll
                for (int k = 0; k < 32; k += 8) {
                    const uint32_t v = (x >> k) & 0xFFu;
                    if (v < 64)
                        atomicAdd(&h[wave][v], 1u);
                    else
                        ++bad;
                }
            }
        }
        __syncthreads();
        if (row < n) hist[row * 64 + lane] = h[wave][lane];
        __syncthreads();
    }
    if (bad) atomicAdd(invalid, bad);
}

// a[i] = max(a[i], b[i]) over count bytes: 16 bytes per lane where both pointers allow it, the rest byte by byte
__global__ __launch_bounds__(256) void hll_merge_kernel(uint8_t *__restrict__ a, const uint8_t *__restrict__ b, int64_t count, int wide) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, me = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t n16 = wide ? count >> 4 : 0;
    uint4 *a4 = reinterpret_cast<uint4 *>(a);
    const uint4 *b4 = reinterpret_cast<const uint4 *>(b);
    for (int64_t i = me; i < n16; i += stride) {
        uint4 x = a4[i];
        const uint4 y = b4[i];
        x.x = byte_max4(x.x, y.x);
        x.y = byte_max4(x.y, y.y);
        x.z = byte_max4(x.z, y.z);
        x.w = byte_max4(x.w, y.w);
        a4[i] = x;
    }
    for (int64_t i = (n16 << 4) + me; i < count; i += stride) a[i] = a[i] > b[i] ? a[i] : b[i];
}

// out[g, :] = max over the rows offsets[g] .. offsets[g + 1] of reg; one thread per four registers of one group
__global__ __launch_bounds__(256) void hll_union_kernel(const uint8_t *__restrict__ reg, int m, const int64_t *__restrict__ offsets,
                                                        int64_t n_groups, uint8_t *__restrict__ out) {
    const int quads = m / 4;
    const int64_t items = n_groups * quads, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t item = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; item < items; item += stride) {
        const int64_t g = item / quads;
        const int q = (int)(item - g * quads);
        uint32_t acc = 0;
        for (int64_t row = offsets[g]; row < offsets[g + 1]; ++row)
            acc = byte_max4(acc, reinterpret_cast<const uint32_t *>(reg + row * (int64_t)m)[q]);
        reinterpret_cast<uint32_t *>(out + g * (int64_t)m)[q] = acc;
    }
}

template <int LAYOUT, class T>
int launch_bulk_layout(mhx_ctx *ctx, const T *d_hv, const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets, int64_t total, int p,
                       int hash_bits, int64_t split, const uint8_t *d_init, int64_t init_stride, uint8_t *d_out,
                       unsigned long long *d_overflow) {
    const int64_t m = (int64_t)1 << p;
    const int per_block = LAYOUT == kLayoutWave ? 4 : 1;
    const size_t lds = (size_t)per_block * (LAYOUT == kLayoutBytes ? m : 4 * m);
    if (lds > (size_t)ctx->lds_per_block) return fail(MHX_ERR_UNSUPPORTED, "%zu bytes of LDS per workgroup are not available", lds);
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n_sets + per_block - 1) / per_block, (int64_t)ctx->num_cus * 32));
    hipLaunchKernelGGL((hll_bulk_kernel<LAYOUT, T>), dim3((unsigned)blocks), dim3(256), lds, ctx->stream, d_hv, d_offsets, fixed_len, n_sets,
                       p, hash_bits, split, d_init, init_stride, d_out, d_overflow);
    MHX_HIP_CHECK(hipGetLastError());
    // a set can only be longer than the threshold when the whole array is (fixed length: every set is, or none)
    const bool may_split = d_offsets ? total > split : fixed_len > split;
    if (!may_split) return MHX_OK;
    const int64_t chunk = std::max<int64_t>(split, (total + (int64_t)ctx->num_cus * 8 - 1) / ((int64_t)ctx->num_cus * 8));
    const int64_t parts = (total + chunk - 1) / chunk;
    if (parts >= ((int64_t)1 << 31)) return fail(MHX_ERR_INVALID, "hll.split_tokens %lld cuts %lld tokens into too many parts", (long long)split, (long long)total);
    constexpr int kSplitLayout = LAYOUT == kLayoutBytes ? kLayoutBytes : kLayoutWords;
    const size_t lds2 = std::max<size_t>(64, (size_t)(kSplitLayout == kLayoutBytes ? m : 4 * m));
    hipLaunchKernelGGL((hll_split_kernel<kSplitLayout, T>), dim3((unsigned)parts), dim3(256), lds2, ctx->stream, d_hv, d_offsets, fixed_len,
                       n_sets, total, chunk, p, hash_bits, split, d_out, d_overflow);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

template <class T>
int launch_bulk_typed(mhx_ctx *ctx, const T *d_hv, const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets, int64_t total, int p,
                      int hash_bits, int64_t split, const uint8_t *d_init, int64_t init_stride, uint8_t *d_out,
                      unsigned long long *d_overflow) {
    switch (hll_layout(p)) {
    case kLayoutWave:
        return launch_bulk_layout<kLayoutWave, T>(ctx, d_hv, d_offsets, fixed_len, n_sets, total, p, hash_bits, split, d_init, init_stride, d_out, d_overflow);
    case kLayoutWords:
        return launch_bulk_layout<kLayoutWords, T>(ctx, d_hv, d_offsets, fixed_len, n_sets, total, p, hash_bits, split, d_init, init_stride, d_out, d_overflow);
    default:
        return launch_bulk_layout<kLayoutBytes, T>(ctx, d_hv, d_offsets, fixed_len, n_sets, total, p, hash_bits, split, d_init, init_stride, d_out, d_overflow);
    }
}

}  // namespace

int hll_layout(int p) { return p <= kWaveMaxP ? kLayoutWave : p <= kWordMaxP ? kLayoutWords : kLayoutBytes; }

int launch_hll_bulk(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets,
                    int64_t total_tokens, int p, int hash_bits, const uint8_t *d_init, int64_t init_stride, uint8_t *d_out,
                    int64_t *d_overflow) {
    if (n_sets == 0) return MHX_OK;
    const int64_t split = ctx->opt_hll_split_tokens > 0 ? ctx->opt_hll_split_tokens : kHllSplitTokens;
    unsigned long long *ovf = reinterpret_cast<unsigned long long *>(d_overflow);
    if (hv_dtype == MHX_U32)
        return launch_bulk_typed(ctx, static_cast<const uint32_t *>(d_hv), d_offsets, fixed_len, n_sets, total_tokens, p, hash_bits, split, d_init,
                                 init_stride, d_out, ovf);
    return launch_bulk_typed(ctx, static_cast<const uint64_t *>(d_hv), d_offsets, fixed_len, n_sets, total_tokens, p, hash_bits, split, d_init,
                             init_stride, d_out, ovf);
}

int launch_hll_histogram(mhx_ctx *ctx, const uint8_t *d_reg, int64_t n, int p, uint32_t *d_hist, int64_t *d_invalid) {
    if (n == 0) return MHX_OK;
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((n + 3) / 4, (int64_t)ctx->num_cus * 32));
    hipLaunchKernelGGL(hll_histogram_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, d_reg, n, 1 << p, d_hist,
                       reinterpret_cast<unsigned long long *>(d_invalid));
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_hll_merge(mhx_ctx *ctx, uint8_t *d_a, const uint8_t *d_b, int64_t count) {
    if (count == 0) return MHX_OK;
    const int wide = (((uintptr_t)d_a | (uintptr_t)d_b) & 15) == 0;
    hipLaunchKernelGGL(hll_merge_kernel, dim3(grid_for(ctx, (count + 15) / 16, 32)), dim3(256), 0, ctx->stream, d_a, d_b, count, wide);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_hll_union_groups(mhx_ctx *ctx, const uint8_t *d_reg, int p, const int64_t *d_group_offsets, int64_t n_groups, uint8_t *d_out) {
    if (n_groups == 0) return MHX_OK;
    const int64_t items = n_groups * ((int64_t)1 << p) / 4;
    hipLaunchKernelGGL(hll_union_kernel, dim3(grid_for(ctx, items, 32)), dim3(256), 0, ctx->stream, d_reg, 1 << p, d_group_offsets, n_groups,
                       d_out);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
