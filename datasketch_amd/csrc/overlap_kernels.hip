// overlap_kernels.hip -- exact overlap counts of listed pairs of hashed sets (mhx_overlap_*; no counterpart in the reference;
// datasketch_amd/overlap.py is the definition).
//
// Set i is hv[set_offsets[i] .. set_offsets[i + 1]), repeats allowed; pair p = (i, j) gets counts[p] = (|Si n Sj|, |Si|, |Sj|)
// over DISTINCT values.  One workgroup of 256 threads per pair builds an open-addressing hash set sized for that pair:
//
//   table   `slots` keys (uint32 or uint64) with linear probing, slots = the power of two >= max(64, 2 m) for the m items of the
//           two sets with repeats: at most half full, so it never fills; behind the keys two bit maps of one bit per slot,
//           in_a ("the key of this slot occurs in A") and hit ("... and B has found it").  Only the slots of this pair are cleared.
//   phase A every thread inserts items of Si: compare-and-swap on the slot from the empty value.  The swap that wins counts one
//           towards a and sets the slot's in_a bit; meeting the own key (before the swap or as its answer) counts nothing.
//   barrier
//   phase B items of Sj are looked up.  Found in a slot with in_a set: fetch-or on the hit bit, and the thread that sees the bit
//           clear counts one towards inter.  Not found: inserted by compare-and-swap, and the swap that wins counts one "B only".
//           Found in a B-only slot, or the swap lost to the same key: nothing.  b = inter + B only.
//   The empty value is all ones; it cannot be stored as a key, so two flags remember whether A and B hold it, and the end adds them.
//
// Every probe loop is bounded by the slot count: whatever the arrays hold, a pair is left after at most `slots` steps per item.
//
// Two classes.  LDS: pairs whose table fits a workgroup's LDS (header + keys + bit maps <= ctx->lds_per_block: m <= 8192 at 64-bit
// keys, 16384 at 32-bit on gfx950).  They are binned by table size -- up to three launches whose dynamic LDS is the bin's cap, so
// that a launch of small pairs keeps several workgroups per CU, and the pairs of the smallest bin (up to 1024 slots) get one wave
// each instead of a workgroup.  Both are kept by measurement; option "overlap.bins" = 1: one launch with the largest
// size, 2: bins with a workgroup per pair everywhere.  Global: larger pairs, the same algorithm on a table in scratch -- one table per workgroup of a capped grid,
// sized from the caller's bound on a set, cleared by its workgroup before each pair.  There every access to the table is an
// agent-scope atomic, so that nothing of it is ever held in the CU's L1: a plain load could be served from a line fetched before
// another wave's atomic changed it in L2.
//
// Routing is one classify launch on the device: it reads the pairs and the offsets, answers invalid pairs (-1, -1, -1) and empty
// ones (0, 0, 0) itself, and appends every other pair to the list of its class with one atomic per wave and class.  The pair
// kernels walk their list in a grid-stride loop over a grid sized from ctx->num_cus; the list lengths stay on the device.
#include "mhx_internal.h"

namespace mhx {
namespace {

constexpr int kThreads = 256;
constexpr int kHeaderBytes = 64;   // the pair's counters, in front of an LDS table
constexpr uint64_t kMinSlots = 64;  // (two words per bit map at least)
constexpr int kMaxBins = 3;
constexpr int kGlobalClass = kMaxBins, kClasses = kMaxBins + 1;
constexpr uint64_t kBinSlots[kMaxBins - 1] = {1024, 4096};  // caps of the small bins; the last bin takes the rest
constexpr size_t kTableBudget = (size_t)256 << 20;          // scratch for the global tables, unless one alone is larger

__host__ __device__ __forceinline__ uint64_t slots_for(uint64_t m) {
    uint64_t s = kMinSlots;
    while (s < 2 * m) s <<= 1;
    return s;
}
__host__ __device__ __forceinline__ uint64_t table_bytes(uint64_t slots, uint64_t key_bytes) { return slots * key_bytes + 2 * (slots / 8); }

template <class K>
struct Hash;
template <>
struct Hash<uint32_t> {
    static __device__ __forceinline__ uint64_t slot(uint32_t k, int lg) {
        const uint32_t h = (k ^ (k >> 15)) * 0x9E3779B1u;
        return lg <= 32 ? (uint64_t)(h >> (32 - lg)) : (uint64_t)h << (lg - 32);  // (a global table of many repeats may have more than 2^32 slots)
    }
};
template <>
struct Hash<unsigned long long> {
    static __device__ __forceinline__ uint64_t slot(unsigned long long k, int lg) { return ((k ^ (k >> 32)) * 0x9E3779B97F4A7C15ull) >> (64 - lg); }
};

// LDS: workgroup scope (plain DS operations); scratch: agent scope (see the head of the file)
template <int SCOPE, class T>
__device__ __forceinline__ T ld(T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE, class T>
__device__ __forceinline__ void st(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, SCOPE); }
template <int SCOPE, class T>
__device__ __forceinline__ T cas(T *p, T expected, T v) {
    __hip_atomic_compare_exchange_strong(p, &expected, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return expected;  // what the word held
}

struct Header {  // in LDS
    uint32_t a, inter, b_only, sentinel;  // sentinel: bit 0 = A holds the empty value, bit 1 = B does
};

// one pair on a table of `slots` = 1 << lg slots; every thread of the workgroup calls it.  hdr is zeroed here.
template <class K, int SCOPE, int THREADS>
__device__ __forceinline__ void overlap_pair(const K *__restrict__ hv, int64_t a0, int64_t a1, int64_t b0, int64_t b1, K *keys, uint64_t slots,
                                             int lg, Header *hdr, int32_t *__restrict__ out) {
    constexpr K kEmpty = ~(K)0;
    uint32_t *in_a = reinterpret_cast<uint32_t *>(keys + slots), *hit = in_a + slots / 32;
    const uint64_t mask = slots - 1;
    const int tid = threadIdx.x;
    for (uint64_t s = tid; s < slots; s += THREADS) st<SCOPE>(keys + s, kEmpty);
    for (uint64_t w = tid; w < slots / 16; w += THREADS) st<SCOPE>(in_a + w, 0u);  // both bit maps: they are adjacent
    if (tid == 0) *hdr = Header{0, 0, 0, 0};
    if (SCOPE == __HIP_MEMORY_SCOPE_AGENT) __threadfence();
    __syncthreads();

    uint32_t n_a = 0, flags = 0;
    for (int64_t t = a0 + tid; t < a1; t += THREADS) {
        const K k = hv[t];
        if (k == kEmpty) {
            flags |= 1;
            continue;
        }
        uint64_t s = Hash<K>::slot(k, lg);
        for (uint64_t probe = 0; probe < slots; ++probe, s = (s + 1) & mask) {
            K cur = ld<SCOPE>(keys + s);
            if (cur == kEmpty) {
                cur = cas<SCOPE>(keys + s, kEmpty, k);
                if (cur == kEmpty) {
                    ++n_a;
                    __hip_atomic_fetch_or(in_a + (s >> 5), 1u << (s & 31), __ATOMIC_RELAXED, SCOPE);
                    break;
                }
            }
            if (cur == k) break;
        }
    }
    if (n_a) atomicAdd(&hdr->a, n_a);
    if (SCOPE == __HIP_MEMORY_SCOPE_AGENT) __threadfence();
    __syncthreads();

    uint32_t n_inter = 0, n_b = 0;
    for (int64_t t = b0 + tid; t < b1; t += THREADS) {
        const K k = hv[t];
        if (k == kEmpty) {
            flags |= 2;
            continue;
        }
        uint64_t s = Hash<K>::slot(k, lg);
        for (uint64_t probe = 0; probe < slots; ++probe, s = (s + 1) & mask) {
            K cur = ld<SCOPE>(keys + s);
            if (cur == kEmpty) {
                cur = cas<SCOPE>(keys + s, kEmpty, k);
                if (cur == kEmpty) {
                    ++n_b;
                    break;
                }
            }
            if (cur == k) {
                const uint32_t bit = 1u << (s & 31);
                // in_a is complete since the barrier; a slot B filled has its bit clear
                if ((ld<SCOPE>(in_a + (s >> 5)) & bit) && !(__hip_atomic_fetch_or(hit + (s >> 5), bit, __ATOMIC_RELAXED, SCOPE) & bit)) ++n_inter;
                break;
            }
        }
    }
    if (n_inter) atomicAdd(&hdr->inter, n_inter);
    if (n_b) atomicAdd(&hdr->b_only, n_b);
    if (flags) atomicOr(&hdr->sentinel, flags);
    __syncthreads();
    if (tid == 0) {
        const uint32_t in_both = hdr->sentinel == 3 ? 1 : 0;
        out[0] = (int32_t)(hdr->inter + in_both);
        out[1] = (int32_t)(hdr->a + (hdr->sentinel & 1));
        out[2] = (int32_t)(hdr->inter + hdr->b_only + (hdr->sentinel >> 1));
    }
    __syncthreads();  // the header and the table are the next pair's
}

__device__ __forceinline__ int log2_of(uint64_t pow2) { return 63 - __clzll((long long)pow2); }

// the pairs of one LDS bin: list[0 .. *n_list) names them.  THREADS = 256: a workgroup per pair; 64: one wave per pair
template <class K, int THREADS>
__global__ __launch_bounds__(THREADS) void overlap_lds_kernel(const K *__restrict__ hv, const int64_t *__restrict__ set_offsets,
                                                               const int64_t *__restrict__ pairs, const uint32_t *__restrict__ list,
                                                               const uint32_t *__restrict__ n_list, int32_t *__restrict__ counts) {
    extern __shared__ __align__(16) unsigned char lds[];
    Header *hdr = reinterpret_cast<Header *>(lds);
    K *keys = reinterpret_cast<K *>(lds + kHeaderBytes);
    const uint32_t n = *n_list;
    for (uint32_t at = blockIdx.x; at < n; at += gridDim.x) {
        const int64_t p = list[at], i = pairs[2 * p], j = pairs[2 * p + 1];
        const int64_t a0 = set_offsets[i], a1 = set_offsets[i + 1], b0 = set_offsets[j], b1 = set_offsets[j + 1];
        const uint64_t slots = slots_for((uint64_t)((a1 - a0) + (b1 - b0)));  // (the classify pass put the pair here: it fits)
        overlap_pair<K, __HIP_MEMORY_SCOPE_WORKGROUP, THREADS>(hv, a0, a1, b0, b1, keys, slots, log2_of(slots), hdr, counts + 3 * p);
    }
}

// the pairs above the LDS limit: workgroup b owns the table at tables + b * table_stride bytes
template <class K>
__global__ __launch_bounds__(kThreads) void overlap_global_kernel(const K *__restrict__ hv, const int64_t *__restrict__ set_offsets,
                                                                  const int64_t *__restrict__ pairs, const uint32_t *__restrict__ list,
                                                                  const uint32_t *__restrict__ n_list, unsigned char *tables,
                                                                  uint64_t table_stride, int32_t *__restrict__ counts) {
    __shared__ Header hdr;
    K *keys = reinterpret_cast<K *>(tables + (uint64_t)blockIdx.x * table_stride);
    const uint32_t n = *n_list;
    for (uint32_t at = blockIdx.x; at < n; at += gridDim.x) {
        const int64_t p = list[at], i = pairs[2 * p], j = pairs[2 * p + 1];
        const int64_t a0 = set_offsets[i], a1 = set_offsets[i + 1], b0 = set_offsets[j], b1 = set_offsets[j + 1];
        const uint64_t slots = slots_for((uint64_t)((a1 - a0) + (b1 - b0)));  // <= the stride's: neither set exceeds max_set_items
        overlap_pair<K, __HIP_MEMORY_SCOPE_AGENT, kThreads>(hv, a0, a1, b0, b1, keys, slots, log2_of(slots), &hdr, counts + 3 * p);
    }
}

struct Bins {
    int n;                      // LDS bins in use (0: every pair with an item is global)
    uint64_t slots[kMaxBins];   // the largest table of each, ascending
    int64_t lds_max_items;      // more items than this: the global class
};

// lists: uint32 [kClasses][list_stride], list_stride >= n_pairs; n_lists: uint32 [kClasses], zeroed
__global__ __launch_bounds__(kThreads) void overlap_classify_kernel(const int64_t *__restrict__ set_offsets, int64_t n_sets, int64_t max_set_items,
                                                                    const int64_t *__restrict__ pairs, int64_t n_pairs, Bins bins,
                                                                    uint32_t *__restrict__ lists, int64_t list_stride, uint32_t *n_lists,
                                                                    int32_t *__restrict__ counts, unsigned long long *invalid) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    const int lane = threadIdx.x & 63;
    unsigned long long bad = 0;
    for (int64_t base = (int64_t)blockIdx.x * kThreads; base < n_pairs; base += stride) {  // (whole waves stay in: the ballots below)
        const int64_t p = base + threadIdx.x;
        int cls = -1;
        if (p < n_pairs) {
            const int64_t i = pairs[2 * p], j = pairs[2 * p + 1];
            int64_t a = -1, b = -1;
            if (i >= 0 && i < n_sets && j >= 0 && j < n_sets) {
                a = set_offsets[i + 1] - set_offsets[i];
                b = set_offsets[j + 1] - set_offsets[j];
            }
            if (a < 0 || b < 0 || a > max_set_items || b > max_set_items) {
                ++bad;
                counts[3 * p] = counts[3 * p + 1] = counts[3 * p + 2] = -1;
            } else if (a + b == 0) {
                counts[3 * p] = counts[3 * p + 1] = counts[3 * p + 2] = 0;
            } else if (a + b > bins.lds_max_items) {
                cls = kGlobalClass;
            } else {
                const uint64_t slots = slots_for((uint64_t)(a + b));
                cls = 0;
                while (cls < bins.n - 1 && slots > bins.slots[cls]) ++cls;
            }
        }
        for (int c = 0; c < kClasses; ++c) {
            const unsigned long long mask = __ballot(cls == c);
            if (!mask) continue;
            const int leader = __ffsll((long long)mask) - 1;
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(n_lists + c, (uint32_t)__popcll(mask));
            first = (uint32_t)__shfl((int)first, leader);
            if (cls == c) lists[(int64_t)c * list_stride + first + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = (uint32_t)p;
        }
    }
    if (bad && invalid) atomicAdd(invalid, bad);
}

template <class K>
int launch_typed(mhx_ctx *ctx, const K *d_hv, const int64_t *d_set_offsets, int64_t n_sets, int64_t max_set_items, const int64_t *d_pairs,
                 int64_t n_pairs, int32_t *d_counts, int64_t *d_invalid) {
    const int hv_dtype = sizeof(K) == 4 ? MHX_U32 : MHX_U64;
    Bins bins{};
    bins.lds_max_items = overlap_lds_max_items(hv_dtype, ctx->lds_per_block);
    const int64_t m_bound = 2 * max_set_items;  // what a pair of this call can hold
    if (bins.lds_max_items > 0 && m_bound > 0) {
        const uint64_t top = slots_for((uint64_t)std::min(m_bound, bins.lds_max_items));
        if (ctx->opt_overlap_bins != 1)
            for (int b = 0; b < kMaxBins - 1; ++b)
                if (kBinSlots[b] < top) bins.slots[bins.n++] = kBinSlots[b];
        bins.slots[bins.n++] = top;
    }
    const bool global = m_bound > bins.lds_max_items;
    // scratch[4]: list lengths | lists | the global tables
    const size_t list_bytes = pad256(sizeof(uint32_t) * (size_t)n_pairs), list_stride = list_bytes / sizeof(uint32_t);
    uint64_t table_stride = 0;
    int64_t n_tables = 0;
    if (global) {
        table_stride = pad256(table_bytes(slots_for((uint64_t)m_bound), sizeof(K)));
        n_tables = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(n_pairs, (int64_t)ctx->num_cus * 2), (int64_t)(kTableBudget / table_stride)));
    }
    if (int rc = ctx->ensure_scratch(4, 256 + kClasses * list_bytes + (size_t)n_tables * table_stride)) return rc;
    uint32_t *n_lists = static_cast<uint32_t *>(ctx->scratch[4]);
    uint32_t *lists = reinterpret_cast<uint32_t *>(static_cast<char *>(ctx->scratch[4]) + 256);
    unsigned char *tables = reinterpret_cast<unsigned char *>(lists) + kClasses * list_bytes;
    MHX_HIP_CHECK(hipMemsetAsync(n_lists, 0, 256, ctx->stream));
    hipLaunchKernelGGL(overlap_classify_kernel, dim3(grid_for(ctx, n_pairs, 4)), dim3(kThreads), 0, ctx->stream, d_set_offsets, n_sets, max_set_items,
                       d_pairs, n_pairs, bins, lists, (int64_t)list_stride, n_lists, d_counts, reinterpret_cast<unsigned long long *>(d_invalid));
    MHX_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < bins.n; ++b) {
        const size_t lds = kHeaderBytes + (size_t)table_bytes(bins.slots[b], sizeof(K));
        // the smallest bin: one wave per pair (measured faster than a workgroup at up to 512 items; "overlap.bins" = 2: A/B)
        const bool wave = ctx->opt_overlap_bins == 0 && bins.slots[b] <= kBinSlots[0];
        // as many workgroups per CU as its LDS holds of this bin's tables, and 2048 threads at the most
        const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(wave ? 32 : 8, ctx->lds_per_block / (int64_t)lds));
        const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(n_pairs, (int64_t)ctx->num_cus * per_cu));
        const uint32_t *list = lists + (size_t)b * list_stride;
        if (wave) {
            MHX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&overlap_lds_kernel<K, 64>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((overlap_lds_kernel<K, 64>), dim3(grid), dim3(64), lds, ctx->stream, d_hv, d_set_offsets, d_pairs, list, n_lists + b, d_counts);
        } else {
            MHX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&overlap_lds_kernel<K, kThreads>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((overlap_lds_kernel<K, kThreads>), dim3(grid), dim3(kThreads), lds, ctx->stream, d_hv, d_set_offsets, d_pairs, list, n_lists + b, d_counts);
        }
        MHX_HIP_CHECK(hipGetLastError());
    }
    if (global) {
        hipLaunchKernelGGL(overlap_global_kernel<K>, dim3((unsigned)n_tables), dim3(kThreads), 0, ctx->stream, d_hv, d_set_offsets, d_pairs,
                           lists + (size_t)kGlobalClass * list_stride, n_lists + kGlobalClass, tables, table_stride, d_counts);
        MHX_HIP_CHECK(hipGetLastError());
    }
    return MHX_OK;
}

}  // namespace

int64_t overlap_lds_max_items(int hv_dtype, int64_t lds_per_block) {
    const uint64_t key_bytes = hv_dtype == MHX_U32 ? 4 : 8;
    uint64_t slots = 0;
    for (uint64_t s = kMinSlots; s <= ((uint64_t)1 << 31) && (int64_t)(kHeaderBytes + table_bytes(s, key_bytes)) <= lds_per_block; s <<= 1) slots = s;
    return (int64_t)(slots / 2);
}

int launch_overlap_pairs(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_set_offsets, int64_t n_sets, int64_t max_set_items,
                         const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts, int64_t *d_invalid) {
    if (n_pairs == 0 || n_sets == 0) return MHX_OK;
    if (hv_dtype == MHX_U32)
        return launch_typed(ctx, static_cast<const uint32_t *>(d_hv), d_set_offsets, n_sets, max_set_items, d_pairs, n_pairs, d_counts, d_invalid);
    return launch_typed(ctx, static_cast<const unsigned long long *>(d_hv), d_set_offsets, n_sets, max_set_items, d_pairs, n_pairs, d_counts, d_invalid);
}

}  // namespace mhx
