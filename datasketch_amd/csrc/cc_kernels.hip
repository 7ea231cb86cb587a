// cc_kernels.hip -- connected components of a row graph: near-duplicate clusters (mhx_cc_*; no counterpart in the reference).
//
// One array uint32 labels[n] is the parent forest of a lock-free union-find while links are added and the answer afterwards.
// Four launches: init (labels[i] = i), any number of link launches -- over listed pairs, or over the runs of equal digests of
// sorted bands, where linking every row to its predecessor in the run gives the components of the run's L (L - 1) / 2 pairs
// with L - 1 edges -- and finish (labels[i] = root of i).
//
// Invariants.
//   * Roots hook larger under smaller.  unite(u, v) walks both rows to their roots and does atomicCAS(&labels[hi], hi, lo) with
//     lo < hi; when the swap fails it goes on from the value the swap returned (hi's new parent) and lo.  So labels[i] <= i
//     always holds, a word only ever goes down, a row that has stopped being a root never becomes one again, and the root of a
//     tree is its smallest row.  After finish labels[i] is the smallest row number of i's component: one answer whatever the
//     order in which workgroups, launches and lanes ran.
//   * Writes during a link launch.  Every write to labels is an agent-scope atomic: the hooking swap, and the atomicMin that
//     points a row at its grandparent while a walk passes (path halving: the new value is an ancestor and smaller).  Every read
//     of a walk is a relaxed agent-scope atomic load.  A plain store would sit in one XCD's L2 where an atomic from another XCD
//     does not see it, and a plain load may be served from a line the CU's L1 has held since before another CU wrote it.  An old
//     value is harmless here -- it is still an ancestor, and the swap on a former root fails and returns the current parent --
//     a write that an atomic of another XCD does not see is not.  init and finish are launches of their own: between launches
//     on one stream everything is visible, so they use plain loads and stores.  (Inside finish a lane may read a word another
//     lane is replacing by its root: old and new value are both ancestors of the row, and a root's word is rewritten with itself.)
//   * No lane waits for another lane.  A walk strictly descends (labels[x] < x for every row that is no root), so it ends after
//     at most x steps.  A failed swap means the word of hi went down, and the next attempt starts below hi: one unite(u, v)
//     makes at most max(u, v) + 1 swaps and fewer than (max(u, v) + 1)^2 loads whatever the other lanes do (far fewer with the
//     halving).  There is no spin on a flag and no barrier between workgroups.
//   * An edge with an endpoint outside [0, n) is not followed; a thread that met any adds their number to *invalid once (as the
//     HyperLogLog kernels count overflowing hashes); invalid may be nullptr, the edges are skipped all the same.
#include "mhx_internal.h"

namespace mhx {
namespace {

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x; rows passed on the way are pointed at their grandparents
__device__ __forceinline__ uint32_t cc_find(uint32_t *labels, uint32_t x) {
    for (;;) {
        const uint32_t p = cc_load(labels + x);
        if (p == x) return x;
        const uint32_t g = cc_load(labels + p);
        if (g == p) return p;
        atomicMin(labels + x, g);
        x = g;
    }
}

__device__ __forceinline__ void cc_unite(uint32_t *labels, uint32_t u, uint32_t v) {
    for (;;) {
        u = cc_find(labels, u);
        v = cc_find(labels, v);
        if (u == v) return;
        const uint32_t lo = u < v ? u : v, hi = u < v ? v : u;
        const uint32_t seen = atomicCAS(labels + hi, hi, lo);
        if (seen == hi) return;
        u = seen;  // hi has been hooked under `seen` < hi meanwhile
        v = lo;
    }
}

__global__ __launch_bounds__(256) void cc_init_kernel(uint32_t *__restrict__ labels, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) labels[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void cc_link_pairs_kernel(uint32_t *labels, int64_t n, const int64_t *__restrict__ pairs, int64_t n_pairs,
                                                            const int32_t *__restrict__ counts, int32_t min_count,
                                                            unsigned long long *invalid) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) {
        if (counts && counts[p] < min_count) continue;
        const int64_t u = pairs[2 * p], v = pairs[2 * p + 1];
        if (u < 0 || u >= n || v < 0 || v >= n) {
            ++bad;
            continue;
        }
        if (u != v) cc_unite(labels, (uint32_t)u, (uint32_t)v);
    }
    if (bad && invalid) atomicAdd(invalid, bad);
}

// position p > 0 of band j: rows[j][p - 1] and rows[j][p] are linked when their digests are equal
__global__ __launch_bounds__(256) void cc_link_bands_kernel(uint32_t *labels, int64_t n, const uint64_t *__restrict__ digests,
                                                            const uint32_t *__restrict__ rows, int64_t n_sigs, int64_t total,
                                                            unsigned long long *invalid) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long bad = 0;
    // pos = at % n_sigs, carried along: one 64-bit division per thread, not one per position
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = stride % n_sigs;
    int64_t pos = first % n_sigs;
    for (int64_t at = first; at < total; at += stride, pos += step, pos -= pos >= n_sigs ? n_sigs : 0) {
        if (pos == 0 || digests[at] != digests[at - 1]) continue;  // (the first position of a band has no predecessor in it)
        const uint32_t u = rows[at - 1], v = rows[at];
        if ((int64_t)u >= n || (int64_t)v >= n) {
            ++bad;
            continue;
        }
        if (u != v) cc_unite(labels, u, v);
    }
    if (bad && invalid) atomicAdd(invalid, bad);
}

__global__ __launch_bounds__(256) void cc_finish_kernel(uint32_t *labels, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint32_t x = (uint32_t)i, p = labels[x];
        while (p != x) {
            x = p;
            p = labels[x];
        }
        labels[i] = x;
    }
}

}  // namespace

int launch_cc_init(mhx_ctx *ctx, uint32_t *d_labels, int64_t n) {
    if (n == 0) return MHX_OK;
    hipLaunchKernelGGL(cc_init_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, d_labels, n);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_cc_link_pairs(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const int64_t *d_pairs, int64_t n_pairs, const int32_t *d_counts,
                         int32_t min_count, int64_t *d_invalid) {
    if (n_pairs == 0) return MHX_OK;
    hipLaunchKernelGGL(cc_link_pairs_kernel, dim3(grid_for(ctx, n_pairs)), dim3(256), 0, ctx->stream, d_labels, n, d_pairs, n_pairs,
                       d_counts, min_count, reinterpret_cast<unsigned long long *>(d_invalid));
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_cc_link_bands(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows,
                         int64_t n_sigs, int32_t bands, int64_t *d_invalid) {
    const int64_t total = n_sigs * bands;
    if (total == 0) return MHX_OK;
    hipLaunchKernelGGL(cc_link_bands_kernel, dim3(grid_for(ctx, total)), dim3(256), 0, ctx->stream, d_labels, n, d_sorted_digests,
                       d_sorted_rows, n_sigs, total, reinterpret_cast<unsigned long long *>(d_invalid));
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_cc_finish(mhx_ctx *ctx, uint32_t *d_labels, int64_t n) {
    if (n == 0) return MHX_OK;
    hipLaunchKernelGGL(cc_finish_kernel, dim3(grid_for(ctx, n)), dim3(256), 0, ctx->stream, d_labels, n);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
