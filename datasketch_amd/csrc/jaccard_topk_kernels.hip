// jaccard_topk_kernels.hip -- exact top-k neighbours by agreeing positions (mhx_jaccard_topk*, mhx_bbit_jaccard_topk*): for
// every row i of A the k rows j of B with the most agreeing positions, without the n_a x n_b matrix.
//
// Order: a candidate is the packed key (count << 32) | (0xFFFFFFFF - j); a larger key is a better candidate, so the best k
// are (count descending, row ascending), a strict total order -- the answer does not depend on how B is cut.  Rows are
// numbered below 2^32 - 1, so a key is never 0: 0 is the empty entry of a list.  min_count is a floor key (min_count << 32),
// below which nothing is admitted.
//
// Strip kernel: a workgroup owns one 128-row tile of A and walks a contiguous segment of B's 128-row tiles, counting each
// tile with the matrix kernel's staging and 8 x 8 register loop (jaccard_tile_count.inc).  The 128 rows keep their k best keys
// sorted in LDS ([128][k], dynamic); a row's last entry is its admission bar.  After a tile a thread tests its 64 keys
// against the 8 bars of its rows: one barrier when nothing passes.  Otherwise the passing keys go to an LDS queue and the
// four waves drain it, a wave holding the list of the entry's row one key per lane: the insert position is
// popcount(ballot(mine > key)), the lanes behind it shift by one __shfl_up.  A tile that admits more than the queue holds
// (the first of a strip admits all 16 384) is drained in 8 rounds, one sub-tile row each (at most 2048 keys).
//
// Stream kernel (dense rows, few probes): the probes sit in LDS (in registers when a lane reads one 16-byte piece per row),
// a group of L lanes reads a row of B with 16-byte loads and compares it with up to 8 probes, __shfl_xor sums the group, and
// every wave keeps its own lists in registers, one key per lane -- no barrier, no queue.
//
// Either kernel writes one sorted partial list per (row of A, segment) to scratch; the merge kernel folds the S partial
// lists of a row (and, for the host forms' B blocks, the list so far) into the final one and unpacks it.
#include "jaccard_tile.h"

namespace mhx {
namespace {

using namespace jtile;

constexpr int kQueue = 2048;       // keys the strip kernel's queue holds: one sub-tile row of every thread (256 x 8)
constexpr int kStreamProbes = 8;   // probes per stream launch
constexpr int kAhead = 4;          // rows of B a lane group of the stream kernel has in flight

__device__ __forceinline__ uint64_t pack_key(int32_t count, int64_t j) {
    return ((uint64_t)(uint32_t)count << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)j);
}

// `key` into the descending list a wave holds one entry per lane (lanes >= topk hold nothing); returns the lane's entry
__device__ __forceinline__ uint64_t list_insert(uint64_t mine, uint64_t key, int lane, int topk) {
    const int pos = __popcll(__ballot(lane < topk && mine > key));
    const uint64_t up = (uint64_t)__shfl_up((long long)mine, 1);
    if (pos < topk && lane >= pos) mine = lane == pos ? key : up;
    return mine;
}

__device__ __forceinline__ bool row_live(const uint32_t *__restrict__ live, int64_t j) {
    return live == nullptr || ((live[j >> 5] >> (j & 31)) & 1u) != 0;
}

struct TopkArgs {
    const uint32_t *live;   // live rows of B, or nullptr
    uint64_t floor_key;     // keys must exceed it (min_count)
    int32_t topk;
    int32_t self;           // B is A: j == i is no candidate
    int64_t seg_tiles;      // strip: tiles of B per segment
    int64_t segments;
    uint64_t *partial;      // [segments][n_a][topk]
};

// dynamic LDS: uint64 lists[128][topk]
template <int SLOT, bool WIDE>
__global__ __launch_bounds__(kThreads, 2) void jaccard_topk_strip_kernel(const uint32_t *__restrict__ a, int64_t n_a,
                                                                         const uint32_t *__restrict__ b, int64_t n_b, int32_t W,
                                                                         int32_t num_perm, TopkArgs tk) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lists[];
    __shared__ __attribute__((aligned(16))) uint32_t As[kChunk][kLdsRow];
    __shared__ __attribute__((aligned(16))) uint32_t Bs[kChunk][kLdsRow];
    __shared__ __attribute__((aligned(16))) uint32_t Ah[WIDE ? kChunk : 1][WIDE ? kLdsRow : 4];
    __shared__ __attribute__((aligned(16))) uint32_t Bh[WIDE ? kChunk : 1][WIDE ? kLdsRow : 4];
    __shared__ uint64_t q_key[kQueue];
    __shared__ uint8_t q_row[kQueue];
    __shared__ unsigned int q_n, q_total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    const int topk = tk.topk;
    const int64_t ti = blockIdx.x / tk.segments, seg = blockIdx.x - ti * tk.segments;
    const int64_t i0 = ti * kTile;
    const int64_t tiles_n = (n_b + kTile - 1) / kTile;
    // words past the end of a row: never equal in the dense kinds (A 0, B 1), equal (no differing slot) in the b-bit kind
    const uint32_t pad_b = SLOT <= 0 ? 1u : 0u;
    const int chunks = (W + kChunk - 1) / kChunk;
    const int64_t t_begin = seg * tk.seg_tiles, t_end = min(tiles_n, t_begin + tk.seg_tiles);

    for (int e = tid; e < kTile * topk; e += kThreads) lists[e] = 0;
    // (the barriers of the first tile's counting loop order these stores before the first bar is read)

    for (int64_t tj = t_begin; tj < t_end; ++tj) {
        const int64_t j0 = tj * kTile;
#include "jaccard_tile_count.inc"

        // the 8 bars of the thread's rows (count, 0xFFFFFFFF - row: the halves of a key, compared as such so that no 64-bit
        // key is formed for the 64 tests), and which of its rows / columns are candidates at all
        uint32_t bar_hi[8], bar_lo[8], low[8];
        uint32_t row_ok = 0, col_ok = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint64_t last = lists[rowof(ty, r) * topk + topk - 1];
            const uint64_t bar = last > tk.floor_key ? last : tk.floor_key;
            bar_hi[r] = (uint32_t)(bar >> 32);
            bar_lo[r] = (uint32_t)bar;
            row_ok |= (i0 + rowof(ty, r) < n_a ? 1u : 0u) << r;
            const int64_t j = j0 + rowof(tx, r);
            low[r] = 0xFFFFFFFFu - (uint32_t)j;
            col_ok |= (j < n_b && row_live(tk.live, j) ? 1u : 0u) << r;
        }
        const bool diagonal = tk.self && i0 == j0 && ty == tx;  // element (r, r) of this thread is a row against itself
        auto count_of = [&](int r, int q) { return SLOT <= 0 ? acc[r][q] : (uint32_t)num_perm - acc[r][q]; };
        auto key_of = [&](int r, int q) { return ((uint64_t)count_of(r, q) << 32) | low[q]; };
        auto passes = [&](int r, int q) {
            const uint32_t c = count_of(r, q);
            return ((row_ok >> r) & (col_ok >> q) & 1u) != 0 && !(diagonal && r == q) &&
                   (c > bar_hi[r] || (c == bar_hi[r] && low[q] > bar_lo[r]));
        };
        // bit 8 r + q: element (r, q) passes.  (Two registers; the 64 predicates themselves would be kept as 64 lane masks.)
        uint32_t pass_lo = 0, pass_hi = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                pass_lo |= (passes(r, q) ? 1u : 0u) << (8 * r + q);
                pass_hi |= (passes(r + 4, q) ? 1u : 0u) << (8 * r + q);
            }
        if (!__syncthreads_or((pass_lo | pass_hi) != 0)) continue;  // the common case once the lists have filled

        if (tid == 0) q_total = 0;
        __syncthreads();
        if (pass_lo | pass_hi) atomicAdd(&q_total, (unsigned)(__popc(pass_lo) + __popc(pass_hi)));
        __syncthreads();
        const bool one_round = q_total <= (unsigned)kQueue;
        const int rounds = one_round ? 1 : 8;
        for (int round = 0; round < rounds; ++round) {
            if (tid == 0) q_n = 0;
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                if (!one_round && r != round) continue;
                const uint32_t bits = ((r < 4 ? pass_lo : pass_hi) >> (8 * (r & 3))) & 0xFFu;
                if (bits == 0) continue;
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if ((bits >> q) & 1u) {
                        const unsigned slot = atomicAdd(&q_n, 1u);  // < kQueue: at most 8 per thread in a round of one row
                        q_key[slot] = key_of(r, q);
                        q_row[slot] = (uint8_t)rowof(ty, r);
                    }
            }
            __syncthreads();
            const int n = (int)q_n;
            // wave w inserts the keys of the rows with (row >> 2) & 3 == w: a row's list has one owner, the order of the queue
            // does not matter (the list ends as the best k of what it held and what was queued)
            for (int e = 0; e < n; ++e) {
                const int row = q_row[e];
                if (((row >> 2) & 3) != wave) continue;
                uint64_t *list = lists + row * topk;
                const uint64_t mine = lane < topk ? list[lane] : 0;
                const uint64_t now = list_insert(mine, q_key[e], lane, topk);
                if (lane < topk) list[lane] = now;
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();
        }
    }

    __syncthreads();
    uint64_t *out = tk.partial + (seg * n_a + i0) * topk;
    const int64_t rows_here = min((int64_t)kTile, n_a - i0);
    for (int64_t e = tid; e < rows_here * topk; e += kThreads) out[e] = lists[e];
}

// One wave per segment of B's rows, up to kStreamProbes probes (rows q0 .. q0 + nq - 1 of A).  L lanes share a row of B
// (a power of two), a lane reads the 16-byte pieces l, l + L, ... of the row; VEC: rows are multiples of 16 bytes at 16-byte
// aligned addresses.  Dynamic LDS: the probes, nq rows of W elements.  QUAD: weighted rows, an element is one 16-byte (k, t) sample.
template <bool WIDE, bool QUAD = false>
__global__ __launch_bounds__(256) void jaccard_topk_stream_kernel(const uint32_t *__restrict__ a, int64_t n_a, int64_t q0, int nq,
                                                                  const uint32_t *__restrict__ b, int64_t n_b, int32_t W, int L,
                                                                  int vec, int64_t seg_rows, TopkArgs tk) {
    extern __shared__ __attribute__((aligned(16))) uint32_t probes[];
    constexpr int kPer = QUAD ? 1 : WIDE ? 2 : 4;       // elements per 16-byte piece
    constexpr int kWordsPer = QUAD ? 4 : WIDE ? 2 : 1;  // 32-bit words per element
    const int tid = threadIdx.x, lane = tid & 63;
    const int topk = tk.topk;
    const int pieces = (W + kPer - 1) / kPer;       // per row
    const int row_words = pieces * 4;               // a probe's stride in LDS, padded to whole pieces
    // probes into LDS; the padding never equals a row's (A 0, B 1)
    for (int e = tid; e < nq * row_words; e += 256) {
        const int q = e / row_words, w = e - q * row_words;
        probes[e] = w < W * kWordsPer ? a[(q0 + q) * (int64_t)W * kWordsPer + w] : 0u;
    }
    __syncthreads();

    const int64_t seg = (int64_t)blockIdx.x * 4 + (tid >> 6);
    if (seg >= tk.segments) return;  // (no barrier below)
    const int64_t r_begin = seg * seg_rows, r_end = min(n_b, r_begin + seg_rows);
    const int G = 64 / L, g = lane / L, l = lane - g * L;
    const bool single = pieces <= L;  // one piece per lane: the probes' pieces stay in registers
    uint32_t hx[kStreamProbes], hy[kStreamProbes], hz[kStreamProbes], hw[kStreamProbes];
#pragma unroll
    for (int q = 0; q < kStreamProbes; ++q) {
        const bool mine = single && q < nq && l < pieces;
        const uint32_t *src = &probes[mine ? q * row_words + l * 4 : 0];
        hx[q] = mine ? src[0] : 0u;
        hy[q] = mine ? src[1] : 0u;
        hz[q] = mine ? src[2] : 0u;
        hw[q] = mine ? src[3] : 0u;
    }

    uint64_t list[kStreamProbes], bar[kStreamProbes];
#pragma unroll
    for (int q = 0; q < kStreamProbes; ++q) {
        list[q] = 0;
        bar[q] = tk.floor_key;
    }

    auto equal_in = [](uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3, uint32_t y0, uint32_t y1, uint32_t y2, uint32_t y3) -> uint32_t {
        if (QUAD) return (uint32_t)(x0 == y0 && x1 == y1 && x2 == y2 && x3 == y3);
        if (WIDE) return (uint32_t)(x0 == y0 && x1 == y1) + (uint32_t)(x2 == y2 && x3 == y3);
        return (uint32_t)(x0 == y0) + (uint32_t)(x1 == y1) + (uint32_t)(x2 == y2) + (uint32_t)(x3 == y3);
    };

    // kAhead rows per lane group and trip: their loads are issued together, then compared.  The counts of two probes share a
    // register (16 bits each: a row has at most 2048 elements, what the probes' LDS allows), halving the shuffles
    for (int64_t r0 = r_begin; r0 < r_end; r0 += G * kAhead) {  // the same trip count for every lane of the wave
        uint32_t c2[kAhead][kStreamProbes / 2];
#pragma unroll
        for (int u = 0; u < kAhead; ++u)
#pragma unroll
            for (int h = 0; h < kStreamProbes / 2; ++h) c2[u][h] = 0;
        for (int p = l; p < pieces; p += L) {
            uint32_t y[kAhead][4];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int64_t j = r0 + u * G + g;
                y[u][0] = y[u][1] = y[u][2] = y[u][3] = 1u;
                if (j < r_end) {
                    const uint32_t *row = b + j * (int64_t)W * kWordsPer;
                    if (vec) {
                        const uint4 v = *reinterpret_cast<const uint4 *>(row + p * 4);
                        y[u][0] = v.x, y[u][1] = v.y, y[u][2] = v.z, y[u][3] = v.w;
                    } else {  // word by word; past the end of the row the padding of B
                        const int w0 = p * 4, words = W * kWordsPer;
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (w0 + c < words) y[u][c] = row[w0 + c];
                    }
                }
            }
#pragma unroll
            for (int q = 0; q < kStreamProbes; ++q) {
                if (q >= nq) continue;  // uniform
                uint32_t x0 = hx[q], x1 = hy[q], x2 = hz[q], x3 = hw[q];
                if (!single) {
                    const uint4 x = *reinterpret_cast<const uint4 *>(&probes[q * row_words + p * 4]);
                    x0 = x.x, x1 = x.y, x2 = x.z, x3 = x.w;
                }
#pragma unroll
                for (int u = 0; u < kAhead; ++u) c2[u][q >> 1] += equal_in(x0, x1, x2, x3, y[u][0], y[u][1], y[u][2], y[u][3]) << (16 * (q & 1));
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            const int64_t j = r0 + u * G + g;
            const bool have = j < r_end;
            const bool candidate = have && l == 0 && row_live(tk.live, have ? j : 0);
#pragma unroll
            for (int q = 0; q < kStreamProbes; ++q) {
                if (q >= nq) continue;  // uniform
                if ((q & 1) == 0)
                    for (int o = 1; o < L; o <<= 1) c2[u][q >> 1] += (uint32_t)__shfl_xor((int)c2[u][q >> 1], o);
                const uint32_t c = (c2[u][q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
                const uint64_t key = pack_key((int32_t)c, j);
                uint64_t pending = __ballot(candidate && !(tk.self && j == q0 + q) && key > bar[q]);
                while (pending) {  // at most G rows
                    const int src = __ffsll((unsigned long long)pending) - 1;
                    pending &= pending - 1;
                    const uint64_t k_src = (uint64_t)__shfl((long long)key, src);
                    list[q] = list_insert(list[q], k_src, lane, topk);
                    const uint64_t last = (uint64_t)__shfl((long long)list[q], topk - 1);
                    bar[q] = last > tk.floor_key ? last : tk.floor_key;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < kStreamProbes; ++q)
        if (q < nq && lane < topk) tk.partial[(seg * n_a + q0 + q) * topk + lane] = list[q];
}

// One workgroup per row of A: the best k of the row's list so far (`have`, or nullptr) and its `segments` partial lists, whose
// rows are numbered from row_offset.  keys_out (may be `have`) receives the packed list, rows / counts the unpacked one
// (either may be nullptr).  A wave takes 64 partial lists at a time, one per lane, entry by entry: lists are descending with
// their empty entries last, so a lane is done at its first key that does not enter; wave 0 then folds the four waves' lists.
__global__ __launch_bounds__(256) void jaccard_topk_merge_kernel(const uint64_t *have, const uint64_t *__restrict__ partial,
                                                                 int64_t segments, int64_t n_a, int32_t topk, uint32_t row_offset,
                                                                 uint64_t *keys_out, int64_t *__restrict__ rows,
                                                                 int32_t *__restrict__ counts) {
    __shared__ uint64_t folded[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t i = blockIdx.x; i < n_a; i += gridDim.x) {
        uint64_t mine = wave == 0 && have != nullptr && lane < topk ? have[i * topk + lane] : 0;
        for (int64_t s0 = (int64_t)wave * 64; s0 < segments; s0 += 256) {
            bool active = s0 + lane < segments;
            const uint64_t *list = partial + ((active ? s0 + lane : 0) * n_a + i) * topk;
            for (int e = 0; e < topk; ++e) {
                uint64_t key = active ? list[e] : 0;
                if (key != 0) key -= row_offset;  // the low word is 0xFFFFFFFF - row
                const uint64_t last = (uint64_t)__shfl((long long)mine, topk - 1);
                active = active && key > last;  // (an empty entry is 0)
                uint64_t pending = __ballot(active);
                if (pending == 0) break;
                while (pending) {
                    const int src = __ffsll((unsigned long long)pending) - 1;
                    pending &= pending - 1;
                    mine = list_insert(mine, (uint64_t)__shfl((long long)key, src), lane, topk);
                }
            }
        }
        folded[wave][lane] = lane < topk ? mine : 0;
        __syncthreads();
        if (wave == 0) {
            for (int w = 1; w < 4; ++w)
                for (int e = 0; e < topk; ++e) {
                    const uint64_t key = folded[w][e];
                    if (key <= (uint64_t)__shfl((long long)mine, topk - 1)) break;  // (0: the list's end)
                    mine = list_insert(mine, key, lane, topk);
                }
            if (lane < topk) {
                if (keys_out != nullptr) keys_out[i * topk + lane] = mine;
                if (rows != nullptr) {
                    rows[i * topk + lane] = mine == 0 ? -1 : (int64_t)(0xFFFFFFFFu - (uint32_t)mine);
                    counts[i * topk + lane] = mine == 0 ? -1 : (int32_t)(mine >> 32);
                }
            }
        }
        __syncthreads();  // `folded` is free for the next row
    }
}

int next_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

}  // namespace

int launch_jaccard_topk(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t num_perm,
                        int32_t bb, const uint32_t *d_live, int32_t min_count, int32_t topk, bool self, const uint64_t *d_have,
                        uint32_t row_offset, uint64_t *d_keys_out, int64_t *d_rows, int32_t *d_counts) {
    const Shape s = shape_of(sig_dtype, num_perm, bb);
    const int64_t tiles_m = (n_a + kTile - 1) / kTile, tiles_n = (n_b + kTile - 1) / kTile;
    int64_t segments = 0;
    if (n_b > 0 && min_count <= num_perm) {
        // 0 auto: the stream kernel for dense rows up to the measured break-even number of probes.  profiles/jaccard_topk_bench.jsonl
        // (uint32, K = 128, k = 10): 16 probes take 2.27 ms on the stream kernel and 2.56 ms on the strip kernel against 10^6 rows,
        // 7.67 ms and 11.56 ms against 10^7; 32 probes take 4.52 / 2.77 ms and 15.31 / 11.79 ms.
        const int64_t kStreamBelow = 16;
        const bool quad = s.slot < 0;  // weighted rows: the stream kernel's element is a sample, s.W / 4 of them per row
        const int per = quad ? 1 : s.wide ? 2 : 4, words_per = quad ? 4 : s.wide ? 2 : 1;
        const int32_t elems = quad ? s.W / 4 : s.W;
        const int pieces = (elems + per - 1) / per;  // 16-byte pieces of a dense row
        const size_t stream_lds = sizeof(uint32_t) * 4 * (size_t)pieces * kStreamProbes;
        // (path 2 asks for the stream kernel wherever it exists: dense and weighted rows whose probes fit in 64 KiB of LDS)
        const bool stream = s.slot <= 0 && stream_lds <= (64u << 10) &&
                            (ctx->opt_jaccard_topk_path == 2 || (ctx->opt_jaccard_topk_path == 0 && n_a <= kStreamBelow));
        TopkArgs tk{};
        tk.live = d_live;
        tk.floor_key = min_count > 0 ? (uint64_t)min_count << 32 : 0;
        tk.topk = topk;
        tk.self = self ? 1 : 0;
        const int64_t forced = ctx->opt_jaccard_topk_segments;
        if (stream) {
            // a wave per segment; enough of them to keep every CU's loads in flight (three per SIMD), 1024 rows each at least
            int64_t want = forced > 0 ? forced : std::min<int64_t>((int64_t)ctx->num_cus * 12, (n_b + 1023) / 1024);
            want = std::max<int64_t>(1, std::min(want, tiles_n));
            const int64_t seg_rows = (n_b + want - 1) / want;
            segments = (n_b + seg_rows - 1) / seg_rows;
            tk.segments = segments;
            if (int rc = ctx->ensure_scratch(4, sizeof(uint64_t) * (size_t)segments * (size_t)n_a * (size_t)topk)) return rc;
            tk.partial = (uint64_t *)ctx->scratch[4];
            const int L = std::min(64, next_pow2(pieces));
            const size_t row_bytes = sizeof(uint32_t) * (size_t)elems * words_per;
            const int vec = (row_bytes % 16 == 0 && ((uintptr_t)d_b & 15) == 0) ? 1 : 0;
            const size_t lds = stream_lds;
            const dim3 grid((unsigned)((segments + 3) / 4));
            for (int64_t q0 = 0; q0 < n_a; q0 += kStreamProbes) {
                const int nq = (int)std::min<int64_t>(kStreamProbes, n_a - q0);
                if (quad)
                    hipLaunchKernelGGL((jaccard_topk_stream_kernel<false, true>), grid, dim3(256), lds, ctx->stream, (const uint32_t *)d_a, n_a, q0, nq,
                                       (const uint32_t *)d_b, n_b, elems, L, vec, seg_rows, tk);
                else if (s.wide)
                    hipLaunchKernelGGL(jaccard_topk_stream_kernel<true>, grid, dim3(256), lds, ctx->stream, (const uint32_t *)d_a, n_a, q0, nq,
                                       (const uint32_t *)d_b, n_b, s.W, L, vec, seg_rows, tk);
                else
                    hipLaunchKernelGGL(jaccard_topk_stream_kernel<false>, grid, dim3(256), lds, ctx->stream, (const uint32_t *)d_a, n_a, q0, nq,
                                       (const uint32_t *)d_b, n_b, s.W, L, vec, seg_rows, tk);
            }
        } else {
            // segments so that tiles_m x S fills the machine (two workgroups per CU), a strip of 32 tiles at least: the first
            // tile of a strip admits every pair
            const int64_t per_cu = 2;
            int64_t want = forced > 0 ? forced
                                      : std::min<int64_t>(((int64_t)ctx->num_cus * per_cu + tiles_m - 1) / tiles_m, std::max<int64_t>(1, tiles_n / 32));
            want = std::max<int64_t>(1, std::min(want, tiles_n));
            tk.seg_tiles = (tiles_n + want - 1) / want;
            segments = (tiles_n + tk.seg_tiles - 1) / tk.seg_tiles;
            tk.segments = segments;
            if (int rc = ctx->ensure_scratch(4, sizeof(uint64_t) * (size_t)segments * (size_t)n_a * (size_t)topk)) return rc;
            tk.partial = (uint64_t *)ctx->scratch[4];
            const int64_t blocks = tiles_m * segments;
            if (blocks >= ((int64_t)1 << 31)) return fail(MHX_ERR_INVALID, "too many tiles for one top-k launch");
            const size_t lds = sizeof(uint64_t) * (size_t)kTile * (size_t)topk;
            const dim3 grid((unsigned)blocks);
            const uint32_t *a = (const uint32_t *)d_a, *b = (const uint32_t *)d_b;
#define MHX_STRIP(S, WD)                                                                                                          \
    do {                                                                                                                          \
        MHX_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&jaccard_topk_strip_kernel<S, WD>),                       \
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                  \
        hipLaunchKernelGGL((jaccard_topk_strip_kernel<S, WD>), grid, dim3(kThreads), lds, ctx->stream, a, n_a, b, n_b, s.W, num_perm, tk); \
    } while (0)
            switch (s.slot) {
                case -1: MHX_STRIP(-1, false); break;
                case 0: if (s.wide) MHX_STRIP(0, true); else MHX_STRIP(0, false); break;
                case 1: MHX_STRIP(1, false); break;
                case 2: MHX_STRIP(2, false); break;
                case 4: MHX_STRIP(4, false); break;
                case 8: MHX_STRIP(8, false); break;
                case 16: MHX_STRIP(16, false); break;
                default: MHX_STRIP(32, false); break;
            }
#undef MHX_STRIP
        }
        MHX_HIP_CHECK(hipGetLastError());
    }
    // (no candidates at all: the merge of nothing writes the padding)
    hipLaunchKernelGGL(jaccard_topk_merge_kernel, dim3((unsigned)std::min<int64_t>(n_a, 1 << 20)), dim3(256), 0, ctx->stream, d_have,
                       (const uint64_t *)ctx->scratch[4], segments, n_a, topk, row_offset, d_keys_out, d_rows, d_counts);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
