// words_kernels.hip -- text to its normal form on the device: every word of a byte-mode corpus, translated, followed by one space
// (datasketch_amd/shingle.py: word_table, words, normalize_words are the definition).
//
// For byte i of document d, with word(i) = table[b[i]] != 0:
//   start(i) = word(i) and (i is the first byte of d, or !word(i-1))
//   end(i)   = word(i) and (i is the last byte of d,  or !word(i+1))
// Byte i emits word(i) + end(i) output bytes (its translation, then the space that closes the word); word j starts at the
// output position of its start byte.  That is two exclusive sums over the corpus -- output bytes and words -- and a compaction.
//
// Layout.  The corpus is cut into GRANULES of 16 bytes, one per lane and one 16-byte load each, and TILES of 256 granules, one
// per workgroup: device_scan.h's tile (256 threads x 16 items), so its tile-offsets kernel turns the tile sums of both counters
// into tile offsets.  Granules are cut on 16-byte ADDRESSES, not on byte indices: the kernels work in v = i + (d_bytes & 15), so
// that every load is aligned whatever the caller's pointer, and bytes outside [0, n_bytes) are separators nobody loads -- a granule
// that straddles an end of the corpus falls back to its aligned dwords that hold at least one byte of it.
// Document boundaries are a bitmap in v ("a document starts here"), zeroed and then set with one atomicOr per doc_offsets entry;
// the byte kernels read 16 (+1) bits of it per granule, and nobody binary-searches per granule.  Bit n_bytes is set by the last
// entry: it ends the last word.
//
// Launches: memset + mark (bitmap), count (tile sums of both counters), device_scan.h's tile offsets twice (which also leave the
// two totals), then -- after the caller has read the totals and checked its capacities -- emit.  Emit scans the tile again,
// compacts the tile's output bytes into LDS and writes them with 16-byte stores (byte stores for the unaligned head and tail only),
// scatters item_offsets, and writes word_doc_offsets[d] where a granule holds the boundary: one binary search per distinct
// boundary, then the run of documents that share it.  The entries equal to n_bytes (trailing empty documents and the last one)
// and item_offsets[n_words] belong to the last tile.  No grid is capped: one workgroup per tile, one thread per doc_offsets entry.
#include "device_scan.h"
#include "mhx_internal.h"

namespace mhx {
namespace {

constexpr int kGranule = 16, kTileThreads = 256, kTileBytes = kGranule * kTileThreads;
static_assert(kTileBytes == kScanTile, "the tile sums feed device_scan.h's tile offsets");

struct WordTable {  // the 256-byte translate table, by value in the kernel arguments
    uint32_t w[64];
};

__global__ __launch_bounds__(256) void words_mark_kernel(const int64_t *__restrict__ doc_offsets, int64_t n_entries, int mis,
                                                         uint32_t *__restrict__ bitmap) {
    const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (d >= n_entries) return;
    const int64_t v = doc_offsets[d] + mis;
    atomicOr(&bitmap[v >> 5], 1u << (v & 31));
}

// is byte v (outside the tile) a word byte?  Loads the aligned dword that holds it; nothing outside [lo, hi) is touched.
__device__ __forceinline__ uint32_t edge_is_word(const uint8_t *ab, int64_t v, int64_t lo, int64_t hi, const uint8_t *tab) {
    if (v < lo || v >= hi) return 0;
    const uint32_t dw = reinterpret_cast<const uint32_t *>(ab)[v >> 2];
    return tab[(dw >> (8 * (int)(v & 3))) & 255u] != 0;
}

// What one lane knows of its granule: the bytes, and per byte (bit k = byte 16 g + k) whether it is a word byte, starts a word,
// ends one, and starts a document.
struct Granule {
    uint32_t b[4];
    uint32_t word, start, end, docs;
};

// All 256 threads call this.  ab = d_bytes rounded down to 16 bytes; [lo, hi) = the corpus in v.  tab: the table in LDS, already
// visible; nb: 258 words of LDS.
__device__ __forceinline__ Granule load_granule(const uint8_t *ab, int64_t lo, int64_t hi, const uint32_t *__restrict__ bitmap,
                                                const uint8_t *tab, uint32_t *nb) {
    const int tid = threadIdx.x;
    const int64_t g = (int64_t)blockIdx.x * kTileThreads + tid, v0 = g * kGranule;
    Granule r;
    if (v0 >= (lo & ~(int64_t)3) && v0 + kGranule <= ((hi + 3) & ~(int64_t)3)) {
        const uint4 q = *reinterpret_cast<const uint4 *>(ab + v0);
        r.b[0] = q.x, r.b[1] = q.y, r.b[2] = q.z, r.b[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t v = v0 + 4 * j;
            r.b[j] = v + 4 > lo && v < hi ? reinterpret_cast<const uint32_t *>(ab)[v >> 2] : 0u;
        }
    }
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < kGranule; ++k) {
        const uint32_t c = (r.b[k >> 2] >> (8 * (k & 3))) & 255u;
        const int64_t v = v0 + k;
        if (tab[c] != 0 && v >= lo && v < hi) word |= 1u << k;
    }
    // the bitmap: 16 bits of this granule, and the first of the next one (a word ends where the next document starts)
    const uint32_t docs17 = ((bitmap[g >> 1] >> ((g & 1) * 16)) & 0xFFFFu) | (((bitmap[(g + 1) >> 1] >> (((g + 1) & 1) * 16)) & 1u) << 16);
    nb[tid + 1] = word;
    if (tid == 0) nb[0] = edge_is_word(ab, v0 - 1, lo, hi, tab) << 15;
    if (tid == kTileThreads - 1) nb[kTileThreads + 1] = edge_is_word(ab, v0 + kGranule, lo, hi, tab);
    __syncthreads();
    const uint32_t prev = (nb[tid] >> 15) & 1u, next = nb[tid + 2] & 1u;
    const uint32_t word17 = word | (next << 16);
    r.word = word;
    r.start = word & (docs17 | ~((word << 1) | prev)) & 0xFFFFu;
    r.end = word & ((docs17 >> 1) | ~(word17 >> 1)) & 0xFFFFu;
    // a boundary at or behind the end of the corpus is not this lane's to report (emit: the last tile)
    const int64_t left = hi - v0;
    r.docs = docs17 & 0xFFFFu & (left >= kGranule ? 0xFFFFu : left <= 0 ? 0u : (1u << left) - 1u);
    return r;
}

// inclusive scan of one uint32 per thread over the workgroup (the two counters of a tile fit 16 bits each: <= 8192 and <= 4096)
__device__ __forceinline__ uint32_t block_inclusive_scan32(uint32_t v, uint32_t *tmp4) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += up;
    }
    if (lane == 63) tmp4[wave] = v;
    __syncthreads();
    uint32_t add = 0;
    for (int w = 0; w < wave; ++w) add += tmp4[w];
    return v + add;
}

__device__ __forceinline__ void table_to_lds(const WordTable &table, uint32_t *tab32) {
    if (threadIdx.x < 64) tab32[threadIdx.x] = table.w[threadIdx.x];
    __syncthreads();
}

// packed counters of a granule: output bytes in the low half, words in the high half
__device__ __forceinline__ uint32_t granule_counts(const Granule &r) {
    return (uint32_t)(__popc(r.word) + __popc(r.end)) | ((uint32_t)__popc(r.start) << 16);
}

__global__ __launch_bounds__(256) void words_count_kernel(const uint8_t *ab, int64_t lo, int64_t hi, const uint32_t *__restrict__ bitmap,
                                                          WordTable table, uint64_t *__restrict__ tile_bytes,
                                                          uint64_t *__restrict__ tile_words) {
    __shared__ uint32_t tab32[64], nb[kTileThreads + 2], tmp[4];
    table_to_lds(table, tab32);
    const Granule r = load_granule(ab, lo, hi, bitmap, reinterpret_cast<const uint8_t *>(tab32), nb);
    const uint32_t incl = block_inclusive_scan32(granule_counts(r), tmp);
    if (threadIdx.x == kTileThreads - 1) {
        tile_bytes[blockIdx.x] = incl & 0xFFFFu;
        tile_words[blockIdx.x] = incl >> 16;
    }
}

// the first entry of doc_offsets[0 .. n_entries) that is >= at
__device__ __forceinline__ int64_t first_entry_at(const int64_t *__restrict__ doc_offsets, int64_t n_entries, int64_t at) {
    int64_t a = 0, b = n_entries;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if (doc_offsets[m] < at) a = m + 1; else b = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void words_emit_kernel(const uint8_t *ab, int64_t lo, int64_t hi, const uint32_t *__restrict__ bitmap,
                                                         WordTable table, const uint64_t *__restrict__ tile_bytes,
                                                         const uint64_t *__restrict__ tile_words, const int64_t *__restrict__ doc_offsets,
                                                         int64_t n_docs, uint8_t *__restrict__ out, int64_t *__restrict__ item_offsets,
                                                         int64_t *__restrict__ word_doc_offsets) {
    __shared__ uint32_t tab32[64], nb[kTileThreads + 2], tmp[4];
    // the tile's output, shifted so that LDS byte x lies at global address (out + tile offset - shift) + x: 16-byte chunks of the
    // one are 16-byte chunks of the other.  At most 2 * kTileBytes bytes behind a shift of at most 15.
    __shared__ uint4 stage4[(2 * kTileBytes + 16) / 16 + 1];
    uint8_t *stage = reinterpret_cast<uint8_t *>(stage4);
    const uint8_t *tab = reinterpret_cast<const uint8_t *>(tab32);
    table_to_lds(table, tab32);
    const Granule r = load_granule(ab, lo, hi, bitmap, tab, nb);
    const uint32_t mine = granule_counts(r), incl = block_inclusive_scan32(mine, tmp), excl = incl - mine;
    const int64_t byte0 = (int64_t)tile_bytes[blockIdx.x], word0 = (int64_t)tile_words[blockIdx.x];
    const int shift = (int)((uintptr_t)(out + byte0) & 15);

    // this granule: bytes into LDS, word starts into item_offsets, document boundaries into word_doc_offsets
    uint32_t at = shift + (excl & 0xFFFFu);
    int64_t word = word0 + (excl >> 16);
    const int64_t v0 = ((int64_t)blockIdx.x * kTileThreads + threadIdx.x) * kGranule;
    if (r.word | r.docs) {
#pragma unroll
        for (int k = 0; k < kGranule; ++k) {
            const uint32_t bit = 1u << k;
            if (r.docs & bit) {
                const int64_t i = v0 + k - lo;
                for (int64_t d = first_entry_at(doc_offsets, n_docs + 1, i); d <= n_docs && doc_offsets[d] == i; ++d) word_doc_offsets[d] = word;
            }
            if (r.start & bit) item_offsets[word++] = byte0 + (int64_t)(at - shift);
            if (r.word & bit) stage[at++] = tab[(r.b[k >> 2] >> (8 * (k & 3))) & 255u];
            if (r.end & bit) stage[at++] = 0x20;
        }
    }
    __shared__ uint32_t tile_total;
    if (threadIdx.x == kTileThreads - 1) tile_total = incl;
    __syncthreads();
    const uint32_t total = tile_total, n_stage = total & 0xFFFFu;

    // the tile's bytes out: whole 16-byte chunks as they are, the head and the tail -- chunks it shares with its neighbours -- by bytes
    uint8_t *base = out + byte0 - shift;  // 16-byte aligned
    const uint32_t first = shift, last = shift + n_stage;  // LDS bytes [first, last)
    for (uint32_t c = threadIdx.x; c * 16 < last; c += kTileThreads) {
        const uint32_t x0 = c * 16;
        if (x0 >= first && x0 + 16 <= last) {
            *reinterpret_cast<uint4 *>(base + x0) = stage4[c];
        } else {
            for (uint32_t x = x0 < first ? first : x0; x < x0 + 16 && x < last; ++x) base[x] = stage[x];
        }
    }

    // the last tile: the end of the last word, and the documents that start at n_bytes
    if (blockIdx.x == gridDim.x - 1) {
        const int64_t n_words = word0 + (total >> 16);
        if (threadIdx.x == 0) item_offsets[n_words] = byte0 + n_stage;
        for (int64_t d = first_entry_at(doc_offsets, n_docs + 1, hi - lo) + threadIdx.x; d <= n_docs; d += kTileThreads) word_doc_offsets[d] = n_words;
    }
}

struct WordsPlan {  // where the launches keep their state in scratch[4], as a function of the corpus alone
    const uint8_t *ab;
    int64_t lo, hi, n_tiles;
    size_t bitmap_bytes, total_bytes;
    uint32_t *bitmap(mhx_ctx *ctx) const { return static_cast<uint32_t *>(ctx->scratch[4]); }
    uint64_t *tile_bytes(mhx_ctx *ctx) const { return reinterpret_cast<uint64_t *>(static_cast<char *>(ctx->scratch[4]) + bitmap_bytes); }
    uint64_t *tile_words(mhx_ctx *ctx) const { return tile_bytes(ctx) + n_tiles; }
    uint64_t *totals(mhx_ctx *ctx) const { return tile_bytes(ctx) + 2 * n_tiles; }
};

WordsPlan words_plan(const uint8_t *d_bytes, int64_t n_bytes) {
    WordsPlan p;
    const int mis = (int)((uintptr_t)d_bytes & 15);
    p.ab = d_bytes - mis;
    p.lo = mis;
    p.hi = mis + n_bytes;
    p.n_tiles = (p.hi + kTileBytes - 1) / kTileBytes;
    // one bit per byte of every tile, and the word behind them: bit `hi` of a corpus that fills its last tile, and the "next
    // granule" of the last lane
    p.bitmap_bytes = pad256(sizeof(uint32_t) * (size_t)(p.n_tiles * (kTileBytes / 32) + 1));
    p.total_bytes = p.bitmap_bytes + sizeof(uint64_t) * (size_t)(2 * p.n_tiles + 2);
    return p;
}

WordTable words_table(const uint8_t *table) {
    WordTable t;
    for (int i = 0; i < 64; ++i)
        t.w[i] = (uint32_t)table[4 * i] | (uint32_t)table[4 * i + 1] << 8 | (uint32_t)table[4 * i + 2] << 16 | (uint32_t)table[4 * i + 3] << 24;
    return t;
}

}  // namespace

// Counts: enqueues bitmap, tile sums and tile offsets, then reads the two totals back (blocking).  n_bytes > 0, n_docs > 0.
int launch_words_count(mhx_ctx *ctx, const uint8_t *d_bytes, int64_t n_bytes, const int64_t *d_doc_offsets, int64_t n_docs,
                       const uint8_t *table, int64_t *n_words, int64_t *n_out_bytes) {
    *n_words = *n_out_bytes = 0;
    if (n_bytes == 0) return MHX_OK;
    const WordsPlan p = words_plan(d_bytes, n_bytes);
    if (p.n_tiles >= (int64_t)1 << 31 || n_docs >= (int64_t)1 << 39) return fail(MHX_ERR_UNSUPPORTED, "a corpus of more than 2^43 bytes or 2^39 documents");
    if (int rc = ctx->ensure_scratch(4, p.total_bytes)) return rc;
    MHX_HIP_CHECK(hipMemsetAsync(p.bitmap(ctx), 0, p.bitmap_bytes, ctx->stream));
    hipLaunchKernelGGL(words_mark_kernel, dim3((unsigned)((n_docs + 1 + 255) / 256)), dim3(256), 0, ctx->stream, d_doc_offsets, n_docs + 1,
                       (int)p.lo, p.bitmap(ctx));
    hipLaunchKernelGGL(words_count_kernel, dim3((unsigned)p.n_tiles), dim3(kTileThreads), 0, ctx->stream, p.ab, p.lo, p.hi, p.bitmap(ctx),
                       words_table(table), p.tile_bytes(ctx), p.tile_words(ctx));
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, p.tile_bytes(ctx), p.n_tiles, p.totals(ctx));
    hipLaunchKernelGGL(scan_tile_offsets_kernel, dim3(1), dim3(1024), 0, ctx->stream, p.tile_words(ctx), p.n_tiles, p.totals(ctx) + 1);
    MHX_HIP_CHECK(hipGetLastError());
    uint64_t totals[2] = {0, 0};
    MHX_HIP_CHECK(hipMemcpyAsync(totals, p.totals(ctx), sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n_out_bytes = (int64_t)totals[0];
    *n_words = (int64_t)totals[1];
    return MHX_OK;
}

// Emits what launch_words_count counted, for the same corpus and table, nothing having used scratch[4] in between: d_out holds
// n_out_bytes bytes, d_item_offsets n_words + 1 entries, d_word_doc_offsets n_docs + 1.  Enqueues only.
int launch_words_emit(mhx_ctx *ctx, const uint8_t *d_bytes, int64_t n_bytes, const int64_t *d_doc_offsets, int64_t n_docs,
                      const uint8_t *table, uint8_t *d_out, int64_t *d_item_offsets, int64_t *d_word_doc_offsets) {
    if (n_bytes == 0) {  // no word: every document starts at word 0, and so does the end of the last word
        MHX_HIP_CHECK(hipMemsetAsync(d_word_doc_offsets, 0, sizeof(int64_t) * (size_t)(n_docs + 1), ctx->stream));
        MHX_HIP_CHECK(hipMemsetAsync(d_item_offsets, 0, sizeof(int64_t), ctx->stream));
        return MHX_OK;
    }
    const WordsPlan p = words_plan(d_bytes, n_bytes);
    hipLaunchKernelGGL(words_emit_kernel, dim3((unsigned)p.n_tiles), dim3(kTileThreads), 0, ctx->stream, p.ab, p.lo, p.hi, p.bitmap(ctx),
                       words_table(table), p.tile_bytes(ctx), p.tile_words(ctx), d_doc_offsets, n_docs, d_out, d_item_offsets,
                       d_word_doc_offsets);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
