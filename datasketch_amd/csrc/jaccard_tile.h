// jaccard_tile.h -- the 128 x 128 tile of agreeing-position counts that the all-pairs Jaccard kernels share: the matrix /
// threshold kernel (jaccard_kernels.hip) and the top-k strip kernel (jaccard_topk_kernels.hip) stage and count a tile with
// the same code (jaccard_tile_count.inc) and differ in what they do with the 8 x 8 register sub-tile afterwards.
#pragma once

#include "mhx_internal.h"

namespace mhx {
namespace jtile {

constexpr int kTile = 128;         // rows of A and of B per workgroup tile
constexpr int kChunk = 16;         // 32-bit words per row and LDS stage
constexpr int kLdsRow = kTile + 4; // [word][row] stride in words: 16-byte aligned, successive words 4 banks apart
constexpr int kThreads = 256;
constexpr int kStage = kChunk * kTile / kThreads;  // words of A (and of B) one thread stages per chunk

// Kind of row: dense uint32 (SLOT 0, !WIDE), dense uint64 (SLOT 0, WIDE), b-bit packed blocks (SLOT = slot width), weighted
// (SLOT -1, !WIDE): int64 (k, t) samples, a row of S samples is 4 S 32-bit words and a position agrees when all four words of
// the sample do -- a sample never straddles a 16-word chunk, and the padding words (A 0, B 1) fill whole samples.
template <int SLOT>
__device__ __forceinline__ uint32_t slot_low_bits() {
    return SLOT == 1 ? 0xFFFFFFFFu : SLOT == 2 ? 0x55555555u : SLOT == 4 ? 0x11111111u : SLOT == 8 ? 0x01010101u
         : SLOT == 16 ? 0x00010001u : 0x00000001u;
}

// number of slots of width SLOT that differ between x and y (the slots never straddle a 32-bit word)
template <int SLOT>
__device__ __forceinline__ uint32_t differing_slots(uint32_t x, uint32_t y) {
    uint32_t z = x ^ y;
#pragma unroll
    for (int sh = 1; sh < SLOT; sh <<= 1) z |= z >> sh;
    return (uint32_t)__builtin_popcount(z & slot_low_bits<SLOT>());
}

// sub-tile element (r, q) of thread (ty, tx) is pair (i0 + rowof(ty, r), j0 + rowof(tx, q))
__device__ __forceinline__ int rowof(int t4, int r) { return (r < 4 ? 0 : 64) + t4 * 4 + (r & 3); }

// words per row and kernel selection shared by the launchers.  b == kWeightedRows: k samples of (k, t); any other b < 0: dense rows
// of sig_dtype; else b-bit blocks.
struct Shape {
    int slot;   // 0 dense, -1 weighted
    bool wide;  // dense uint64
    int32_t W;
};

inline Shape shape_of(int sig_dtype, int32_t k, int32_t b) {
    if (b == kWeightedRows) return Shape{-1, false, 4 * k};
    if (b < 0) return Shape{0, sig_dtype == MHX_U64, k};
    const int slot = bbit_slot_size(b);
    const int per = 64 / slot;
    return Shape{slot, false, 2 * ((k + per - 1) / per)};
}

}  // namespace jtile
}  // namespace mhx
