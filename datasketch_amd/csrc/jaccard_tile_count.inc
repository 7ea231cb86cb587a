// jaccard_tile_count.inc -- the body that stages and counts one 128 x 128 tile, included (not called) by the all-pairs kernels:
// jaccard_tile_kernel (jaccard_kernels.hip) and jaccard_topk_strip_kernel (jaccard_topk_kernels.hip).  Text rather than a device
// function: handed the accumulators by reference the compiler keeps a second copy of the 64 registers around the chunk loop.
// In scope at the point of inclusion: template parameters SLOT, WIDE; a, n_a, b, n_b, W; the tile origin i0, j0; tid, ty, tx;
// pad_b, chunks; the LDS stages As, Bs, Ah, Bh.  Defines acc[8][8], the thread's 8 x 8 counts (b-bit kinds: differing slots).
// SLOT < 0: weighted rows, staged word by word like uint32 rows and counted sample by sample (4 words, see jaccard_tile.h).
// Holds barriers: every thread of the workgroup passes through it.
    // staging: thread tid moves word (tid & 15) of the chunk for rows (tid >> 4) + 16 e of the A and the B tile
    const int srow = tid >> 4, sw = tid & 15;
    uint32_t ok_a = 0, ok_b = 0;  // bit e: row srow + 16 e exists
#pragma unroll
    for (int e = 0; e < kStage; ++e) {
        ok_a |= (i0 + srow + 16 * e < n_a ? 1u : 0u) << e;
        ok_b |= (j0 + srow + 16 * e < n_b ? 1u : 0u) << e;
    }
    const int64_t step = 16 * (int64_t)W;  // elements between the rows a thread stages
    uint32_t ra[kStage], rb[kStage], rah[WIDE ? kStage : 1], rbh[WIDE ? kStage : 1];
    auto fetch = [&](int c) {
        const int w = c * kChunk + sw;
        const uint32_t va = w < W ? ok_a : 0u, vb = w < W ? ok_b : 0u;
        if (WIDE) {
            const uint64_t *pa = reinterpret_cast<const uint64_t *>(a) + (i0 + srow) * W + w;
            const uint64_t *pb = reinterpret_cast<const uint64_t *>(b) + (j0 + srow) * W + w;
#pragma unroll
            for (int e = 0; e < kStage; ++e) {
                const uint64_t x = (va >> e) & 1u ? pa[e * step] : 0ull;
                const uint64_t y = (vb >> e) & 1u ? pb[e * step] : (uint64_t)pad_b;
                ra[e] = (uint32_t)x;
                rah[e] = (uint32_t)(x >> 32);
                rb[e] = (uint32_t)y;
                rbh[e] = (uint32_t)(y >> 32);
            }
        } else {
            const uint32_t *pa = a + (i0 + srow) * W + w;
            const uint32_t *pb = b + (j0 + srow) * W + w;
#pragma unroll
            for (int e = 0; e < kStage; ++e) {
                ra[e] = (va >> e) & 1u ? pa[e * step] : 0u;
                rb[e] = (vb >> e) & 1u ? pb[e * step] : pad_b;
            }
        }
    };

    uint32_t acc[8][8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[r][c] = 0;

    fetch(0);
    for (int c = 0; c < chunks; ++c) {
        __syncthreads();  // the previous chunk's reads are done
        int high = 0;
#pragma unroll
        for (int e = 0; e < kStage; ++e) {
            As[sw][srow + 16 * e] = ra[e];
            Bs[sw][srow + 16 * e] = rb[e];
            if (WIDE) {
                Ah[sw][srow + 16 * e] = rah[e];
                Bh[sw][srow + 16 * e] = rbh[e];
                high |= (rah[e] | rbh[e]) != 0;
            }
        }
        if (WIDE) high = __syncthreads_or(high);
        else __syncthreads();
        if (c + 1 < chunks) fetch(c + 1);  // in flight while this chunk is counted
        const int kn = min(kChunk, W - c * kChunk);  // words of this chunk (b = 1, K = 128 rows are 4 words)

        if (SLOT < 0) {  // a (k, t) sample is words kk .. kk + 3 of the chunk (kn is a multiple of 4): equal when all four are
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int kk = 0; kk < kn; kk += 4) {
                uint32_t x[4][8], y[4][8];
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    *reinterpret_cast<uint4 *>(&x[w][0]) = *reinterpret_cast<const uint4 *>(&As[kk + w][ty * 4]);
                    *reinterpret_cast<uint4 *>(&x[w][4]) = *reinterpret_cast<const uint4 *>(&As[kk + w][64 + ty * 4]);
                    *reinterpret_cast<uint4 *>(&y[w][0]) = *reinterpret_cast<const uint4 *>(&Bs[kk + w][tx * 4]);
                    *reinterpret_cast<uint4 *>(&y[w][4]) = *reinterpret_cast<const uint4 *>(&Bs[kk + w][64 + tx * 4]);
                }
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        uint32_t d = (x[0][r] ^ y[0][q]) | (x[1][r] ^ y[1][q]) | (x[2][r] ^ y[2][q]) | (x[3][r] ^ y[3][q]);
                        // (opaque: left to itself the compiler compares word by word, 4 v_cmp and 3 ANDs of lane masks per cell
                        // -- more masks in flight than there are scalar registers, 214 lane spills per trip)
                        asm("" : "+v"(d));
                        acc[r][q] += d == 0 ? 1u : 0u;
                    }
            }
        } else if (!WIDE || !high) {  // (uint64 chunks whose high words are all zero take the 32-bit comparison)
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int kk = 0; kk < kn; ++kk) {
                uint32_t x[8], y[8];
                *reinterpret_cast<uint4 *>(&x[0]) = *reinterpret_cast<const uint4 *>(&As[kk][ty * 4]);
                *reinterpret_cast<uint4 *>(&x[4]) = *reinterpret_cast<const uint4 *>(&As[kk][64 + ty * 4]);
                *reinterpret_cast<uint4 *>(&y[0]) = *reinterpret_cast<const uint4 *>(&Bs[kk][tx * 4]);
                *reinterpret_cast<uint4 *>(&y[4]) = *reinterpret_cast<const uint4 *>(&Bs[kk][64 + tx * 4]);
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        if (SLOT == 0) acc[r][q] += x[r] == y[q] ? 1u : 0u;
                        else acc[r][q] += differing_slots<SLOT == 0 ? 1 : SLOT>(x[r], y[q]);
                    }
            }
        } else {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int kk = 0; kk < kn; ++kk) {
                uint32_t x[8], y[8], xh[8], yh[8];
                *reinterpret_cast<uint4 *>(&x[0]) = *reinterpret_cast<const uint4 *>(&As[kk][ty * 4]);
                *reinterpret_cast<uint4 *>(&x[4]) = *reinterpret_cast<const uint4 *>(&As[kk][64 + ty * 4]);
                *reinterpret_cast<uint4 *>(&y[0]) = *reinterpret_cast<const uint4 *>(&Bs[kk][tx * 4]);
                *reinterpret_cast<uint4 *>(&y[4]) = *reinterpret_cast<const uint4 *>(&Bs[kk][64 + tx * 4]);
                *reinterpret_cast<uint4 *>(&xh[0]) = *reinterpret_cast<const uint4 *>(&Ah[kk][ty * 4]);
                *reinterpret_cast<uint4 *>(&xh[4]) = *reinterpret_cast<const uint4 *>(&Ah[kk][64 + ty * 4]);
                *reinterpret_cast<uint4 *>(&yh[0]) = *reinterpret_cast<const uint4 *>(&Bh[kk][tx * 4]);
                *reinterpret_cast<uint4 *>(&yh[4]) = *reinterpret_cast<const uint4 *>(&Bh[kk][64 + tx * 4]);
#pragma unroll
                for (int r = 0; r < 8; ++r)
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc[r][q] += ((x[r] ^ y[q]) | (xh[r] ^ yh[q])) == 0 ? 1u : 0u;
            }
        }
    }
