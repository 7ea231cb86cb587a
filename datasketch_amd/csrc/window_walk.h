// window_walk.h -- a wave's walk over the windows of a corpus (datasketch_amd/shingle.py is the definition of a window) with the
// per-window hash as a template parameter: window -> document, the part that tests/window_owner_model.py pins.  Instantiated by
// xxh_windows_kernel (xxh_kernels.hip).  sha1_windows_kernel (sha1_kernels.hip) keeps its own text of the same walk: instantiating
// this template there changed its generated code ("xxHash in place"), and that kernel's generated code is not to change.
#pragma once

#include "mhx_internal.h"

namespace mhx {

// The last document d of [0, n_docs) with set_offsets[d] <= t, for a t that is the same in every lane (all 64 active): documents
// without a window share their offset with the next one, so this is the document that owns window t.  64 probes per step --
// three steps at 10^5 documents, four at 10^7 -- where a binary search takes one dependent load per bit.
__device__ __forceinline__ int64_t wave_owner_of(const int64_t *__restrict__ set_offsets, int64_t n_docs, int64_t t, int lane) {
    int64_t lo = 0, hi = n_docs - 1;  // set_offsets[lo] <= t throughout; the owner is in [lo, hi]
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t probe = lo + (int64_t)(lane + 1) * step;
        const bool holds = probe <= hi && set_offsets[probe] <= t;
        const int64_t found = lo + (int64_t)__popcll(__ballot(holds)) * step;  // the offsets are sorted: the lanes that hold are a prefix
        hi = std::min<int64_t>(hi, found + step - 1);
        lo = found;
    }
    return lo;
}

// Window t of the corpus is `width` consecutive items of one document -- bytes (item_offsets == nullptr), or byte tokens item i =
// bytes[item_offsets[i] .. item_offsets[i + 1]) -- or the whole document where it has fewer; set_offsets[d] is the first window of
// document d.  One thread per window; a wave takes `per_wave` consecutive windows (a multiple of 64), 64 per trip, and stores
// out[t] = hash(address of the window's first byte, its length in bytes).
// Window -> document: the wave finds the owner of its first window once (wave_owner_of) and keeps that document's offsets in
// scalar registers.  A trip whose 64 windows all lie in it -- most trips, where documents are longer than 64 windows -- loads
// no offset at all.  Otherwise the lanes load the offsets of the next 64 documents, one each, and every lane counts by a binary
// search across the lanes (six ds_bpermute) how many of them start at or before its window; a ballot counts those that start
// at or before the next trip's first window, which moves the wave's document on.  A trip that spans more than 64 documents
// takes further such batches.
template <typename OutT, class Hash>
__device__ __forceinline__ void walk_windows(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ item_offsets,
                                             const int64_t *__restrict__ doc_offsets, const int64_t *__restrict__ set_offsets, int64_t n_docs,
                                             int64_t n_windows, int64_t width, int64_t per_wave, OutT *__restrict__ out, Hash hash) {
    const int lane = (int)(threadIdx.x & 63u);
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int64_t base = wave * per_wave;
    const int64_t end = std::min<int64_t>(base + per_wave, n_windows);
    if (base >= end) return;
    // the document of window `base` (the same in every lane): its first window, the next document's, its items
    int64_t cur = wave_owner_of(set_offsets, n_docs, base, lane);
    int64_t cur_window = set_offsets[cur], cur_next = set_offsets[cur + 1], cur_item0 = doc_offsets[cur], cur_items = doc_offsets[cur + 1] - cur_item0;
    for (; base < end; base += 64) {
        const int64_t last = std::min<int64_t>(base + 63, n_windows - 1);
        const int64_t t = base + lane;
        int64_t window0 = cur_window, item0 = cur_item0, items = cur_items;
        if (last >= cur_next) {  // (the same in every lane) the trip reaches into later documents
            int64_t d = cur, moved = 0;
            for (int64_t next = cur + 1;; next += 64) {
                // where the documents next .. next + 63 start, relative to base and cut to [0, 65]: sorted; lane's window is `lane`,
                // the next trip's first window is 64.  Past the last document stands set_offsets[n_docs] = n_windows.
                const int64_t j = next + lane;
                const uint32_t rel = (uint32_t)std::min<int64_t>(std::max<int64_t>(set_offsets[std::min<int64_t>(j, n_docs)] - base, 0), 65);
                const uint32_t rel_63 = (uint32_t)__builtin_amdgcn_readlane((int)rel, 63);
                uint32_t started = 0;  // of the documents next .. next + 62
#pragma unroll
                for (uint32_t s = 32; s; s >>= 1)
                    if ((uint32_t)__shfl((int)rel, (int)(started + s - 1)) <= (uint32_t)lane) started += s;
                d += rel_63 <= (uint32_t)lane ? 64 : started;
                moved += __popcll(__ballot(j < n_docs && rel <= 64u));
                if (rel_63 > 64u || next + 63 >= n_docs) break;
            }
            d = std::min<int64_t>(d, n_docs - 1);  // (lanes past the last window)
            window0 = set_offsets[d];
            item0 = doc_offsets[d];
            items = doc_offsets[d + 1] - item0;
            cur = std::min<int64_t>(cur + moved, n_docs - 1);
            cur_window = set_offsets[cur];
            cur_next = set_offsets[cur + 1];
            cur_item0 = doc_offsets[cur];
            cur_items = doc_offsets[cur + 1] - cur_item0;
        }
        if (t >= n_windows) continue;
        const int64_t first = item0 + (t - window0);
        const int64_t count = std::min<int64_t>(width, items);  // a short document is one window
        int64_t beg = first, len = count;
        if (item_offsets) {
            beg = item_offsets[first];
            len = item_offsets[first + count] - beg;
        }
        out[t] = hash(reinterpret_cast<uintptr_t>(bytes) + (uintptr_t)beg, len);
    }
}

}  // namespace mhx
