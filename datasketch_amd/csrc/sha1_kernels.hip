// sha1_kernels.hip -- the reference's default token hash on the device.
//
// Reference: datasketch/hashfunc.py:5-15   sha1_hash32(data) = first 4 bytes of SHA1(data), little-endian
//            datasketch/hashfunc.py:17-28  sha1_hash64(data) = first 8 bytes, little-endian
// called once per token from MinHash.update / update_batch (datasketch/minhash.py:221, :262-263).
// In Python that per-token call is >100x the cost of the permutation kernel; here a corpus of byte
// tokens (one packed byte buffer + int64 offsets, the CSR of bytes) is hashed by one thread per
// token and the uint32 / uint64 results feed mhx_minhash_bulk_dev directly.
//
// SHA-1 (FIPS 180-4) with a 16-word circular message schedule in registers; 80 rounds fully
// unrolled.  Tokens are read as aligned dwords and re-aligned with v_alignbyte (a token may start at
// any byte); an aligned dword is only loaded if it holds at least one byte of the token, so the
// kernel never touches memory past the packed buffer's last dword.
//
// sha1_windows_kernel hashes the shingles of a corpus in place (datasketch_amd/shingle.py): the overlapping windows of a
// document are read where they lie, one thread per window, under the same load rule.
#include "mhx_internal.h"

namespace mhx {
namespace {

__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) { return __builtin_rotateleft32(x, n); }

// little-endian dword k (bytes 4k..4k+3) of the token's byte stream; bytes at or past `len` are 0
__device__ __forceinline__ uint32_t stream_word(const uint32_t *__restrict__ aligned, uint32_t shift, int64_t len,
                                                int64_t k) {
    const int64_t first = 4 * k;  // stream position of this word's first byte
    if (first >= len) return 0;
    // aligned dwords j = k and k+1 cover stream bytes [4j - shift, 4j - shift + 4)
    const uint32_t lo = aligned[k];
    const bool need_hi = shift != 0 && (4 * (k + 1) - (int64_t)shift) < len;
    const uint32_t hi = need_hi ? aligned[k + 1] : 0u;
    uint32_t w = __builtin_amdgcn_alignbyte(hi, lo, shift);
    const int64_t valid = len - first;  // > 0
    if (valid < 4) w &= (1u << (8 * (uint32_t)valid)) - 1u;
    return w;
}

// message word k (big-endian, as SHA-1 consumes it) of the PADDED message: data, 0x80, zeros, bit length
__device__ __forceinline__ uint32_t padded_word(const uint32_t *__restrict__ aligned, uint32_t shift, int64_t len,
                                                int64_t k, int64_t total_words) {
    uint32_t w = stream_word(aligned, shift, len, k);
    const int64_t first = 4 * k;
    if (len >= first && len < first + 4) w |= 0x80u << (8 * (uint32_t)(len - first));
    w = __builtin_bswap32(w);
    const uint64_t bits = (uint64_t)len * 8u;
    if (k == total_words - 2) w = (uint32_t)(bits >> 32);
    if (k == total_words - 1) w = (uint32_t)bits;
    return w;
}

// the 80 rounds over one 16-word block (w is consumed as the circular message schedule)
__device__ __forceinline__ void sha1_rounds(uint32_t (&w)[16], uint32_t &h0, uint32_t &h1, uint32_t &h2, uint32_t &h3, uint32_t &h4) {
    uint32_t a = h0, b = h1, c = h2, d = h3, e = h4;
#pragma unroll
    for (int t = 0; t < 80; ++t) {
        uint32_t wt;
        if (t < 16) {
            wt = w[t];
        } else {
            wt = rotl(w[(t - 3) & 15] ^ w[(t - 8) & 15] ^ w[(t - 14) & 15] ^ w[t & 15], 1);
            w[t & 15] = wt;
        }
        uint32_t f, kc;
        if (t < 20) {
            f = (b & c) | (~b & d);
            kc = 0x5A827999u;
        } else if (t < 40) {
            f = b ^ c ^ d;
            kc = 0x6ED9EBA1u;
        } else if (t < 60) {
            f = (b & c) | (b & d) | (c & d);
            kc = 0x8F1BBCDCu;
        } else {
            f = b ^ c ^ d;
            kc = 0xCA62C1D6u;
        }
        const uint32_t tmp = rotl(a, 5) + f + e + kc + wt;
        e = d;
        d = c;
        c = rotl(b, 30);
        b = a;
        a = tmp;
    }
    h0 += a;
    h1 += b;
    h2 += c;
    h3 += d;
    h4 += e;
}

// SHA-1 of the `len` bytes at `addr` (any length, any alignment): the first two digest words
__device__ __forceinline__ void sha1_any(uintptr_t addr, int64_t len, uint32_t &d0, uint32_t &d1) {
    const uint32_t shift = (uint32_t)(addr & 3u);
    const uint32_t *aligned = reinterpret_cast<const uint32_t *>(addr - shift);
    const int64_t n_blocks = (len + 8) / 64 + 1;
    const int64_t total_words = n_blocks * 16;
    uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
    for (int64_t blk = 0; blk < n_blocks; ++blk) {
        uint32_t w[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) w[i] = padded_word(aligned, shift, len, blk * 16 + i, total_words);
        sha1_rounds(w, h0, h1, h2, h3, h4);
    }
    d0 = h0;
    d1 = h1;
}

// The same for a message whose padded form is one block: 16 message words, no block loop, 32-bit arithmetic.  kDataWords: the
// message words that can hold data or the 0x80 behind it -- len <= 4 * kDataWords - 1; 14 covers every one-block message
// (len <= 55), 3 the byte shingles of up to 11 bytes, whose other words are zero at compile time.  The data lies in at most
// kDataWords + 1 aligned dwords; dword j is loaded only if it holds a byte of the message (the rule of stream_word).
template <int kDataWords>
__device__ __forceinline__ void sha1_one_block(uintptr_t addr, uint32_t len, uint32_t &d0, uint32_t &d1) {
    const uint32_t shift = (uint32_t)(addr & 3u);
    const uint32_t *aligned = reinterpret_cast<const uint32_t *>(addr - shift);
    const uint32_t n_dwords = len ? (shift + len + 3u) >> 2 : 0u;
    uint32_t raw[kDataWords + 1];
#pragma unroll
    for (uint32_t j = 0; j < kDataWords + 1; ++j) raw[j] = j < n_dwords ? aligned[j] : 0u;
    uint32_t w[16];
#pragma unroll
    for (uint32_t k = 0; k < 14; ++k) {
        if (k >= kDataWords) {
            w[k] = 0;
            continue;
        }
        uint32_t v = __builtin_amdgcn_alignbyte(raw[k + 1], raw[k], shift);
        const int32_t valid = (int32_t)len - (int32_t)(4 * k);  // message bytes from this word on
        if (valid <= 0) v = 0;
        else if (valid < 4) v &= (1u << (8 * (uint32_t)valid)) - 1u;
        if (valid >= 0 && valid < 4) v |= 0x80u << (8 * (uint32_t)valid);
        w[k] = __builtin_bswap32(v);
    }
    w[14] = 0;
    w[15] = len * 8u;
    uint32_t h0 = 0x67452301u, h1 = 0xEFCDAB89u, h2 = 0x98BADCFEu, h3 = 0x10325476u, h4 = 0xC3D2E1F0u;
    sha1_rounds(w, h0, h1, h2, h3, h4);
    d0 = h0;
    d1 = h1;
}

// digest bytes are h0, h1, ... big-endian; the reference unpacks the first 4 / 8 of them "<I" / "<Q"
template <typename OutT>
__device__ __forceinline__ OutT digest_value(uint32_t h0, uint32_t h1) {
    const uint32_t lo = __builtin_bswap32(h0);
    if (sizeof(OutT) == 4) return (OutT)lo;
    return (OutT)(((uint64_t)__builtin_bswap32(h1) << 32) | lo);
}

template <typename OutT>
__global__ __launch_bounds__(256) void sha1_tokens_kernel(const uint8_t *__restrict__ bytes,
                                                          const int64_t *__restrict__ offsets, int64_t n_tokens,
                                                          OutT *__restrict__ out) {
    for (int64_t tok = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tok < n_tokens;
         tok += (int64_t)gridDim.x * blockDim.x) {
        const int64_t beg = offsets[tok];
        const int64_t len = offsets[tok + 1] - beg;
        uint32_t h0, h1;
        sha1_any(reinterpret_cast<uintptr_t>(bytes) + (uintptr_t)beg, len, h0, h1);
        out[tok] = digest_value<OutT>(h0, h1);
    }
}

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

// Shingles hashed in place (datasketch_amd/shingle.py is the definition): window t of the corpus is `width` consecutive items
// of one document -- bytes (item_offsets == nullptr), or byte tokens item i = bytes[item_offsets[i] .. item_offsets[i + 1]) --
// or the whole document where it has fewer; set_offsets[d] is the first window of document d.  One thread per window; a wave
// takes `per_wave` consecutive windows (a multiple of 64), 64 per trip.
// Window -> document: the wave finds the owner of its first window once (wave_owner_of) and keeps that document's offsets in
// scalar registers.  A trip whose 64 windows all lie in it -- most trips, where documents are longer than 64 windows -- loads
// no offset at all.  Otherwise the lanes load the offsets of the next 64 documents, one each, and every lane counts by a binary
// search across the lanes (six ds_bpermute) how many of them start at or before its window; a ballot counts those that start
// at or before the next trip's first window, which moves the wave's document on.  A trip that spans more than 64 documents
// takes further such batches.
// kDataWords: 14 = windows of any length; 3 = the launcher knows that no window has more than 11 bytes (sha1_one_block).
template <typename OutT, int kDataWords>
__global__ __launch_bounds__(256) void sha1_windows_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ item_offsets,
                                                           const int64_t *__restrict__ doc_offsets,
                                                           const int64_t *__restrict__ set_offsets, int64_t n_docs,
                                                           int64_t n_windows, int64_t width, int64_t per_wave, OutT *__restrict__ out) {
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
        const uintptr_t addr = reinterpret_cast<uintptr_t>(bytes) + (uintptr_t)beg;
        uint32_t h0, h1;
        if (kDataWords < 14)  // the launcher's choice: byte shingles of at most 4 * kDataWords - 1 bytes
            sha1_one_block<kDataWords>(addr, (uint32_t)len, h0, h1);
        else if (len <= 55)
            sha1_one_block<14>(addr, (uint32_t)len, h0, h1);
        else
            sha1_any(addr, len, h0, h1);
        out[t] = digest_value<OutT>(h0, h1);
    }
}

}  // namespace

int launch_sha1_tokens(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n_tokens,
                       int out_dtype, void *d_out) {
    if (n_tokens == 0) return MHX_OK;
    const int64_t want = (n_tokens + 255) / 256;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 32));
    if (out_dtype == MHX_U32)
        hipLaunchKernelGGL(sha1_tokens_kernel<uint32_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_offsets,
                           n_tokens, static_cast<uint32_t *>(d_out));
    else if (out_dtype == MHX_U64)
        hipLaunchKernelGGL(sha1_tokens_kernel<uint64_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_offsets,
                           n_tokens, static_cast<uint64_t *>(d_out));
    else
        return fail(MHX_ERR_INVALID, "unknown out_dtype %d", out_dtype);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_sha1_windows(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_item_offsets, const int64_t *d_doc_offsets,
                        const int64_t *d_set_offsets, int64_t n_docs, int64_t n_windows, int64_t width, int out_dtype, void *d_out) {
    if (n_windows == 0) return MHX_OK;
    // a capped grid as in launch_sha1_tokens; its waves share the windows out in consecutive runs of whole trips
    const int64_t want = (n_windows + 255) / 256;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 32));
    const int64_t waves = (int64_t)blocks * 4;
    const int64_t per_wave = ((n_windows + waves - 1) / waves + 63) / 64 * 64;
    const bool brief = !d_item_offsets && width <= 11;  // byte shingles of at most 11 bytes: three message words
    if (out_dtype != MHX_U32 && out_dtype != MHX_U64) return fail(MHX_ERR_INVALID, "unknown out_dtype %d", out_dtype);
    auto launch = [&](auto kernel, auto *out) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_item_offsets, d_doc_offsets, d_set_offsets, n_docs,
                           n_windows, width, per_wave, out);
    };
    if (out_dtype == MHX_U32) {
        if (brief) launch(sha1_windows_kernel<uint32_t, 3>, static_cast<uint32_t *>(d_out));
        else launch(sha1_windows_kernel<uint32_t, 14>, static_cast<uint32_t *>(d_out));
    } else {
        if (brief) launch(sha1_windows_kernel<uint64_t, 3>, static_cast<uint64_t *>(d_out));
        else launch(sha1_windows_kernel<uint64_t, 14>, static_cast<uint64_t *>(d_out));
    }
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
