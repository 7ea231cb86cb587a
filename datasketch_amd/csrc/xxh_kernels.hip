// xxh_kernels.hip -- xxHash on the device: the second, cheap token hash beside SHA-1 (sha1_kernels.hip).
//
// datasketch_amd/hashfunc.py is the definition: xxh32_hash32(data) = XXH32(data, seed 0), xxh64_hash64(data) = XXH64(data, seed 0),
// the canonical integer values of the published algorithm (github.com/Cyan4973/xxHash, doc/xxhash_spec.md).  OutT selects the
// function as hash_dtype selects between the two SHA-1 widths: uint32_t runs XXH32, uint64_t runs XXH64.
//
// One thread per token (xxh_tokens_kernel) or per window (xxh_windows_kernel, over the shared walk of window_walk.h).  Loads follow
// the rule of stream_word in sha1_kernels.hip: a token is read as naturally aligned dwords, funnel-shifted (v_alignbyte) to the
// token's alignment, and an aligned dword is loaded only if it holds at least one byte of the token -- nothing before the first
// byte's word, nothing past the last byte's word.
#include "mhx_internal.h"
#include "window_walk.h"

namespace mhx {
namespace {

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) { return __builtin_rotateleft32(x, n); }
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int n) { return __builtin_rotateleft64(x, n); }

// The bytes of a token as a stream of little-endian dwords.  Aligned dword j of the token covers stream bytes [4j - shift,
// 4j - shift + 4); n_dwords of them hold a byte of the token, and only those are loaded.  next() returns stream bytes
// [4k, 4k + 4) for k = 0, 1, ...; bytes at or past the token's end are whatever the last loaded dword holds, or zero.
struct ByteStream {
    const uint32_t *__restrict__ aligned;
    uint32_t shift;
    int64_t n_dwords, j;
    uint32_t cur;

    __device__ __forceinline__ ByteStream(uintptr_t addr, int64_t len) {
        shift = (uint32_t)(addr & 3u);
        aligned = reinterpret_cast<const uint32_t *>(addr - shift);
        n_dwords = len > 0 ? ((int64_t)shift + len + 3) >> 2 : 0;
        cur = n_dwords > 0 ? aligned[0] : 0u;
        j = 1;
    }
    __device__ __forceinline__ uint32_t next() {
        const uint32_t hi = j < n_dwords ? aligned[j] : 0u;
        const uint32_t w = __builtin_amdgcn_alignbyte(hi, cur, shift);
        cur = hi;
        ++j;
        return w;
    }
    __device__ __forceinline__ uint64_t next64() {
        const uint32_t lo = next();
        return ((uint64_t)next() << 32) | lo;
    }
};

constexpr uint32_t kP32_1 = 0x9E3779B1u, kP32_2 = 0x85EBCA77u, kP32_3 = 0xC2B2AE3Du, kP32_4 = 0x27D4EB2Fu, kP32_5 = 0x165667B1u;
constexpr uint64_t kP64_1 = 0x9E3779B185EBCA87ull, kP64_2 = 0xC2B2AE3D27D4EB4Full, kP64_3 = 0x165667B19E3779F9ull,
                   kP64_4 = 0x85EBCA77C2B2AE63ull, kP64_5 = 0x27D4EB2F165667C5ull;

__device__ __forceinline__ uint32_t xxh32_round(uint32_t acc, uint32_t w) { return rotl32(acc + w * kP32_2, 13) * kP32_1; }
__device__ __forceinline__ uint64_t xxh64_round(uint64_t acc, uint64_t w) { return rotl64(acc + w * kP64_2, 31) * kP64_1; }
__device__ __forceinline__ uint64_t xxh64_merge(uint64_t h, uint64_t v) { return (h ^ xxh64_round(0, v)) * kP64_1 + kP64_4; }

// XXH32, seed 0, of the `len` bytes at `addr` (any length, any alignment)
__device__ __forceinline__ uint32_t xxh32_any(uintptr_t addr, int64_t len) {
    ByteStream in(addr, len);
    int64_t left = len;
    uint32_t h;
    if (len >= 16) {
        uint32_t v1 = kP32_1 + kP32_2, v2 = kP32_2, v3 = 0, v4 = 0u - kP32_1;
        for (; left >= 16; left -= 16) {
            v1 = xxh32_round(v1, in.next());
            v2 = xxh32_round(v2, in.next());
            v3 = xxh32_round(v3, in.next());
            v4 = xxh32_round(v4, in.next());
        }
        h = rotl32(v1, 1) + rotl32(v2, 7) + rotl32(v3, 12) + rotl32(v4, 18);
    } else {
        h = kP32_5;
    }
    h += (uint32_t)len;
    for (; left >= 4; left -= 4) h = rotl32(h + in.next() * kP32_3, 17) * kP32_4;
    if (left > 0) {
        uint32_t w = in.next();
        for (; left > 0; --left, w >>= 8) h = rotl32(h + (w & 0xFFu) * kP32_5, 11) * kP32_1;
    }
    h ^= h >> 15;
    h *= kP32_2;
    h ^= h >> 13;
    h *= kP32_3;
    h ^= h >> 16;
    return h;
}

// XXH64, seed 0.  The 64 x 64 -> 64 multiplies by constants are plain C++: the compiler builds them from v_mad_u64_u32 and
// v_mul_lo_u32 (the listing is quoted in DESIGN.md).
__device__ __forceinline__ uint64_t xxh64_any(uintptr_t addr, int64_t len) {
    ByteStream in(addr, len);
    int64_t left = len;
    uint64_t h;
    if (len >= 32) {
        uint64_t v1 = kP64_1 + kP64_2, v2 = kP64_2, v3 = 0, v4 = 0ull - kP64_1;
        for (; left >= 32; left -= 32) {
            v1 = xxh64_round(v1, in.next64());
            v2 = xxh64_round(v2, in.next64());
            v3 = xxh64_round(v3, in.next64());
            v4 = xxh64_round(v4, in.next64());
        }
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xxh64_merge(h, v1);
        h = xxh64_merge(h, v2);
        h = xxh64_merge(h, v3);
        h = xxh64_merge(h, v4);
    } else {
        h = kP64_5;
    }
    h += (uint64_t)len;
    for (; left >= 8; left -= 8) h = rotl64(h ^ xxh64_round(0, in.next64()), 27) * kP64_1 + kP64_4;
    if (left >= 4) {
        h = rotl64(h ^ ((uint64_t)in.next() * kP64_1), 23) * kP64_2 + kP64_3;
        left -= 4;
    }
    if (left > 0) {
        uint32_t w = in.next();
        for (; left > 0; --left, w >>= 8) h = rotl64(h ^ ((uint64_t)(w & 0xFFu) * kP64_5), 11) * kP64_1;
    }
    h ^= h >> 33;
    h *= kP64_2;
    h ^= h >> 29;
    h *= kP64_3;
    h ^= h >> 32;
    return h;
}

template <typename OutT>
__device__ __forceinline__ OutT xxh_of(uintptr_t addr, int64_t len) {
    if (sizeof(OutT) == 4) return (OutT)xxh32_any(addr, len);
    return (OutT)xxh64_any(addr, len);
}

template <typename OutT>
__global__ __launch_bounds__(256) void xxh_tokens_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ offsets,
                                                         int64_t n_tokens, OutT *__restrict__ out) {
    for (int64_t tok = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; tok < n_tokens; tok += (int64_t)gridDim.x * blockDim.x) {
        const int64_t beg = offsets[tok];
        const int64_t len = offsets[tok + 1] - beg;
        out[tok] = xxh_of<OutT>(reinterpret_cast<uintptr_t>(bytes) + (uintptr_t)beg, len);
    }
}

// shingles hashed in place: the walk of window_walk.h with xxHash per window
template <typename OutT>
__global__ __launch_bounds__(256) void xxh_windows_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ item_offsets,
                                                          const int64_t *__restrict__ doc_offsets, const int64_t *__restrict__ set_offsets,
                                                          int64_t n_docs, int64_t n_windows, int64_t width, int64_t per_wave,
                                                          OutT *__restrict__ out) {
    walk_windows<OutT>(bytes, item_offsets, doc_offsets, set_offsets, n_docs, n_windows, width, per_wave, out,
                       [](uintptr_t addr, int64_t len) { return xxh_of<OutT>(addr, len); });
}

}  // namespace

int launch_xxh_tokens(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_offsets, int64_t n_tokens, int out_dtype, void *d_out) {
    if (n_tokens == 0) return MHX_OK;
    const int64_t want = (n_tokens + 255) / 256;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 32));
    if (out_dtype == MHX_U32)
        hipLaunchKernelGGL(xxh_tokens_kernel<uint32_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_offsets, n_tokens,
                           static_cast<uint32_t *>(d_out));
    else if (out_dtype == MHX_U64)
        hipLaunchKernelGGL(xxh_tokens_kernel<uint64_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_offsets, n_tokens,
                           static_cast<uint64_t *>(d_out));
    else
        return fail(MHX_ERR_INVALID, "unknown out_dtype %d", out_dtype);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

int launch_xxh_windows(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_item_offsets, const int64_t *d_doc_offsets,
                       const int64_t *d_set_offsets, int64_t n_docs, int64_t n_windows, int64_t width, int out_dtype, void *d_out) {
    if (n_windows == 0) return MHX_OK;
    // the grid and the shares of launch_sha1_windows: a capped grid whose waves take consecutive runs of whole trips
    const int64_t want = (n_windows + 255) / 256;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)ctx->num_cus * 32));
    const int64_t waves = (int64_t)blocks * 4;
    const int64_t per_wave = ((n_windows + waves - 1) / waves + 63) / 64 * 64;
    if (out_dtype == MHX_U32)
        hipLaunchKernelGGL(xxh_windows_kernel<uint32_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_item_offsets, d_doc_offsets,
                           d_set_offsets, n_docs, n_windows, width, per_wave, static_cast<uint32_t *>(d_out));
    else if (out_dtype == MHX_U64)
        hipLaunchKernelGGL(xxh_windows_kernel<uint64_t>, dim3(blocks), dim3(256), 0, ctx->stream, d_bytes, d_item_offsets, d_doc_offsets,
                           d_set_offsets, n_docs, n_windows, width, per_wave, static_cast<uint64_t *>(d_out));
    else
        return fail(MHX_ERR_INVALID, "unknown out_dtype %d", out_dtype);
    MHX_HIP_CHECK(hipGetLastError());
    return MHX_OK;
}

}  // namespace mhx
