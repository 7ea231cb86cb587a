// mhx_api.hip -- C ABI of libmhx (include/mhx.h): context, device memory, events and the
// host-buffer entry points that stage through device scratch.  Product code: no oracle here.
#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <system_error>
#include <thread>
#include <vector>

#include "mhx_internal.h"

namespace mhx {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

void forgive() { g_last_error.clear(); }

int fail(int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int bbit_slot_size(int b) {  // ref: datasketch/b_bit_minhash.py:147-160
    if (b == 1) return 1;
    if (b == 2) return 2;
    if (b <= 4) return 4;
    if (b <= 8) return 8;
    if (b <= 16) return 16;
    return 32;
}

// ---- device allocations of the library, all through here -------------------------------------------------------
// Normally hipMalloc / hipFree.  In guard mode (environment MHX_GUARD_ALLOC=<align>, or mhx_debug_guard_alloc) every
// allocation is mapped with the HIP virtual-memory API between two reserved, UNMAPPED granules and placed so that its
// last byte (align > 0; rounded up to `align` bytes) or its first byte (align < 0) abuts an unmapped page: a kernel that
// reads or writes past what it was given faults ("Memory access fault by GPU node ...") instead of silently touching a
// neighbour.  tests/test_guard_pages.py runs the GPU parity suite this way.
namespace {
struct GuardRec {
    void *va = nullptr;      // reserved range: [granule unmapped][mapped][granule unmapped]
    size_t reserved = 0, mapped = 0, granule = 0;
    hipMemGenericAllocationHandle_t handle{};
};
std::mutex g_guard_mu;
std::unordered_map<void *, GuardRec> g_guard;
int g_guard_align = -0x7fffffff;  // not read yet
unsigned long long g_guard_count = 0;

int guard_align() {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    if (g_guard_align == -0x7fffffff) {
        const char *e = getenv("MHX_GUARD_ALLOC");
        int a = e ? atoi(e) : 0;
        const int m = a < 0 ? -a : a;
        if (a != 0 && (m > 4096 || (m & (m - 1)))) {  // the rule of mhx_debug_guard_alloc: 0 or +-(a power of two <= 4096)
            fprintf(stderr, "libmhx: MHX_GUARD_ALLOC=%s is not 0 or +-(a power of two <= 4096): guard pages stay off\n", e);
            a = 0;
        }
        g_guard_align = a;
    }
    return g_guard_align;
}

hipError_t guard_malloc(void **p, size_t bytes, int align) {
    int device = 0;
    hipError_t e = hipGetDevice(&device);
    if (e != hipSuccess) return e;
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum);
    if (e != hipSuccess) return e;
    if (gran == 0) return hipErrorNotSupported;
    const size_t a = (size_t)(align < 0 ? -align : align);
    const size_t want = (std::max<size_t>(bytes, 1) + a - 1) / a * a;
    GuardRec r;
    r.granule = gran;
    r.mapped = (want + gran - 1) / gran * gran;
    r.reserved = r.mapped + 2 * gran;
    e = hipMemAddressReserve(&r.va, r.reserved, gran, nullptr, 0);
    if (e != hipSuccess) return e;
    e = hipMemCreate(&r.handle, r.mapped, &prop, 0);
    if (e != hipSuccess) {
        (void)hipMemAddressFree(r.va, r.reserved);
        return e;
    }
    char *lo = static_cast<char *>(r.va) + gran;
    e = hipMemMap(lo, r.mapped, 0, r.handle, 0);
    if (e == hipSuccess) {
        hipMemAccessDesc acc = {};
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(lo, r.mapped, &acc, 1);
        if (e != hipSuccess) (void)hipMemUnmap(lo, r.mapped);
    }
    if (e != hipSuccess) {
        (void)hipMemRelease(r.handle);
        (void)hipMemAddressFree(r.va, r.reserved);
        return e;
    }
    *p = align < 0 ? lo : lo + (r.mapped - want);
    std::lock_guard<std::mutex> lk(g_guard_mu);
    g_guard[*p] = r;
    ++g_guard_count;
    return hipSuccess;
}
}  // namespace

// caller: a block handed out by mhx_dev_alloc (placed with the guard alignment as it is); the library's own blocks --
// staging, tables, rocPRIM temporaries -- keep the 256-byte alignment hipMalloc gives them and that they are carved up by
// Poison mode (environment MHX_POISON_ALLOC=<byte 0..255>, or mhx_debug_poison_alloc): every fresh block is filled with
// that byte before it is handed out.  hipMalloc's memory is zero on a freshly booted board and whatever the previous
// tenant left on a used one; a kernel that reads a word nobody wrote works on the first and faults -- or answers
// wrongly -- on the second, box by box.  0xFF makes such a read a NaN, a -1 or a huge offset, every time.
static int g_poison = -0x7fffffff;  // not read yet
static int poison_byte() {
    std::lock_guard<std::mutex> lk(g_guard_mu);
    if (g_poison == -0x7fffffff) {
        const char *e = getenv("MHX_POISON_ALLOC");
        g_poison = e ? (atoi(e) & 255) : -1;
    }
    return g_poison;
}

hipError_t dev_malloc(void **p, size_t bytes, bool caller) {
    int align = guard_align();
    hipError_t e;
    if (align == 0) {
        e = hipMalloc(p, bytes);
    } else {
        if (!caller) align = align < 0 ? std::min(align, -256) : std::max(align, 256);
        e = guard_malloc(p, bytes, align);
    }
    const int poison = poison_byte();
    if (e == hipSuccess && poison >= 0) {
        e = hipMemset(*p, poison, bytes);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return e;
}

hipError_t dev_free(void *p) {
    if (!p) return hipSuccess;
    GuardRec r;
    {
        std::lock_guard<std::mutex> lk(g_guard_mu);
        const auto it = g_guard.find(p);
        if (it == g_guard.end()) return hipFree(p);
        r = it->second;
        g_guard.erase(it);
    }
    // The physical pages go back, the address range stays reserved for the life of the process: a range handed out again
    // (hipMemAddressFree, then a new reservation at the same address) was read through STALE translations by the next
    // kernels on this driver -- whole inputs seen as zeros or as the previous tenant's bytes (measured: 172 of 407 guard
    // cases wrong with address reuse, none without; profiles/r04_guard_pages.txt).  A freed block thus stays an
    // unmapped hole, which is what a use-after-free should hit anyway.
    hipError_t e = hipDeviceSynchronize();
    char *lo = static_cast<char *>(r.va) + r.granule;
    const hipError_t e1 = hipMemUnmap(lo, r.mapped), e2 = hipMemRelease(r.handle);
    if (e == hipSuccess) e = e1;
    if (e == hipSuccess) e = e2;
    return e;
}

bool guard_mode() { return guard_align() != 0; }

}  // namespace mhx

using mhx::fail;

// ---- what the entry points share: the way in, the argument checks (one wording per condition), host staging ----------
// Every entry starts here: the handle, then the lock of its context -- before any field of the context is read.
#define MHX_ENTER(handle, ctxp)                                      \
    if (!(handle)) return fail(MHX_ERR_INVALID, #handle " is NULL"); \
    MHX_GUARD(ctxp)

#define MHX_TRY(expr)                  \
    do {                               \
        if (int _rc = (expr)) return _rc; \
    } while (0)

namespace {

// An operation has one checked core; `Where` says whether its data pointers are the caller's device buffers (the core only
// enqueues) or host arrays (the core stages them through scratch and blocks until the results are back).
enum Where { kDevice, kHost };
#define MHX_REQUIRE_POINTERS(cond, where) MHX_REQUIRE(cond, "NULL %s pointer", (where) == kHost ? "host" : "device")

// the argument checks that several entries share: one wording each
#define MHX_CHECK_DTYPE(code) MHX_REQUIRE((code) == MHX_U64 || (code) == MHX_U32, "bad " #code " %d", code)
#define MHX_CHECK_B(b) MHX_REQUIRE((b) >= 0 && (b) <= 32, "b must be an integer in [0, 32]")  // (the fused pack + digest entry alone asks for b >= 1)
#define MHX_CHECK_BANDS(bands, r, k) MHX_REQUIRE((bands) > 0 && (r) > 0 && (int64_t)(bands) * (r) <= (k), "bands*r must be in (0, num_perm]")
#define MHX_CHECK_LAYOUT(layout) MHX_REQUIRE((layout) == MHX_ROW_MAJOR || (layout) == MHX_BAND_MAJOR, "bad layout %d", layout)
#define MHX_CHECK_BYTEORDER(order) MHX_REQUIRE((order) == MHX_LITTLE_ENDIAN || (order) == MHX_BIG_ENDIAN, "unknown byte order %d", order)
#define MHX_CHECK_ROWS32(n) MHX_REQUIRE((n) < ((int64_t)1 << 32), "more than 2^32-1 rows per call")  // rows are numbered in 32 bits

int32_t num_blocks(int32_t k, int32_t b) {  // uint64 blocks of a b-bit row
    const int per = 64 / mhx::bbit_slot_size(b);
    return (k + per - 1) / per;
}

// Host staging: a host entry names the pieces it wants in the context's scratch slots, commit() grows the slots, and
// the pieces are addressed from then on.  Pieces of one slot start on 256-byte boundaries, in the order they were asked
// for; a slot is asked to hold exactly the end of its last piece -- in guard mode that is the end of its mapping, so a
// kernel that reads past a staged input faults -- unless ask() names another size.
struct Stage {
    enum Slot { In = 0, Aux = 1, Out = 2, Offsets = 3 };
    struct Piece {
        int slot;
        size_t at, bytes;
    };

    explicit Stage(mhx_ctx *c) : ctx(c) {}

    Piece piece(Slot slot, size_t bytes) {
        const size_t at = (size[slot] + 255) & ~(size_t)255;
        size[slot] = at + bytes;
        asked[slot] = true;
        return Piece{slot, at, bytes};
    }
    // the size the slot is grown to where that is not the end of its last piece: the slack some entries have always
    // carried behind their inputs.  Nothing is known to need it; the sizes are kept as they were.
    void ask(Slot slot, size_t bytes) { size[slot] = bytes; }

    int commit() {
        for (int slot = 0; slot < 5; ++slot)
            if (asked[slot]) MHX_TRY(ctx->ensure_scratch(slot, size[slot]));
        return MHX_OK;
    }
    template <class T>
    T *at(const Piece &p) const { return reinterpret_cast<T *>(static_cast<char *>(ctx->scratch[p.slot]) + p.at); }

    int upload(const Piece &p, const void *host, size_t bytes) const {
        if (bytes) MHX_HIP_CHECK(hipMemcpyAsync(at<void>(p), host, bytes, hipMemcpyHostToDevice, ctx->stream));
        return MHX_OK;
    }
    int upload(const Piece &p, const void *host) const { return upload(p, host, p.bytes); }
    int download(void *host, const Piece &p, size_t bytes) const {
        MHX_HIP_CHECK(hipMemcpyAsync(host, at<void>(p), bytes, hipMemcpyDeviceToHost, ctx->stream));
        return MHX_OK;
    }
    int download(void *host, const Piece &p) const { return download(host, p, p.bytes); }
    int synchronize() const {
        MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return MHX_OK;
    }
    int fetch(void *host, const Piece &p) const {  // the last piece of a call: down, then wait
        MHX_TRY(download(host, p));
        return synchronize();
    }

    mhx_ctx *ctx;
    size_t size[5] = {0, 0, 0, 0, 0};
    bool asked[5] = {false, false, false, false, false};
};

// the plainest host form: one array up (In), the launch, one array back (Out), then wait
template <class Launch>
int through_scratch(mhx_ctx *ctx, const void *in, size_t in_bytes, void *out, size_t out_bytes, Launch launch) {
    Stage s(ctx);
    const auto p_in = s.piece(Stage::In, in_bytes), p_out = s.piece(Stage::Out, out_bytes);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_in, in));
    MHX_TRY(launch(s.at<void>(p_in), s.at<void>(p_out)));
    return s.fetch(out, p_out);
}

}  // namespace

int mhx_ctx::activate() const {
    MHX_HIP_CHECK(hipSetDevice(device));
    return MHX_OK;
}

int mhx_ctx::ensure_scratch(int slot, size_t bytes) {
    // (guard mode: exactly what was asked for, every time, so that the end of the slot is the end of the mapping)
    const bool guard = mhx::guard_mode();
    if (guard ? (bytes == scratch_bytes[slot] && scratch[slot]) : bytes <= scratch_bytes[slot]) return MHX_OK;
    const size_t old = guard ? 0 : scratch_bytes[slot];
    if (scratch[slot]) {
        MHX_HIP_CHECK(hipStreamSynchronize(stream));
        MHX_HIP_CHECK(mhx::dev_free(scratch[slot]));
        scratch[slot] = nullptr;
        scratch_bytes[slot] = 0;
    }
    // grow geometrically so repeated slightly larger calls do not reallocate every time
    size_t want = std::max(bytes, old + old / 2);
    if (!guard) want = (want + 255) & ~(size_t)255;
    hipError_t e = mhx::dev_malloc(&scratch[slot], want);
    if (e != hipSuccess && want != bytes) {
        want = (bytes + 255) & ~(size_t)255;
        e = mhx::dev_malloc(&scratch[slot], want);
    }
    if (e != hipSuccess) {
        scratch[slot] = nullptr;
        return fail(MHX_ERR_OOM, "device scratch allocation of %zu bytes failed: %s", want,
                    hipGetErrorString(e));
    }
    scratch_bytes[slot] = want;
    return MHX_OK;
}

int mhx_ctx::ensure_copy_streams() {
    if (!copy_in) MHX_HIP_CHECK(hipStreamCreateWithFlags(&copy_in, hipStreamNonBlocking));
    if (!copy_out) MHX_HIP_CHECK(hipStreamCreateWithFlags(&copy_out, hipStreamNonBlocking));
    return MHX_OK;
}

int mhx_ctx::ensure_redo(int64_t n_sets) {
    if (n_sets <= redo_capacity && d_redo) return MHX_OK;
    if (d_redo) {
        (void)hipStreamSynchronize(stream);
        (void)mhx::dev_free(d_redo);
        d_redo = nullptr;
        redo_capacity = 0;
    }
    const int64_t cap = std::max<int64_t>(n_sets + n_sets / 4, 1024);
    hipError_t e = mhx::dev_malloc(reinterpret_cast<void **>(&d_redo), (size_t)cap + 64);
    if (e != hipSuccess) {
        d_redo = nullptr;
        return fail(MHX_ERR_OOM, "redo flag allocation of %lld bytes failed: %s", (long long)cap, hipGetErrorString(e));
    }
    redo_capacity = cap;
    return MHX_OK;
}

int mhx_ctx::ensure_work() {
    if (d_work) return MHX_OK;
    hipError_t e = mhx::dev_malloc(reinterpret_cast<void **>(&d_work), mhx::kWorkBytes);
    if (e != hipSuccess) {
        d_work = nullptr;
        return fail(MHX_ERR_OOM, "work counter allocation failed: %s", hipGetErrorString(e));
    }
    // on the kernels' own stream (created non-blocking: nothing orders the null stream before it); word 8, what the last call
    // learned about the corpus, lives across calls
    MHX_HIP_CHECK(hipMemsetAsync(d_work, 0, mhx::kWorkBytes, stream));
    return MHX_OK;
}

extern "C" {

const char *mhx_last_error(void) { return mhx::g_last_error.c_str(); }

const char *mhx_version(void) { return "mhx 0.1.0 (gfx950)"; }

int mhx_device_count(int *count) {
    if (!count) return fail(MHX_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return MHX_OK;  // "no device" is an answer, not an error (ref: minhash.py:38-48)
    }
    *count = n;
    return MHX_OK;
}

int mhx_ctx_create(int device, mhx_ctx **out) {
    if (!out) return fail(MHX_ERR_INVALID, "ctx out pointer is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(MHX_ERR_NO_DEVICE, "no HIP device is available");
    }
    if (device < 0 || device >= n) return fail(MHX_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    MHX_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    MHX_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    mhx_ctx *ctx = new mhx_ctx();
    ctx->device = device;
    ctx->num_cus = ctx->hw_cus = prop.multiProcessorCount;
    ctx->lds_per_block = (int64_t)prop.sharedMemPerBlock;
    ctx->hbm_bytes = (int64_t)prop.totalGlobalMem;
    snprintf(ctx->name, sizeof(ctx->name), "%s (%s)", prop.name, prop.gcnArchName);
    hipError_t e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete ctx;
        return fail(MHX_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return MHX_OK;
}

int mhx_ctx_destroy(mhx_ctx *ctx) {
    if (!ctx) return MHX_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 5; ++i)
        if (ctx->scratch[i]) (void)mhx::dev_free(ctx->scratch[i]);
    if (ctx->d_stats) (void)mhx::dev_free(ctx->d_stats);
    if (ctx->d_redo) (void)mhx::dev_free(ctx->d_redo);
    if (ctx->d_work) (void)mhx::dev_free(ctx->d_work);
    if (ctx->copy_in) (void)hipStreamDestroy(ctx->copy_in);
    if (ctx->copy_out) (void)hipStreamDestroy(ctx->copy_out);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return MHX_OK;
}

int mhx_ctx_synchronize(mhx_ctx *ctx) {
    MHX_ENTER(ctx, ctx);
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

int mhx_ctx_release_scratch(mhx_ctx *ctx) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < 5; ++i) {
        if (ctx->scratch[i]) MHX_HIP_CHECK(mhx::dev_free(ctx->scratch[i]));
        ctx->scratch[i] = nullptr;
        ctx->scratch_bytes[i] = 0;
    }
    if (ctx->d_redo) {
        MHX_HIP_CHECK(mhx::dev_free(ctx->d_redo));
        ctx->d_redo = nullptr;
        ctx->redo_capacity = 0;
    }
    return MHX_OK;
}

int mhx_ctx_device_info(mhx_ctx *ctx, char *name, int name_len, int *cus, int64_t *hbm_bytes) {
    MHX_ENTER(ctx, ctx);
    if (name && name_len > 0) {
        strncpy(name, ctx->name, (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (cus) *cus = ctx->hw_cus;
    if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
    return MHX_OK;
}

// The values an option takes (tests/option_cases.py DOMAIN restates this table; tests/test_option_ledger.py compares the keys): a set of
// values where the text of mhx.h lists them, else a range [lo, hi] -- `step` != 0: 0 or a multiple of step in the range.  `text` is what
// a refusal says after "<key> must be ".
namespace {
struct OptionDomain {
    int n_values;
    int64_t values[9];
    int64_t lo, hi, step;
    const char *text;
};
constexpr int64_t kAny = INT64_MAX;
const OptionDomain kFlag{2, {0, 1}, 0, 0, 0, "0 or 1"};
const OptionDomain kThree{3, {0, 1, 2}, 0, 0, 0, "0, 1 or 2"};
// blocks_per_cu: the launchers that read it size grids of min(work, CUs * n) workgroups of at most 512 threads (minhash_kernels.hip
// launch_typed: 256; weighted_kernels.hip launch_weighted_dense_walk: 64 * waves <= 512 and 256, launch_weighted_csr_walk: 256), and a
// launch takes fewer than 2^32 threads along x: n <= (2^32 - 1) / (512 * CUs), 32767 at the MI355X's 256 CUs (it also fits launch_typed's int)
int64_t max_blocks_per_cu(const mhx_ctx *ctx) { return (int64_t)0xFFFFFFFFll / (512 * (int64_t)std::max(1, ctx->hw_cus)); }
}  // namespace

int mhx_ctx_set_option(mhx_ctx *ctx, const char *key, int64_t value) {
    static const struct {
        const char *key;
        int64_t mhx_ctx::*field;
        OptionDomain domain;
    } options[] = {
        {"minhash.path", &mhx_ctx::opt_minhash_path, kThree},
        {"minhash.split", &mhx_ctx::opt_minhash_split, kThree},
        {"minhash.packed", &mhx_ctx::opt_minhash_packed, kThree},
        {"minhash.ties", &mhx_ctx::opt_minhash_ties, kFlag},
        {"minhash.p3", &mhx_ctx::opt_minhash_p3, kFlag},
        {"minhash.share", &mhx_ctx::opt_minhash_share, kFlag},
        {"minhash.adapt", &mhx_ctx::opt_minhash_adapt, kFlag},
        {"blocks_per_cu", &mhx_ctx::opt_blocks_per_cu, {0, {}, 0, 0, 0, nullptr}},  // 0 .. max_blocks_per_cu(ctx), below
        {"minhash.alias", &mhx_ctx::opt_minhash_alias, {0, {}, -1, kAny, 0, ">= -1"}},
        {"minhash.prefetch", &mhx_ctx::opt_minhash_prefetch, kThree},
        {"weighted.path", &mhx_ctx::opt_weighted_path, kThree},
        {"weighted.direct", &mhx_ctx::opt_weighted_direct, {0, {}, 0, 1000, 0, "in [0, 1000] (per mille of the columns)"}},
        {"weighted.split", &mhx_ctx::opt_weighted_split, kFlag},
        {"weighted.tail", &mhx_ctx::opt_weighted_tail, {0, {}, 0, 5, 0, "in [0, 5]"}},
        {"weighted.debug", &mhx_ctx::opt_weighted_debug, {5, {0, 1, 2, 4, 8}, 0, 0, 0, "0, 1, 2, 4 or 8"}},
        {"weighted.kernel", &mhx_ctx::opt_weighted_kernel, kThree},
        {"weighted.plan", &mhx_ctx::opt_weighted_plan, kFlag},
        {"weighted.rescue", &mhx_ctx::opt_weighted_rescue, {0, {}, -kAny - 1, 64, 0, "<= 64 (the lanes of a wave; < 0 = never)"}},
        {"weighted.min_dim", &mhx_ctx::opt_weighted_min_dim, {0, {}, 0, 4096, 4, "0 or a multiple of 4 in [4, 4096]"}},
        {"host.chunk_bytes", &mhx_ctx::opt_host_chunk_bytes, {0, {}, -kAny - 1, kAny, 0, "an int64"}},
        {"lsh.sort_bits", &mhx_ctx::opt_lsh_sort_bits, {0, {}, 0, 64, 0, "in [0, 64]"}},
        {"lsh.gather", &mhx_ctx::opt_lsh_gather, kFlag},
        {"lsh.sort", &mhx_ctx::opt_lsh_sort, kFlag},
        {"lsh.levels", &mhx_ctx::opt_lsh_levels, {2, {0, 2}, 0, 0, 0, "0 or 2"}},
        {"lsh.chunk", &mhx_ctx::opt_lsh_chunk, {2, {0, 8}, 0, 0, 0, "0 or 8"}},
        {"lsh.team", &mhx_ctx::opt_lsh_team, {3, {0, 256, 1024}, 0, 0, 0, "0, 256 or 1024"}},
        {"lsh.bigbins", &mhx_ctx::opt_lsh_bigbins, kThree},
        {"pack.fused", &mhx_ctx::opt_pack_fused, kFlag},
        {"weighted.refill", &mhx_ctx::opt_weighted_refill, {9, {0, 1, 2, 3, 5, 6, 8, 9, 13}, 0, 0, 0, "0, 1, 2, 3, 5, 6, 8, 9 or 13"}},
        {"lsh.prehash", &mhx_ctx::opt_lsh_prehash, kFlag},
        {"lsh.merge_items", &mhx_ctx::opt_lsh_merge_items, {3, {0, 8, 16}, 0, 0, 0, "0, 8 or 16"}},
        {"hll.split_tokens", &mhx_ctx::opt_hll_split_tokens, {0, {}, 0, kAny, 0, ">= 0"}},
        {"bloom.lanes", &mhx_ctx::opt_bloom_lanes, {3, {0, 1, 16}, 0, 0, 0, "0, 1 or 16"}},
        {"jaccard.topk_path", &mhx_ctx::opt_jaccard_topk_path, kThree},
        {"jaccard.topk_segments", &mhx_ctx::opt_jaccard_topk_segments, {0, {}, 0, kAny, 0, ">= 0"}},
        {"debug.cus", &mhx_ctx::opt_debug_cus, {0, {}, 0, 0, 0, nullptr}},  // 0 .. the device's CU count, below
        {"overlap.bins", &mhx_ctx::opt_overlap_bins, kThree},
    };
    if (!ctx || !key) return fail(MHX_ERR_INVALID, "ctx/key is NULL");
    MHX_GUARD(ctx);
    for (const auto &o : options) {
        if (strcmp(key, o.key)) continue;
        const OptionDomain &d = o.domain;
        if (o.field == &mhx_ctx::opt_debug_cus) {
            MHX_REQUIRE(value >= 0 && value <= ctx->hw_cus, "debug.cus must be 0 (the device's %d CUs) or in [1, %d], got %lld", ctx->hw_cus, ctx->hw_cus,
                        (long long)value);
        } else if (o.field == &mhx_ctx::opt_blocks_per_cu) {
            MHX_REQUIRE(value >= 0 && value <= max_blocks_per_cu(ctx), "blocks_per_cu must be in [0, %lld] (a grid of this device's %d CUs x 512 threads stays below 2^32), got %lld",
                        (long long)max_blocks_per_cu(ctx), ctx->hw_cus, (long long)value);
        } else {
            bool ok = false;
            for (int i = 0; i < d.n_values; ++i) ok = ok || value == d.values[i];
            if (!d.n_values) ok = value >= d.lo && value <= d.hi && (d.step == 0 || value % d.step == 0);
            MHX_REQUIRE(ok, "%s must be %s", o.key, d.text);
        }
        ctx->*o.field = value;
        if (o.field == &mhx_ctx::opt_debug_cus) ctx->num_cus = value ? (int)value : ctx->hw_cus;
        return MHX_OK;
    }
    return fail(MHX_ERR_INVALID, "unknown option '%s'", key);
}

// What the previous MinHash call on this context learned about the corpus (d_work word 8, written by the last launch of every
// call and read by the first launch of the next one): 0 = one-candidate proof first, 1 = most sets defeat it (tie-tolerant proof
// first), 2 = heavily repeated tokens.  Timings depend on it, results never; reset = 1 puts it back to 0 (a fresh context).
int mhx_ctx_minhash_mode(mhx_ctx *ctx, int reset, int *mode) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(ctx->activate());
    MHX_TRY(ctx->ensure_work());
    unsigned int word = 0;
    MHX_HIP_CHECK(hipMemcpyAsync(&word, ctx->d_work + 8, sizeof(word), hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (mode) *mode = (int)word;
    if (reset) MHX_HIP_CHECK(hipMemsetAsync(ctx->d_work + 8, 0, sizeof(word), ctx->stream));
    return MHX_OK;
}

// Which sets of the last MinHash call left the fast path (see mhx.h).  The flags are the launches' own hand-over bytes: the sieve
// launch writes 0 / 1 for every set, the second launch turns the 1 of a set it could not certify either into 2.
int mhx_ctx_minhash_flags(mhx_ctx *ctx, int64_t n_sets, uint8_t *flags) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(ctx->activate());
    MHX_REQUIRE(n_sets >= 0 && (flags || n_sets == 0), "NULL flags");
    if (ctx->redo_sets != n_sets || (n_sets > 0 && !ctx->d_redo))
        return fail(MHX_ERR_INVALID, "the last MinHash call on this context kept flags for %lld sets, not %lld (one huge set split over waves and "
                    "minhash.path != 0 keep none)", (long long)ctx->redo_sets, (long long)n_sets);
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (n_sets > 0) MHX_HIP_CHECK(hipMemcpy(flags, ctx->d_redo, (size_t)n_sets, hipMemcpyDeviceToHost));
    return MHX_OK;
}

int mhx_ctx_counters(mhx_ctx *ctx, int enable, uint64_t out[MHX_NUM_COUNTERS]) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (out) {
        for (int i = 0; i < MHX_NUM_COUNTERS; ++i) out[i] = 0;
        if (ctx->d_stats)
            MHX_HIP_CHECK(hipMemcpy(out, ctx->d_stats, sizeof(uint64_t) * MHX_NUM_COUNTERS, hipMemcpyDeviceToHost));
    }
    if (enable && !ctx->d_stats) {
        hipError_t e = mhx::dev_malloc(reinterpret_cast<void **>(&ctx->d_stats), sizeof(uint64_t) * MHX_NUM_COUNTERS);
        if (e != hipSuccess) {
            ctx->d_stats = nullptr;
            return fail(MHX_ERR_OOM, "counter allocation failed: %s", hipGetErrorString(e));
        }
    }
    if (!enable && ctx->d_stats) {
        MHX_HIP_CHECK(mhx::dev_free(ctx->d_stats));
        ctx->d_stats = nullptr;
    }
    // on the kernels' own stream, as ensure_work()'s: the launches that count are ordered behind the reset by the stream, not by
    // whether a null-stream memset happens to have finished when it returns (tests/stream_order_cases.py: reset, call, read)
    if (ctx->d_stats) MHX_HIP_CHECK(hipMemsetAsync(ctx->d_stats, 0, sizeof(uint64_t) * MHX_NUM_COUNTERS, ctx->stream));
    return MHX_OK;
}

// ---- device memory -------------------------------------------------------------------------
int mhx_debug_guard_alloc(int align, int64_t *granule, int64_t *live) {
    if (align != 0 && (align < -4096 || align > 4096 || ((align < 0 ? -align : align) & ((align < 0 ? -align : align) - 1))))
        return fail(MHX_ERR_INVALID, "guard alignment must be 0 (off) or +-(a power of two <= 4096), got %d", align);
    (void)mhx::guard_mode();  // read the environment first: this call overrides it
    {
        std::lock_guard<std::mutex> lk(mhx::g_guard_mu);
        mhx::g_guard_align = align;
        if (live) *live = (int64_t)mhx::g_guard.size();
    }
    if (granule) {
        *granule = 0;
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            return align ? fail(MHX_ERR_NO_DEVICE, "no HIP device is available") : MHX_OK;
        }
        int device = 0;
        MHX_HIP_CHECK(hipGetDevice(&device));
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned;
        prop.location.type = hipMemLocationTypeDevice;
        prop.location.id = device;
        size_t g = 0;
        hipError_t e = hipMemGetAllocationGranularity(&g, &prop, hipMemAllocationGranularityMinimum);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(MHX_ERR_UNSUPPORTED, "hipMemGetAllocationGranularity failed: %s", hipGetErrorString(e));
        }
        *granule = (int64_t)g;
    }
    return MHX_OK;
}

int mhx_debug_poison_alloc(int byte_value) {
    if (byte_value < -1 || byte_value > 255) return fail(MHX_ERR_INVALID, "poison byte must be -1 (off) or 0..255, got %d", byte_value);
    (void)mhx::poison_byte();  // read the environment first: this call overrides it
    std::lock_guard<std::mutex> lk(mhx::g_guard_mu);
    mhx::g_poison = byte_value;
    return MHX_OK;
}

int mhx_dev_alloc(mhx_ctx *ctx, size_t bytes, void **dptr) {
    if (!ctx || !dptr) return fail(MHX_ERR_INVALID, "ctx/dptr is NULL");
    MHX_GUARD(ctx);
    *dptr = nullptr;
    MHX_TRY(ctx->activate());
    hipError_t e = mhx::dev_malloc(dptr, bytes ? bytes : 1, true);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MHX_ERR_OOM, "device allocation of %zu bytes failed: %s", bytes, hipGetErrorString(e));
    }
    return MHX_OK;
}

int mhx_dev_free(mhx_ctx *ctx, void *dptr) {
    MHX_ENTER(ctx, ctx);
    if (!dptr) return MHX_OK;
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    MHX_HIP_CHECK(mhx::dev_free(dptr));
    return MHX_OK;
}

int mhx_host_alloc(mhx_ctx *ctx, size_t bytes, void **ptr) {
    if (!ctx || !ptr) return fail(MHX_ERR_INVALID, "ctx/ptr is NULL");
    MHX_GUARD(ctx);
    *ptr = nullptr;
    MHX_TRY(ctx->activate());
    hipError_t e = hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(MHX_ERR_OOM, "hipHostMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    return MHX_OK;
}

int mhx_host_free(mhx_ctx *ctx, void *ptr) {
    if (!ptr) return MHX_OK;
    if (!ctx) {  // the context that allocated it is gone (and with it every transfer that could still use the block)
        MHX_HIP_CHECK(hipHostFree(ptr));
        return MHX_OK;
    }
    MHX_GUARD(ctx);
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->copy_in) MHX_HIP_CHECK(hipStreamSynchronize(ctx->copy_in));
    MHX_HIP_CHECK(hipHostFree(ptr));
    return MHX_OK;
}

int mhx_memcpy_h2d(mhx_ctx *ctx, void *dst, const void *src, size_t bytes) {
    MHX_ENTER(ctx, ctx);
    if (!bytes) return MHX_OK;
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

int mhx_memcpy_d2h(mhx_ctx *ctx, void *dst, const void *src, size_t bytes) {
    MHX_ENTER(ctx, ctx);
    if (!bytes) return MHX_OK;
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return MHX_OK;
}

int mhx_memcpy_d2d(mhx_ctx *ctx, void *dst, const void *src, size_t bytes) {
    MHX_ENTER(ctx, ctx);
    if (!bytes) return MHX_OK;
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return MHX_OK;
}

int mhx_memset_dev(mhx_ctx *ctx, void *dst, int byte_value, size_t bytes) {
    MHX_ENTER(ctx, ctx);
    if (!bytes) return MHX_OK;
    MHX_TRY(ctx->activate());
    MHX_HIP_CHECK(hipMemsetAsync(dst, byte_value, bytes, ctx->stream));
    return MHX_OK;
}

// ---- events --------------------------------------------------------------------------------
int mhx_event_create(mhx_ctx *ctx, mhx_event **ev) {
    if (!ctx || !ev) return fail(MHX_ERR_INVALID, "ctx/ev is NULL");
    MHX_GUARD(ctx);
    MHX_TRY(ctx->activate());
    mhx_event *e = new mhx_event();
    e->ctx = ctx;
    hipError_t err = hipEventCreate(&e->ev);
    if (err != hipSuccess) {
        delete e;
        return fail(MHX_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(err));
    }
    *ev = e;
    return MHX_OK;
}

int mhx_event_record(mhx_event *ev) {
    if (!ev) return fail(MHX_ERR_INVALID, "event is NULL");
    MHX_GUARD(ev->ctx);
    MHX_HIP_CHECK(hipEventRecord(ev->ev, ev->ctx->stream));
    return MHX_OK;
}

int mhx_event_synchronize(mhx_event *ev) {
    if (!ev) return fail(MHX_ERR_INVALID, "event is NULL");
    MHX_HIP_CHECK(hipEventSynchronize(ev->ev));
    return MHX_OK;
}

int mhx_event_elapsed_ms(mhx_event *start, mhx_event *stop, float *ms) {
    if (!start || !stop || !ms) return fail(MHX_ERR_INVALID, "event/ms is NULL");
    MHX_HIP_CHECK(hipEventElapsedTime(ms, start->ev, stop->ev));
    return MHX_OK;
}

int mhx_event_destroy(mhx_event *ev) {
    if (!ev) return MHX_OK;
    (void)hipEventDestroy(ev->ev);
    delete ev;
    return MHX_OK;
}

// ---- MinHash -------------------------------------------------------------------------------
int mhx_perm_create(mhx_ctx *ctx, const uint64_t *a, const uint64_t *b, int32_t num_perm,
                    mhx_perm **out) {
    if (!ctx || !a || !b || !out) return fail(MHX_ERR_INVALID, "NULL argument");
    MHX_GUARD(ctx);
    MHX_REQUIRE(num_perm > 0, "num_perm must be positive, got %d", num_perm);
    MHX_TRY(ctx->activate());
    mhx_perm *p = new mhx_perm();
    p->ctx = ctx;
    p->num_perm = num_perm;
    const size_t bytes = sizeof(uint64_t) * (size_t)num_perm;
    hipError_t e = mhx::dev_malloc((void **)&p->d_a, 2 * bytes);
    if (e != hipSuccess) {
        delete p;
        return fail(MHX_ERR_OOM, "hipMalloc for permutations failed: %s", hipGetErrorString(e));
    }
    p->d_b = p->d_a + num_perm;
    e = hipMemcpyAsync(p->d_a, a, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->d_b, b, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)mhx::dev_free(p->d_a);
        delete p;
        return fail(MHX_ERR_HIP, "uploading permutations failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return MHX_OK;
}

int mhx_perm_destroy(mhx_perm *perm) {
    if (!perm) return MHX_OK;
    MHX_GUARD(perm->ctx);
    (void)hipSetDevice(perm->ctx->device);
    (void)hipStreamSynchronize(perm->ctx->stream);
    (void)mhx::dev_free(perm->d_a);
    delete perm;
    return MHX_OK;
}

static int check_bulk(int64_t n_sets, int hv_dtype, int out_dtype) {
    MHX_REQUIRE(n_sets >= 0, "n_sets must be >= 0");
    MHX_CHECK_DTYPE(hv_dtype);
    MHX_CHECK_DTYPE(out_dtype);
    return MHX_OK;
}

int mhx_minhash_bulk_dev(mhx_perm *perm, const void *d_hv, int hv_dtype, const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets,
                         int64_t total_tokens, const uint64_t *d_init, int64_t init_stride, void *d_out, int out_dtype) {
    MHX_ENTER(perm, perm->ctx);
    MHX_TRY(check_bulk(n_sets, hv_dtype, out_dtype));
    MHX_REQUIRE(d_offsets || fixed_len >= 0, "fixed_len must be >= 0 when offsets is NULL");
    MHX_REQUIRE(init_stride == 0 || init_stride >= perm->num_perm, "init_stride must be 0 or >= num_perm");
    MHX_REQUIRE(total_tokens >= 0, "total_tokens must be >= 0");
    if (n_sets == 0) return MHX_OK;
    MHX_REQUIRE(d_out, "d_out is NULL");
    MHX_REQUIRE(d_hv || total_tokens == 0, "d_hv is NULL");
    MHX_TRY(perm->ctx->activate());
    return mhx::launch_minhash_bulk(perm, d_hv, hv_dtype, d_offsets, fixed_len, n_sets, total_tokens,
                                    d_init, init_stride, d_out, out_dtype);
}

extern "C++" {
namespace {

constexpr int kNoSecondThread = -1000;  // internal: bulk_pipelined could not start its download thread

// One piece of a pipelined host call: sets [s0, s1) whose tokens are hv[t0, t1).
struct Piece {
    int64_t s0, s1, t0, t1;
};

// Cut the corpus into pieces of about `target` bytes (tokens in + signature rows out); a piece is
// at least one set, so one enormous set still becomes one piece.
std::vector<Piece> cut_pieces(const int64_t *offsets, int64_t fixed_len, int64_t n_sets, int64_t k, int64_t target,
                              int64_t tok_size = 8, int64_t out_size = 8) {
    std::vector<Piece> pieces;
    int64_t s0 = 0;
    while (s0 < n_sets) {
        int64_t s1;
        if (offsets) {
            // largest s1 with tok_size*(offsets[s1]-offsets[s0]) + out_size*k*(s1-s0) <= target: the cost is increasing in s1
            int64_t lo = s0 + 1, hi = n_sets;
            while (lo < hi) {
                const int64_t mid = lo + (hi - lo + 1) / 2;
                const int64_t cost = tok_size * (offsets[mid] - offsets[s0]) + out_size * k * (mid - s0);
                if (cost <= target) lo = mid; else hi = mid - 1;
            }
            s1 = lo;
        } else {
            const int64_t per_set = tok_size * fixed_len + out_size * k;
            s1 = std::min(n_sets, s0 + std::max<int64_t>(1, target / per_set));
        }
        Piece p;
        p.s0 = s0;
        p.s1 = s1;
        p.t0 = offsets ? offsets[s0] : s0 * fixed_len;
        p.t1 = offsets ? offsets[s1] : s1 * fixed_len;
        pieces.push_back(p);
        s0 = s1;
    }
    return pieces;
}

// Host corpus -> host signatures with the three legs overlapped: this thread uploads piece i+1
// (copy_in stream) while the kernels of piece i run (ctx->stream) and a second thread downloads the
// rows of piece i-1 (copy_out stream).  PCIe is full duplex, so a large call costs about
// max(upload, download) instead of their sum.  Device buffers hold the whole corpus (no reuse
// hazards); offsets stay absolute, so a piece is just a window of sets.
int bulk_pipelined(mhx_perm *perm, const char *hv, int hv_dtype, const int64_t *offsets, int64_t fixed_len, int64_t n_sets,
                   const uint64_t *init, int64_t init_stride, char *out, int out_dtype, char *d_hv, int64_t *d_off,
                   uint64_t *d_init, char *d_out, const std::vector<Piece> &pieces) {
    mhx_ctx *ctx = perm->ctx;
    const int64_t k = perm->num_perm;
    const size_t ts = hv_dtype == MHX_U32 ? 4 : 8, os = out_dtype == MHX_U32 ? 4 : 8;  // element sizes
    if (int rc = ctx->ensure_copy_streams()) return rc;
    const size_t n_pieces = pieces.size();
    std::vector<hipEvent_t> uploaded(n_pieces, nullptr), computed(n_pieces, nullptr);
    auto destroy_events = [&]() {
        for (hipEvent_t e : uploaded) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : computed) if (e) (void)hipEventDestroy(e);
    };
    for (size_t i = 0; i < n_pieces; ++i) {
        hipError_t e = hipEventCreateWithFlags(&uploaded[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&computed[i], hipEventDisableTiming);
        if (e != hipSuccess) {
            destroy_events();
            return fail(MHX_ERR_HIP, "hipEventCreate failed: %s", hipGetErrorString(e));
        }
    }
    // the download thread may only wait on an event after this thread has recorded it
    std::mutex mu;
    std::condition_variable cv;
    size_t recorded = 0;
    bool stop = false;
    hipError_t down_err = hipSuccess;
    auto download = [&]() {
        hipError_t e = hipSetDevice(ctx->device);
        for (size_t i = 0; i < n_pieces && e == hipSuccess; ++i) {
            {
                std::unique_lock<std::mutex> lock(mu);
                cv.wait(lock, [&] { return recorded > i || stop; });
                if (recorded <= i) break;  // stopped before this piece was launched
            }
            const Piece &p = pieces[i];
            e = hipStreamWaitEvent(ctx->copy_out, computed[i], 0);
            if (e == hipSuccess)
                e = hipMemcpyAsync(out + os * (size_t)(p.s0 * k), d_out + os * (size_t)(p.s0 * k), os * (size_t)((p.s1 - p.s0) * k),
                                   hipMemcpyDeviceToHost, ctx->copy_out);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->copy_out);
        down_err = e;
    };
    std::thread downloader;
    try {
        downloader = std::thread(download);
    } catch (const std::system_error &) {  // no thread to be had: the caller runs the call in one piece
        destroy_events();
        return kNoSecondThread;
    }
    auto finish = [&](int rc) -> int {
        {
            std::lock_guard<std::mutex> lock(mu);
            stop = true;
        }
        cv.notify_all();
        downloader.join();
        (void)hipStreamSynchronize(ctx->copy_in);
        (void)hipStreamSynchronize(ctx->stream);
        destroy_events();
        if (rc) return rc;
        if (down_err != hipSuccess) return fail(MHX_ERR_HIP, "downloading signatures failed: %s", hipGetErrorString(down_err));
        return MHX_OK;
    };
    for (size_t i = 0; i < n_pieces; ++i) {  // offsets stay absolute: hv[t] sits at d_hv[t]
        const Piece &p = pieces[i];
        hipError_t e = hipSuccess;
        if (p.t1 > p.t0)
            e = hipMemcpyAsync(d_hv + ts * (size_t)p.t0, hv + ts * (size_t)p.t0, ts * (size_t)(p.t1 - p.t0), hipMemcpyHostToDevice,
                               ctx->copy_in);
        if (e == hipSuccess && init && init_stride)
            e = hipMemcpyAsync(d_init + p.s0 * init_stride, init + p.s0 * init_stride,
                               sizeof(uint64_t) * (size_t)((p.s1 - p.s0) * init_stride), hipMemcpyHostToDevice, ctx->copy_in);
        if (e == hipSuccess) e = hipEventRecord(uploaded[i], ctx->copy_in);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, uploaded[i], 0);
        if (e != hipSuccess) return finish(fail(MHX_ERR_HIP, "uploading tokens failed: %s", hipGetErrorString(e)));
        const char *piece_hv = offsets ? d_hv : d_hv + ts * (size_t)p.t0;
        const int64_t *piece_off = offsets ? d_off + p.s0 : nullptr;
        const uint64_t *piece_init = !init ? nullptr : (init_stride ? d_init + p.s0 * init_stride : d_init);
        const int64_t first = offsets ? p.t0 : 0, last = offsets ? p.t1 : p.t1 - p.t0;
        if (int rc = mhx::launch_minhash_bulk(perm, piece_hv, hv_dtype, piece_off, fixed_len, p.s1 - p.s0, last,
                                              piece_init, init_stride, d_out + os * (size_t)(p.s0 * k), out_dtype, first))
            return finish(rc);
        e = hipEventRecord(computed[i], ctx->stream);
        if (e != hipSuccess) return finish(fail(MHX_ERR_HIP, "hipEventRecord failed: %s", hipGetErrorString(e)));
        {
            std::lock_guard<std::mutex> lock(mu);
            recorded = i + 1;
        }
        cv.notify_all();
    }
    return finish(MHX_OK);
}

}  // namespace
}  // extern "C++"

int mhx_minhash_bulk_typed(mhx_perm *perm, const void *hv, int hv_dtype, const int64_t *offsets, int64_t fixed_len,
                           int64_t n_sets, const uint64_t *init, int64_t init_stride, void *out, int out_dtype) {
    MHX_ENTER(perm, perm->ctx);
    MHX_TRY(check_bulk(n_sets, hv_dtype, out_dtype));
    if (n_sets == 0) return MHX_OK;
    MHX_REQUIRE(out, "out is NULL");
    MHX_REQUIRE(offsets || fixed_len >= 0, "fixed_len must be >= 0 when offsets is NULL");
    mhx_ctx *ctx = perm->ctx;
    MHX_TRY(ctx->activate());
    const int64_t k = perm->num_perm;
    const size_t ts = hv_dtype == MHX_U32 ? 4 : 8, os = out_dtype == MHX_U32 ? 4 : 8;
    int64_t total = 0;
    if (offsets) {
        MHX_REQUIRE(offsets[0] >= 0, "offsets[0] must be >= 0");
        for (int64_t i = 0; i < n_sets; ++i)
            MHX_REQUIRE(offsets[i + 1] >= offsets[i], "offsets must be non-decreasing (row %lld)", (long long)i);
        total = offsets[n_sets];
    } else {
        total = n_sets * fixed_len;
    }
    MHX_REQUIRE(hv || total == 0, "hv is NULL");
    const size_t init_bytes = init ? sizeof(uint64_t) * (size_t)(init_stride ? n_sets * init_stride : k) : 0;
    Stage s(ctx);
    const auto p_hv = s.piece(Stage::In, ts * (size_t)total);
    const auto p_off = s.piece(Stage::Aux, offsets ? sizeof(int64_t) * (size_t)(n_sets + 1) : 0);
    const auto p_init = s.piece(Stage::Aux, init_bytes);
    const auto p_out = s.piece(Stage::Out, os * (size_t)(n_sets * k));
    s.ask(Stage::In, p_hv.bytes + 256);
    s.ask(Stage::Aux, p_off.bytes + init_bytes + 512);
    MHX_TRY(s.commit());
    char *d_hv = s.at<char>(p_hv), *d_out = s.at<char>(p_out);
    int64_t *d_off = offsets ? s.at<int64_t>(p_off) : nullptr;
    uint64_t *d_init = init ? s.at<uint64_t>(p_init) : nullptr;

    // large corpora: upload, kernels and download overlap piece by piece
    const int64_t chunk_opt = ctx->opt_host_chunk_bytes;
    const int64_t target = chunk_opt > 0 ? chunk_opt : (int64_t)96 << 20;
    const bool pipelined = chunk_opt > 0 || (chunk_opt == 0 && p_hv.bytes + p_out.bytes > ((size_t)256 << 20));
    if (pipelined) {
        const std::vector<Piece> pieces = cut_pieces(offsets, fixed_len, n_sets, k, target, (int64_t)ts, (int64_t)os);
        if (pieces.size() > 1) {
            // small operands first, on the compute stream: every piece's kernels are ordered after them
            MHX_TRY(s.upload(p_off, offsets));
            if (init && !init_stride) MHX_TRY(s.upload(p_init, init));
            const int rc = bulk_pipelined(perm, (const char *)hv, hv_dtype, offsets, fixed_len, n_sets, init, init_stride,
                                          (char *)out, out_dtype, d_hv, d_off, d_init, d_out, pieces);
            if (rc != kNoSecondThread) return rc;
        }
    }
    MHX_TRY(s.upload(p_hv, hv));
    MHX_TRY(s.upload(p_off, offsets));
    MHX_TRY(s.upload(p_init, init));
    MHX_TRY(mhx::launch_minhash_bulk(perm, d_hv, hv_dtype, d_off, fixed_len, n_sets, total, d_init, init_stride, d_out, out_dtype));
    return s.fetch(out, p_out);
}

int mhx_minhash_bulk(mhx_perm *perm, const uint64_t *hv, const int64_t *offsets, int64_t fixed_len,
                     int64_t n_sets, const uint64_t *init, int64_t init_stride, uint64_t *out) {
    return mhx_minhash_bulk_typed(perm, hv, MHX_U64, offsets, fixed_len, n_sets, init, init_stride, out, MHX_U64);
}

// ---- token hashing (sha1_hash32 / sha1_hash64 of byte tokens) ----------------------------------
static int check_sha1(int64_t n_tokens, int out_dtype) {
    MHX_REQUIRE(n_tokens >= 0, "n_tokens must be >= 0");
    MHX_CHECK_DTYPE(out_dtype);
    return MHX_OK;
}

// the token hash of a text source (MHX_HASH_*): checked in the entry, dispatched on in Source::hash() and nowhere else
#define MHX_CHECK_HASH_KIND(kind) MHX_REQUIRE((kind) == MHX_HASH_SHA1 || (kind) == MHX_HASH_XXH, "unknown hash_kind %d", kind)

int mhx_sha1_tokens_dev(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_byte_offsets, int64_t n_tokens, int out_dtype, void *d_out) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_sha1(n_tokens, out_dtype));
    if (n_tokens == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_byte_offsets && d_out, kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_sha1_tokens(ctx, d_bytes, d_byte_offsets, n_tokens, out_dtype, d_out);
}

extern "C++" {
namespace {

// ---- text to sketches: a corpus becomes sets of hashes (a source), the hashes become a sketch (a sink) ------------------------
// The three sources -- Tokens here, Windows and Words further down -- have the same members, so that a sink is a function
// template over its source and neither knows the other:
//   kNoOut                   what a NULL `out` answers
//   check_sizes(), n_sets()  the scalar arguments; a corpus of no sets is done before any array is looked at
//   check_arrays()           the host arrays, checked
//   stage(ctx)               the corpus into scratch, a Stage of the source's own: bytes -> In (alone), every offset array -> Offsets
//   max_hashes()             a bound on the number of hashes, known once staged: what the sink sizes its hash piece by
//   reserve(s)               Aux pieces of the source's own in the SINK's Stage, behind init | hashes (one Stage per slot and
//                            call: a slot that grows is reallocated)
//   hash(s, dtype, d_hv)     the launches that fill d_hv; d_sets and n_hashes hold from then on
//   host_sets()              the set offsets on the host, from hash() on: a sink that needs the size of a set reads it here

// The slack behind the staged bytes of a Tokens source.  The SHA-1 entries keep the 256 bytes they have always had; the xxHash
// kernels get none, so that the byte slot ends with the last token and tests/xxh_guard_cases.py holds xxh_tokens_kernel to the
// last byte of an exact-size allocation.
constexpr size_t tokens_in_slack(int hash_kind) { return hash_kind == MHX_HASH_XXH ? 0 : 256; }

// packed byte tokens: token i is bytes[byte_offsets[i] .. byte_offsets[i+1]], set j owns tokens set_offsets[j] .. set_offsets[j+1]
// (set_offsets NULL: the tokens alone, for mhx_sha1_tokens).  Offsets: byte offsets | set offsets.
struct Tokens {
    static constexpr const char *kNoOut = "out/set_offsets is NULL";
    const uint8_t *bytes;
    const int64_t *byte_offsets;
    int64_t n_tokens;
    const int64_t *set_offsets;
    int64_t n;
    size_t aux_slack;  // the slack reserve() leaves behind the hashes (see Stage::ask): its entry says how much it has always carried
    int hash_kind = MHX_HASH_SHA1;
    size_t in_slack = 256;  // what stage() leaves behind the bytes: 256 is what the SHA-1 entries have always carried (see tokens_in_slack)
    uint8_t *d_bytes = nullptr;
    int64_t *d_boffs = nullptr, *d_sets = nullptr;
    int64_t n_hashes = 0;

    int check_sizes() const {
        MHX_REQUIRE(n >= 0 && n_tokens >= 0, "n_sets and n_tokens must be >= 0");
        return MHX_OK;
    }
    int64_t n_sets() const { return n; }
    int64_t max_hashes() const { return n_tokens; }
    const int64_t *host_sets() const { return set_offsets; }

    int check_tokens() const {
        MHX_REQUIRE(byte_offsets, "byte_offsets is NULL");
        MHX_REQUIRE(byte_offsets[0] == 0, "byte_offsets[0] must be 0");
        for (int64_t i = 0; i < n_tokens; ++i)
            MHX_REQUIRE(byte_offsets[i + 1] >= byte_offsets[i], "byte_offsets must be non-decreasing (token %lld)", (long long)i);
        MHX_REQUIRE(bytes || byte_offsets[n_tokens] == 0, "bytes is NULL");
        return MHX_OK;
    }
    int check_arrays() const {
        MHX_REQUIRE(set_offsets, "%s", kNoOut);
        MHX_REQUIRE(set_offsets[0] == 0 && set_offsets[n] == n_tokens, "set_offsets must run from 0 to n_tokens");
        for (int64_t i = 0; i < n; ++i)
            MHX_REQUIRE(set_offsets[i + 1] >= set_offsets[i], "set_offsets must be non-decreasing (set %lld)", (long long)i);
        return n_tokens > 0 ? check_tokens() : MHX_OK;  // (no token: bytes and byte_offsets are not looked at)
    }

    int stage(mhx_ctx *ctx) {
        Stage s(ctx);
        Stage::Piece p_bytes{Stage::In, 0, 0}, p_boffs{Stage::Offsets, 0, 0}, p_sets{Stage::Offsets, 0, 0};
        if (n_tokens > 0) {
            p_bytes = s.piece(Stage::In, (size_t)byte_offsets[n_tokens]);
            s.ask(Stage::In, std::max<size_t>(p_bytes.bytes + in_slack, 8));
            p_boffs = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n_tokens + 1));
        }
        if (set_offsets) p_sets = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n + 1));
        MHX_TRY(s.commit());
        if (n_tokens > 0) {
            d_bytes = s.at<uint8_t>(p_bytes);
            d_boffs = s.at<int64_t>(p_boffs);
        }
        if (set_offsets) d_sets = s.at<int64_t>(p_sets);
        MHX_TRY(s.upload(p_bytes, bytes));
        MHX_TRY(s.upload(p_boffs, byte_offsets));
        return s.upload(p_sets, set_offsets);
    }
    void reserve(Stage &s) const {
        if (aux_slack) s.ask(Stage::Aux, s.size[Stage::Aux] + aux_slack);
    }
    int hash(const Stage &s, int dtype, void *d_hv) {
        n_hashes = n_tokens;
        if (hash_kind == MHX_HASH_XXH) return mhx::launch_xxh_tokens(s.ctx, d_bytes, d_boffs, n_tokens, dtype, d_hv);
        return mhx::launch_sha1_tokens(s.ctx, d_bytes, d_boffs, n_tokens, dtype, d_hv);
    }
};

}  // namespace
}  // extern "C++"

int mhx_sha1_tokens(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int out_dtype, void *out) {
    return mhx_hash_tokens(ctx, bytes, byte_offsets, n_tokens, MHX_HASH_SHA1, out_dtype, out);
}

int mhx_hash_tokens(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_kind, int out_dtype, void *out) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    MHX_TRY(check_sha1(n_tokens, out_dtype));
    if (n_tokens == 0) return MHX_OK;
    MHX_REQUIRE(out, "out is NULL");
    MHX_TRY(ctx->activate());
    Tokens src{bytes, byte_offsets, n_tokens, nullptr, 0, 0, hash_kind, tokens_in_slack(hash_kind)};
    MHX_TRY(src.check_tokens());
    MHX_TRY(src.stage(ctx));
    Stage s(ctx);
    const auto p_out = s.piece(Stage::Out, (size_t)n_tokens * (out_dtype == MHX_U32 ? 4 : 8));
    MHX_TRY(s.commit());
    MHX_TRY(src.hash(s, out_dtype, s.at<void>(p_out)));
    return s.fetch(out, p_out);
}

int mhx_minhash_update_batch(mhx_perm *perm, const uint64_t *hv, int64_t n, uint64_t *hashvalues) {
    MHX_ENTER(perm, perm->ctx);
    MHX_REQUIRE(n >= 0, "n must be >= 0");
    if (n == 0) return MHX_OK;  // ref: minhash.py:265-266
    MHX_REQUIRE(hv && hashvalues, "hv/hashvalues is NULL");
    return mhx_minhash_bulk(perm, hv, nullptr, n, 1, hashvalues, 0, hashvalues);
}

static int minhash_merge(mhx_ctx *ctx, const uint64_t *x, const uint64_t *y, int64_t count, uint64_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(count >= 0, "count must be >= 0");
    if (count == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(x && y && out, where);
    MHX_TRY(ctx->activate());
    if (where == kDevice) return mhx::launch_minhash_merge(ctx, x, y, count, out);
    Stage s(ctx);
    const auto p_x = s.piece(Stage::In, sizeof(uint64_t) * (size_t)count), p_y = s.piece(Stage::Out, p_x.bytes);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_x, x));
    MHX_TRY(s.upload(p_y, y));
    MHX_TRY(mhx::launch_minhash_merge(ctx, s.at<uint64_t>(p_x), s.at<uint64_t>(p_y), count, s.at<uint64_t>(p_x)));
    return s.fetch(out, p_x);
}

int mhx_minhash_merge_dev(mhx_ctx *ctx, const uint64_t *d_x, const uint64_t *d_y, int64_t count, uint64_t *d_out) {
    return minhash_merge(ctx, d_x, d_y, count, d_out, kDevice);
}

int mhx_minhash_merge(mhx_ctx *ctx, const uint64_t *x, const uint64_t *y, int64_t count, uint64_t *out) {
    return minhash_merge(ctx, x, y, count, out, kHost);
}

// ---- packing, band digests, sorted bands, Lean records -----------------------------------------------------------------
// One core per operation.  The host forms (where == kHost) take uint64 signatures: the matrix goes to In, the results come
// back from Out.
int mhx_bbit_num_blocks(int32_t num_perm, int32_t b, int32_t *num_blocks_out) {
    if (!num_blocks_out) return fail(MHX_ERR_INVALID, "num_blocks is NULL");
    MHX_CHECK_B(b);
    MHX_REQUIRE(num_perm > 0, "num_perm must be positive");
    *num_blocks_out = num_blocks(num_perm, b);
    return MHX_OK;
}

static int bbit_pack(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t k, int32_t b, uint64_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_B(b);
    MHX_REQUIRE(k > 0 && n >= 0, "bad shape");
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && out, where);
    MHX_TRY(ctx->activate());
    auto launch = [&](const void *d_sig, void *d_out) { return mhx::launch_bbit_pack(ctx, d_sig, sig_dtype, n, k, b, (uint64_t *)d_out); };
    if (where == kDevice) return launch(sig, out);
    return through_scratch(ctx, sig, sizeof(uint64_t) * (size_t)(n * k), out, sizeof(uint64_t) * (size_t)(n * num_blocks(k, b)), launch);
}

int mhx_bbit_pack_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int32_t b, uint64_t *d_out) {
    return bbit_pack(ctx, d_sig, sig_dtype, n, k, b, d_out, kDevice);
}

int mhx_bbit_pack_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n, int32_t k, int32_t b, uint64_t *d_out) {
    return mhx_bbit_pack_dev_typed(ctx, d_sig, MHX_U64, n, k, b, d_out);
}

int mhx_bbit_pack(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t b, uint64_t *out) {
    return bbit_pack(ctx, sig, MHX_U64, n, k, b, out, kHost);
}

static int bbit_unpack(mhx_ctx *ctx, const uint64_t *blocks, int64_t n, int32_t k, int32_t b, uint32_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(k > 0 && n >= 0, "bad shape");
    MHX_CHECK_B(b);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(blocks && out, where);
    MHX_TRY(ctx->activate());
    auto launch = [&](const void *d_blocks, void *d_out) { return mhx::launch_bbit_unpack(ctx, (const uint64_t *)d_blocks, n, k, b, (uint32_t *)d_out); };
    if (where == kDevice) return launch(blocks, out);
    return through_scratch(ctx, blocks, sizeof(uint64_t) * (size_t)n * num_blocks(k, b), out, sizeof(uint32_t) * (size_t)n * k, launch);
}

int mhx_bbit_unpack_dev(mhx_ctx *ctx, const uint64_t *d_blocks, int64_t n, int32_t k, int32_t b, uint32_t *d_out) {
    return bbit_unpack(ctx, d_blocks, n, k, b, d_out, kDevice);
}

int mhx_bbit_unpack(mhx_ctx *ctx, const uint64_t *blocks, int64_t n, int32_t k, int32_t b, uint32_t *out) {
    return bbit_unpack(ctx, blocks, n, k, b, out, kHost);
}

static int band_keys(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0, "bad shape");
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && out, where);
    MHX_TRY(ctx->activate());
    auto launch = [&](const void *d_sig, void *d_out) { return mhx::launch_band_keys(ctx, (const uint64_t *)d_sig, n, k, bands, r, (uint64_t *)d_out); };
    if (where == kDevice) return launch(sig, out);
    return through_scratch(ctx, sig, sizeof(uint64_t) * (size_t)(n * k), out, sizeof(uint64_t) * (size_t)(n * bands * r), launch);
}

int mhx_band_keys_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *d_out) {
    return band_keys(ctx, d_sig, n, k, bands, r, d_out, kDevice);
}

int mhx_band_keys(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *out) {
    return band_keys(ctx, sig, n, k, bands, r, out, kHost);
}

static int band_digests(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t k, int32_t bands, int32_t r, int layout,
                        uint64_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0, "bad shape");
    MHX_CHECK_LAYOUT(layout);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && out, where);
    MHX_TRY(ctx->activate());
    auto launch = [&](const void *d_sig, void *d_out) { return mhx::launch_band_digests(ctx, d_sig, sig_dtype, n, k, bands, r, (uint64_t *)d_out, layout); };
    if (where == kDevice) return launch(sig, out);
    return through_scratch(ctx, sig, sizeof(uint64_t) * (size_t)(n * k), out, sizeof(uint64_t) * (size_t)(n * bands), launch);
}

int mhx_band_digests_layout_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int32_t bands,
                                int32_t r, int layout, uint64_t *d_out) {
    return band_digests(ctx, d_sig, sig_dtype, n, k, bands, r, layout, d_out, kDevice);
}

int mhx_band_digests_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *d_out) {
    return mhx_band_digests_layout_dev(ctx, d_sig, sig_dtype, n, k, bands, r, MHX_ROW_MAJOR, d_out);
}

int mhx_band_digests_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *d_out) {
    return mhx_band_digests_layout_dev(ctx, d_sig, MHX_U64, n, k, bands, r, MHX_ROW_MAJOR, d_out);
}

int mhx_band_digests(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t bands, int32_t r, uint64_t *out) {
    return band_digests(ctx, sig, MHX_U64, n, k, bands, r, MHX_ROW_MAJOR, out, kHost);
}

// b-bit blocks and band digests of the same matrix: one read when the shape allows the fused kernel, the two kernels otherwise
int mhx_bbit_pack_band_digests_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int32_t b,
                                   int32_t bands, int32_t r, int digest_layout, uint64_t *d_blocks, uint64_t *d_digests, int *fused) {
    if (fused) *fused = 0;
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_REQUIRE(b >= 1 && b <= 32, "b must be in [1, 32]");
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0 && k > 0, "bad shape");
    MHX_CHECK_LAYOUT(digest_layout);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_sig && d_blocks && d_digests, kDevice);
    MHX_TRY(ctx->activate());
    bool done = false;
    if (ctx->opt_pack_fused != 1)
        MHX_TRY(mhx::launch_bbit_digest_fused(ctx, d_sig, sig_dtype, n, k, b, bands, r, d_blocks, d_digests, digest_layout, &done));
    if (fused) *fused = done ? 1 : 0;
    if (done) return MHX_OK;
    MHX_TRY(mhx::launch_bbit_pack(ctx, d_sig, sig_dtype, n, k, b, d_blocks));
    return mhx::launch_band_digests(ctx, d_sig, sig_dtype, n, k, bands, r, d_digests, digest_layout);
}

static int lsh_sort_bands(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t k, int32_t bands, int32_t r,
                          uint64_t *sorted_digests, uint32_t *sorted_rows, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0, "bad shape");
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && sorted_digests && sorted_rows, where);
    MHX_TRY(ctx->activate());
    if (where == kDevice) return mhx::launch_lsh_sort_bands(ctx, sig, sig_dtype, n, k, bands, r, sorted_digests, sorted_rows);
    Stage s(ctx);
    const auto p_sig = s.piece(Stage::In, sizeof(uint64_t) * (size_t)(n * k));
    const auto p_dig = s.piece(Stage::Out, sizeof(uint64_t) * (size_t)n * bands);
    const auto p_rows = s.piece(Stage::Out, sizeof(uint32_t) * (size_t)n * bands);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_sig, sig));
    MHX_TRY(mhx::launch_lsh_sort_bands(ctx, s.at<void>(p_sig), sig_dtype, n, k, bands, r, s.at<uint64_t>(p_dig), s.at<uint32_t>(p_rows)));
    MHX_TRY(s.download(sorted_digests, p_dig));
    return s.fetch(sorted_rows, p_rows);
}

int mhx_lsh_sort_bands_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int32_t bands,
                                 int32_t r, uint64_t *d_sorted_digests, uint32_t *d_sorted_rows) {
    return lsh_sort_bands(ctx, d_sig, sig_dtype, n, k, bands, r, d_sorted_digests, d_sorted_rows, kDevice);
}

int mhx_lsh_sort_bands_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n, int32_t k, int32_t bands, int32_t r,
                           uint64_t *d_sorted_digests, uint32_t *d_sorted_rows) {
    return mhx_lsh_sort_bands_dev_typed(ctx, d_sig, MHX_U64, n, k, bands, r, d_sorted_digests, d_sorted_rows);
}

int mhx_lsh_sort_bands(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t bands, int32_t r,
                       uint64_t *sorted_digests, uint32_t *sorted_rows) {
    return lsh_sort_bands(ctx, sig, MHX_U64, n, k, bands, r, sorted_digests, sorted_rows, kHost);
}

int mhx_lsh_sort_digests_layout_dev(mhx_ctx *ctx, const uint64_t *d_digests, int64_t n, int32_t bands, int layout, uint64_t *d_sorted_digests,
                                    uint32_t *d_sorted_rows) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n >= 0 && bands > 0, "bad shape");
    MHX_CHECK_LAYOUT(layout);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_digests && d_sorted_digests && d_sorted_rows, kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_sort_bands(ctx, d_digests, layout == MHX_BAND_MAJOR ? mhx::kSigDigestsBM : mhx::kSigDigests, n, bands, bands, 1,
                                      d_sorted_digests, d_sorted_rows);
}

int mhx_lsh_sort_digests_dev(mhx_ctx *ctx, const uint64_t *d_digests, int64_t n, int32_t bands, uint64_t *d_sorted_digests, uint32_t *d_sorted_rows) {
    return mhx_lsh_sort_digests_layout_dev(ctx, d_digests, n, bands, MHX_ROW_MAJOR, d_sorted_digests, d_sorted_rows);
}

int mhx_lsh_candidate_pairs_dev(mhx_ctx *ctx, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows, int64_t n,
                                int32_t bands, int64_t *d_pairs, int64_t capacity, int64_t *n_pairs, int64_t *n_raw) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_pairs, "n_pairs is NULL");
    MHX_REQUIRE(bands > 0 && n >= 0 && capacity >= 0, "bad shape");
    MHX_CHECK_ROWS32(n);
    *n_pairs = 0;
    if (n_raw) *n_raw = 0;
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_sorted_digests && d_sorted_rows && (d_pairs || capacity == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_candidate_pairs(ctx, d_sorted_digests, d_sorted_rows, n, bands, d_pairs, capacity, n_pairs, n_raw);
}

// host signatures -> candidate pairs: the sort and the pair kernel back to back.  Out: sorted digests | sorted rows | pairs
int mhx_lsh_candidate_pairs(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int32_t bands, int32_t r,
                            int64_t *pairs, int64_t capacity, int64_t *n_pairs, int64_t *n_raw) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_pairs, "n_pairs is NULL");
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0 && capacity >= 0, "bad shape");
    *n_pairs = 0;
    if (n_raw) *n_raw = 0;
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && (pairs || capacity == 0), kHost);
    MHX_TRY(ctx->activate());
    Stage s(ctx);
    const auto p_sig = s.piece(Stage::In, sizeof(uint64_t) * (size_t)(n * k));
    const auto p_dig = s.piece(Stage::Out, sizeof(uint64_t) * (size_t)n * bands);
    const auto p_rows = s.piece(Stage::Out, sizeof(uint32_t) * (size_t)n * bands);
    const auto p_pairs = s.piece(Stage::Out, sizeof(int64_t) * 2 * (size_t)capacity);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_sig, sig));
    MHX_TRY(mhx::launch_lsh_sort_bands(ctx, s.at<void>(p_sig), MHX_U64, n, k, bands, r, s.at<uint64_t>(p_dig), s.at<uint32_t>(p_rows)));
    MHX_TRY(mhx::launch_lsh_candidate_pairs(ctx, s.at<uint64_t>(p_dig), s.at<uint32_t>(p_rows), n, bands, s.at<int64_t>(p_pairs), capacity,
                                            n_pairs, n_raw));
    if (*n_pairs > 0 && *n_pairs <= capacity) MHX_TRY(s.download(pairs, p_pairs, sizeof(int64_t) * 2 * (size_t)*n_pairs));
    return s.synchronize();
}

int mhx_lsh_query_dev(mhx_ctx *ctx, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows, int64_t n,
                      int32_t bands, int32_t r, const void *d_query_sig, const void *d_index_sig, int sig_dtype,
                      int32_t k, int64_t m, int64_t *d_pairs, int64_t capacity, int64_t *n_pairs) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_pairs, "n_pairs is NULL");
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BANDS(bands, r, k);
    MHX_REQUIRE(n >= 0 && m >= 0 && capacity >= 0, "bad shape");
    MHX_CHECK_ROWS32(n);
    MHX_CHECK_ROWS32(m);
    *n_pairs = 0;
    if (n == 0 || m == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_sorted_digests && d_sorted_rows && d_query_sig && (d_pairs || capacity == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_query(ctx, d_sorted_digests, d_sorted_rows, n, bands, r, d_query_sig, d_index_sig, sig_dtype, k, m,
                                 d_pairs, capacity, n_pairs);
}

int mhx_lsh_ensemble_query_dev(mhx_ctx *ctx, const mhx_ensemble_level *levels, int32_t n_levels, const int64_t *start, int32_t n_parts,
                               const void *d_index_sig, int sig_dtype, int32_t k, const void *d_query_sig, int64_t m,
                               const uint8_t *d_choice, const int32_t *params, int32_t n_params, int64_t *d_pairs, int64_t capacity,
                               int64_t *n_pairs) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_pairs, "n_pairs is NULL");
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_REQUIRE(k > 0 && n_parts >= 0 && m >= 0 && capacity >= 0, "bad shape");
    MHX_REQUIRE(n_levels > 0 && n_levels <= MHX_ENSEMBLE_MAX_LEVELS, "n_levels must be in [1, %d]", MHX_ENSEMBLE_MAX_LEVELS);
    MHX_REQUIRE(n_params > 0 && n_params <= MHX_ENSEMBLE_MAX_PARAMS, "n_params must be in [1, %d]", MHX_ENSEMBLE_MAX_PARAMS);
    MHX_REQUIRE_POINTERS(levels && start && params, kHost);
    MHX_REQUIRE(start[0] == 0, "start[0] must be 0");
    for (int32_t p = 0; p < n_parts; ++p) MHX_REQUIRE(start[p] <= start[p + 1], "start must ascend");
    const int64_t n = start[n_parts];
    MHX_CHECK_ROWS32(n);
    MHX_CHECK_ROWS32(m);
    for (int32_t l = 0; l < n_levels; ++l) MHX_CHECK_BANDS(levels[l].bands, levels[l].r, k);
    for (int32_t c = 0; c < n_params; ++c) {
        const int32_t level = params[2 * c], b = params[2 * c + 1];
        MHX_REQUIRE(level >= 0 && level < n_levels, "params row %d names level %d of %d", c, level, n_levels);
        MHX_REQUIRE(b >= 0 && b <= levels[level].bands, "params row %d: b = %d is not in [0, %d], the bands of its level", c, b,
                    levels[level].bands);
    }
    *n_pairs = 0;
    if (n == 0 || m == 0 || n_parts == 0) return MHX_OK;
    bool buffers = true;
    for (int32_t l = 0; l < n_levels; ++l) buffers = buffers && levels[l].d_digests && levels[l].d_rows;
    MHX_REQUIRE_POINTERS(buffers && d_index_sig && d_query_sig && d_choice && (d_pairs || capacity == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_ensemble_query(ctx, levels, n_levels, start, n_parts, d_index_sig, sig_dtype, k, d_query_sig, m, d_choice, params,
                                          n_params, d_pairs, capacity, n_pairs);
}

// uint64 words per row of the Jaccard cores: k dense elements, the blocks of k b-bit values, or k weighted (k, t) samples
static size_t jaccard_row_words(int32_t k, int32_t b) {
    return b == mhx::kWeightedRows ? 2 * (size_t)k : b < 0 ? (size_t)k : (size_t)num_blocks(k, b);
}

// Agreeing positions of listed pairs.  b < 0: dense rows of sig_dtype (kWeightedRows: weighted rows of k samples), else b-bit
// blocks.  The host form takes the n rows both ends of a pair index (In), the pairs (Aux) and returns the counts (Out).
static int listed_pairs(mhx_ctx *ctx, const void *rows_a, const void *rows_b, int64_t n, int sig_dtype, int32_t k, int32_t b,
                        const int64_t *pairs, int64_t n_pairs, int32_t *counts, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    if (b >= 0) MHX_CHECK_B(b);
    MHX_REQUIRE(k > 0 && n >= 0 && n_pairs >= 0, "bad shape");
    if (n_pairs == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(rows_a && rows_b && pairs && counts, where);
    MHX_TRY(ctx->activate());
    Stage s(ctx);
    Stage::Piece p_counts{};
    if (where == kHost) {
        for (int64_t p = 0; p < 2 * n_pairs; ++p)
            MHX_REQUIRE(pairs[p] >= 0 && pairs[p] < n, "pair index %lld out of range [0,%lld)", (long long)pairs[p], (long long)n);
        const auto p_rows = s.piece(Stage::In, sizeof(uint64_t) * (size_t)n * jaccard_row_words(k, b));
        const auto p_pairs = s.piece(Stage::Aux, sizeof(int64_t) * 2 * (size_t)n_pairs);
        p_counts = s.piece(Stage::Out, sizeof(int32_t) * (size_t)n_pairs);
        MHX_TRY(s.commit());
        MHX_TRY(s.upload(p_rows, rows_a));
        MHX_TRY(s.upload(p_pairs, pairs));
        rows_a = rows_b = s.at<void>(p_rows);
        pairs = s.at<int64_t>(p_pairs);
    }
    int32_t *d_counts = where == kHost ? s.at<int32_t>(p_counts) : counts;
    if (b == mhx::kWeightedRows) MHX_TRY(mhx::launch_weighted_jaccard_pairs(ctx, rows_a, rows_b, k, pairs, n_pairs, d_counts));
    else if (b < 0) MHX_TRY(mhx::launch_jaccard_pairs(ctx, rows_a, rows_b, sig_dtype, k, pairs, n_pairs, d_counts));
    else MHX_TRY(mhx::launch_bbit_jaccard(ctx, (const uint64_t *)rows_a, (const uint64_t *)rows_b, k, b, pairs, n_pairs, d_counts));
    return where == kHost ? s.fetch(counts, p_counts) : MHX_OK;
}

int mhx_jaccard_pairs_dev_typed(mhx_ctx *ctx, const void *d_sig_a, const void *d_sig_b, int sig_dtype, int32_t k,
                                const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts) {
    return listed_pairs(ctx, d_sig_a, d_sig_b, 0, sig_dtype, k, -1, d_pairs, n_pairs, d_counts, kDevice);
}

int mhx_jaccard_pairs_dev(mhx_ctx *ctx, const uint64_t *d_sig_a, const uint64_t *d_sig_b, int32_t k,
                          const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts) {
    return mhx_jaccard_pairs_dev_typed(ctx, d_sig_a, d_sig_b, MHX_U64, k, d_pairs, n_pairs, d_counts);
}

int mhx_jaccard_pairs(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    return listed_pairs(ctx, sig, sig, n, MHX_U64, k, -1, pairs, n_pairs, counts, kHost);
}

int mhx_bbit_jaccard_pairs_dev(mhx_ctx *ctx, const uint64_t *d_blocks_a, const uint64_t *d_blocks_b, int32_t k, int32_t b,
                               const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts) {
    MHX_CHECK_B(b);
    return listed_pairs(ctx, d_blocks_a, d_blocks_b, 0, MHX_U64, k, b, d_pairs, n_pairs, d_counts, kDevice);
}

int mhx_bbit_jaccard_pairs(mhx_ctx *ctx, const uint64_t *blocks, int64_t n, int32_t k, int32_t b, const int64_t *pairs,
                           int64_t n_pairs, int32_t *counts) {
    MHX_CHECK_B(b);
    return listed_pairs(ctx, blocks, blocks, n, MHX_U64, k, b, pairs, n_pairs, counts, kHost);
}

static int lean_serialize(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t k, int64_t seed, int byteorder, uint8_t *out,
                          Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(k > 0 && n >= 0, "bad shape");
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BYTEORDER(byteorder);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && out, where);
    MHX_TRY(ctx->activate());
    auto launch = [&](const void *d_sig, void *d_out) { return mhx::launch_lean_serialize(ctx, d_sig, sig_dtype, n, k, seed, byteorder, (uint8_t *)d_out); };
    if (where == kDevice) return launch(sig, out);
    return through_scratch(ctx, sig, sizeof(uint64_t) * (size_t)(n * k), out, (size_t)n * (12 + 4 * (size_t)k), launch);
}

int mhx_lean_serialize_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t k, int64_t seed, int byteorder, uint8_t *d_out) {
    return lean_serialize(ctx, d_sig, sig_dtype, n, k, seed, byteorder, d_out, kDevice);
}

int mhx_lean_serialize_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n, int32_t k, int64_t seed, uint8_t *d_out) {
    return mhx_lean_serialize_dev_typed(ctx, d_sig, MHX_U64, n, k, seed, MHX_LITTLE_ENDIAN, d_out);
}

int mhx_lean_serialize(mhx_ctx *ctx, const uint64_t *sig, int64_t n, int32_t k, int64_t seed, uint8_t *out) {
    return lean_serialize(ctx, sig, MHX_U64, n, k, seed, MHX_LITTLE_ENDIAN, out, kHost);
}

// records -> [n, k] hashvalues + seeds.  The host form: a record whose length field is not k: MHX_ERR_INVALID, nothing written
static int lean_deserialize(mhx_ctx *ctx, const uint8_t *records, int64_t n, int32_t k, int byteorder, int sig_dtype, void *sig,
                            int64_t *seeds, uint32_t *d_bad, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(k > 0 && n >= 0, "bad shape");
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BYTEORDER(byteorder);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(records && sig, where);
    if (where == kDevice) MHX_REQUIRE(((uintptr_t)records & 3) == 0, "records must be 4-byte aligned");
    MHX_TRY(ctx->activate());
    if (where == kDevice) return mhx::launch_lean_deserialize(ctx, records, n, k, byteorder, sig_dtype, sig, seeds, d_bad);
    Stage s(ctx);
    const auto p_rec = s.piece(Stage::In, (size_t)n * (12 + 4 * (size_t)k));
    const auto p_sig = s.piece(Stage::Out, sizeof(uint64_t) * (size_t)n * k);
    const auto p_seeds = s.piece(Stage::Out, (size_t)n * 8);
    const auto p_bad = s.piece(Stage::Out, sizeof(unsigned int));
    s.ask(Stage::Out, p_bad.at + 256);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_rec, records));
    MHX_HIP_CHECK(hipMemsetAsync(s.at<void>(p_bad), 0, sizeof(unsigned int), ctx->stream));
    MHX_TRY(mhx::launch_lean_deserialize(ctx, s.at<uint8_t>(p_rec), n, k, byteorder, sig_dtype, s.at<void>(p_sig), s.at<int64_t>(p_seeds),
                                         s.at<unsigned int>(p_bad)));
    unsigned int bad = 0;
    MHX_TRY(s.fetch(&bad, p_bad));
    if (bad) return fail(MHX_ERR_INVALID, "%u of %lld records do not hold %d hash values (length field)", bad, (long long)n, k);
    MHX_TRY(s.download(sig, p_sig));
    if (seeds) MHX_TRY(s.download(seeds, p_seeds));
    return s.synchronize();
}

int mhx_lean_deserialize_dev(mhx_ctx *ctx, const uint8_t *d_records, int64_t n, int32_t k, int byteorder, int sig_dtype, void *d_sig,
                             int64_t *d_seeds, uint32_t *d_bad) {
    return lean_deserialize(ctx, d_records, n, k, byteorder, sig_dtype, d_sig, d_seeds, d_bad, kDevice);
}

int mhx_lean_deserialize(mhx_ctx *ctx, const uint8_t *records, int64_t n, int32_t k, int byteorder, uint64_t *sig, int64_t *seeds) {
    return lean_deserialize(ctx, records, n, k, byteorder, MHX_U64, sig, seeds, nullptr, kHost);
}

// ---- weighted ------------------------------------------------------------------------------
int mhx_wgen_create(mhx_ctx *ctx, const float *rs, const float *ln_cs, const float *betas,
                    int32_t sample_size, int32_t dim, mhx_wgen **out) {
    if (!ctx || !rs || !ln_cs || !betas || !out) return fail(MHX_ERR_INVALID, "NULL argument");
    MHX_GUARD(ctx);
    MHX_REQUIRE(sample_size > 0 && dim > 0, "sample_size and dim must be positive");
    if (int rc = ctx->activate()) return rc;
    mhx_wgen *g = new mhx_wgen();
    g->ctx = ctx;
    g->sample_size = sample_size;
    g->dim = dim;
    g->s_pad = (sample_size + 63) / 64 * 64;
    const size_t n = (size_t)sample_size * dim;
    const size_t t_bytes = sizeof(float) * 5 * (size_t)g->s_pad * dim;
    g->table_fast = true;
    for (size_t j = 0; j < n && g->table_fast; ++j) {
        const float m = fabsf(rs[j]);
        g->table_fast = m >= 0x1p-40f && m <= 0x1p40f;  // false for NaN / inf / 0 as well
    }
    // the walk's bound wants r > 0 and finite ln_c, beta (monotone ln_a); its table builder sorts a sample's columns in LDS
    g->walk_ok = g->table_fast && dim <= 16384;
    for (size_t j = 0; j < n && g->walk_ok; ++j)
        g->walk_ok = rs[j] > 0.0f && fabsf(ln_cs[j]) < __builtin_inff() && fabsf(betas[j]) < __builtin_inff();
    const size_t a_bytes = sizeof(float) * 4 * (size_t)g->s_pad * (size_t)dim;
    const float plan0[8] = {__builtin_nanf(""), 0.0f, 0.0f, 0.0f, __builtin_nanf(""), 0.0f, 0.0f, 0.0f};  // two WalkPlan records: no tables yet
    hipError_t e = mhx::dev_malloc((void **)&g->d_params, t_bytes);
    if (e == hipSuccess) e = mhx::dev_malloc((void **)&g->d_aos, a_bytes);
    if (e == hipSuccess && g->walk_ok) e = mhx::dev_malloc((void **)&g->d_walk_a, a_bytes);
    if (e == hipSuccess && g->walk_ok) e = mhx::dev_malloc((void **)&g->d_walk_c, a_bytes / 4);
    if (e == hipSuccess && g->walk_ok) e = mhx::dev_malloc(&g->d_walk_plan, sizeof(plan0));
    if (e == hipSuccess && g->walk_ok) e = hipMemcpyAsync(g->d_walk_plan, plan0, sizeof(plan0), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && g->walk_ok) e = hipMemsetAsync(g->d_walk_a, 0, a_bytes, ctx->stream);  // lanes behind sample_size load from here too
    if (e == hipSuccess && g->walk_ok) e = hipMemsetAsync(g->d_walk_c, 0, a_bytes / 4, ctx->stream);
    if (e != hipSuccess) {
        (void)mhx::dev_free(g->d_params);
        (void)mhx::dev_free(g->d_aos);
        (void)mhx::dev_free(g->d_walk_a);
        (void)mhx::dev_free(g->d_walk_c);
        (void)mhx::dev_free(g->d_walk_plan);
        delete g;
        return fail(MHX_ERR_OOM, "hipMalloc for weighted parameters failed: %s", hipGetErrorString(e));
    }
    int rc = ctx->ensure_scratch(0, 3 * n * sizeof(float));
    if (rc == MHX_OK) {
        float *d = (float *)ctx->scratch[0];
        e = hipMemcpyAsync(d, rs, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d + n, ln_cs, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d + 2 * n, betas, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) rc = fail(MHX_ERR_HIP, "uploading weighted parameters failed: %s", hipGetErrorString(e));
        if (rc == MHX_OK) rc = mhx::launch_wgen_transpose(g, d, d + n, d + 2 * n);
        if (rc == MHX_OK && hipStreamSynchronize(ctx->stream) != hipSuccess)
            rc = fail(MHX_ERR_HIP, "weighted parameter transpose failed");
    }
    if (rc != MHX_OK) {
        (void)mhx::dev_free(g->d_params);
        (void)mhx::dev_free(g->d_aos);
        (void)mhx::dev_free(g->d_walk_a);
        (void)mhx::dev_free(g->d_walk_c);
        (void)mhx::dev_free(g->d_walk_plan);
        delete g;
        return rc;
    }
    *out = g;
    return MHX_OK;
}

int mhx_wgen_destroy(mhx_wgen *gen) {
    if (!gen) return MHX_OK;
    MHX_GUARD(gen->ctx);
    (void)hipSetDevice(gen->ctx->device);
    (void)hipStreamSynchronize(gen->ctx->stream);
    (void)mhx::dev_free(gen->d_params);
    (void)mhx::dev_free(gen->d_aos);
    (void)mhx::dev_free(gen->d_walk_a);
    (void)mhx::dev_free(gen->d_walk_c);
    (void)mhx::dev_free(gen->d_walk_plan);
    delete gen;
    return MHX_OK;
}

int mhx_weighted_minhash_many_dev(mhx_wgen *gen, const int64_t *d_indptr, const int32_t *d_indices, const float *d_values, int values_are_logs,
                                  int64_t n_rows, int64_t nnz, int64_t *d_out, uint8_t *d_nonempty) {
    MHX_ENTER(gen, gen->ctx);
    MHX_REQUIRE(n_rows >= 0 && nnz >= 0, "bad shape");
    if (n_rows == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_indptr && d_out && d_nonempty, kDevice);
    MHX_REQUIRE_POINTERS((d_indices && d_values) || nnz == 0, kDevice);
    MHX_TRY(gen->ctx->activate());
    return mhx::launch_weighted(gen, d_indptr, d_indices, d_values, values_are_logs, n_rows, nnz, d_out,
                                d_nonempty);
}

// CSR rows on the host.  In: indices | values;  Aux: indptr;  Out: samples | nonempty
int mhx_weighted_minhash_many(mhx_wgen *gen, const int64_t *indptr, const int32_t *indices, const float *values, int values_are_logs, int64_t n_rows,
                              int64_t *out, uint8_t *nonempty) {
    MHX_ENTER(gen, gen->ctx);
    MHX_REQUIRE(n_rows >= 0, "bad shape");
    if (n_rows == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(indptr && out && nonempty, kHost);
    mhx_ctx *ctx = gen->ctx;
    MHX_TRY(ctx->activate());
    for (int64_t i = 0; i < n_rows; ++i)
        MHX_REQUIRE(indptr[i + 1] >= indptr[i], "indptr must be non-decreasing (row %lld)", (long long)i);
    MHX_REQUIRE(indptr[0] == 0, "indptr[0] must be 0");
    const int64_t nnz = indptr[n_rows];
    MHX_REQUIRE_POINTERS((indices && values) || nnz == 0, kHost);
    for (int64_t j = 0; j < nnz; ++j)
        MHX_REQUIRE(indices[j] >= 0 && indices[j] < gen->dim, "column index %d out of range [0,%d)", indices[j], gen->dim);
    Stage s(ctx);
    const auto p_idx = s.piece(Stage::In, sizeof(int32_t) * (size_t)nnz);
    const auto p_val = s.piece(Stage::In, sizeof(float) * (size_t)nnz);
    const auto p_ptr = s.piece(Stage::Aux, sizeof(int64_t) * (size_t)(n_rows + 1));
    const auto p_out = s.piece(Stage::Out, sizeof(int64_t) * 2 * (size_t)gen->sample_size * (size_t)n_rows);
    const auto p_ne = s.piece(Stage::Out, (size_t)n_rows);
    s.ask(Stage::In, p_val.at + p_val.bytes + 256);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_ptr, indptr));
    MHX_TRY(s.upload(p_idx, indices));
    MHX_TRY(s.upload(p_val, values));
    MHX_TRY(mhx::launch_weighted(gen, s.at<int64_t>(p_ptr), s.at<int32_t>(p_idx), s.at<float>(p_val), values_are_logs, n_rows, nnz,
                                 s.at<int64_t>(p_out), s.at<uint8_t>(p_ne)));
    MHX_TRY(s.download(out, p_out));
    return s.fetch(nonempty, p_ne);
}

int mhx_weighted_logf(mhx_ctx *ctx, const float *x, int64_t n, float *out) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n >= 0, "bad shape");
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(x && out, kHost);
    MHX_TRY(ctx->activate());
    return through_scratch(ctx, x, sizeof(float) * (size_t)n, out, sizeof(float) * (size_t)n,
                           [&](const void *d_x, void *d_out) { return mhx::launch_weighted_log(ctx, (const float *)d_x, n, (float *)d_out); });
}

}  // extern "C" (the feed's state and helpers are C++)

// A dense weighted call in pieces: two device slots, so that the upload of piece i+1 (copy_in), the evaluation of
// piece i (ctx->stream) and the download of piece i-1 (copy_out) run side by side.
struct mhx_wfeed {
    mhx_wgen *gen = nullptr;
    int values_are_logs = 0;
    int64_t piece_rows = 0;
    float *d_x[2] = {nullptr, nullptr};
    char *d_res[2] = {nullptr, nullptr};  // out int64[piece_rows, S, 2] | nonempty uint8[piece_rows]
    size_t ne_off = 0;
    hipEvent_t uploaded[2] = {nullptr, nullptr}, computed[2] = {nullptr, nullptr};
    int64_t fed = 0;
    // the piece fed last: evaluated (or being evaluated) on the device, results not yet on the host
    int64_t *pend_out = nullptr;
    uint8_t *pend_ne = nullptr;
    int64_t pend_rows = 0;
    int pend_slot = 0;
};

namespace {

// bring the pending piece down (blocks until it is on the host)
int feed_drain(mhx_wfeed *f) {
    if (!f->pend_rows) return MHX_OK;
    mhx_ctx *ctx = f->gen->ctx;
    const int slot = f->pend_slot;
    const size_t out_bytes = sizeof(int64_t) * 2 * (size_t)f->gen->sample_size * (size_t)f->pend_rows;
    const int64_t rows = f->pend_rows;
    f->pend_rows = 0;
    MHX_HIP_CHECK(hipStreamWaitEvent(ctx->copy_out, f->computed[slot], 0));
    MHX_HIP_CHECK(hipMemcpyAsync(f->pend_out, f->d_res[slot], out_bytes, hipMemcpyDeviceToHost, ctx->copy_out));
    MHX_HIP_CHECK(hipMemcpyAsync(f->pend_ne, f->d_res[slot] + f->ne_off, (size_t)rows, hipMemcpyDeviceToHost, ctx->copy_out));
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->copy_out));
    return MHX_OK;
}

// rows per piece of a one-call dense evaluation: about 64 MiB of input + output, at least 4096 rows (fewer leave
// CUs without a row block), whole row blocks of 8
int64_t dense_piece_rows(const mhx_wgen *gen) {
    const int64_t per_row = 4 * (int64_t)gen->dim + 16 * (int64_t)gen->sample_size;
    return std::max<int64_t>(4096, ((64ll << 20) / per_row) & ~7ll);
}

}  // namespace

extern "C" {

int mhx_weighted_dense_begin(mhx_wgen *gen, int values_are_logs, int64_t piece_rows, mhx_wfeed **feed) {
    if (!gen) return fail(MHX_ERR_INVALID, "gen is NULL");
    MHX_GUARD(gen->ctx);
    MHX_REQUIRE(feed, "feed is NULL");
    *feed = nullptr;
    MHX_REQUIRE(piece_rows > 0, "piece_rows must be positive");
    mhx_ctx *ctx = gen->ctx;
    if (int rc = ctx->activate()) return rc;
    if (int rc = ctx->ensure_copy_streams()) return rc;
    mhx_wfeed *f = new (std::nothrow) mhx_wfeed();
    if (!f) return fail(MHX_ERR_OOM, "out of host memory");
    f->gen = gen;
    f->values_are_logs = values_are_logs;
    f->piece_rows = piece_rows;
    const size_t x_bytes = sizeof(float) * (size_t)piece_rows * (size_t)gen->dim;
    const size_t out_bytes = sizeof(int64_t) * 2 * (size_t)gen->sample_size * (size_t)piece_rows;
    f->ne_off = (out_bytes + 255) & ~(size_t)255;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = mhx::dev_malloc(reinterpret_cast<void **>(&f->d_x[i]), x_bytes);
        if (e == hipSuccess) e = mhx::dev_malloc(reinterpret_cast<void **>(&f->d_res[i]), f->ne_off + (size_t)piece_rows);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->uploaded[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&f->computed[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) {
        (void)mhx_weighted_dense_end(f);
        return fail(e == hipErrorOutOfMemory ? MHX_ERR_OOM : MHX_ERR_HIP, "buffers for pieces of %lld rows: %s", (long long)piece_rows,
                    hipGetErrorString(e));
    }
    *feed = f;
    return MHX_OK;
}

int mhx_weighted_dense_feed(mhx_wfeed *f, const float *x, int64_t n_rows, int64_t *out, uint8_t *nonempty) {
    if (!f) return fail(MHX_ERR_INVALID, "feed is NULL");
    mhx_ctx *ctx = f->gen->ctx;
    MHX_GUARD(ctx);
    MHX_REQUIRE(n_rows >= 0 && n_rows <= f->piece_rows, "a piece holds at most %lld rows", (long long)f->piece_rows);
    if (n_rows == 0) return MHX_OK;
    MHX_REQUIRE(x && out && nonempty, "NULL host pointer");
    if (int rc = ctx->activate()) return rc;
    const int slot = (int)(f->fed & 1);
    // the slot's input was read by the evaluation of the piece before last; its results came down during the last feed
    if (f->fed >= 2) MHX_HIP_CHECK(hipEventSynchronize(f->computed[slot]));
    const size_t x_bytes = sizeof(float) * (size_t)n_rows * (size_t)f->gen->dim;
    MHX_HIP_CHECK(hipMemcpyAsync(f->d_x[slot], x, x_bytes, hipMemcpyHostToDevice, ctx->copy_in));
    MHX_HIP_CHECK(hipEventRecord(f->uploaded[slot], ctx->copy_in));
    MHX_HIP_CHECK(hipStreamWaitEvent(ctx->stream, f->uploaded[slot], 0));
    if (int rc = mhx::launch_weighted_dense(f->gen, f->d_x[slot], f->values_are_logs, n_rows, reinterpret_cast<int64_t *>(f->d_res[slot]),
                                            reinterpret_cast<uint8_t *>(f->d_res[slot] + f->ne_off)))
        return rc;
    MHX_HIP_CHECK(hipEventRecord(f->computed[slot], ctx->stream));
    ++f->fed;
    if (int rc = feed_drain(f)) return rc;  // the previous piece, while this one is evaluated
    f->pend_out = out;
    f->pend_ne = nonempty;
    f->pend_rows = n_rows;
    f->pend_slot = slot;
    MHX_HIP_CHECK(hipStreamSynchronize(ctx->copy_in));  // a pinned x is copied asynchronously: it is free from here on
    return MHX_OK;
}

int mhx_weighted_dense_end(mhx_wfeed *f) {
    if (!f) return MHX_OK;
    mhx_ctx *ctx = f->gen->ctx;
    MHX_GUARD(ctx);
    int rc = ctx->activate();
    if (!rc) rc = feed_drain(f);
    if (ctx->copy_in) (void)hipStreamSynchronize(ctx->copy_in);
    (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 2; ++i) {
        if (f->d_x[i]) (void)mhx::dev_free(f->d_x[i]);
        if (f->d_res[i]) (void)mhx::dev_free(f->d_res[i]);
        if (f->uploaded[i]) (void)hipEventDestroy(f->uploaded[i]);
        if (f->computed[i]) (void)hipEventDestroy(f->computed[i]);
    }
    delete f;
    return rc;
}

static int weighted_dense(mhx_wgen *gen, const float *x, int values_are_logs, int64_t n_rows, int64_t *out, uint8_t *nonempty, Where where) {
    MHX_ENTER(gen, gen->ctx);
    MHX_REQUIRE(n_rows >= 0, "bad shape");
    if (n_rows == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(x && out && nonempty, where);
    mhx_ctx *ctx = gen->ctx;
    MHX_TRY(ctx->activate());
    if (where == kDevice) return mhx::launch_weighted_dense(gen, x, values_are_logs, n_rows, out, nonempty);
    const int64_t piece = dense_piece_rows(gen);
    if (n_rows >= 2 * piece && ctx->opt_host_chunk_bytes >= 0) {  // upload, evaluation and download side by side
        mhx_wfeed *f = nullptr;
        MHX_TRY(mhx_weighted_dense_begin(gen, values_are_logs, piece, &f));
        int rc = MHX_OK;
        for (int64_t lo = 0; lo < n_rows && !rc; lo += piece) {
            const int64_t rows = std::min(piece, n_rows - lo);
            rc = mhx_weighted_dense_feed(f, x + (size_t)lo * (size_t)gen->dim, rows, out + (size_t)lo * 2 * (size_t)gen->sample_size,
                                         nonempty + lo);
        }
        const int rc_end = mhx_weighted_dense_end(f);
        return rc ? rc : rc_end;
    }
    Stage s(ctx);
    const auto p_x = s.piece(Stage::In, sizeof(float) * (size_t)n_rows * (size_t)gen->dim);
    const auto p_out = s.piece(Stage::Out, sizeof(int64_t) * 2 * (size_t)gen->sample_size * (size_t)n_rows);
    const auto p_ne = s.piece(Stage::Out, (size_t)n_rows);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_x, x));
    MHX_TRY(mhx::launch_weighted_dense(gen, s.at<float>(p_x), values_are_logs, n_rows, s.at<int64_t>(p_out), s.at<uint8_t>(p_ne)));
    MHX_TRY(s.download(out, p_out));
    return s.fetch(nonempty, p_ne);
}

int mhx_weighted_minhash_many_dense_dev(mhx_wgen *gen, const float *d_x, int values_are_logs, int64_t n_rows, int64_t *d_out, uint8_t *d_nonempty) {
    return weighted_dense(gen, d_x, values_are_logs, n_rows, d_out, d_nonempty, kDevice);
}

int mhx_weighted_minhash_many_dense(mhx_wgen *gen, const float *x, int values_are_logs, int64_t n_rows, int64_t *out, uint8_t *nonempty) {
    return weighted_dense(gen, x, values_are_logs, n_rows, out, nonempty, kHost);
}

// ---- all-pairs Jaccard (jaccard_kernels.hip) -------------------------------------------------
// Shared argument checks.  b < 0: dense rows of sig_dtype (kWeightedRows: weighted rows of k samples), else b-bit blocks.
static int check_all_pairs(int64_t n_a, int64_t n_b, int sig_dtype, int32_t k, int32_t b) {
    MHX_CHECK_DTYPE(sig_dtype);
    if (b >= 0) MHX_CHECK_B(b);
    MHX_REQUIRE(k > 0, "%s must be positive", b == mhx::kWeightedRows ? "samples" : "num_perm");
    MHX_REQUIRE(n_a >= 0 && n_b >= 0, "bad shape");
    MHX_CHECK_ROWS32(n_a);
    MHX_CHECK_ROWS32(n_b);
    return MHX_OK;
}

// The matrix of counts.  Host form: B staged once (Aux); A and the counts go through In / Out in row blocks
static int all_pairs_matrix(mhx_ctx *ctx, const void *a, int64_t n_a, const void *b, int64_t n_b, int sig_dtype, int32_t k, int32_t bb,
                            int32_t *counts, int64_t ldc, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_all_pairs(n_a, n_b, sig_dtype, k, bb));
    if (!b) {
        b = a;
        n_b = n_a;
    }
    if (where == kHost) ldc = n_b;  // the host matrix is dense
    MHX_REQUIRE(ldc >= n_b, "ldc must be >= n_b");
    if (n_a == 0 || n_b == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(a && counts, where);
    MHX_TRY(ctx->activate());
    if (where == kDevice) return mhx::launch_jaccard_matrix(ctx, a, n_a, b, n_b, sig_dtype, k, bb, counts, ldc);
    const size_t row_bytes = sizeof(uint64_t) * jaccard_row_words(k, bb);
    const size_t out_row = sizeof(int32_t) * (size_t)n_b;
    const int64_t block = std::max<int64_t>(1, std::min<int64_t>(n_a, (int64_t)((256ull << 20) / out_row)));
    Stage s(ctx);
    const auto p_b = s.piece(Stage::Aux, row_bytes * (size_t)n_b);
    const auto p_a = s.piece(Stage::In, row_bytes * (size_t)block);
    const auto p_counts = s.piece(Stage::Out, out_row * (size_t)block);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_b, b));
    for (int64_t i0 = 0; i0 < n_a; i0 += block) {
        const int64_t m = std::min<int64_t>(block, n_a - i0);
        MHX_TRY(s.upload(p_a, (const char *)a + (size_t)i0 * row_bytes, row_bytes * (size_t)m));
        MHX_TRY(mhx::launch_jaccard_matrix(ctx, s.at<void>(p_a), m, s.at<void>(p_b), n_b, sig_dtype, k, bb, s.at<int32_t>(p_counts), n_b));
        MHX_TRY(s.download(counts + i0 * n_b, p_counts, out_row * (size_t)m));
        MHX_TRY(s.synchronize());
    }
    return MHX_OK;
}

// Pairs with at least min_count agreeing positions.  Host form: A in In, B in Aux, pairs | counts in Out
static int all_pairs_threshold(mhx_ctx *ctx, const void *a, int64_t n_a, const void *b, int64_t n_b, int sig_dtype, int32_t k, int32_t bb,
                               int32_t min_count, int64_t *pairs, int32_t *counts, int64_t capacity, int64_t *n_pairs, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_pairs, "n_pairs is NULL");
    *n_pairs = 0;
    MHX_TRY(check_all_pairs(n_a, n_b, sig_dtype, k, bb));
    MHX_REQUIRE(capacity >= 0, "bad capacity");
    if (!b) n_b = n_a;
    if (n_a == 0 || n_b == 0 || min_count > k) return MHX_OK;
    MHX_REQUIRE_POINTERS(a && ((pairs && counts) || capacity == 0), where);
    MHX_TRY(ctx->activate());
    if (where == kDevice)
        return mhx::launch_jaccard_threshold(ctx, a, n_a, b, n_b, sig_dtype, k, bb, min_count, pairs, counts, capacity, n_pairs);
    const size_t row_bytes = sizeof(uint64_t) * jaccard_row_words(k, bb);
    Stage s(ctx);
    const auto p_a = s.piece(Stage::In, row_bytes * (size_t)n_a);
    const auto p_b = b ? s.piece(Stage::Aux, row_bytes * (size_t)n_b) : Stage::Piece{};
    const auto p_pairs = s.piece(Stage::Out, sizeof(int64_t) * 2 * (size_t)capacity);
    const auto p_counts = s.piece(Stage::Out, sizeof(int32_t) * (size_t)capacity);
    s.ask(Stage::Out, p_counts.at + p_counts.bytes + 256);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_a, a));
    if (b) MHX_TRY(s.upload(p_b, b));
    MHX_TRY(mhx::launch_jaccard_threshold(ctx, s.at<void>(p_a), n_a, b ? s.at<void>(p_b) : nullptr, n_b, sig_dtype, k, bb, min_count,
                                          capacity ? s.at<int64_t>(p_pairs) : nullptr, capacity ? s.at<int32_t>(p_counts) : nullptr,
                                          capacity, n_pairs));
    if (*n_pairs > 0 && *n_pairs <= capacity) {
        MHX_TRY(s.download(pairs, p_pairs, sizeof(int64_t) * 2 * (size_t)*n_pairs));
        MHX_TRY(s.download(counts, p_counts, sizeof(int32_t) * (size_t)*n_pairs));
    }
    return s.synchronize();
}

// The k best rows of B per row of A.  Host form: A staged once (In), B streams through Aux in row blocks whose lists the merge
// kernel folds into the running ones (Offsets), the unpacked lists come back through Out
static int all_pairs_topk(mhx_ctx *ctx, const void *a, int64_t n_a, const void *b, int64_t n_b, int sig_dtype, int32_t k, int32_t bb,
                          const uint32_t *live_bits, int32_t min_count, int32_t topk, int64_t *rows, int32_t *counts, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_all_pairs(n_a, n_b, sig_dtype, k, bb));
    MHX_REQUIRE(topk >= 1 && topk <= MHX_TOPK_MAX, "k must be in [1, %d]", MHX_TOPK_MAX);
    const bool self = b == nullptr;
    if (self) n_b = n_a;
    if (n_a == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(a && rows && counts, where);
    MHX_TRY(ctx->activate());
    if (where == kDevice)
        return mhx::launch_jaccard_topk(ctx, a, n_a, self ? a : b, n_b, sig_dtype, k, bb, live_bits, min_count, topk, self, nullptr, 0, nullptr,
                                        rows, counts);
    const size_t row_bytes = sizeof(uint64_t) * jaccard_row_words(k, bb);
    const size_t list_bytes = (size_t)n_a * (size_t)topk;
    const size_t block_bytes = ctx->opt_host_chunk_bytes > 0 ? (size_t)ctx->opt_host_chunk_bytes : (size_t)256 << 20;
    const int64_t block = self ? n_b : std::max<int64_t>(1, std::min<int64_t>(n_b, (int64_t)(block_bytes / row_bytes)));
    Stage s(ctx);
    const auto p_a = s.piece(Stage::In, row_bytes * (size_t)n_a);
    const auto p_b = self ? Stage::Piece{} : s.piece(Stage::Aux, row_bytes * (size_t)block);
    const auto p_keys = s.piece(Stage::Offsets, sizeof(uint64_t) * list_bytes);
    const auto p_rows = s.piece(Stage::Out, sizeof(int64_t) * list_bytes);
    const auto p_counts = s.piece(Stage::Out, sizeof(int32_t) * list_bytes);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_a, a));
    int64_t j0 = 0;
    do {  // (once, with nothing to compare, when B is empty: the padding)
        const int64_t m = std::min<int64_t>(block, n_b - j0);
        const bool first = j0 == 0, last = j0 + m >= n_b;
        if (!self) MHX_TRY(s.upload(p_b, (const char *)b + (size_t)j0 * row_bytes, row_bytes * (size_t)m));  // (stream order: behind the previous block's kernels)
        MHX_TRY(mhx::launch_jaccard_topk(ctx, s.at<void>(p_a), n_a, self ? s.at<void>(p_a) : s.at<void>(p_b), m, sig_dtype, k, bb, nullptr,
                                         min_count, topk, self, first ? nullptr : s.at<uint64_t>(p_keys), (uint32_t)j0,
                                         s.at<uint64_t>(p_keys), last ? s.at<int64_t>(p_rows) : nullptr,
                                         last ? s.at<int32_t>(p_counts) : nullptr));
        j0 += m;
    } while (j0 < n_b);
    MHX_TRY(s.download(rows, p_rows));
    return s.fetch(counts, p_counts);
}

int mhx_jaccard_matrix_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t num_perm,
                           int32_t *d_counts, int64_t ldc) {
    return all_pairs_matrix(ctx, d_a, n_a, d_b, n_b, sig_dtype, num_perm, -1, d_counts, ldc, kDevice);
}

int mhx_jaccard_matrix(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b, int32_t num_perm, int32_t *counts) {
    return all_pairs_matrix(ctx, a, n_a, b, n_b, MHX_U64, num_perm, -1, counts, 0, kHost);
}

int mhx_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t num_perm,
                                    int32_t min_count, int64_t *d_pairs, int32_t *d_counts, int64_t capacity, int64_t *n_pairs) {
    return all_pairs_threshold(ctx, d_a, n_a, d_b, n_b, sig_dtype, num_perm, -1, min_count, d_pairs, d_counts, capacity, n_pairs, kDevice);
}

int mhx_jaccard_threshold_pairs(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b, int32_t num_perm,
                                int32_t min_count, int64_t *pairs, int32_t *counts, int64_t capacity, int64_t *n_pairs) {
    return all_pairs_threshold(ctx, a, n_a, b, n_b, MHX_U64, num_perm, -1, min_count, pairs, counts, capacity, n_pairs, kHost);
}

// (the b-bit entries check b themselves: a negative b means dense rows to the cores)
int mhx_bbit_jaccard_matrix_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b, int32_t num_perm,
                                int32_t b, int32_t *d_counts, int64_t ldc) {
    MHX_CHECK_B(b);
    return all_pairs_matrix(ctx, d_a, n_a, d_b, n_b, MHX_U64, num_perm, b, d_counts, ldc, kDevice);
}

int mhx_bbit_jaccard_matrix(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b, int32_t num_perm,
                            int32_t b, int32_t *counts) {
    MHX_CHECK_B(b);
    return all_pairs_matrix(ctx, a, n_a, b_blocks, n_b, MHX_U64, num_perm, b, counts, 0, kHost);
}

int mhx_bbit_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b, int32_t num_perm,
                                         int32_t b, int32_t min_count, int64_t *d_pairs, int32_t *d_counts, int64_t capacity, int64_t *n_pairs) {
    if (n_pairs) *n_pairs = 0;
    MHX_CHECK_B(b);
    return all_pairs_threshold(ctx, d_a, n_a, d_b, n_b, MHX_U64, num_perm, b, min_count, d_pairs, d_counts, capacity, n_pairs, kDevice);
}

int mhx_bbit_jaccard_threshold_pairs(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b, int32_t num_perm, int32_t b,
                                     int32_t min_count, int64_t *pairs, int32_t *counts, int64_t capacity, int64_t *n_pairs) {
    if (n_pairs) *n_pairs = 0;
    MHX_CHECK_B(b);
    return all_pairs_threshold(ctx, a, n_a, b_blocks, n_b, MHX_U64, num_perm, b, min_count, pairs, counts, capacity, n_pairs, kHost);
}

int mhx_jaccard_topk_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype, int32_t num_perm,
                         const uint32_t *d_b_live_bits, int32_t min_count, int32_t k, int64_t *d_rows, int32_t *d_counts) {
    return all_pairs_topk(ctx, d_a, n_a, d_b, n_b, sig_dtype, num_perm, -1, d_b_live_bits, min_count, k, d_rows, d_counts, kDevice);
}

int mhx_jaccard_topk(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b, int32_t num_perm, int32_t min_count,
                     int32_t k, int64_t *rows, int32_t *counts) {
    return all_pairs_topk(ctx, a, n_a, b, n_b, MHX_U64, num_perm, -1, nullptr, min_count, k, rows, counts, kHost);
}

int mhx_bbit_jaccard_topk_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b, int32_t num_perm, int32_t b,
                              const uint32_t *d_b_live_bits, int32_t min_count, int32_t k, int64_t *d_rows, int32_t *d_counts) {
    MHX_CHECK_B(b);
    return all_pairs_topk(ctx, d_a, n_a, d_b, n_b, MHX_U64, num_perm, b, d_b_live_bits, min_count, k, d_rows, d_counts, kDevice);
}

int mhx_bbit_jaccard_topk(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b, int32_t num_perm, int32_t b,
                          int32_t min_count, int32_t k, int64_t *rows, int32_t *counts) {
    MHX_CHECK_B(b);
    return all_pairs_topk(ctx, a, n_a, b_blocks, n_b, MHX_U64, num_perm, b, nullptr, min_count, k, rows, counts, kHost);
}

// ---- weighted Jaccard (mhx_weighted_jaccard.h): the cores above on rows of (k, t) samples --------
int mhx_weighted_jaccard_pairs_dev(mhx_ctx *ctx, const int64_t *d_sig_a, const int64_t *d_sig_b, int32_t samples, const int64_t *d_pairs,
                                   int64_t n_pairs, int32_t *d_counts) {
    return listed_pairs(ctx, d_sig_a, d_sig_b, 0, MHX_U64, samples, mhx::kWeightedRows, d_pairs, n_pairs, d_counts, kDevice);
}

int mhx_weighted_jaccard_pairs(mhx_ctx *ctx, const int64_t *sig, int64_t n, int32_t samples, const int64_t *pairs, int64_t n_pairs,
                               int32_t *counts) {
    return listed_pairs(ctx, sig, sig, n, MHX_U64, samples, mhx::kWeightedRows, pairs, n_pairs, counts, kHost);
}

int mhx_weighted_jaccard_matrix_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b, int32_t samples,
                                    int32_t *d_counts, int64_t ldc) {
    return all_pairs_matrix(ctx, d_a, n_a, d_b, n_b, MHX_U64, samples, mhx::kWeightedRows, d_counts, ldc, kDevice);
}

int mhx_weighted_jaccard_matrix(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b, int32_t samples,
                                int32_t *counts) {
    return all_pairs_matrix(ctx, a, n_a, b, n_b, MHX_U64, samples, mhx::kWeightedRows, counts, 0, kHost);
}

int mhx_weighted_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b, int32_t samples,
                                             int32_t min_count, int64_t *d_pairs, int32_t *d_counts, int64_t capacity, int64_t *n_pairs) {
    return all_pairs_threshold(ctx, d_a, n_a, d_b, n_b, MHX_U64, samples, mhx::kWeightedRows, min_count, d_pairs, d_counts, capacity, n_pairs,
                               kDevice);
}

int mhx_weighted_jaccard_threshold_pairs(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b, int32_t samples,
                                         int32_t min_count, int64_t *pairs, int32_t *counts, int64_t capacity, int64_t *n_pairs) {
    return all_pairs_threshold(ctx, a, n_a, b, n_b, MHX_U64, samples, mhx::kWeightedRows, min_count, pairs, counts, capacity, n_pairs, kHost);
}

int mhx_weighted_jaccard_topk_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b, int32_t samples,
                                  const uint32_t *d_b_live_bits, int32_t min_count, int32_t k, int64_t *d_rows, int32_t *d_counts) {
    return all_pairs_topk(ctx, d_a, n_a, d_b, n_b, MHX_U64, samples, mhx::kWeightedRows, d_b_live_bits, min_count, k, d_rows, d_counts, kDevice);
}

int mhx_weighted_jaccard_topk(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b, int32_t samples, int32_t min_count,
                              int32_t k, int64_t *rows, int32_t *counts) {
    return all_pairs_topk(ctx, a, n_a, b, n_b, MHX_U64, samples, mhx::kWeightedRows, nullptr, min_count, k, rows, counts, kHost);
}

int mhx_lsh_bands_merge_dev(mhx_ctx *ctx, const uint64_t *d_dig_a, const uint32_t *d_rows_a, int64_t n_a, const uint64_t *d_dig_b,
                            const uint32_t *d_rows_b, int64_t n_b, uint32_t row_offset_b, int32_t bands, uint64_t *d_dig_out,
                            uint32_t *d_rows_out) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(bands > 0, "bands must be positive");
    MHX_REQUIRE(n_a >= 0 && n_b >= 0, "bad shape");
    MHX_REQUIRE(n_a + n_b < ((int64_t)1 << 32), "more than 2^32-1 entries per band");
    if (n_a + n_b == 0) return MHX_OK;
    MHX_REQUIRE((n_a == 0 || (d_dig_a && d_rows_a)) && (n_b == 0 || (d_dig_b && d_rows_b)) && d_dig_out && d_rows_out,
                "NULL device pointer");
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_bands_merge(ctx, d_dig_a, d_rows_a, n_a, d_dig_b, d_rows_b, n_b, row_offset_b, bands, d_dig_out, d_rows_out);
}

int mhx_lsh_bands_compact_dev(mhx_ctx *ctx, const uint64_t *d_dig, const uint32_t *d_rows, int64_t n, int32_t bands,
                              const uint32_t *d_live_bits, int64_t n_live, uint64_t *d_dig_out, uint32_t *d_rows_out) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(bands > 0, "bands must be positive");
    MHX_REQUIRE(n >= 0 && n_live >= 0 && n_live <= n, "bad shape");
    MHX_CHECK_ROWS32(n);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE(d_dig && d_rows && d_live_bits && ((d_dig_out && d_rows_out) || n_live == 0), "NULL device pointer");
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_bands_compact(ctx, d_dig, d_rows, n, bands, d_live_bits, n_live, d_dig_out, d_rows_out);
}

int mhx_rows_compact_dev(mhx_ctx *ctx, const void *d_src, int64_t row_bytes, int64_t n_rows, const uint32_t *d_live_bits, void *d_dst,
                         int64_t *n_kept) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_kept, "n_kept is NULL");
    *n_kept = 0;
    MHX_REQUIRE(row_bytes > 0 && n_rows >= 0, "bad shape");
    MHX_CHECK_ROWS32(n_rows);
    MHX_REQUIRE(n_rows == 0 || row_bytes <= INT64_MAX / n_rows, "row_bytes * n_rows overflows");
    if (n_rows == 0) return MHX_OK;
    MHX_REQUIRE(d_src && d_live_bits && d_dst, "NULL device pointer");
    MHX_TRY(ctx->activate());
    return mhx::launch_rows_compact(ctx, d_src, row_bytes, n_rows, d_live_bits, d_dst, n_kept);
}

int mhx_lsh_forest_build_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t row_words, int32_t l,
                                   int32_t tree_words, uint32_t *d_order) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_REQUIRE(l > 0 && l < 65536, "l must be in [1, 65535]");
    MHX_REQUIRE(tree_words > 0 && row_words > 0 && (int64_t)l * tree_words <= row_words, "l * tree_words must be in [1, row_words]");
    MHX_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), "n_sigs must be in [0, 2^32)");
    if (n == 0) return MHX_OK;
    MHX_REQUIRE(d_sig && d_order, "NULL device pointer");
    MHX_TRY(ctx->activate());
    return mhx::launch_lsh_forest_build(ctx, d_sig, sig_dtype, n, row_words, l, tree_words, d_order);
}

int mhx_lsh_forest_query_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t row_words, int32_t l,
                                   int32_t tree_words, int32_t w, const uint32_t *d_order, const void *d_probes, int64_t m, int32_t k,
                                   uint32_t *d_slots, int32_t *d_counts) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_REQUIRE(l > 0 && l < 65536, "l must be in [1, 65535]");
    MHX_REQUIRE(tree_words > 0 && row_words > 0 && (int64_t)l * tree_words <= row_words, "l * tree_words must be in [1, row_words]");
    MHX_REQUIRE((w == 1 || w == 2) && tree_words % w == 0 && tree_words / w < 65536, "w must be 1 or 2 and divide tree_words");
    MHX_REQUIRE(k > 0, "k must be positive");
    MHX_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), "n_sigs must be in [0, 2^32)");
    MHX_REQUIRE(m >= 0 && m < ((int64_t)1 << 31), "m must be in [0, 2^31)");
    if (m == 0) return MHX_OK;
    MHX_REQUIRE(d_counts, "NULL device pointer");
    MHX_TRY(ctx->activate());
    if (n == 0) {
        MHX_HIP_CHECK(hipMemsetAsync(d_counts, 0, sizeof(int32_t) * (size_t)m, ctx->stream));
        return MHX_OK;
    }
    MHX_REQUIRE(d_sig && d_order && d_probes && d_slots, "NULL device pointer");
    return mhx::launch_lsh_forest_query(ctx, d_sig, sig_dtype, n, row_words, l, tree_words, w, d_order, d_probes, m, k, d_slots, d_counts);
}

// ---- HyperLogLog (ref: datasketch/hyperloglog.py) ------------------------------------------------------------------------
static int check_hll(int p, int hash_bits) {
    MHX_REQUIRE(p >= 4 && p <= 16, "p=%d should be in range [4 : 16]", p);  // ref: hyperloglog.py:56-57
    MHX_REQUIRE(hash_bits == 32 || hash_bits == 64, "hash_bits must be 32 (HyperLogLog) or 64 (HyperLogLog++), not %d", hash_bits);
    return MHX_OK;
}
// rows are read and written as 32-bit words
#define MHX_CHECK_HLL_ALIGNED(ptr) MHX_REQUIRE(((uintptr_t)(ptr) & 3) == 0, #ptr " must be 4-byte aligned")

int mhx_hll_layout(int p, int *layout) {
    MHX_TRY(check_hll(p, 32));
    MHX_REQUIRE(layout, "layout is NULL");
    *layout = mhx::hll_layout(p);
    return MHX_OK;
}

static int hll_bulk(mhx_ctx *ctx, const void *hv, int hv_dtype, const int64_t *offsets, int64_t fixed_len, int64_t n_sets, int64_t total_tokens,
                    int p, int hash_bits, const uint8_t *init, int64_t init_stride, uint8_t *out, int64_t *overflow, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_sets >= 0, "n_sets must be >= 0");
    MHX_CHECK_DTYPE(hv_dtype);
    MHX_TRY(check_hll(p, hash_bits));
    const int64_t m = (int64_t)1 << p;
    MHX_REQUIRE(offsets || fixed_len >= 0, "fixed_len must be >= 0 when offsets is NULL");
    MHX_REQUIRE(init_stride == 0 || init_stride == m, "init_stride must be 0 (one shared row) or m = %lld", (long long)m);
    const bool can_overflow = hv_dtype == MHX_U64 && hash_bits == 32;
    MHX_REQUIRE(overflow || !can_overflow, "uint64 hashes at hash_bits = 32 need the overflow counter");
    if (where == kHost && overflow) *overflow = 0;
    if (n_sets == 0) {
        if (where == kDevice && overflow) {
            MHX_TRY(ctx->activate());
            MHX_HIP_CHECK(hipMemsetAsync(overflow, 0, sizeof(int64_t), ctx->stream));
        }
        return MHX_OK;
    }
    MHX_REQUIRE_POINTERS(out, where);
    MHX_TRY(ctx->activate());
    if (where == kDevice) {
        MHX_REQUIRE(total_tokens >= 0, "total_tokens must be >= 0");
        MHX_REQUIRE(hv || total_tokens == 0, "d_hv is NULL");
        MHX_CHECK_HLL_ALIGNED(out);
        MHX_CHECK_HLL_ALIGNED(init);
        if (overflow) MHX_HIP_CHECK(hipMemsetAsync(overflow, 0, sizeof(int64_t), ctx->stream));
        return mhx::launch_hll_bulk(ctx, hv, hv_dtype, offsets, fixed_len, n_sets, total_tokens, p, hash_bits, init, init_stride, out, overflow);
    }
    int64_t total = n_sets * fixed_len;
    if (offsets) {
        MHX_REQUIRE(offsets[0] >= 0, "offsets[0] must be >= 0");
        for (int64_t i = 0; i < n_sets; ++i)
            MHX_REQUIRE(offsets[i + 1] >= offsets[i], "offsets must be non-decreasing (row %lld)", (long long)i);
        total = offsets[n_sets];
    }
    MHX_REQUIRE(hv || total == 0, "hv is NULL");
    Stage s(ctx);
    const auto p_hv = s.piece(Stage::In, (hv_dtype == MHX_U32 ? 4 : 8) * (size_t)total);
    if (total == 0) s.ask(Stage::In, 8);
    Stage::Piece p_off{Stage::Aux, 0, 0}, p_init{Stage::Aux, 0, 0};
    if (offsets) p_off = s.piece(Stage::Aux, sizeof(int64_t) * (size_t)(n_sets + 1));
    if (init) p_init = s.piece(Stage::Aux, (size_t)(init_stride ? n_sets * m : m));
    const auto p_out = s.piece(Stage::Out, (size_t)(n_sets * m)), p_ovf = s.piece(Stage::Out, sizeof(int64_t));
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_hv, hv));
    MHX_TRY(s.upload(p_off, offsets));
    MHX_TRY(s.upload(p_init, init));
    MHX_HIP_CHECK(hipMemsetAsync(s.at<void>(p_ovf), 0, sizeof(int64_t), ctx->stream));
    MHX_TRY(mhx::launch_hll_bulk(ctx, s.at<void>(p_hv), hv_dtype, offsets ? s.at<int64_t>(p_off) : nullptr, fixed_len, n_sets, total, p, hash_bits,
                                 init ? s.at<uint8_t>(p_init) : nullptr, init_stride, s.at<uint8_t>(p_out), s.at<int64_t>(p_ovf)));
    int64_t count = 0;
    MHX_TRY(s.download(&count, p_ovf));
    MHX_TRY(s.fetch(out, p_out));
    if (overflow) *overflow = count;
    return MHX_OK;
}

int mhx_hll_bulk_dev(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets,
                     int64_t total_tokens, int32_t p, int32_t hash_bits, const uint8_t *d_init, int64_t init_stride, uint8_t *d_out,
                     int64_t *d_overflow) {
    return hll_bulk(ctx, d_hv, hv_dtype, d_offsets, fixed_len, n_sets, total_tokens, p, hash_bits, d_init, init_stride, d_out, d_overflow, kDevice);
}

int mhx_hll_bulk_typed(mhx_ctx *ctx, const void *hv, int hv_dtype, const int64_t *offsets, int64_t fixed_len, int64_t n_sets, int32_t p,
                       int32_t hash_bits, const uint8_t *init, int64_t init_stride, uint8_t *out, int64_t *overflow) {
    return hll_bulk(ctx, hv, hv_dtype, offsets, fixed_len, n_sets, 0, p, hash_bits, init, init_stride, out, overflow, kHost);
}

static int hll_histogram(mhx_ctx *ctx, const uint8_t *reg, int64_t n, int p, uint32_t *hist, int64_t *invalid, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_hll(p, 32));
    MHX_REQUIRE(n >= 0, "n must be >= 0");
    MHX_REQUIRE_POINTERS(invalid, where);
    MHX_TRY(ctx->activate());
    if (where == kHost) *invalid = 0;
    else MHX_HIP_CHECK(hipMemsetAsync(invalid, 0, sizeof(int64_t), ctx->stream));
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(reg && hist, where);
    if (where == kDevice) {
        MHX_CHECK_HLL_ALIGNED(reg);
        return mhx::launch_hll_histogram(ctx, reg, n, p, hist, invalid);
    }
    Stage s(ctx);
    const auto p_reg = s.piece(Stage::In, (size_t)n << p);
    const auto p_hist = s.piece(Stage::Out, sizeof(uint32_t) * 64 * (size_t)n), p_bad = s.piece(Stage::Out, sizeof(int64_t));
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_reg, reg));
    MHX_HIP_CHECK(hipMemsetAsync(s.at<void>(p_bad), 0, sizeof(int64_t), ctx->stream));
    MHX_TRY(mhx::launch_hll_histogram(ctx, s.at<uint8_t>(p_reg), n, p, s.at<uint32_t>(p_hist), s.at<int64_t>(p_bad)));
    MHX_TRY(s.download(invalid, p_bad));
    return s.fetch(hist, p_hist);
}

int mhx_hll_histogram_dev(mhx_ctx *ctx, const uint8_t *d_reg, int64_t n, int32_t p, uint32_t *d_hist, int64_t *d_invalid) {
    return hll_histogram(ctx, d_reg, n, p, d_hist, d_invalid, kDevice);
}

int mhx_hll_histogram(mhx_ctx *ctx, const uint8_t *reg, int64_t n, int32_t p, uint32_t *hist, int64_t *invalid) {
    return hll_histogram(ctx, reg, n, p, hist, invalid, kHost);
}

int mhx_hll_merge_dev(mhx_ctx *ctx, uint8_t *d_a, const uint8_t *d_b, int64_t count) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(count >= 0, "count must be >= 0");
    if (count == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_a && d_b, kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_hll_merge(ctx, d_a, d_b, count);
}

static int hll_union_groups(mhx_ctx *ctx, const uint8_t *reg, int64_t n_rows, int p, const int64_t *group_offsets, int64_t n_groups,
                            uint8_t *out, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_hll(p, 32));
    MHX_REQUIRE(n_rows >= 0 && n_groups >= 0, "n_rows and n_groups must be >= 0");
    if (n_groups == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(group_offsets && out && (reg || n_rows == 0), where);
    MHX_TRY(ctx->activate());
    if (where == kDevice) {
        MHX_CHECK_HLL_ALIGNED(reg);
        MHX_CHECK_HLL_ALIGNED(out);
        return mhx::launch_hll_union_groups(ctx, reg, p, group_offsets, n_groups, out);
    }
    MHX_REQUIRE(group_offsets[0] >= 0 && group_offsets[n_groups] <= n_rows, "group_offsets must stay inside [0, n_rows]");
    for (int64_t g = 0; g < n_groups; ++g)
        MHX_REQUIRE(group_offsets[g + 1] >= group_offsets[g], "group_offsets must be non-decreasing (group %lld)", (long long)g);
    Stage s(ctx);
    const auto p_reg = s.piece(Stage::In, (size_t)n_rows << p);
    if (n_rows == 0) s.ask(Stage::In, 8);
    const auto p_off = s.piece(Stage::Aux, sizeof(int64_t) * (size_t)(n_groups + 1));
    const auto p_out = s.piece(Stage::Out, (size_t)n_groups << p);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_reg, reg));
    MHX_TRY(s.upload(p_off, group_offsets));
    MHX_TRY(mhx::launch_hll_union_groups(ctx, s.at<uint8_t>(p_reg), p, s.at<int64_t>(p_off), n_groups, s.at<uint8_t>(p_out)));
    return s.fetch(out, p_out);
}

int mhx_hll_union_groups_dev(mhx_ctx *ctx, const uint8_t *d_reg, int64_t n_rows, int32_t p, const int64_t *d_group_offsets, int64_t n_groups,
                             uint8_t *d_out) {
    return hll_union_groups(ctx, d_reg, n_rows, p, d_group_offsets, n_groups, d_out, kDevice);
}

int mhx_hll_union_groups(mhx_ctx *ctx, const uint8_t *reg, int64_t n_rows, int32_t p, const int64_t *group_offsets, int64_t n_groups,
                         uint8_t *out) {
    return hll_union_groups(ctx, reg, n_rows, p, group_offsets, n_groups, out, kHost);
}

// ---- shingles: the windows of a document hashed in place (datasketch_amd/shingle.py is the definition) ---------------------
static int check_windows(int64_t n_docs, int64_t width) {
    MHX_REQUIRE(width >= 1, "width must be >= 1");
    MHX_REQUIRE(n_docs >= 0, "n_docs must be >= 0");
    return MHX_OK;
}

int mhx_shingle_window_offsets(const int64_t *doc_offsets, int64_t n_docs, int64_t width, int64_t *set_offsets) {
    MHX_TRY(check_windows(n_docs, width));
    MHX_REQUIRE(doc_offsets && set_offsets, "doc_offsets/set_offsets is NULL");
    set_offsets[0] = 0;
    for (int64_t d = 0; d < n_docs; ++d) {
        const int64_t items = doc_offsets[d + 1] - doc_offsets[d];
        MHX_REQUIRE(items >= 0, "doc_offsets must be non-decreasing (document %lld)", (long long)d);
        set_offsets[d + 1] = set_offsets[d] + (items == 0 ? 0 : items < width ? 1 : items - width + 1);
    }
    return MHX_OK;
}

int mhx_sha1_windows_dev(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_item_offsets, const int64_t *d_doc_offsets,
                         const int64_t *d_set_offsets, int64_t n_docs, int64_t n_windows, int64_t width, int out_dtype, void *d_out) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_windows(n_docs, width));
    MHX_REQUIRE(n_windows >= 0, "n_windows must be >= 0");
    MHX_CHECK_DTYPE(out_dtype);
    if (n_docs == 0 || n_windows == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_doc_offsets && d_set_offsets && d_out, kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_sha1_windows(ctx, d_bytes, d_item_offsets, d_doc_offsets, d_set_offsets, n_docs, n_windows, width, out_dtype, d_out);
}

extern "C++" {
namespace {

// windows over the bytes (item_offsets NULL) or the tokens of documents: a source (see Tokens).  Offsets: item offsets | document
// offsets | set offsets.
struct Windows {
    static constexpr const char *kNoOut = "out is NULL";
    const uint8_t *bytes;
    const int64_t *item_offsets;
    int64_t n_items;
    const int64_t *doc_offsets;
    int64_t n_docs, width;
    int hash_kind = MHX_HASH_SHA1;
    std::vector<int64_t> set_offsets;  // (alive until the call has synchronised: it is uploaded from)
    int64_t n_bytes = 0, n_hashes = 0;  // n_hashes: the number of windows, known from check_arrays() on
    uint8_t *d_bytes = nullptr;
    int64_t *d_items = nullptr, *d_docs = nullptr, *d_sets = nullptr;

    int check_sizes() const { return check_windows(n_docs, width); }
    int64_t n_sets() const { return n_docs; }
    int64_t max_hashes() const { return n_hashes; }
    const int64_t *host_sets() const { return set_offsets.data(); }

    int check_arrays() {
        MHX_REQUIRE(n_items >= 0, "n_items must be >= 0");
        MHX_REQUIRE(doc_offsets, "doc_offsets is NULL");
        MHX_REQUIRE(doc_offsets[0] == 0 && doc_offsets[n_docs] == n_items, "doc_offsets must run from 0 to n_items");
        if (item_offsets) {
            MHX_REQUIRE(item_offsets[0] == 0, "item_offsets[0] must be 0");
            for (int64_t i = 0; i < n_items; ++i)
                MHX_REQUIRE(item_offsets[i + 1] >= item_offsets[i], "item_offsets must be non-decreasing (item %lld)", (long long)i);
        }
        n_bytes = item_offsets ? item_offsets[n_items] : n_items;
        MHX_REQUIRE(bytes || n_bytes == 0, "bytes is NULL");
        set_offsets.resize((size_t)n_docs + 1);
        MHX_TRY(mhx_shingle_window_offsets(doc_offsets, n_docs, width, set_offsets.data()));
        n_hashes = set_offsets[(size_t)n_docs];
        return MHX_OK;
    }

    int stage(mhx_ctx *ctx) {
        Stage s(ctx);
        const auto p_bytes = s.piece(Stage::In, (size_t)n_bytes);
        if (n_bytes == 0) s.ask(Stage::In, 8);
        Stage::Piece p_items{Stage::Offsets, 0, 0};
        if (item_offsets) p_items = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n_items + 1));
        const auto p_docs = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n_docs + 1)), p_sets = s.piece(Stage::Offsets, p_docs.bytes);
        MHX_TRY(s.commit());
        d_bytes = s.at<uint8_t>(p_bytes);
        d_items = item_offsets ? s.at<int64_t>(p_items) : nullptr;
        d_docs = s.at<int64_t>(p_docs);
        d_sets = s.at<int64_t>(p_sets);
        MHX_TRY(s.upload(p_bytes, bytes));
        MHX_TRY(s.upload(p_items, item_offsets));
        MHX_TRY(s.upload(p_docs, doc_offsets));
        return s.upload(p_sets, set_offsets.data());
    }
    void reserve(Stage &) const {}
    int hash(const Stage &s, int dtype, void *d_hv) const {
        if (hash_kind == MHX_HASH_XXH) return mhx::launch_xxh_windows(s.ctx, d_bytes, d_items, d_docs, d_sets, n_docs, n_hashes, width, dtype, d_hv);
        return mhx::launch_sha1_windows(s.ctx, d_bytes, d_items, d_docs, d_sets, n_docs, n_hashes, width, dtype, d_hv);
    }
};

}  // namespace
}  // extern "C++"

int mhx_sha1_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                     int64_t n_docs, int64_t width, int out_dtype, void *out) {
    return mhx_hash_windows(ctx, bytes, item_offsets, n_items, doc_offsets, n_docs, width, MHX_HASH_SHA1, out_dtype, out);
}

int mhx_hash_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                     int64_t n_docs, int64_t width, int hash_kind, int out_dtype, void *out) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    Windows src{bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_kind};
    MHX_TRY(src.check_sizes());
    MHX_CHECK_DTYPE(out_dtype);
    if (n_docs == 0) return MHX_OK;
    MHX_TRY(src.check_arrays());
    if (src.n_hashes == 0) return MHX_OK;
    MHX_REQUIRE(out, "out is NULL");
    MHX_TRY(ctx->activate());
    MHX_TRY(src.stage(ctx));
    Stage s(ctx);
    const auto p_out = s.piece(Stage::Out, (size_t)src.n_hashes * (out_dtype == MHX_U32 ? 4 : 8));
    MHX_TRY(s.commit());
    MHX_TRY(src.hash(s, out_dtype, s.at<void>(p_out)));
    return s.fetch(out, p_out);
}

// ---- word shingles: text tokenised and normalised on the device (datasketch_amd/shingle.py is the definition) ---------------
static int check_words(int64_t n_bytes, int64_t n_docs, const uint8_t *table) {
    MHX_REQUIRE(n_bytes >= 0, "n_bytes must be >= 0");
    MHX_REQUIRE(n_docs >= 0, "n_docs must be >= 0");
    MHX_REQUIRE(table, "table is NULL");
    MHX_REQUIRE(table[0] == 0, "table[0] must be 0: byte 0 is always a separator");
    return MHX_OK;
}

// what follows the count, for device and host forms alike: the sizing call, the capacities, the outputs
static int check_words_outputs(const void *out_bytes, int64_t cap_bytes, const void *item_offsets, int64_t cap_words,
                               const void *word_doc_offsets, int64_t n_words, int64_t n_out_bytes, Where where, bool *emit) {
    *emit = false;
    if (!out_bytes && !item_offsets && !word_doc_offsets) return MHX_OK;  // a sizing call
    if (n_words > cap_words || n_out_bytes > cap_bytes)
        return fail(MHX_ERR_CAPACITY, "the normal form has %lld words and %lld bytes; the outputs hold %lld and %lld", (long long)n_words,
                    (long long)n_out_bytes, (long long)cap_words, (long long)cap_bytes);
    MHX_REQUIRE_POINTERS(item_offsets && word_doc_offsets && (out_bytes || n_out_bytes == 0), where);
    *emit = true;
    return MHX_OK;
}

int mhx_words_normalize_dev(mhx_ctx *ctx, const uint8_t *d_bytes, int64_t n_bytes, const int64_t *d_doc_offsets, int64_t n_docs,
                            const uint8_t *table, uint8_t *d_out_bytes, int64_t cap_bytes, int64_t *d_item_offsets, int64_t cap_words,
                            int64_t *d_word_doc_offsets, int64_t *n_words, int64_t *n_out_bytes) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_words && n_out_bytes, "n_words/n_out_bytes is NULL");
    *n_words = *n_out_bytes = 0;
    MHX_TRY(check_words(n_bytes, n_docs, table));
    MHX_REQUIRE(cap_bytes >= 0 && cap_words >= 0, "cap_bytes and cap_words must be >= 0");
    if (n_docs == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_doc_offsets && (d_bytes || n_bytes == 0), kDevice);
    MHX_TRY(ctx->activate());
    MHX_TRY(mhx::launch_words_count(ctx, d_bytes, n_bytes, d_doc_offsets, n_docs, table, n_words, n_out_bytes));
    bool emit = false;
    MHX_TRY(check_words_outputs(d_out_bytes, cap_bytes, d_item_offsets, cap_words, d_word_doc_offsets, *n_words, *n_out_bytes, kDevice, &emit));
    if (!emit) return MHX_OK;
    return mhx::launch_words_emit(ctx, d_bytes, n_bytes, d_doc_offsets, n_docs, table, d_out_bytes, d_item_offsets, d_word_doc_offsets);
}

extern "C++" {
namespace {

// the words of raw text in windows of `width`: a source (see Tokens).  Offsets: document offsets | word offsets of the documents |
// set offsets.  stage() also counts -- it blocks -- since everything after it is sized by the count; reserve() names where the
// normalised text and its item offsets go.
struct Words {
    static constexpr const char *kNoOut = "out is NULL";
    const uint8_t *bytes;
    int64_t n_bytes;
    const int64_t *doc_offsets;
    int64_t n_docs;
    const uint8_t *table;
    int64_t width;
    int hash_kind = MHX_HASH_SHA1;
    int64_t n_words = 0, n_out_bytes = 0, n_hashes = 0;
    uint8_t *d_bytes = nullptr;
    int64_t *d_docs = nullptr, *d_wdocs = nullptr, *d_sets = nullptr;
    Stage::Piece p_text{Stage::Aux, 0, 0}, p_items{Stage::Aux, 0, 0};
    std::vector<int64_t> wdocs, sets;  // (alive until the call has synchronised: they are uploaded from)

    int check_sizes() const {
        MHX_TRY(check_windows(n_docs, width));
        return check_words(n_bytes, n_docs, table);
    }
    int64_t n_sets() const { return n_docs; }
    int64_t max_hashes() const { return n_words; }  // (a document has no more windows than words)
    const int64_t *host_sets() const { return sets.data(); }  // (from hash() on)

    int check_arrays() const {
        MHX_REQUIRE(doc_offsets, "doc_offsets is NULL");
        MHX_REQUIRE(bytes || n_bytes == 0, "bytes is NULL");
        MHX_REQUIRE(doc_offsets[0] == 0 && doc_offsets[n_docs] == n_bytes, "doc_offsets must run from 0 to n_bytes");
        for (int64_t d = 0; d < n_docs; ++d)
            MHX_REQUIRE(doc_offsets[d + 1] >= doc_offsets[d], "doc_offsets must be non-decreasing (document %lld)", (long long)d);
        return MHX_OK;
    }

    int stage(mhx_ctx *ctx) {
        Stage s(ctx);
        const auto p_bytes = s.piece(Stage::In, (size_t)n_bytes);
        if (n_bytes == 0) s.ask(Stage::In, 8);
        const auto p_docs = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n_docs + 1)), p_wdocs = s.piece(Stage::Offsets, p_docs.bytes),
                   p_sets = s.piece(Stage::Offsets, p_docs.bytes);
        MHX_TRY(s.commit());
        d_bytes = s.at<uint8_t>(p_bytes);
        d_docs = s.at<int64_t>(p_docs);
        d_wdocs = s.at<int64_t>(p_wdocs);
        d_sets = s.at<int64_t>(p_sets);
        MHX_TRY(s.upload(p_bytes, bytes));
        MHX_TRY(s.upload(p_docs, doc_offsets));
        return mhx::launch_words_count(ctx, d_bytes, n_bytes, d_docs, n_docs, table, &n_words, &n_out_bytes);
    }
    void reserve(Stage &s) {
        p_text = s.piece(Stage::Aux, (size_t)n_out_bytes);
        p_items = s.piece(Stage::Aux, sizeof(int64_t) * (size_t)(n_words + 1));
    }

    int emit(mhx_ctx *ctx, uint8_t *d_text, int64_t *d_items) const {
        return mhx::launch_words_emit(ctx, d_bytes, n_bytes, d_docs, n_docs, table, d_text, d_items, d_wdocs);
    }
    // the set offsets of the windows of `width` words: 8 bytes per document down, mhx_shingle_window_offsets, 8 bytes up.  Blocks.
    int window_offsets(mhx_ctx *ctx) {
        wdocs.resize((size_t)n_docs + 1);
        sets.resize((size_t)n_docs + 1);
        const size_t bytes = sizeof(int64_t) * (size_t)(n_docs + 1);
        MHX_HIP_CHECK(hipMemcpyAsync(wdocs.data(), d_wdocs, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MHX_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        MHX_TRY(mhx_shingle_window_offsets(wdocs.data(), n_docs, width, sets.data()));
        n_hashes = sets[(size_t)n_docs];
        MHX_HIP_CHECK(hipMemcpyAsync(d_sets, sets.data(), bytes, hipMemcpyHostToDevice, ctx->stream));
        return MHX_OK;
    }
    int hash(const Stage &s, int dtype, void *d_hv) {
        MHX_TRY(emit(s.ctx, s.at<uint8_t>(p_text), s.at<int64_t>(p_items)));
        MHX_TRY(window_offsets(s.ctx));
        if (hash_kind == MHX_HASH_XXH)
            return mhx::launch_xxh_windows(s.ctx, s.at<uint8_t>(p_text), s.at<int64_t>(p_items), d_wdocs, d_sets, n_docs, n_hashes, width, dtype, d_hv);
        return mhx::launch_sha1_windows(s.ctx, s.at<uint8_t>(p_text), s.at<int64_t>(p_items), d_wdocs, d_sets, n_docs, n_hashes, width, dtype, d_hv);
    }
};

}  // namespace
}  // extern "C++"

int mhx_words_normalize(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                        const uint8_t *table, uint8_t *out_bytes, int64_t cap_bytes, int64_t *item_offsets, int64_t cap_words,
                        int64_t *word_doc_offsets, int64_t *n_words, int64_t *n_out_bytes) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n_words && n_out_bytes, "n_words/n_out_bytes is NULL");
    *n_words = *n_out_bytes = 0;
    MHX_TRY(check_words(n_bytes, n_docs, table));
    MHX_REQUIRE(cap_bytes >= 0 && cap_words >= 0, "cap_bytes and cap_words must be >= 0");
    if (n_docs == 0) return MHX_OK;
    Words w{bytes, n_bytes, doc_offsets, n_docs, table, /*width: no windows here*/ 0};
    MHX_TRY(w.check_arrays());
    MHX_TRY(ctx->activate());
    MHX_TRY(w.stage(ctx));
    *n_words = w.n_words;
    *n_out_bytes = w.n_out_bytes;
    bool emit = false;
    MHX_TRY(check_words_outputs(out_bytes, cap_bytes, item_offsets, cap_words, word_doc_offsets, w.n_words, w.n_out_bytes, kHost, &emit));
    if (!emit) return MHX_OK;
    Stage s(ctx);
    const auto p_text = s.piece(Stage::Out, (size_t)w.n_out_bytes), p_items = s.piece(Stage::Out, sizeof(int64_t) * (size_t)(w.n_words + 1));
    MHX_TRY(s.commit());
    MHX_TRY(w.emit(ctx, s.at<uint8_t>(p_text), s.at<int64_t>(p_items)));
    if (w.n_out_bytes) MHX_TRY(s.download(out_bytes, p_text));
    MHX_TRY(s.download(item_offsets, p_items));
    MHX_HIP_CHECK(hipMemcpyAsync(word_doc_offsets, w.d_wdocs, sizeof(int64_t) * (size_t)(n_docs + 1), hipMemcpyDeviceToHost, ctx->stream));
    return s.synchronize();
}

// ---- the sinks, and their entries: a source constructed, a sink called (the third sink, overlaps_of, is at the end of the file) ---
extern "C++" {
namespace {

// Aux: init | hashes (uint32 or uint64) | whatever the source reserves;  Out: signatures
template <class Source>
int minhash_of(mhx_perm *perm, Source &&src, int hash_dtype, const uint64_t *init, int64_t init_stride, void *out, int out_dtype) {
    MHX_REQUIRE(hash_dtype == MHX_U32 || hash_dtype == MHX_U64, "hash_dtype must be MHX_U32 (sha1_hash32) or MHX_U64 (sha1_hash64)");
    MHX_CHECK_DTYPE(out_dtype);
    MHX_REQUIRE(init_stride == 0 || init_stride >= perm->num_perm, "init_stride must be 0 or >= num_perm");
    MHX_TRY(src.check_sizes());
    const int64_t n = src.n_sets(), k = perm->num_perm;
    if (n == 0) return MHX_OK;
    MHX_REQUIRE(out, "%s", src.kNoOut);
    MHX_TRY(src.check_arrays());
    mhx_ctx *ctx = perm->ctx;
    MHX_TRY(ctx->activate());
    MHX_TRY(src.stage(ctx));
    Stage s(ctx);
    const auto p_init = s.piece(Stage::Aux, init ? sizeof(uint64_t) * (size_t)(init_stride ? n * init_stride : k) : 0);
    const auto p_hv = s.piece(Stage::Aux, (hash_dtype == MHX_U32 ? 4 : 8) * (size_t)src.max_hashes());
    src.reserve(s);
    const auto p_out = s.piece(Stage::Out, (out_dtype == MHX_U32 ? 4 : 8) * (size_t)(n * k));
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_init, init));
    MHX_TRY(src.hash(s, hash_dtype, s.at<void>(p_hv)));
    MHX_TRY(mhx::launch_minhash_bulk(perm, s.at<void>(p_hv), hash_dtype, src.d_sets, 0, n, src.n_hashes, init ? s.at<uint64_t>(p_init) : nullptr,
                                     init_stride, s.at<void>(p_out), out_dtype));
    return s.fetch(out, p_out);
}

// Aux: init | hashes (sha1_hash32 / sha1_hash64: they fit hash_bits by construction) | whatever the source reserves;  Out: registers
template <class Source>
int hll_of(mhx_ctx *ctx, Source &&src, int32_t hash_bits, int32_t p, const uint8_t *init, int64_t init_stride, uint8_t *out) {
    MHX_TRY(check_hll(p, hash_bits));
    const int64_t m = (int64_t)1 << p;
    MHX_REQUIRE(init_stride == 0 || init_stride == m, "init_stride must be 0 (one shared row) or m = %lld", (long long)m);
    MHX_TRY(src.check_sizes());
    const int64_t n = src.n_sets();
    if (n == 0) return MHX_OK;
    MHX_REQUIRE(out, "%s", src.kNoOut);
    MHX_TRY(src.check_arrays());
    MHX_TRY(ctx->activate());
    MHX_TRY(src.stage(ctx));
    const int hash_dtype = hash_bits == 32 ? MHX_U32 : MHX_U64;
    Stage s(ctx);
    const auto p_init = s.piece(Stage::Aux, init ? (size_t)(init_stride ? n * m : m) : 0);
    const auto p_hv = s.piece(Stage::Aux, (hash_bits == 32 ? 4 : 8) * (size_t)src.max_hashes());
    src.reserve(s);
    const auto p_out = s.piece(Stage::Out, (size_t)(n * m));
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_init, init));
    MHX_TRY(src.hash(s, hash_dtype, s.at<void>(p_hv)));
    MHX_TRY(mhx::launch_hll_bulk(ctx, s.at<void>(p_hv), hash_dtype, src.d_sets, 0, n, src.n_hashes, p, hash_bits,
                                 init ? s.at<uint8_t>(p_init) : nullptr, init_stride, s.at<uint8_t>(p_out), nullptr));
    return s.fetch(out, p_out);
}

}  // namespace
}  // extern "C++"

int mhx_minhash_bulk_bytes(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, const int64_t *set_offsets,
                           int64_t n_sets, const uint64_t *init, int64_t init_stride, uint64_t *out) {
    return mhx_minhash_bulk_bytes_typed(perm, bytes, byte_offsets, n_tokens, MHX_U32, set_offsets, n_sets, init, init_stride, out);
}

int mhx_minhash_bulk_bytes_typed(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_dtype,
                                 const int64_t *set_offsets, int64_t n_sets, const uint64_t *init, int64_t init_stride, uint64_t *out) {
    return mhx_minhash_bulk_bytes_typed_hashed(perm, bytes, byte_offsets, n_tokens, hash_dtype, MHX_HASH_SHA1, set_offsets, n_sets, init, init_stride, out);
}

int mhx_minhash_bulk_bytes_typed_hashed(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_dtype,
                                        int hash_kind, const int64_t *set_offsets, int64_t n_sets, const uint64_t *init, int64_t init_stride,
                                        uint64_t *out) {
    MHX_ENTER(perm, perm->ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return minhash_of(perm, Tokens{bytes, byte_offsets, n_tokens, set_offsets, n_sets, /*aux_slack*/ 256, hash_kind, tokens_in_slack(hash_kind)}, hash_dtype, init, init_stride, out,
                      MHX_U64);
}

int mhx_hll_bulk_bytes(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int32_t hash_bits,
                       const int64_t *set_offsets, int64_t n_sets, int32_t p, const uint8_t *init, int64_t init_stride, uint8_t *out) {
    return mhx_hll_bulk_bytes_hashed(ctx, bytes, byte_offsets, n_tokens, hash_bits, MHX_HASH_SHA1, set_offsets, n_sets, p, init, init_stride, out);
}

int mhx_hll_bulk_bytes_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int32_t hash_bits, int hash_kind,
                              const int64_t *set_offsets, int64_t n_sets, int32_t p, const uint8_t *init, int64_t init_stride, uint8_t *out) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return hll_of(ctx, Tokens{bytes, byte_offsets, n_tokens, set_offsets, n_sets, /*aux_slack*/ 0, hash_kind, tokens_in_slack(hash_kind)}, hash_bits, p, init, init_stride, out);
}

int mhx_minhash_bulk_windows_typed(mhx_perm *perm, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                   const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype, const uint64_t *init,
                                   int64_t init_stride, void *out, int out_dtype) {
    return mhx_minhash_bulk_windows_typed_hashed(perm, bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_dtype, MHX_HASH_SHA1, init,
                                                 init_stride, out, out_dtype);
}

int mhx_minhash_bulk_windows_typed_hashed(mhx_perm *perm, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                          const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype, int hash_kind,
                                          const uint64_t *init, int64_t init_stride, void *out, int out_dtype) {
    MHX_ENTER(perm, perm->ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return minhash_of(perm, Windows{bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_kind}, hash_dtype, init, init_stride, out, out_dtype);
}

int mhx_hll_bulk_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                         int64_t n_docs, int64_t width, int32_t hash_bits, int32_t p, const uint8_t *init, int64_t init_stride, uint8_t *out) {
    return mhx_hll_bulk_windows_hashed(ctx, bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_bits, MHX_HASH_SHA1, p, init, init_stride, out);
}

int mhx_hll_bulk_windows_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                                int64_t n_docs, int64_t width, int32_t hash_bits, int hash_kind, int32_t p, const uint8_t *init,
                                int64_t init_stride, uint8_t *out) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return hll_of(ctx, Windows{bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_kind}, hash_bits, p, init, init_stride, out);
}

int mhx_minhash_bulk_words_typed(mhx_perm *perm, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                 const uint8_t *table, int64_t width, int hash_dtype, const uint64_t *init, int64_t init_stride, void *out,
                                 int out_dtype) {
    return mhx_minhash_bulk_words_typed_hashed(perm, bytes, n_bytes, doc_offsets, n_docs, table, width, hash_dtype, MHX_HASH_SHA1, init, init_stride,
                                               out, out_dtype);
}

int mhx_minhash_bulk_words_typed_hashed(mhx_perm *perm, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                        const uint8_t *table, int64_t width, int hash_dtype, int hash_kind, const uint64_t *init,
                                        int64_t init_stride, void *out, int out_dtype) {
    MHX_ENTER(perm, perm->ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return minhash_of(perm, Words{bytes, n_bytes, doc_offsets, n_docs, table, width, hash_kind}, hash_dtype, init, init_stride, out, out_dtype);
}

int mhx_hll_bulk_words(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                       const uint8_t *table, int64_t width, int32_t hash_bits, int32_t p, const uint8_t *init, int64_t init_stride,
                       uint8_t *out) {
    return mhx_hll_bulk_words_hashed(ctx, bytes, n_bytes, doc_offsets, n_docs, table, width, hash_bits, MHX_HASH_SHA1, p, init, init_stride, out);
}

int mhx_hll_bulk_words_hashed(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                              const uint8_t *table, int64_t width, int32_t hash_bits, int hash_kind, int32_t p, const uint8_t *init,
                              int64_t init_stride, uint8_t *out) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return hll_of(ctx, Words{bytes, n_bytes, doc_offsets, n_docs, table, width, hash_kind}, hash_bits, p, init, init_stride, out);
}

// ---- MinHashLSHBloom: per-band Bloom filters (ref: datasketch/lsh_bloom.py) ----------------------------------------------
static int check_bloom(int32_t bands, int64_t n_blocks) {
    MHX_REQUIRE(bands > 0 && bands <= (1 << 24), "bands must be in [1, 2^24]");
    MHX_REQUIRE(n_blocks >= 1 && n_blocks < ((int64_t)1 << 32), "n_blocks must be in [1, 2^32-1]");  // the block is chosen by a 32 x 32 bit product
    return MHX_OK;
}
// a filter is whole 64-byte blocks; lines are read 16 bytes at a time
#define MHX_CHECK_BLOOM_ALIGNED(ptr) MHX_REQUIRE(((uintptr_t)(ptr) & 63) == 0, #ptr " must be 64-byte aligned")

// insert, query, or query then insert (hit != NULL: the answers refer to the filter before the call).  The filter is the caller's
// device array whatever `where` says; `where` is about the signatures and the answers.
static int bloom_apply(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                       int64_t n_blocks, uint32_t *d_filter, uint8_t *hit, bool query, bool insert, Where where) {
    MHX_ENTER(ctx, ctx);
    MHX_REQUIRE(n >= 0, "n must be >= 0");
    MHX_CHECK_DTYPE(sig_dtype);
    MHX_CHECK_BANDS(bands, r, num_perm);
    MHX_TRY(check_bloom(bands, n_blocks));
    MHX_REQUIRE(k >= 1 && k <= 32, "k must be in [1, 32]");
    MHX_REQUIRE(d_filter, "d_filter is NULL");
    MHX_CHECK_BLOOM_ALIGNED(d_filter);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(sig && (hit || !query), where);
    MHX_TRY(ctx->activate());
    const uint32_t nb = (uint32_t)n_blocks;
    if (where == kDevice) {
        if (query) MHX_TRY(mhx::launch_bloom_query(ctx, sig, sig_dtype, n, num_perm, bands, r, k, nb, d_filter, hit));
        if (insert) MHX_TRY(mhx::launch_bloom_insert(ctx, sig, sig_dtype, n, num_perm, bands, r, k, nb, d_filter));
        return MHX_OK;
    }
    // the signatures go up once, whatever follows
    Stage s(ctx);
    const auto p_sig = s.piece(Stage::In, (sig_dtype == MHX_U32 ? 4 : 8) * (size_t)n * (size_t)num_perm);
    Stage::Piece p_hit{Stage::Out, 0, 0};
    if (query) p_hit = s.piece(Stage::Out, (size_t)n);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_sig, sig));
    if (query) MHX_TRY(mhx::launch_bloom_query(ctx, s.at<void>(p_sig), sig_dtype, n, num_perm, bands, r, k, nb, d_filter, s.at<uint8_t>(p_hit)));
    if (insert) MHX_TRY(mhx::launch_bloom_insert(ctx, s.at<void>(p_sig), sig_dtype, n, num_perm, bands, r, k, nb, d_filter));
    if (query) return s.fetch(hit, p_hit);
    return s.synchronize();
}

int mhx_bloom_insert_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                         int64_t n_blocks, uint32_t *d_filter) {
    return bloom_apply(ctx, d_sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, nullptr, false, true, kDevice);
}

int mhx_bloom_query_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                        int64_t n_blocks, uint32_t *d_filter, uint8_t *d_hit, int then_insert) {
    return bloom_apply(ctx, d_sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, d_hit, true, then_insert != 0, kDevice);
}

int mhx_bloom_insert(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                     int64_t n_blocks, uint32_t *d_filter) {
    return bloom_apply(ctx, sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, nullptr, false, true, kHost);
}

int mhx_bloom_query(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r, int32_t k,
                    int64_t n_blocks, uint32_t *d_filter, uint8_t *hit, int then_insert) {
    return bloom_apply(ctx, sig, sig_dtype, n, num_perm, bands, r, k, n_blocks, d_filter, hit, true, then_insert != 0, kHost);
}

int mhx_bloom_union_dev(mhx_ctx *ctx, uint32_t *d_dst, const uint32_t *d_src, int32_t bands, int64_t n_blocks) {
    MHX_ENTER(ctx, ctx);
    MHX_TRY(check_bloom(bands, n_blocks));
    MHX_REQUIRE_POINTERS(d_dst && d_src, kDevice);
    MHX_CHECK_BLOOM_ALIGNED(d_dst);
    MHX_CHECK_BLOOM_ALIGNED(d_src);
    MHX_TRY(ctx->activate());
    return mhx::launch_bloom_union(ctx, d_dst, d_src, (int64_t)bands * n_blocks * 16);
}

// ---- Near-duplicate clusters: connected components (cc_kernels.hip) -----------------------------------------------------------
// rows are numbered in 32 bits and a label is a row number
#define MHX_CHECK_CC_ROWS(n) MHX_REQUIRE((n) >= 0 && (n) < ((int64_t)1 << 32), "n must be in [0, 2^32-1]")

// init (finish == false) or finish over labels[n]
static int cc_sweep(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, bool finish) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_CC_ROWS(n);
    if (n == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_labels, kDevice);
    MHX_TRY(ctx->activate());
    return finish ? mhx::launch_cc_finish(ctx, d_labels, n) : mhx::launch_cc_init(ctx, d_labels, n);
}

static int cc_link_pairs(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const int64_t *d_pairs, int64_t n_pairs, const int32_t *d_counts,
                         int32_t min_count, int64_t *d_invalid) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_CC_ROWS(n);
    MHX_REQUIRE(n_pairs >= 0, "n_pairs must be >= 0");
    if (n_pairs == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_pairs && (d_labels || n == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_cc_link_pairs(ctx, d_labels, n, d_pairs, n_pairs, d_counts, min_count, d_invalid);
}

static int cc_link_bands(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows,
                         int64_t n_sigs, int32_t bands, int64_t *d_invalid) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_CC_ROWS(n);
    MHX_REQUIRE(n_sigs >= 0 && bands >= 0, "n_sigs and bands must be >= 0");
    MHX_REQUIRE(bands == 0 || n_sigs <= INT64_MAX / bands, "bands * n_sigs does not fit 63 bits");
    if (n_sigs == 0 || bands == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_sorted_digests && d_sorted_rows && (d_labels || n == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_cc_link_bands(ctx, d_labels, n, d_sorted_digests, d_sorted_rows, n_sigs, bands, d_invalid);
}

int mhx_cc_init_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n) { return cc_sweep(ctx, d_labels, n, false); }

int mhx_cc_link_pairs_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const int64_t *d_pairs, int64_t n_pairs, const int32_t *d_counts,
                          int32_t min_count, int64_t *d_invalid) {
    return cc_link_pairs(ctx, d_labels, n, d_pairs, n_pairs, d_counts, min_count, d_invalid);
}

int mhx_cc_link_bands_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows,
                          int64_t n_sigs, int32_t bands, int64_t *d_invalid) {
    return cc_link_bands(ctx, d_labels, n, d_sorted_digests, d_sorted_rows, n_sigs, bands, d_invalid);
}

int mhx_cc_finish_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n) { return cc_sweep(ctx, d_labels, n, true); }

// the host form: pairs (In) and counts (Aux) up, the three cores on the staged arrays, labels | invalid (Out) back
int mhx_cc_pairs(mhx_ctx *ctx, const int64_t *pairs, int64_t n_pairs, const int32_t *counts, int32_t min_count, int64_t n, uint32_t *labels,
                 int64_t *invalid) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_CC_ROWS(n);
    MHX_REQUIRE(n_pairs >= 0, "n_pairs must be >= 0");
    if (invalid) *invalid = 0;
    if (n == 0 && n_pairs == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS((labels || n == 0) && (pairs || n_pairs == 0), kHost);
    MHX_TRY(ctx->activate());
    Stage s(ctx);
    Stage::Piece p_pairs{Stage::In, 0, 0}, p_counts{Stage::Aux, 0, 0};
    if (n_pairs) p_pairs = s.piece(Stage::In, sizeof(int64_t) * 2 * (size_t)n_pairs);
    if (n_pairs && counts) p_counts = s.piece(Stage::Aux, sizeof(int32_t) * (size_t)n_pairs);
    // (an empty labels piece keeps its place in front of the counter: nothing is launched over it)
    const auto p_labels = s.piece(Stage::Out, sizeof(uint32_t) * (size_t)n), p_bad = s.piece(Stage::Out, sizeof(int64_t));
    MHX_TRY(s.commit());
    if (n_pairs) MHX_TRY(s.upload(p_pairs, pairs));
    if (n_pairs && counts) MHX_TRY(s.upload(p_counts, counts));
    MHX_HIP_CHECK(hipMemsetAsync(s.at<void>(p_bad), 0, sizeof(int64_t), ctx->stream));
    uint32_t *d_labels = s.at<uint32_t>(p_labels);
    MHX_TRY(cc_sweep(ctx, d_labels, n, false));
    MHX_TRY(cc_link_pairs(ctx, d_labels, n, n_pairs ? s.at<int64_t>(p_pairs) : nullptr, n_pairs,
                          n_pairs && counts ? s.at<int32_t>(p_counts) : nullptr, min_count, s.at<int64_t>(p_bad)));
    MHX_TRY(cc_sweep(ctx, d_labels, n, true));
    if (invalid) MHX_TRY(s.download(invalid, p_bad));
    if (n) return s.fetch(labels, p_labels);
    return s.synchronize();
}

// ---- Exact overlap of listed pairs (overlap_kernels.hip; datasketch_amd/overlap.py is the definition) ------------------------------
#define MHX_CHECK_OVERLAP_PAIRS(n_pairs) MHX_REQUIRE((n_pairs) >= 0 && (n_pairs) < ((int64_t)1 << 31), "n_pairs must be in [0, 2^31-1]")

int mhx_overlap_limits(int hv_dtype, int64_t lds_per_block, int64_t *lds_max_items) {
    MHX_REQUIRE(lds_max_items, "lds_max_items is NULL");
    MHX_CHECK_DTYPE(hv_dtype);
    MHX_REQUIRE(lds_per_block >= 0, "lds_per_block must be >= 0");
    *lds_max_items = mhx::overlap_lds_max_items(hv_dtype, lds_per_block);
    return MHX_OK;
}

int mhx_overlap_pairs_dev(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_set_offsets, int64_t n_sets, int64_t max_set_items,
                          const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts, int64_t *d_invalid) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(hv_dtype);
    MHX_REQUIRE(n_sets >= 0, "n_sets must be >= 0");
    MHX_CHECK_OVERLAP_PAIRS(n_pairs);
    MHX_REQUIRE(max_set_items >= 0 && max_set_items < ((int64_t)1 << 31), "max_set_items must be in [0, 2^31-1]: a set has fewer than 2^31 items");
    if (n_pairs == 0 || n_sets == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(d_set_offsets && d_pairs && d_counts && (d_hv || max_set_items == 0), kDevice);
    MHX_TRY(ctx->activate());
    return mhx::launch_overlap_pairs(ctx, d_hv, hv_dtype, d_set_offsets, n_sets, max_set_items, d_pairs, n_pairs, d_counts, d_invalid);
}

extern "C++" {
namespace {

// the pairs of a host entry against checked offsets: every index in range, and the largest named set (fewer than 2^31 items)
int check_overlap_pairs(const int64_t *pairs, int64_t n_pairs, const int64_t *set_offsets, int64_t n_sets, int64_t *max_set_items) {
    for (int64_t e = 0; e < 2 * n_pairs; ++e)
        MHX_REQUIRE(pairs[e] >= 0 && pairs[e] < n_sets, "pair index out of range (pair %lld: %lld, %lld sets)", (long long)(e / 2),
                    (long long)pairs[e], (long long)n_sets);
    int64_t most = 0;
    for (int64_t e = 0; e < 2 * n_pairs; ++e) most = std::max(most, set_offsets[pairs[e] + 1] - set_offsets[pairs[e]]);
    MHX_REQUIRE(most < ((int64_t)1 << 31), "a set of 2^31 or more items (%lld)", (long long)most);
    *max_set_items = most;
    return MHX_OK;
}

// the third sink.  Aux: hashes (uint32 or uint64) | whatever the source reserves | pairs;  Out: counts
template <class Source>
int overlaps_of(mhx_ctx *ctx, Source &&src, int hash_dtype, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    MHX_REQUIRE(hash_dtype == MHX_U32 || hash_dtype == MHX_U64, "hash_dtype must be MHX_U32 (sha1_hash32) or MHX_U64 (sha1_hash64)");
    MHX_CHECK_OVERLAP_PAIRS(n_pairs);
    MHX_TRY(src.check_sizes());
    if (n_pairs == 0) return MHX_OK;
    MHX_REQUIRE(pairs && counts, "pairs/counts is NULL");
    const int64_t n = src.n_sets();
    MHX_REQUIRE(n > 0, "pair index out of range (the corpus has no set)");
    for (int64_t e = 0; e < 2 * n_pairs; ++e)
        MHX_REQUIRE(pairs[e] >= 0 && pairs[e] < n, "pair index out of range (pair %lld: %lld, %lld sets)", (long long)(e / 2), (long long)pairs[e],
                    (long long)n);
    MHX_TRY(src.check_arrays());
    MHX_TRY(ctx->activate());
    MHX_TRY(src.stage(ctx));
    Stage s(ctx);
    const auto p_hv = s.piece(Stage::Aux, (hash_dtype == MHX_U32 ? 4 : 8) * (size_t)src.max_hashes());
    src.reserve(s);
    const auto p_pairs = s.piece(Stage::Aux, sizeof(int64_t) * 2 * (size_t)n_pairs);
    const auto p_out = s.piece(Stage::Out, sizeof(int32_t) * 3 * (size_t)n_pairs);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_pairs, pairs));
    MHX_TRY(src.hash(s, hash_dtype, s.at<void>(p_hv)));
    int64_t max_set_items = 0;
    MHX_TRY(check_overlap_pairs(pairs, n_pairs, src.host_sets(), n, &max_set_items));
    MHX_TRY(mhx::launch_overlap_pairs(ctx, s.at<void>(p_hv), hash_dtype, src.d_sets, n, max_set_items, s.at<int64_t>(p_pairs), n_pairs,
                                      s.at<int32_t>(p_out), nullptr));
    return s.fetch(counts, p_out);
}

}  // namespace
}  // extern "C++"

int mhx_overlap_pairs(mhx_ctx *ctx, const void *hv, int hv_dtype, const int64_t *set_offsets, int64_t n_sets, const int64_t *pairs,
                      int64_t n_pairs, int32_t *counts) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_DTYPE(hv_dtype);
    MHX_REQUIRE(n_sets >= 0, "n_sets must be >= 0");
    MHX_CHECK_OVERLAP_PAIRS(n_pairs);
    if (n_pairs == 0) return MHX_OK;
    MHX_REQUIRE_POINTERS(pairs && counts, kHost);
    MHX_REQUIRE(n_sets > 0, "pair index out of range (there is no set)");
    MHX_REQUIRE_POINTERS(set_offsets, kHost);
    MHX_REQUIRE(set_offsets[0] == 0, "set_offsets[0] must be 0");
    for (int64_t i = 0; i < n_sets; ++i)
        MHX_REQUIRE(set_offsets[i + 1] >= set_offsets[i], "set_offsets must be non-decreasing (set %lld)", (long long)i);
    const int64_t total = set_offsets[n_sets];
    MHX_REQUIRE_POINTERS(hv || total == 0, kHost);
    int64_t max_set_items = 0;
    MHX_TRY(check_overlap_pairs(pairs, n_pairs, set_offsets, n_sets, &max_set_items));
    MHX_TRY(ctx->activate());
    Stage s(ctx);
    const auto p_hv = s.piece(Stage::In, (hv_dtype == MHX_U32 ? 4 : 8) * (size_t)total);
    if (total == 0) s.ask(Stage::In, 8);
    const auto p_sets = s.piece(Stage::Offsets, sizeof(int64_t) * (size_t)(n_sets + 1));
    const auto p_pairs = s.piece(Stage::Aux, sizeof(int64_t) * 2 * (size_t)n_pairs);
    const auto p_out = s.piece(Stage::Out, sizeof(int32_t) * 3 * (size_t)n_pairs);
    MHX_TRY(s.commit());
    MHX_TRY(s.upload(p_hv, hv));
    MHX_TRY(s.upload(p_sets, set_offsets));
    MHX_TRY(s.upload(p_pairs, pairs));
    MHX_TRY(mhx::launch_overlap_pairs(ctx, s.at<void>(p_hv), hv_dtype, s.at<int64_t>(p_sets), n_sets, max_set_items, s.at<int64_t>(p_pairs),
                                      n_pairs, s.at<int32_t>(p_out), nullptr));
    return s.fetch(counts, p_out);
}

int mhx_overlap_pairs_bytes(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_dtype,
                            const int64_t *set_offsets, int64_t n_sets, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    return mhx_overlap_pairs_bytes_hashed(ctx, bytes, byte_offsets, n_tokens, hash_dtype, MHX_HASH_SHA1, set_offsets, n_sets, pairs, n_pairs, counts);
}

int mhx_overlap_pairs_bytes_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_dtype, int hash_kind,
                                   const int64_t *set_offsets, int64_t n_sets, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return overlaps_of(ctx, Tokens{bytes, byte_offsets, n_tokens, set_offsets, n_sets, /*aux_slack*/ 0, hash_kind, tokens_in_slack(hash_kind)}, hash_dtype, pairs, n_pairs, counts);
}

int mhx_overlap_pairs_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                              int64_t n_docs, int64_t width, int hash_dtype, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    return mhx_overlap_pairs_windows_hashed(ctx, bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_dtype, MHX_HASH_SHA1, pairs, n_pairs, counts);
}

int mhx_overlap_pairs_windows_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items, const int64_t *doc_offsets,
                                     int64_t n_docs, int64_t width, int hash_dtype, int hash_kind, const int64_t *pairs, int64_t n_pairs,
                                     int32_t *counts) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return overlaps_of(ctx, Windows{bytes, item_offsets, n_items, doc_offsets, n_docs, width, hash_kind}, hash_dtype, pairs, n_pairs, counts);
}

int mhx_overlap_pairs_words(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                            const uint8_t *table, int64_t width, int hash_dtype, const int64_t *pairs, int64_t n_pairs, int32_t *counts) {
    return mhx_overlap_pairs_words_hashed(ctx, bytes, n_bytes, doc_offsets, n_docs, table, width, hash_dtype, MHX_HASH_SHA1, pairs, n_pairs, counts);
}

int mhx_overlap_pairs_words_hashed(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                   const uint8_t *table, int64_t width, int hash_dtype, int hash_kind, const int64_t *pairs, int64_t n_pairs,
                                   int32_t *counts) {
    MHX_ENTER(ctx, ctx);
    MHX_CHECK_HASH_KIND(hash_kind);
    return overlaps_of(ctx, Words{bytes, n_bytes, doc_offsets, n_docs, table, width, hash_kind}, hash_dtype, pairs, n_pairs, counts);
}

}  // extern "C"
