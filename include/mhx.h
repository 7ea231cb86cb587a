/*
 * mhx.h -- C ABI of libmhx, the MI355X-native MinHash signature engine.
 *
 * This is the drop-in boundary for ekzhu/datasketch's bulk-hashing hot path.  It is what a
 * ctypes / cffi stub inside the reference would bind in place of its optional CuPy branch
 * (reference datasketch/minhash.py:281-291; binding shown in INTEGRATION.md).  Plain pointers
 * and sizes only: no C++ types, no torch types, no exceptions across the boundary.
 *
 * Conventions
 *   - every function returns an int status (MHX_OK == 0); mhx_last_error() gives the
 *     thread-local message of the last failing call.
 *   - "host" entry points take caller-owned host buffers, block until the result is in host
 *     memory, and never retain the pointers.  "_dev" entry points take device pointers
 *     (from mhx_dev_alloc or any other HIP allocation on the same device), enqueue on the
 *     context's stream and return without synchronising.
 *   - a context owns one device + one HIP stream; calls on one context (and on the perm / wgen /
 *     comm handles created from it) are serialised by a mutex inside the context, so concurrent
 *     callers are safe but do not overlap; distinct contexts are independent (one context per
 *     GPU / per process is the multi-GPU model).
 *   - device buffers handed to "_dev" entry points need NO slack: a kernel reads and writes only the bytes
 *     the argument list describes ([n_sigs, num_perm] elements, offsets[n_sets] tokens ...), and pointers need
 *     only the natural alignment of their element type (wider loads are used where the pointer allows them).
 *     tests/test_guard_pages.py and the `*_guard_cases.py` scripts hold the kernels to this with
 *     mhx_debug_guard_alloc (an unmapped page right behind -- or in front of -- every buffer).
 *     tests/test_gpu_stream_order.py (cases in tests/stream_order_cases.py) holds the "_dev" entry points to the three ordering
 *     promises above -- enqueued without synchronising unless the entry's comment says that it blocks, no host pointer kept after the
 *     return, the work of successive calls on one context taking effect in call order -- by running each behind in-flight work.
 *   - citations "ref:" are paths in the reference repository (ekzhu/datasketch v1.10.0).
 */
#ifndef MHX_H_
#define MHX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_API __attribute__((visibility("default")))

/* ---- status codes ------------------------------------------------------------------------- */
enum {
    MHX_OK = 0,
    MHX_ERR_NO_DEVICE = 1,   /* no usable HIP device: maps to the reference's RuntimeError for
                                gpu_mode='always' (ref: datasketch/minhash.py:272-275)          */
    MHX_ERR_INVALID = 2,     /* bad argument / shape: maps to ValueError                          */
    MHX_ERR_HIP = 3,         /* a HIP runtime call failed                                         */
    MHX_ERR_OOM = 4,         /* device allocation failed                                          */
    MHX_ERR_UNSUPPORTED = 5, /* valid request outside what this build implements                  */
    MHX_ERR_COMM = 6,        /* RCCL failure                                                      */
    MHX_ERR_CAPACITY = 7     /* the caller's output arrays are too small; the sizes needed were
                                stored and nothing was written (mhx_words_normalize*)             */
};

/* element types of token / signature buffers */
enum { MHX_U64 = 0, MHX_U32 = 1 };

typedef struct mhx_ctx mhx_ctx;     /* device + stream + scratch                                  */
typedef struct mhx_perm mhx_perm;   /* MinHash permutations (a[K], b[K]) resident on the device   */
typedef struct mhx_wgen mhx_wgen;   /* WeightedMinHashGenerator parameters resident on the device */
typedef struct mhx_event mhx_event; /* HIP event on the context's stream                          */
typedef struct mhx_comm mhx_comm;   /* RCCL communicator (one rank per context)                   */

/* ---- library / device --------------------------------------------------------------------- */
MHX_API const char *mhx_last_error(void);
MHX_API const char *mhx_version(void);

/* Number of usable devices.  Replaces ref: datasketch/minhash.py:38-48 (_gpu_available). */
MHX_API int mhx_device_count(int *count);

MHX_API int mhx_ctx_create(int device, mhx_ctx **ctx);
MHX_API int mhx_ctx_destroy(mhx_ctx *ctx);
MHX_API int mhx_ctx_synchronize(mhx_ctx *ctx);
/* Free the grow-only device staging buffers of the host entry points (they are re-created on demand): the five scratch
 * slots and the MinHash hand-over flags.  With mhx_debug_poison_alloc on, the next call's scratch is therefore fresh -- it
 * holds nothing but the poison byte, not what an earlier call left there (tests/poison_cases.py calls this before every case). */
MHX_API int mhx_ctx_release_scratch(mhx_ctx *ctx);
/* name: caller buffer (may be NULL); cus: compute units; hbm_bytes: total device memory */
MHX_API int mhx_ctx_device_info(mhx_ctx *ctx, char *name, int name_len, int *cus, int64_t *hbm_bytes);
/* Tuning / test knobs: ("minhash.path", 0 = auto: sieve with dedup / pairwise fallback launches,
 * 1 = exact fold for every pair, 2 = fast fold with exact redo), ("minhash.split", 0 auto,
 * 1 wave per set, 2 split sets over waves), ("minhash.packed", 0 auto: several sets per wave when
 * num_perm <= 96, 1 = always one set per wave, 2 = several sets per wave up to num_perm 128), ("minhash.ties", 0 auto: the second launch tries the
 * tie-tolerant sieve before the dedup pass, 1 = dedup pass only), ("blocks_per_cu", n: workgroups per CU of the capped grids of the MinHash and weighted
 * launchers, 0 auto; n <= (2^32 - 1) / (512 * the device's CUs) -- 32767 on the MI355X's 256 --, so that a grid of CUs * n workgroups of up to 512
 * threads stays below the 2^32 threads a launch takes), ("minhash.prefetch", 0/1/2: never / auto / always),
 * ("debug.cus", tests only: 0 = the device's own compute-unit count, 1 .. that count = every launcher sizes its grid, chunks and segments as if
 * the device had so many (a grid can only shrink, so that small shapes reach the later trips of the grid-stride loops); any other value is
 * MHX_ERR_INVALID; results unaffected, mhx_ctx_device_info keeps reporting the device's count),
 * ("minhash.alias", profiling only: >= 0 makes set i read the tokens of set i & mask),
 * ("minhash.p3", 0 auto: three permutations per lane where that walks the fewest slots -- num_perm 129..192, 257..384, 513..576 --, 1 = never three), ("minhash.share", 0 auto: with three or four
 * permutations per lane, lane groups share a last slot that holds at most 32 permutations -- num_perm 129..160, 193..224 --, 1 = off),
 * ("minhash.adapt", 0 auto: the context remembers on the device whether the last call's sets mostly defeated the one-candidate proof and
 * starts the next call with the tie-tolerant one, 1 = off),
 * ("weighted.kernel", 0 auto: dense rows of up to 4096 columns (a multiple of 4) with 65..256 or 321..384 samples through the fetcher / walker kernel, other dense rows
 * of that width through the one-wave-per-row kernel, 1 = the workgroup-per-row kernel, 2 = one wave per row, sample chunks one after the other),
 * ("weighted.refill", 0 auto; 13 = auto without the fetcher / walker split, 5 / 6 / 8 / 9 = the split with other stripe counts and cached list positions,
 * 1 = round 4's plain loads behind the walk, 2 / 3 = the one-wave-per-row kernel's fetch modes; A/B), ("weighted.plan", 1 = plan and tables in two launches), ("weighted.rescue", n: a walk's last n lanes
 * are taken over by the whole wave, 0 auto = 8, < 0 never),
 * ("weighted.path", 0 auto: dense rows through the bound-ordered walk, CSR rows through the row-block kernels,
 * 1 IEEE division for every element, 2 = every element evaluated: dense rows compacted to CSR first),
 * ("weighted.direct", n: a dense row with at most n stored elements per 1000 columns is evaluated element by element
 * instead of walked, default 100), ("weighted.split", 0 auto: the waves of a workgroup that share 64 samples split the list of a
 * dense row that is evaluated entry by entry, 1 = one wave per 64 samples), ("weighted.tail", profiling: 1 .. 5 force the share of a call's logs that
 * counts as "above the cut" to 0.5, 1, 2, 4, 8 %; 0 = the cheapest by the plan's estimate), ("weighted.debug", profiling only: 1 = stage and scan the rows without walking them,
 * 2 = skip the scan, 4 = (fetcher / walker kernel) every stripe keeps its first row: the walkers alone; results are meaningless;
 * 8 = (fetcher / walker kernel, results unaffected) a hand-over wait that outlasts 2^24 polls traps instead of waiting on),
 * ("host.chunk_bytes", see
 * mhx_minhash_bulk), ("lsh.sort_bits", bits of (band, digest) mhx_lsh_sort_bands hands to the radix sort,
 * 0 = chosen from n; the order is exact for any value, fewer bits leave more to the clean-up pass),
 * ("lsh.gather", 1 = gather the full digests after the sort instead of letting them ride through it),
 * ("lsh.prehash", mhx_lsh_sort_bands on a signature matrix: 0 auto = band digests first (one pass at the stream's rate), then the bucketing; 1 = hash inside
 * the bucketing's first pass),
 * ("lsh.team", bucketing over unit-stride sources: 0 auto = one team of 1024 threads x 8 rows per workgroup from eight items per CU on,
 * 256 = teams of 256 threads x 16 rows (until round 6), 1024 = the one team at any size),
 * ("lsh.bigbins", 0 auto: between 2.56M and 10.2M rows one scatter level into 1024 bins of up to 11 264 elements and the bin pass's big form
 * (two passes over the keys instead of three), 1 = never, 2 = from 4 bins on (tests)),
 * ("weighted.min_dim", dense rows at least this wide -- a multiple of 4, up to 4096 columns -- go to the one-wave-per-row / fetcher-walker kernels:
 * 0 auto = 4, 1024 = the rule until round 6),
 * ("lsh.sort", 0 auto: mhx_lsh_sort_bands buckets the bands in two passes (three beyond 10.2M rows) and falls back to the radix sort when a bin
 * overflows or n > 41M, 1 = radix sort always),
 * ("lsh.merge_items", mhx_lsh_bands_merge_dev: outputs per thread of a 256-thread merge tile, 0 auto = 8, or 8 / 16; results unaffected),
 * ("hll.split_tokens", mhx_hll_bulk*: a set with more tokens than this is split over several workgroups and combined by a max,
 * 0 auto = 32768; results unaffected),
 * ("bloom.lanes", mhx_bloom_*: lanes per (row, band), 0 auto = 16 for the insert (one lane per word of the block) and 1 for the query, the faster
 * mapping of each; 1 / 16 = both operations that way; results unaffected),
 * ("overlap.bins", mhx_overlap_*: 0 auto = pairs whose table fits LDS are binned by table size, each bin is a launch with that
 * much dynamic LDS and the pairs of the smallest bin get one wave each, 1 = one launch sized for the largest table of the call,
 * 2 = the bins of 0 with a workgroup per pair in every bin; results unaffected),
 * ("lsh.levels", bucketing of mhx_lsh_sort_bands: 0 auto = two scatter levels beyond 2^10 bins per band, 2 = two levels whenever there are at least
 * 4 bins (tests)), ("lsh.chunk", bucketing: rows per thread of a scatter pass over a unit-stride source, 0 auto = 16, 8 = eight (A/B)),
 * ("pack.fused", mhx_bbit_pack_band_digests_dev: 0 auto = one read of the matrix where the shape allows, 1 = always the two kernels),
 * ("jaccard.topk_path", mhx_*jaccard_topk*: 0 auto = the stream kernel for dense and weighted rows and few probes, 1 = the strip kernel,
 * 2 = the stream kernel wherever it exists; b-bit rows always take the strip kernel),
 * ("jaccard.topk_segments", mhx_*jaccard_topk*: segments B is cut into, 0 auto = enough to fill the machine, n >= 1 = n, clamped to the number of
 * 128-row tiles of B).
 * Values: a key whose text lists its values takes those and no others ("weighted.refill": 0, 1, 2, 3, 5, 6, 8, 9, 13; "lsh.team": 0, 256, 1024;
 * "weighted.debug": 0, 1, 2, 4, 8; the 0 / 1 keys: 0 or 1); "weighted.direct" 0 .. 1000, "weighted.tail" 0 .. 5, "weighted.min_dim" 0 or a multiple
 * of 4 in 4 .. 4096, "lsh.sort_bits" 0 .. 64, "weighted.rescue" any value up to 64 (the lanes of a wave), "minhash.alias" >= -1,
 * "hll.split_tokens" and "jaccard.topk_segments" >= 0, "host.chunk_bytes" any value.  Anything else is MHX_ERR_INVALID with a message that
 * names the key and its values, and the option keeps the value it had.  Except for the profiling keys "weighted.debug" 1 / 2 / 4 and
 * "minhash.alias" >= 0, timings depend on an option, results never: tests/test_gpu_options.py (cases in tests/option_cases.py) runs every
 * value -- both ends and the middle of a range -- at a shape whose launcher reads it and compares with the reference byte for byte, and
 * tests/test_option_ledger.py fails when a key or a place that reads one has no case. */
MHX_API int mhx_ctx_set_option(mhx_ctx *ctx, const char *key, int64_t value);
/* Kernel event counters since the last call (synchronises the stream, then resets them):
 *   out[0] sets the sieve launch left to the full launch (failed proof, or skipped by the back-off),
 *   out[1] sets redone with the exact fold, out[2] 256-token sieve blocks evaluated,
 *   out[3] sets the full launch had to hash pair by pair (its dedup sieve failed too).
 * enable != 0 starts/keeps counting, 0 stops it (counting costs one atomic per event). */
#define MHX_NUM_COUNTERS 4
MHX_API int mhx_ctx_counters(mhx_ctx *ctx, int enable, uint64_t out[MHX_NUM_COUNTERS]);
/* What the previous MinHash call on this context learned about the corpus and the first launch of the next call acts on:
 * 0 = the one-candidate proof goes first, 1 = most sets defeated it (the tie-tolerant proof goes first), 2 = heavily
 * repeated tokens.  Timings depend on it (so a benchmark may want to know, or to reset it), results never.  reset != 0 puts it
 * back to 0, the state of a fresh context.  mode may be NULL.  Blocking. */
MHX_API int mhx_ctx_minhash_mode(mhx_ctx *ctx, int reset, int *mode);
/* Diagnostics for parity audits: which sets of the LAST mhx_minhash_bulk_dev call on this context left the fast path.  The
 * result of every set is exact whatever its flag says (ref: datasketch/minhash.py:293-297) -- the flag names the launch that
 * produced it, so that a test can check exactly the sets the rare-event paths handled: flags[i] = 0 the first launch's proof
 * held for set i, 1 = set i was done again by the second launch (tie-tolerant / dedup sieve), 2 = hashed pair by pair by the
 * third.  n_sets must be the last call's; a call that kept no flags (one huge set split over waves, minhash.path != 0) is
 * MHX_ERR_INVALID.  With more than 256 permutations (several passes over the sets) the flags are the last pass's.  Blocking. */
MHX_API int mhx_ctx_minhash_flags(mhx_ctx *ctx, int64_t n_sets, uint8_t *flags);

/* ---- device memory + events (so callers can keep corpora resident and time kernels) ------- */
MHX_API int mhx_dev_alloc(mhx_ctx *ctx, size_t bytes, void **dptr);
MHX_API int mhx_dev_free(mhx_ctx *ctx, void *dptr);
/* Debugging: guard pages.  From this call on every device allocation of the library in this process (mhx_dev_alloc, the
 * contexts' staging buffers, permutations, generator tables) is mapped with the HIP virtual-memory API between two
 * unmapped granules, its LAST byte (align > 0; the size is rounded up to `align` bytes: 16, 8, 4, 1 ...) or its FIRST
 * byte (align < 0) abutting the unmapped range, so that an over- or under-read by a kernel raises a GPU memory access
 * fault instead of touching a neighbour.  align = 0 switches back to hipMalloc (live guarded blocks stay valid).  The
 * environment variable MHX_GUARD_ALLOC=<align> does the same from the first allocation (a value that is not 0 or
 * +-(a power of two <= 4096) is reported on stderr and ignored).  granule (may be NULL) receives the mapping granularity
 * in bytes, live (may be NULL) the number of guarded blocks currently allocated.  A debugging mode, not a production one:
 * the virtual address ranges of freed guarded blocks are never reused (a stale pointer must fault, not alias), so a long
 * guarded run grows its address space by (size + 2 granules) per allocation, and every free synchronises the device. */
MHX_API int mhx_debug_guard_alloc(int align, int64_t *granule, int64_t *live);
/* Debugging: poison.  From this call on every fresh device allocation of the library in this process is filled with
 * byte_value (0..255; -1 switches it off) before it is handed out -- what a board that has been in use gives a process
 * anyway, made deterministic: a kernel that reads a word nobody wrote then computes with 0xFF..FF (a NaN, a -1, an
 * offset of 2^64-1) on every box instead of with the zeros of a freshly booted one.  Environment: MHX_POISON_ALLOC=<byte>.
 * (The library's blocks inside guard mode keep hipMalloc's 256-byte alignment; only mhx_dev_alloc's blocks are placed
 * with the guard alignment as given.) */
MHX_API int mhx_debug_poison_alloc(int byte_value);
/* page-locked host memory: buffers a caller fills and hands to the host entry points again and again (the pieces of
 * mhx_weighted_dense_feed, staging for mhx_minhash_bulk) go up by DMA straight from it, about 1.3x the rate of pageable memory */
MHX_API int mhx_host_alloc(mhx_ctx *ctx, size_t bytes, void **ptr);
/* ctx may be NULL once the allocating context has been destroyed (mhx_ctx_destroy does not free these blocks) */
MHX_API int mhx_host_free(mhx_ctx *ctx, void *ptr);
MHX_API int mhx_memcpy_h2d(mhx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
MHX_API int mhx_memcpy_d2h(mhx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* device-to-device copy, enqueued on the context's stream (no synchronisation) */
MHX_API int mhx_memcpy_d2d(mhx_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);
MHX_API int mhx_memset_dev(mhx_ctx *ctx, void *dst_dev, int byte_value, size_t bytes);

MHX_API int mhx_event_create(mhx_ctx *ctx, mhx_event **ev);
MHX_API int mhx_event_record(mhx_event *ev); /* on the owning context's stream */
MHX_API int mhx_event_synchronize(mhx_event *ev);
MHX_API int mhx_event_elapsed_ms(mhx_event *start, mhx_event *stop, float *ms);
MHX_API int mhx_event_destroy(mhx_event *ev);

/* ---- MinHash ------------------------------------------------------------------------------ */
/*
 * Upload permutations (a[k], b[k]) = MinHash.permutations.
 * Replaces ref: datasketch/minhash.py:160-165 (_ensure_gpu_caches).  a, b are host arrays of
 * num_perm uint64 as produced by ref: datasketch/minhash.py:170-184 (kept on the host: legacy
 * numpy RandomState stream).  Any uint64 values are accepted (the reference draws a in [1,p),
 * b in [0,p) with p = 2^61-1, but user-supplied permutations are not range-checked there either).
 */
MHX_API int mhx_perm_create(mhx_ctx *ctx, const uint64_t *a, const uint64_t *b, int32_t num_perm,
                            mhx_perm **perm);
MHX_API int mhx_perm_destroy(mhx_perm *perm);

/*
 * Bulk MinHash over a corpus of pre-hashed token sets, device-resident.
 * Replaces the per-set loop of ref: datasketch/minhash.py:491-522 (generator / bulk) around
 * ref: datasketch/minhash.py:293-297 (update_batch body):
 *     out[i,k] = min( init[i,k],  min_t ((hv[t]*a[k] + b[k]) mod 2^64) mod (2^61-1) & 0xFFFFFFFF )
 * Bit-exact with the numpy path, including the uint64 wrap-around of hv*a+b.
 *
 *   d_hv        token hash values, hv_dtype = MHX_U64 (any uint64) or MHX_U32
 *   d_offsets   int64[n_sets+1] CSR row pointers into d_hv, or NULL for fixed-length sets
 *   fixed_len   tokens per set when d_offsets == NULL (ignored otherwise)
 *   total_tokens  number of elements in d_hv (offsets[n_sets] or n_sets*fixed_len)
 *   d_init      NULL (fresh state 2^32-1, ref :167-168), or uint64 state with row stride
 *               init_stride elements (0 = one [K] prototype shared by every set, K = [n,K])
 *   d_out       [n_sets, K] of out_dtype (MHX_U64 = reference layout; MHX_U32 = compact:
 *               values are < 2^32 unless an init value >= 2^32 survives an empty set, which
 *               MHX_U32 output rejects by saturating to 2^32-1)
 * An empty set leaves its state untouched (ref :265-266).
 */
MHX_API int mhx_minhash_bulk_dev(mhx_perm *perm, const void *d_hv, int hv_dtype,
                                 const int64_t *d_offsets, int64_t fixed_len, int64_t n_sets,
                                 int64_t total_tokens, const uint64_t *d_init, int64_t init_stride,
                                 void *d_out, int out_dtype);

/* Same computation from/to host buffers (H2D, kernel, D2H; blocking).  offsets may be NULL
 * with fixed_len, init may be NULL.  out: uint64 [n_sets, K].  Corpora above 256 MiB are cut
 * into pieces of whole sets whose upload, kernels and download overlap (option
 * "host.chunk_bytes": > 0 piece size in bytes, 0 automatic, < 0 one piece). */
MHX_API int mhx_minhash_bulk(mhx_perm *perm, const uint64_t *hv, const int64_t *offsets,
                             int64_t fixed_len, int64_t n_sets, const uint64_t *init,
                             int64_t init_stride, uint64_t *out);

/* The same with the element types of mhx_minhash_bulk_dev: hv of hv_dtype (MHX_U32: tokens in the range of
 * sha1_hash32, ref: datasketch/hashfunc.py:5-15 -- half the bytes over PCIe), out of out_dtype (MHX_U32: values
 * are < 2^32 by construction, ref: minhash.py:31,297).  mhx_minhash_bulk is the (MHX_U64, MHX_U64) case. */
MHX_API int mhx_minhash_bulk_typed(mhx_perm *perm, const void *hv, int hv_dtype, const int64_t *offsets,
                                   int64_t fixed_len, int64_t n_sets, const uint64_t *init,
                                   int64_t init_stride, void *out, int out_dtype);

/*
 * The reference's default token hash on the device: out[i] = sha1_hash32(token i) (MHX_U32,
 * ref: datasketch/hashfunc.py:5-15: first 4 bytes of the SHA-1 digest, little-endian) or
 * sha1_hash64 (MHX_U64, ref: hashfunc.py:17-28), replacing the per-token Python call of
 * ref: datasketch/minhash.py:221,262-263.  Tokens are byte strings packed back to back in `bytes`;
 * token i is bytes[byte_offsets[i] .. byte_offsets[i+1]) (int64[n_tokens+1], byte_offsets[0] == 0).
 * The uint32 output can be passed straight to mhx_minhash_bulk_dev as hv with hv_dtype MHX_U32.
 */
MHX_API int mhx_sha1_tokens_dev(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_byte_offsets,
                                int64_t n_tokens, int out_dtype, void *d_out);
MHX_API int mhx_sha1_tokens(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets,
                            int64_t n_tokens, int out_dtype, void *out);
/*
 * MinHash.bulk / generator on raw byte tokens with the default hashfunc (ref: minhash.py:491-522
 * with hashfunc = sha1_hash32): H2D of the packed bytes, SHA-1 kernel, MinHash kernel, D2H of
 * out[n_sets, K] uint64.  set_offsets int64[n_sets+1] indexes TOKENS (set i owns tokens
 * set_offsets[i] .. set_offsets[i+1]); init as in mhx_minhash_bulk.
 */
MHX_API int mhx_minhash_bulk_bytes(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets,
                                   int64_t n_tokens, const int64_t *set_offsets, int64_t n_sets,
                                   const uint64_t *init, int64_t init_stride, uint64_t *out);

/* hash_dtype = MHX_U32: sha1_hash32 (mhx_minhash_bulk_bytes), MHX_U64: sha1_hash64 (ref: hashfunc.py:17-28). */
MHX_API int mhx_minhash_bulk_bytes_typed(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets,
                                         int64_t n_tokens, int hash_dtype, const int64_t *set_offsets,
                                         int64_t n_sets, const uint64_t *init, int64_t init_stride,
                                         uint64_t *out);

/*
 * One update_batch on one MinHash state (the reference's GPU seam itself,
 * ref: datasketch/minhash.py:281-291): hashvalues[K] is read, min-combined with the
 * permuted minima of hv[0..n), and written back.  n == 0 is a no-op.
 */
MHX_API int mhx_minhash_update_batch(mhx_perm *perm, const uint64_t *hv, int64_t n,
                                     uint64_t *hashvalues);

/* Elementwise min of two signature matrices (ref: datasketch/minhash.py:337-359 merge,
 * :411-462 union, lean_minhash.py:237-253), count = rows*K elements.  d_out may alias d_x. */
MHX_API int mhx_minhash_merge_dev(mhx_ctx *ctx, const uint64_t *d_x, const uint64_t *d_y,
                                  int64_t count, uint64_t *d_out);
MHX_API int mhx_minhash_merge(mhx_ctx *ctx, const uint64_t *x, const uint64_t *y, int64_t count,
                              uint64_t *out);

/* ---- Weighted MinHash --------------------------------------------------------------------- */
/*
 * Upload generator parameters rs, ln_cs, betas: float32 [sample_size, dim] row-major, exactly the
 * arrays of ref: datasketch/weighted_minhash.py:119-121 (drawn on the host by numpy).
 */
MHX_API int mhx_wgen_create(mhx_ctx *ctx, const float *rs, const float *ln_cs, const float *betas,
                            int32_t sample_size, int32_t dim, mhx_wgen **gen);
MHX_API int mhx_wgen_destroy(mhx_wgen *gen);

/*
 * WeightedMinHashGenerator.minhash_many over a CSR matrix (ref: datasketch/weighted_minhash.py:161-247).
 *   indptr int64[n_rows+1], indices int32[nnz] (sorted within a row, ref :193), values float32[nnz]
 *   values_are_logs != 0: values already hold ln(x) as float32 (parity mode: the host computes
 *     np.log with the same numpy the reference uses; everything downstream is IEEE float32 with
 *     no FMA contraction, so (k, t) are bit-exact);  == 0: the device takes logf(x) itself.
 *   out int64[n_rows, sample_size, 2] = (k, t) pairs (ref :233-239); rows without stored values
 *   get nonempty[row] = 0 (the reference returns None for them, ref :242-247) and zeros in out.
 *   The host entry checks indptr (monotone) and every column index (0 <= index < dim; the reference raises
 *   IndexError there) before anything is uploaded; the _dev entry takes resident arrays as they are: column
 *   indices outside [0, dim) are the caller's error and are not looked for on the device.
 */
MHX_API int mhx_weighted_minhash_many(mhx_wgen *gen, const int64_t *indptr, const int32_t *indices,
                                      const float *values, int values_are_logs, int64_t n_rows,
                                      int64_t *out, uint8_t *nonempty);
MHX_API int mhx_weighted_minhash_many_dev(mhx_wgen *gen, const int64_t *d_indptr,
                                          const int32_t *d_indices, const float *d_values,
                                          int values_are_logs, int64_t n_rows, int64_t nnz,
                                          int64_t *d_out, uint8_t *d_nonempty);

/* The same for DENSE rows x[n_rows, dim] float32 (what the reference first converts with scipy on the host):
 * an entry counts as stored iff its value is not 0 (NaN counts, as for scipy's nonzero()); with
 * values_are_logs != 0 the caller passes ln(x) and ln(0) = -inf marks the absent entries.  The CSR form is
 * built on the device. */
MHX_API int mhx_weighted_minhash_many_dense(mhx_wgen *gen, const float *x, int values_are_logs,
                                            int64_t n_rows, int64_t *out, uint8_t *nonempty);
MHX_API int mhx_weighted_minhash_many_dense_dev(mhx_wgen *gen, const float *d_x, int values_are_logs,
                                                int64_t n_rows, int64_t *d_out, uint8_t *d_nonempty);

/* Dense rows arriving in pieces (a host that takes np.log piece by piece ahead of the device -- parity mode of
 * ref: weighted_minhash.py:212 -- or reads the matrix from disk):
 *   begin  sizes the device buffers for pieces of up to piece_rows rows (two of them, so that piece i+1 goes up while
 *          piece i is evaluated);
 *   feed   uploads x[n_rows, dim] and returns as soon as x may be overwritten; the evaluation of this piece is queued
 *          behind it and the results of the PREVIOUS piece are brought down meanwhile.  out / nonempty of a piece
 *          (same layout as above, n_rows rows) are complete when the next feed, or end, has returned;
 *   end    brings down the last piece and releases the buffers (also to be called after an error).
 * One feed at a time per generator's context; other calls on the context may come in between. */
typedef struct mhx_wfeed mhx_wfeed;
MHX_API int mhx_weighted_dense_begin(mhx_wgen *gen, int values_are_logs, int64_t piece_rows, mhx_wfeed **feed);
MHX_API int mhx_weighted_dense_feed(mhx_wfeed *feed, const float *x, int64_t n_rows, int64_t *out, uint8_t *nonempty);
MHX_API int mhx_weighted_dense_end(mhx_wfeed *feed);

/* out[i] = the float32 logarithm the device-log mode (values_are_logs == 0) takes of x[i]: the one place where the
 * fast mode can differ from numpy's float32 log (ref: weighted_minhash.py:212), exposed so that callers can check
 * the difference against their tolerance (BASELINE: 1e-6 relative). */
MHX_API int mhx_weighted_logf(mhx_ctx *ctx, const float *x, int64_t n, float *out);

/* ---- Packing for downstream consumers ----------------------------------------------------- */
/* Number of uint64 blocks bBitMinHash uses for num_perm values of b bits
 * (ref: datasketch/b_bit_minhash.py:147-172). */
MHX_API int mhx_bbit_num_blocks(int32_t num_perm, int32_t b, int32_t *num_blocks);
/* b-bit packing of a whole signature matrix in the bit order of ref:
 * datasketch/b_bit_minhash.py:37-38,82-97.  sig [n,K] uint64 -> out [n,num_blocks] uint64. */
MHX_API int mhx_bbit_pack_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n_sigs, int32_t num_perm,
                              int32_t b, uint64_t *d_out);
MHX_API int mhx_bbit_pack(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                          int32_t b, uint64_t *out);
/* MinHashLSH band keys: out[n, bands*r] holds each hashvalue byte-swapped to big-endian so that
 * bytes(out[i, j*r:(j+1)*r]) is the key of band j (ref: datasketch/lsh.py:199,344,537-538). */
MHX_API int mhx_band_keys_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n_sigs, int32_t num_perm,
                              int32_t bands, int32_t r, uint64_t *d_out);
MHX_API int mhx_band_keys(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                          int32_t bands, int32_t r, uint64_t *out);
/* 64-bit band digests for device-side bucketing: out[n, bands], out[i,j] = FNV-1a-64 of the band key
 * bytes of band j of row i (the very bytes of mhx_band_keys; what ref: datasketch/lsh.py:540-543 stores
 * for MinHashLSH(hashfunc=fnv1a_64)).  Equal digests <=> same LSH bucket (up to 2^-64 collisions). */
MHX_API int mhx_band_digests_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n_sigs, int32_t num_perm,
                                 int32_t bands, int32_t r, uint64_t *d_out);
MHX_API int mhx_band_digests(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                             int32_t bands, int32_t r, uint64_t *out);
/* LSH bucketing by sort (what the per-band dictionaries of ref: datasketch/lsh.py:326-347,370-400 do by
 * hashing): for every band j, sorted_digests[j*n .. (j+1)*n) are the band-j digests of all n signatures in
 * ascending order and sorted_rows[...] the row numbers in the same order -- every LSH bucket of band j is
 * a run of equal digests.  Rows are uint32 (n < 2^32).  The default two-pass bucketing reads one flag back between its
 * passes (the call synchronises the stream once; with option "lsh.sort" = 1, the radix sort, it only enqueues) and keeps
 * its bin slabs -- about 30 bytes per (row, band) -- in the context's scratch until mhx_ctx_release_scratch. */
MHX_API int mhx_lsh_sort_bands_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n_sigs, int32_t num_perm,
                                   int32_t bands, int32_t r, uint64_t *d_sorted_digests,
                                   uint32_t *d_sorted_rows);
MHX_API int mhx_lsh_sort_bands(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                               int32_t bands, int32_t r, uint64_t *sorted_digests, uint32_t *sorted_rows);
/* The same from digests that are already there: d_digests [n_sigs, bands] as mhx_band_digests* wrote them (a caller that
 * keeps the digest matrix -- config 3 stores it as the index's keys -- does not pay for hashing the bands twice). */
MHX_API int mhx_lsh_sort_digests_dev(mhx_ctx *ctx, const uint64_t *d_digests, int64_t n_sigs, int32_t bands,
                                     uint64_t *d_sorted_digests, uint32_t *d_sorted_rows);
/* Candidate pairs: every pair of rows i < j that share the digest of at least one band -- the rows
 * MinHashLSH.query (ref: datasketch/lsh.py:370-400) would return for each other -- from the output of
 * mhx_lsh_sort_bands.  pairs: int64[capacity, 2], ascending by (i, j), unique.  *n_pairs receives the
 * number of unique pairs; when it exceeds capacity nothing is written and the caller calls again with
 * a larger buffer.  *n_raw (may be NULL) receives the pair count before deduplication across bands.
 * A bucket of L equal keys holds L(L-1)/2 pairs: MHX_ERR_OOM when they do not fit in device memory.
 * Blocking (the counts come back to the host). */
MHX_API int mhx_lsh_candidate_pairs_dev(mhx_ctx *ctx, const uint64_t *d_sorted_digests,
                                        const uint32_t *d_sorted_rows, int64_t n_sigs, int32_t bands,
                                        int64_t *d_pairs, int64_t capacity, int64_t *n_pairs,
                                        int64_t *n_raw);
/* signatures (host) -> band digests -> per-band sort -> candidate pairs (host), one call */
MHX_API int mhx_lsh_candidate_pairs(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                                    int32_t bands, int32_t r, int64_t *pairs, int64_t capacity,
                                    int64_t *n_pairs, int64_t *n_raw);
/* Bulk query: the keys MinHashLSH.query (ref: datasketch/lsh.py:370-431) would return for each of m probe
 * signatures against an index of n signatures held as sorted bands (mhx_lsh_sort_bands*): for every band the
 * probe's digest is located by binary search and the matching run is its bucket.  pairs: int64[capacity, 2] =
 * (probe, index row), ascending, unique; *n_pairs as in mhx_lsh_candidate_pairs_dev (larger than capacity: nothing
 * written, call again).  d_index_sig (may be NULL): the index's own [n, num_perm] matrix of the same sig_dtype;
 * when given, a candidate is kept only if the r words of the band really are equal, so a 64-bit digest
 * collision between different band keys cannot produce a row the reference's dictionaries would not.  Blocking. */
MHX_API int mhx_lsh_query_dev(mhx_ctx *ctx, const uint64_t *d_sorted_digests, const uint32_t *d_sorted_rows,
                              int64_t n_sigs, int32_t bands, int32_t r, const void *d_query_sig,
                              const void *d_index_sig, int sig_dtype, int32_t num_perm, int64_t n_queries,
                              int64_t *d_pairs, int64_t capacity, int64_t *n_pairs);
/* Batched MinHash.jaccard numerators (ref: datasketch/minhash.py:299-324): counts[p] = number of equal
 * positions of rows pairs[p][0] of sig_a and pairs[p][1] of sig_b (both [*, num_perm] uint64; may be the
 * same matrix); the estimate is counts / num_perm.  pairs int64[n_pairs, 2]. */
MHX_API int mhx_jaccard_pairs_dev(mhx_ctx *ctx, const uint64_t *d_sig_a, const uint64_t *d_sig_b,
                                  int32_t num_perm, const int64_t *d_pairs, int64_t n_pairs,
                                  int32_t *d_counts);
MHX_API int mhx_jaccard_pairs(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                              const int64_t *pairs, int64_t n_pairs, int32_t *counts);
/* Batched bBitMinHash.jaccard numerators (ref: datasketch/b_bit_minhash.py:53-72) on packed rows (mhx_bbit_pack*):
 * counts[p] = number of the num_perm positions whose b-bit values agree in rows pairs[p][0] of blocks_a and
 * pairs[p][1] of blocks_b (both [*, num_blocks] uint64; may be the same matrix) -- XOR + popcount on the packed
 * blocks, nothing is unpacked.  The estimate is (counts / num_perm - C1) / (1 - C2) with the reference's C1, C2. */
MHX_API int mhx_bbit_jaccard_pairs_dev(mhx_ctx *ctx, const uint64_t *d_blocks_a, const uint64_t *d_blocks_b,
                                       int32_t num_perm, int32_t b, const int64_t *d_pairs, int64_t n_pairs,
                                       int32_t *d_counts);
MHX_API int mhx_bbit_jaccard_pairs(mhx_ctx *ctx, const uint64_t *blocks, int64_t n_rows, int32_t num_perm, int32_t b,
                                   const int64_t *pairs, int64_t n_pairs, int32_t *counts);
/* The device entry points above for signature matrices of sig_dtype MHX_U64 or MHX_U32 -- uint32 is the compact
 * output of mhx_minhash_bulk_dev and the wire format of the all-gather (values are < 2^32, ref: minhash.py:31,297);
 * results are those of the widened matrix. */
MHX_API int mhx_bbit_pack_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs,
                                    int32_t num_perm, int32_t b, uint64_t *d_out);
MHX_API int mhx_band_digests_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs,
                                       int32_t num_perm, int32_t bands, int32_t r, uint64_t *d_out);
/* Config 5 in one call: the b-bit blocks (mhx_bbit_pack*: ref datasketch/b_bit_minhash.py:78-101) AND the band digests
 * (mhx_band_digests*: ref datasketch/lsh.py:199,344,537-543) of the same [n, num_perm] matrix.  When bands is a power of
 * two <= 64, r is 4, 8 or 16, bands * r == num_perm and rows are 16-byte aligned, ONE kernel reads the matrix once and
 * writes both outputs (*fused = 1); any other shape runs the two kernels one after the other (*fused = 0).  Results are
 * those of the two separate calls, bit for bit.  d_blocks: uint64[n, num_blocks], d_digests: uint64[n, bands] or, with digest_layout =
 * MHX_BAND_MAJOR, uint64[bands, n]. */
MHX_API int mhx_bbit_pack_band_digests_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs,
                                           int32_t num_perm, int32_t b, int32_t bands, int32_t r, int digest_layout,
                                           uint64_t *d_blocks, uint64_t *d_digests, int *fused);
/* Layout of a band-digest matrix on the device.  MHX_ROW_MAJOR: [n, bands] (row i's digests together: the keys of one
 * signature, what a host-side index wants).  MHX_BAND_MAJOR: [bands, n] (band j's digests of all rows together: one
 * array per hashtable, ref datasketch/lsh.py:199 -- and what the bucketing reads with unit stride: from a row-major
 * matrix every 128-byte line is fetched by the four XCDs whose bands share it, 1.30 GB of reads for a 320 MB matrix). */
#define MHX_ROW_MAJOR 0
#define MHX_BAND_MAJOR 1
MHX_API int mhx_band_digests_layout_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs,
                                        int32_t num_perm, int32_t bands, int32_t r, int layout, uint64_t *d_out);
MHX_API int mhx_lsh_sort_digests_layout_dev(mhx_ctx *ctx, const uint64_t *d_digests, int64_t n_sigs, int32_t bands,
                                            int layout, uint64_t *d_sorted_digests, uint32_t *d_sorted_rows);
MHX_API int mhx_lsh_sort_bands_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs,
                                         int32_t num_perm, int32_t bands, int32_t r,
                                         uint64_t *d_sorted_digests, uint32_t *d_sorted_rows);
MHX_API int mhx_jaccard_pairs_dev_typed(mhx_ctx *ctx, const void *d_sig_a, const void *d_sig_b, int sig_dtype,
                                        int32_t num_perm, const int64_t *d_pairs, int64_t n_pairs,
                                        int32_t *d_counts);
/* LeanMinHash.serialize of every row, little-endian: n records of 12+4*K bytes
 * (ref: datasketch/lean_minhash.py:126-175). */
MHX_API int mhx_lean_serialize_dev(mhx_ctx *ctx, const uint64_t *d_sig, int64_t n_sigs,
                                   int32_t num_perm, int64_t seed, uint8_t *d_out);
MHX_API int mhx_lean_serialize(mhx_ctx *ctx, const uint64_t *sig, int64_t n_sigs, int32_t num_perm,
                               int64_t seed, uint8_t *out);
/* The same for a matrix of sig_dtype (MHX_U32: the compact form) in either byte order the reference's `byteorder` argument can ask
 * for: MHX_LITTLE_ENDIAN is '<' (and '@' / '=' on this little-endian host), MHX_BIG_ENDIAN is '>' / '!' (network order). */
#define MHX_LITTLE_ENDIAN 0
#define MHX_BIG_ENDIAN 1
MHX_API int mhx_lean_serialize_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs, int32_t num_perm,
                                         int64_t seed, int byteorder, uint8_t *d_out);
/* The inverse: LeanMinHash.deserialize of n records of 12 + 4*K bytes laid back to back (ref: datasketch/lean_minhash.py:177-214):
 * d_sig [n, K] of sig_dtype receives the hash values, d_seeds (may be NULL) int64[n] each record's seed.  A record whose length
 * field is not num_perm is counted in *d_bad (uint32 on the device, may be NULL; the caller zeroes it) -- the host entry point
 * returns MHX_ERR_INVALID for such a buffer.  Records need 4-byte alignment. */
MHX_API int mhx_lean_deserialize_dev(mhx_ctx *ctx, const uint8_t *d_records, int64_t n_sigs, int32_t num_perm, int byteorder,
                                     int sig_dtype, void *d_sig, int64_t *d_seeds, uint32_t *d_bad);
MHX_API int mhx_lean_deserialize(mhx_ctx *ctx, const uint8_t *records, int64_t n_sigs, int32_t num_perm, int byteorder,
                                 uint64_t *sig, int64_t *seeds);
/* The inverse of mhx_bbit_pack*: bBitMinHash.__setstate__ of every row (ref: datasketch/b_bit_minhash.py:103-125) --
 * blocks [n, num_blocks] uint64 -> the b-bit values [n, num_perm] uint32 (what a restored bBitMinHash holds as hashvalues). */
MHX_API int mhx_bbit_unpack_dev(mhx_ctx *ctx, const uint64_t *d_blocks, int64_t n_sigs, int32_t num_perm, int32_t b,
                                uint32_t *d_out);
MHX_API int mhx_bbit_unpack(mhx_ctx *ctx, const uint64_t *blocks, int64_t n_sigs, int32_t num_perm, int32_t b, uint32_t *out);

/* ---- All-pairs Jaccard --------------------------------------------------------------------- */
/* Every pair of rows of two signature matrices A [n_a, num_perm] and B [n_b, num_perm] of sig_dtype, with no LSH banding in
 * front (no false negatives): counts[i*ldc + j] = the number of positions k where A[i][k] == B[j][k] -- the numerator of
 * MinHash.jaccard (ref: datasketch/minhash.py:299-324), exact on the full element width (uint64 values that differ only in
 * bits 32..63 are not equal).  d_b == NULL compares A with itself (n_b is then n_a).  ldc >= n_b.  Enqueued on the ctx stream.
 * Rows: fewer than 2^32 per matrix. */
MHX_API int mhx_jaccard_matrix_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype,
                                   int32_t num_perm, int32_t *d_counts, int64_t ldc);
/* Host form (uint64 rows, b == NULL: A with itself): counts int32[n_a, n_b]; B is staged once, A and the counts stream
 * through the device in row blocks.  Blocking. */
MHX_API int mhx_jaccard_matrix(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b, int32_t num_perm,
                               int32_t *counts);
/* Thresholded form: every pair (i, j) whose count is >= min_count, ascending by (i, j), each once -- pairs int64[capacity, 2],
 * counts int32[capacity].  d_b == NULL: self-join of A, pairs i < j only.  *n_pairs always receives the exact total; when it
 * exceeds capacity the buffers' contents are unspecified (nothing is written at or past capacity entries) and the caller
 * calls again with a larger buffer.  min_count <= 0 keeps every pair, min_count > num_perm none (nothing is launched).  Keeps a
 * sort's worth of scratch (about 12 bytes per pair found) in the context until mhx_ctx_release_scratch.  Blocking. */
MHX_API int mhx_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype,
                                            int32_t num_perm, int32_t min_count, int64_t *d_pairs, int32_t *d_counts,
                                            int64_t capacity, int64_t *n_pairs);
MHX_API int mhx_jaccard_threshold_pairs(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b,
                                        int32_t num_perm, int32_t min_count, int64_t *pairs, int32_t *counts, int64_t capacity,
                                        int64_t *n_pairs);
/* Top-k form: for every row i of A the k rows j of B with the most agreeing positions, best first by (count descending, row
 * ascending) -- a strict total order, so the answer is unique -- rows int64[n_a, k], counts int32[n_a, k]; a row with fewer
 * than k candidates is padded with row = -1, count = -1.  The n_a x n_b matrix is never formed.  d_b == NULL: the rows of A
 * among themselves (n_b is then n_a), j == i is no candidate.  d_b_live_bits (may be NULL): bit (row & 31) of word row >> 5
 * set = row of B is a candidate, ceil(n_b / 32) words, as mhx_rows_compact_dev.  min_count > 0: rows with fewer agreeing
 * positions are no candidates (min_count > num_perm: only the padding is written).  1 <= k <= MHX_TOPK_MAX, else
 * MHX_ERR_INVALID.  n_a == 0 writes nothing, n_b == 0 only the padding.  Keeps the partial lists (8 bytes x n_a x k x the
 * number of segments B is cut into, at most one per 128 rows of B) as scratch in the context until mhx_ctx_release_scratch.
 * Enqueued on the ctx stream. */
#define MHX_TOPK_MAX 64
/* (exported through MHX_API_TOPK, the same visibility as MHX_API, and bound from _native._PROTOTYPES_TOPK: a list of their own, as
 * MHX_API_EXT and MHX_API_BLOOM below, whose argument checks are tested beside the feature) */
#define MHX_API_TOPK __attribute__((visibility("default")))
MHX_API_TOPK int mhx_jaccard_topk_dev(mhx_ctx *ctx, const void *d_a, int64_t n_a, const void *d_b, int64_t n_b, int sig_dtype,
                                 int32_t num_perm, const uint32_t *d_b_live_bits, int32_t min_count, int32_t k, int64_t *d_rows,
                                 int32_t *d_counts);
/* Host form (uint64 rows, b == NULL: A among itself): A is staged once, B streams through the device in row blocks whose
 * lists are merged into the running ones, so B need not fit on the device beside A.  Blocking. */
MHX_API_TOPK int mhx_jaccard_topk(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b, int64_t n_b, int32_t num_perm,
                             int32_t min_count, int32_t k, int64_t *rows, int32_t *counts);
/* The b-bit twins on packed rows (mhx_bbit_pack*: [n, num_blocks] uint64, num_blocks as mhx_bbit_num_blocks): counts = the
 * positions of num_perm whose b-bit values agree, the `intersection` of bBitMinHash.jaccard (ref:
 * datasketch/b_bit_minhash.py:53-72), counted as num_perm minus the slots that differ (XOR, fold, popcount).  The estimate
 * is (counts / num_perm - C1) / (1 - C2) with the reference's C1, C2.  Arguments otherwise as above; b in [0, 32]. */
MHX_API int mhx_bbit_jaccard_matrix_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b,
                                        int32_t num_perm, int32_t b, int32_t *d_counts, int64_t ldc);
MHX_API int mhx_bbit_jaccard_matrix(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b,
                                    int32_t num_perm, int32_t b, int32_t *counts);
MHX_API int mhx_bbit_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b,
                                                 int32_t num_perm, int32_t b, int32_t min_count, int64_t *d_pairs,
                                                 int32_t *d_counts, int64_t capacity, int64_t *n_pairs);
MHX_API int mhx_bbit_jaccard_threshold_pairs(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b,
                                             int32_t num_perm, int32_t b, int32_t min_count, int64_t *pairs, int32_t *counts,
                                             int64_t capacity, int64_t *n_pairs);
MHX_API_TOPK int mhx_bbit_jaccard_topk_dev(mhx_ctx *ctx, const uint64_t *d_a, int64_t n_a, const uint64_t *d_b, int64_t n_b,
                                      int32_t num_perm, int32_t b, const uint32_t *d_b_live_bits, int32_t min_count, int32_t k,
                                      int64_t *d_rows, int32_t *d_counts);
MHX_API_TOPK int mhx_bbit_jaccard_topk(mhx_ctx *ctx, const uint64_t *a, int64_t n_a, const uint64_t *b_blocks, int64_t n_b,
                                  int32_t num_perm, int32_t b, int32_t min_count, int32_t k, int64_t *rows, int32_t *counts);

/* ---- Live LSH index: the update path of sorted bands ------------------------------------- */
/* The index of datasketch_amd.MinHashLSH (ref: datasketch/lsh.py:326-347 insert, :509-528 remove) is the layout of
 * mhx_lsh_sort_bands*: per band the digests uint64[bands][n] ascending by (digest, row) with their rows uint32[bands][n] (rows are
 * slot numbers of the signature matrix), which mhx_lsh_query_dev and mhx_lsh_candidate_pairs_dev read.  A batch is merged in and
 * removed slots are compacted out; nothing is sorted twice.  Rows and entries per band: fewer than 2^32.
 *
 * Merge, per band, two runs sorted by (digest, row) -- A [bands][n_a] and B [bands][n_b] -- into d_dig_out / d_rows_out
 * [bands][n_a + n_b] (caller-owned, not overlapping the inputs); B's rows get row_offset_b added.  The caller guarantees that every
 * B row after the offset is greater than every A row: ties then go to A and the output is the stable sort of A||B by digest,
 * what mhx_lsh_sort_bands* gives for the union.  Either side may be empty.  Enqueued on the ctx stream. */
MHX_API int mhx_lsh_bands_merge_dev(mhx_ctx *ctx, const uint64_t *d_dig_a, const uint32_t *d_rows_a, int64_t n_a,
                                    const uint64_t *d_dig_b, const uint32_t *d_rows_b, int64_t n_b, uint32_t row_offset_b,
                                    int32_t bands, uint64_t *d_dig_out, uint32_t *d_rows_out);
/* Compact sorted bands [bands][n] whose rows are the slots 0 .. n-1 (each once per band): the entries whose slot is dead in
 * d_live_bits (bit (row & 31) of word row >> 5 set = live; ceil(n / 32) words) are dropped and every other row becomes
 * remap[row], the number of live slots below it, so the order is kept.  d_dig_out / d_rows_out: [bands][n_live], band j from
 * j * n_live.  MHX_ERR_INVALID when the bitmap does not hold n_live live slots or the bands do not hold bands * n_live live
 * entries; nothing is ever written at or past bands * n_live entries.  Blocking. */
MHX_API int mhx_lsh_bands_compact_dev(mhx_ctx *ctx, const uint64_t *d_dig, const uint32_t *d_rows, int64_t n, int32_t bands,
                                      const uint32_t *d_live_bits, int64_t n_live, uint64_t *d_dig_out, uint32_t *d_rows_out);
/* The matrix side of compaction: the live rows (d_live_bits as above, ceil(n_rows / 32) words) of d_src [n_rows][row_bytes]
 * gathered in slot order into d_dst (room for the live rows; not overlapping d_src); *n_kept receives their number.  16-byte
 * loads and stores where both pointers and row_bytes allow them.  Blocking. */
MHX_API int mhx_rows_compact_dev(mhx_ctx *ctx, const void *d_src, int64_t row_bytes, int64_t n_rows, const uint32_t *d_live_bits,
                                 void *d_dst, int64_t *n_kept);

/* ---- LSH Forest: top-k queries over sorted trees ------------------------------------------ */
/* The index of datasketch_amd.MinHashLSHForest (ref: datasketch/lshforest.py).  d_sig is a signature matrix [n_sigs][row_words]
 * of sig_dtype words (a WeightedMinHash row: its (k, t) int64 pairs as 2 words per hash value).  Tree t of l owns the words
 * [t * tree_words, (t + 1) * tree_words) of a row, tree_words = depth * words per hash value; l * tree_words <= row_words, the
 * words past that belong to no tree.  l and the depth are below 65536.
 *
 * Build: d_order uint32[l][n_sigs] (caller-owned) receives, per tree, the rows ascending by (the tree's words compared
 * lexicographically as unsigned integers, row) -- the order of the reference's big-endian byte keys, equal keys in row order.
 * tree_words (uint32) or 2 * tree_words (uint64) stable radix passes over l * n_sigs pairs, whatever the data: rows that are all
 * identical cost what distinct ones do.  l * n_sigs < 2^32.  n_sigs == 0 writes nothing.  Enqueued on the ctx stream. */
MHX_API int mhx_lsh_forest_build_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs, int32_t row_words,
                                           int32_t l, int32_t tree_words, uint32_t *d_order);
/* Query: for each of the m rows of d_probes [m][row_words] (same sig_dtype), the reference's walk -- level r = depth .. 1, tree
 * t = 0 .. l-1, the positions of d_order[t] whose first r hash values (r * w words) equal the probe's, ascending; a row is taken
 * the first time it is met; stop at k rows.  d_slots uint32[m][k] receives the rows of probe i in that order from i * k on and
 * d_counts int32[m] how many (<= k); the cells of d_slots past the count are not written.  w: words per hash value (1 or 2),
 * tree_words a multiple of it.  A probe stages l * min(2k - 1, n_sigs) candidates in LDS: MHX_ERR_INVALID when that exceeds
 * MHX_LSH_FOREST_MAX_CANDIDATES (k = 1024 at l = 8 fits).  m == 0 writes nothing; n_sigs == 0 writes m zero counts.  Enqueued on
 * the ctx stream. */
#define MHX_LSH_FOREST_MAX_CANDIDATES 16384
MHX_API int mhx_lsh_forest_query_dev_typed(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n_sigs, int32_t row_words,
                                           int32_t l, int32_t tree_words, int32_t w, const uint32_t *d_order, const void *d_probes,
                                           int64_t m, int32_t k, uint32_t *d_slots, int32_t *d_counts);

/* ---- LSH Ensemble: containment queries over size partitions -------------------------------- */
/* The index of datasketch_amd.MinHashLSHEnsemble (ref: datasketch/lshensemble.py).  The rows of ONE signature matrix d_index_sig
 * [n][row_words] are sorted by set size, so partition p of n_parts is the slot range [start[p], start[p + 1]) (start: host
 * int64[n_parts + 1], ascending from 0 to n < 2^32).  Every distinct r of the ensemble's parameter table is a level: bands = the
 * number of bands of r words (r counts words: 2 per hash value for WeightedMinHash rows), and two device buffers of bands * n
 * entries, d_digests uint64 and d_rows uint32.  Partition p owns the entries [bands * start[p], bands * start[p + 1]) of both;
 * inside that block band j starts at j * n_p (n_p = the partition's rows) and is ascending by (digest, row) with rows local to the
 * partition -- byte for byte what mhx_lsh_sort_bands_dev_typed writes for the partition's rows, which is how it is built.
 *
 * Query: params is the host table int32[n_params][2] of (level, b) rows, b <= that level's bands; d_choice uint8[m][n_parts] names,
 * per probe and partition, the row of params to use (the reference picks it from upper bound / probe size: floating point, done by
 * the caller).  A byte that is no row of the table (255 by convention) skips the partition.  For every probe q, partition p and
 * band j < b the probe's digest is located by binary search in band j of p's block of the chosen level and the run of equal digests
 * is its bucket; a candidate is kept when the band's r words of probe and index row are equal.  d_pairs int64[capacity][2] =
 * (probe, slot = start[p] + row), ascending, unique; *n_pairs, capacity and the overflow behaviour as in mhx_lsh_query_dev.  The work is
 * the sum of the chosen b, not m * n_parts * bands.  At most MHX_ENSEMBLE_MAX_LEVELS levels and MHX_ENSEMBLE_MAX_PARAMS table rows.
 * Blocking. */
#define MHX_ENSEMBLE_MAX_LEVELS 16
#define MHX_ENSEMBLE_MAX_PARAMS 64
typedef struct mhx_ensemble_level {
    const uint64_t *d_digests; /* uint64[bands * n] */
    const uint32_t *d_rows;    /* uint32[bands * n] */
    int32_t r;                 /* words per band */
    int32_t bands;             /* bands per partition block: r * bands <= row_words */
} mhx_ensemble_level;
MHX_API int mhx_lsh_ensemble_query_dev(mhx_ctx *ctx, const mhx_ensemble_level *levels, int32_t n_levels, const int64_t *start,
                                       int32_t n_parts, const void *d_index_sig, int sig_dtype, int32_t row_words,
                                       const void *d_query_sig, int64_t n_queries, const uint8_t *d_choice,
                                       const int32_t *params, int32_t n_params, int64_t *d_pairs, int64_t capacity,
                                       int64_t *n_pairs);

/* ---- HyperLogLog ------------------------------------------------------------------------------ */
/* Register files of the reference's HyperLogLog (ref: datasketch/hyperloglog.py): m = 2^p registers of one byte per sketch, p in
 * [4, 16] (ref :56-57), a matrix of sketches is uint8 [n, m] row-major -- numpy reads a row as the reference's int8 `reg`
 * (ref :76).  Device pointers to register matrices (d_init, d_out, d_reg) must be 4-byte aligned: rows are moved as 32-bit
 * words.  hash_bits is 32 for HyperLogLog (ref :52) and 64 for the registers of HyperLogLogPlusPlus (ref :348).
 *
 * Which LDS layout mhx_hll_bulk* accumulates a set's registers in at precision p: 0 = one wave per set, one 32-bit word per
 * register; 1 = one workgroup per set, one word per register; 2 = one workgroup per set, packed bytes.  Results do not depend on
 * it; tests read the switch points from here.
 *
 * The HyperLogLog entry points are exported through MHX_API_EXT: the same visibility as MHX_API; they are bound from
 * _native._PROTOTYPES_EXT and their argument checks are tested beside the feature, in tests/test_gpu_hyperloglog.py (the
 * argument table of tests/test_gpu_cabi_arguments.py pins the MHX_API list to itself). */
#define MHX_API_EXT __attribute__((visibility("default")))
MHX_API_EXT int mhx_hll_layout(int p, int *layout);
/*
 * Bulk update, device-resident: what a loop of HyperLogLog.update (ref :136-142) over every token of every set leaves in
 * the registers.  For set i and each hash hv of its tokens
 *     idx = hv & (m - 1);  rank = clz_W(hv >> p) - p + 1  (W = hash_bits, clz_W(0) = W; ref :138-142, :238-246)
 *     out[i, idx] = max(out[i, idx], rank)
 *   d_hv, hv_dtype, d_offsets, fixed_len, n_sets, total_tokens   as in mhx_minhash_bulk_dev (CSR, or NULL offsets + fixed_len)
 *   d_init      NULL (fresh registers, all zero: ref :76), or uint8 registers with row stride init_stride: 0 = one [m] row
 *               shared by every set, m = [n_sets, m]; must not overlap d_out
 *   d_out       uint8 [n_sets, m]; an empty set yields its init row (or zeros)
 *   d_overflow  int64 on the device, set by the call to the number of hashes that do not fit hash_bits -- the reference's
 *               ValueError("Hash value overflow ...") of ref :240-245; such a hash updates nothing, and the registers of
 *               a call that counts any are unspecified.  Only uint64 input at hash_bits = 32 can overflow: for the other
 *               three (hv_dtype, hash_bits) pairs d_overflow may be NULL.
 * A set with more tokens than option "hll.split_tokens" is split over several workgroups; the bytes are the same.
 */
MHX_API_EXT int mhx_hll_bulk_dev(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_offsets, int64_t fixed_len,
                             int64_t n_sets, int64_t total_tokens, int32_t p, int32_t hash_bits, const uint8_t *d_init,
                             int64_t init_stride, uint8_t *d_out, int64_t *d_overflow);
/* The same from / to host buffers (blocking); overflow (host int64, may be NULL where no overflow is possible) receives the
 * count.  offsets are checked to be non-decreasing.  The corpus is staged in one piece: callers cut large corpora into
 * pieces of whole sets themselves (datasketch_amd.HyperLogLog.bulk_registers does). */
MHX_API_EXT int mhx_hll_bulk_typed(mhx_ctx *ctx, const void *hv, int hv_dtype, const int64_t *offsets, int64_t fixed_len,
                               int64_t n_sets, int32_t p, int32_t hash_bits, const uint8_t *init, int64_t init_stride,
                               uint8_t *out, int64_t *overflow);
/* Raw byte tokens with the reference's default hash functions (ref: hyperloglog.py:70 sha1_hash32 for hash_bits = 32, :355
 * sha1_hash64 for hash_bits = 64; datasketch/hashfunc.py:5-28): the packed bytes go up, mhx_sha1_tokens_dev and the register
 * kernel run, out [n_sets, m] comes back.  bytes / byte_offsets / set_offsets as in mhx_minhash_bulk_bytes_typed.  These
 * hashes fit hash_bits by construction: there is no overflow count. */
MHX_API_EXT int mhx_hll_bulk_bytes(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens,
                               int32_t hash_bits, const int64_t *set_offsets, int64_t n_sets, int32_t p, const uint8_t *init,
                               int64_t init_stride, uint8_t *out);
/* hist uint32 [n, 64]: hist[i, v] = the number of registers of row i equal to v -- all an estimator needs: the zero count of
 * the linear counting (ref :162-163) is hist[i, 0], and the harmonic sum np.sum(2.0 ** -reg) of ref :152 is
 * sum_v hist[i, v] * 2^-v.  A register above 63 (no hash of at most 64 bits produces one) is counted into *invalid (int64,
 * set by the call) and into no bin. */
MHX_API_EXT int mhx_hll_histogram_dev(mhx_ctx *ctx, const uint8_t *d_reg, int64_t n, int32_t p, uint32_t *d_hist,
                                  int64_t *d_invalid);
MHX_API_EXT int mhx_hll_histogram(mhx_ctx *ctx, const uint8_t *reg, int64_t n, int32_t p, uint32_t *hist, int64_t *invalid);
/* HyperLogLog.merge of whole matrices (ref :170-183): d_a[i] = max(d_a[i], d_b[i]) over count bytes, in place.  Any
 * alignment and any count; 16 bytes per lane where both pointers are 16-byte aligned. */
MHX_API_EXT int mhx_hll_merge_dev(mhx_ctx *ctx, uint8_t *d_a, const uint8_t *d_b, int64_t count);
/* HyperLogLog.union per group (ref :254-268, np.maximum.reduce): out[g, :] = the register-wise max over the rows
 * group_offsets[g] .. group_offsets[g + 1] of reg [n_rows, m] (int64 [n_groups + 1], non-decreasing, inside [0, n_rows] --
 * checked by the host form, the caller's promise for the _dev form).  An empty group gives zeros. */
MHX_API_EXT int mhx_hll_union_groups_dev(mhx_ctx *ctx, const uint8_t *d_reg, int64_t n_rows, int32_t p,
                                     const int64_t *d_group_offsets, int64_t n_groups, uint8_t *d_out);
MHX_API_EXT int mhx_hll_union_groups(mhx_ctx *ctx, const uint8_t *reg, int64_t n_rows, int32_t p, const int64_t *group_offsets,
                                 int64_t n_groups, uint8_t *out);

/* ---- MinHashLSHBloom: per-band Bloom filters ---------------------------------------------------- */
/* The index of the reference's MinHashLSHBloom (ref: datasketch/lsh_bloom.py) as one device array d_filter
 * uint32 [bands][n_blocks][16], 64-byte aligned: every band owns a cache-line-blocked Bloom filter of n_blocks blocks of 512 bits
 * (16 little-endian 32-bit words), and all the k bits of a key lie in one block.  For row i and band j of a signature matrix
 * [n, num_perm] of sig_dtype (MHX_U32 / MHX_U64; columns from bands * r on are ignored):
 *     s = the sum of the band's r values in uint64, wrapping mod 2^64;  x = s mod (2^61 - 1)          (ref :105, :117)
 *     splitmix64 seeded with x: state = x; per draw state += 0x9E3779B97F4A7C15, z = state,
 *         z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, out = z ^ z >> 31
 *     block = ((out_0 >> 32) * n_blocks) >> 32                       (hence n_blocks in [1, 2^32 - 1])
 *     pos_i = (out_{1 + i / 7} >> 9 * (i % 7)) & 511 for i < k (k in [1, 32]); word pos >> 5, bit pos & 31; positions may repeat
 * The bit layout is this library's own: the reference leaves it to pybloomfilter, whose files are not read.
 * The entry points are exported through MHX_API_BLOOM (the same visibility as MHX_API), bound from _native._PROTOTYPES_BLOOM and
 * their argument checks are tested beside the feature, in tests/test_gpu_lsh_bloom.py. */
#define MHX_API_BLOOM __attribute__((visibility("default")))
/* d_filter |= the masks of every (row, band).  A word whose bits are all set already is read, not written.  Enqueued. */
MHX_API_BLOOM int mhx_bloom_insert_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands,
                                       int32_t r, int32_t k, int64_t n_blocks, uint32_t *d_filter);
/* d_hit uint8 [n]: 1 where some band's mask is wholly in that band's filter (MinHashLSHBloom.query, ref :363-372).  then_insert != 0:
 * a second launch on the same stream inserts every row afterwards -- the answers refer to the filter before the call (rows of one
 * call do not see each other): the streaming near-duplicate step.  Enqueued. */
MHX_API_BLOOM int mhx_bloom_query_dev(mhx_ctx *ctx, const void *d_sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands,
                                      int32_t r, int32_t k, int64_t n_blocks, uint32_t *d_filter, uint8_t *d_hit, int then_insert);
/* The same with host signatures (uploaded once) and host answers; d_filter stays a device array.  Blocking. */
MHX_API_BLOOM int mhx_bloom_insert(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r,
                                   int32_t k, int64_t n_blocks, uint32_t *d_filter);
MHX_API_BLOOM int mhx_bloom_query(mhx_ctx *ctx, const void *sig, int sig_dtype, int64_t n, int32_t num_perm, int32_t bands, int32_t r,
                                  int32_t k, int64_t n_blocks, uint32_t *d_filter, uint8_t *hit, int then_insert);
/* d_dst |= d_src over the bands * n_blocks * 16 words of two filters of equal geometry (merging shards).  Enqueued. */
MHX_API_BLOOM int mhx_bloom_union_dev(mhx_ctx *ctx, uint32_t *d_dst, const uint32_t *d_src, int32_t bands, int64_t n_blocks);

/* ---- Near-duplicate clusters: connected components ----------------------------------------------- */
/* The last step of deduplication (no counterpart in the reference): the rows 0 .. n-1 are the vertices, the edges are listed pairs
 * and / or the runs of equal digests of sorted bands, and d_labels uint32[n] receives for every row the SMALLEST row number of its
 * connected component -- one answer whatever order the edges come in.  labels[i] == i marks the one row to keep per cluster.
 *
 * The call sequence is mhx_cc_init_dev, then any number of link calls of either kind, then mhx_cc_finish_dev, all on one array.
 * Between init and finish the contents of d_labels are opaque (a parent forest of the union-find; only labels[i] <= i is promised),
 * and a link call on an array that init has not filled is undefined.  n in [0, 2^32 - 1]; n == 0, n_pairs == 0 and bands * n_sigs
 * == 0 launch nothing and need no pointers.  All four are enqueued on the ctx stream.
 *
 * d_invalid (may be NULL): an int64 on the device that the link calls ADD to -- the caller zeroes it once -- the number of edges
 * with an endpoint outside [0, n).  Such an edge is never followed, counted or not.
 *
 * The entry points are exported through MHX_API_CC (the same visibility as MHX_API), bound from _native._PROTOTYPES_CC and their
 * argument checks are tested beside the feature, in tests/test_gpu_clusters.py. */
#define MHX_API_CC __attribute__((visibility("default")))
MHX_API_CC int mhx_cc_init_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n);
/* d_pairs int64[n_pairs][2] in any order; duplicates, i > j and i == j are allowed.  d_counts (may be NULL) int32[n_pairs]: pair p
 * takes part only if d_counts[p] >= min_count -- the output of mhx_jaccard_pairs_dev* as it is, with no compaction pass. */
MHX_API_CC int mhx_cc_link_pairs_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const int64_t *d_pairs, int64_t n_pairs,
                                     const int32_t *d_counts, int32_t min_count, int64_t *d_invalid);
/* Sorted bands as mhx_lsh_sort_bands* writes them, digests uint64[bands][n_sigs] and rows uint32[bands][n_sigs]: position p > 0 of
 * band j links rows[j][p - 1] and rows[j][p] when digests[j][p] == digests[j][p - 1].  That gives the components of
 * mhx_lsh_candidate_pairs_dev's graph from at most bands * n_sigs implicit edges: a bucket of L rows costs L - 1 links, not
 * L (L - 1) / 2 pairs.  The last entry of a band and the first of the next are never compared.  A row >= n is an invalid edge. */
MHX_API_CC int mhx_cc_link_bands_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n, const uint64_t *d_sorted_digests,
                                     const uint32_t *d_sorted_rows, int64_t n_sigs, int32_t bands, int64_t *d_invalid);
MHX_API_CC int mhx_cc_finish_dev(mhx_ctx *ctx, uint32_t *d_labels, int64_t n);
/* Host form, blocking: init + link pairs + finish.  labels uint32[n]; *invalid (may be NULL) is set by the call. */
MHX_API_CC int mhx_cc_pairs(mhx_ctx *ctx, const int64_t *pairs, int64_t n_pairs, const int32_t *counts, int32_t min_count, int64_t n,
                            uint32_t *labels, int64_t *invalid);

/* ---- Shingles: the windows of a document hashed in place ------------------------------------------------------------------
 * Not in the reference, which leaves shingling to the caller (`for i in range(len(d) - k + 1): m.update(d[i:i+k])`);
 * datasketch_amd/shingle.py is the definition.  A corpus is one byte buffer and doc_offsets int64[n_docs + 1]; a window is `width`
 * consecutive ITEMS of one document and never crosses into the next one.
 *   byte mode  (item_offsets == NULL): an item is a byte; document d owns bytes doc_offsets[d] .. doc_offsets[d + 1]
 *   token mode: item i is bytes[item_offsets[i] .. item_offsets[i + 1]) (int64[n_items + 1], the byte_offsets of
 *              mhx_sha1_tokens); document d owns items doc_offsets[d] .. doc_offsets[d + 1]; a window is the contiguous byte range
 *              from the start of its first token to the end of its last
 * A document of m items has m - width + 1 windows, exactly one (the whole document) if 0 < m < width, none if m == 0.  Windows are
 * numbered document by document: set_offsets int64[n_docs + 1], the prefix sums of those counts, are the CSR offsets that
 * mhx_minhash_bulk_dev / mhx_hll_bulk_dev take with the window hashes as hv.  Nothing is materialised: the kernel reads the
 * corpus where it lies, one SHA-1 per window, and touches no byte outside bytes[0 .. end of the last item) rounded out to aligned
 * dwords that hold at least one such byte.
 *
 * Exported through MHX_API_SHINGLE (the same visibility as MHX_API), bound from _native._PROTOTYPES_SHINGLE; declared = bound =
 * exported is checked in tests/test_shingle_host.py, the argument checks in tests/test_gpu_shingles.py. */
#define MHX_API_SHINGLE __attribute__((visibility("default")))
/* set_offsets of a corpus: pure host logic, no device.  width >= 1; doc_offsets non-decreasing. */
MHX_API_SHINGLE int mhx_shingle_window_offsets(const int64_t *doc_offsets, int64_t n_docs, int64_t width, int64_t *set_offsets);
/* d_out[t] = sha1_hash32 (MHX_U32) or sha1_hash64 (MHX_U64) of window t, n_windows = set_offsets[n_docs] of them.  The device
 * arrays are TRUSTED: d_set_offsets must be what mhx_shingle_window_offsets gives for d_doc_offsets and width, and the item
 * offsets must be non-decreasing -- nothing on the device checks them.  d_bytes may be NULL when every window is empty. */
MHX_API_SHINGLE int mhx_sha1_windows_dev(mhx_ctx *ctx, const uint8_t *d_bytes, const int64_t *d_item_offsets,
                                         const int64_t *d_doc_offsets, const int64_t *d_set_offsets, int64_t n_docs,
                                         int64_t n_windows, int64_t width, int out_dtype, void *d_out);
/* The host forms (blocking) check their input -- width >= 1; doc_offsets runs from 0 to n_items (the number of bytes in byte mode)
 * and never decreases; item_offsets starts at 0 and never decreases, bytes holds item_offsets[n_items] bytes -- and compute the
 * set offsets themselves.  n_docs == 0 is a no-op.  out: one hash per window, sized by the caller from
 * mhx_shingle_window_offsets. */
MHX_API_SHINGLE int mhx_sha1_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                     const int64_t *doc_offsets, int64_t n_docs, int64_t width, int out_dtype, void *out);
/* Text in, signatures out: the twin of mhx_minhash_bulk_bytes_typed over windows -- the corpus goes up, the windows kernel and the
 * MinHash kernel run, out [n_docs, K] of out_dtype comes back (MHX_U32 as in mhx_minhash_bulk_typed).  init as in
 * mhx_minhash_bulk; a document without a window keeps its init row. */
MHX_API_SHINGLE int mhx_minhash_bulk_windows_typed(mhx_perm *perm, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                                   const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype,
                                                   const uint64_t *init, int64_t init_stride, void *out, int out_dtype);
/* The twin of mhx_hll_bulk_bytes over windows: uint8 registers [n_docs, 2^p]; p, hash_bits, init and init_stride as there. */
MHX_API_SHINGLE int mhx_hll_bulk_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                         const int64_t *doc_offsets, int64_t n_docs, int64_t width, int32_t hash_bits, int32_t p,
                                         const uint8_t *init, int64_t init_stride, uint8_t *out);

/* ---- Word shingles: text tokenised and normalised on the device -----------------------------------------------------------
 * datasketch_amd/shingle.py (word_table, words, word_shingles, normalize_words) is the definition.  table is a 256-byte translate
 * table on the HOST: table[c] == 0 makes byte c a separator, any other value is the byte emitted for c; table[0] must be 0.  A
 * word is a maximal run of non-separator bytes inside one document of a byte-mode corpus (bytes, doc_offsets int64[n_docs + 1]).
 * The normal form of the corpus is a token-mode corpus, the `packed=` triple of the shingle entry points:
 *   out_bytes         every word, translated, followed by one 0x20 -- the last word of a document included
 *   item_offsets      int64[n_words + 1]: item i is word i with its space
 *   word_doc_offsets  int64[n_docs + 1], in words: document d owns words word_doc_offsets[d] .. word_doc_offsets[d + 1]
 * so windows of w items of it are the w-word shingles, whatever separators stood between the words.
 *
 * The capacity protocol of the two normalize entries: the call counts first and ALWAYS stores *n_words and *n_out_bytes (blocking:
 * the totals are read back).  cap_bytes is the number of bytes out_bytes holds, cap_words the number of WORDS item_offsets holds
 * (it has cap_words + 1 entries); word_doc_offsets always has n_docs + 1.  With all three outputs NULL the call is a sizing call
 * and returns MHX_OK.  Otherwise, when n_words > cap_words or n_out_bytes > cap_bytes, nothing is written to any output and the
 * call returns MHX_ERR_CAPACITY (no older code means "your arrays are too small": MHX_ERR_OOM is about device allocations and
 * maps to MemoryError).  Otherwise it emits: exactly n_out_bytes bytes, n_words + 1 and n_docs + 1 entries.  n_docs == 0 is a no-op
 * (the totals are 0).  The kernels touch no input byte outside bytes[0 .. n_bytes) rounded out to aligned dwords that hold at
 * least one such byte.
 *
 * Exported through MHX_API_WORDS (the same visibility as MHX_API), bound from _native._PROTOTYPES_WORDS; declared = bound =
 * exported is checked in tests/test_words_host.py, the argument checks in tests/test_gpu_words.py. */
#define MHX_API_WORDS __attribute__((visibility("default")))
/* Device arrays in and out; they are TRUSTED (d_doc_offsets must run from 0 to n_bytes and never decrease). */
MHX_API_WORDS int mhx_words_normalize_dev(mhx_ctx *ctx, const uint8_t *d_bytes, int64_t n_bytes, const int64_t *d_doc_offsets,
                                          int64_t n_docs, const uint8_t *table, uint8_t *d_out_bytes, int64_t cap_bytes,
                                          int64_t *d_item_offsets, int64_t cap_words, int64_t *d_word_doc_offsets, int64_t *n_words,
                                          int64_t *n_out_bytes);
/* Host arrays in and out, checked: doc_offsets runs from 0 to n_bytes and never decreases, table is non-NULL with table[0] == 0;
 * MHX_ERR_INVALID otherwise. */
MHX_API_WORDS int mhx_words_normalize(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                      const uint8_t *table, uint8_t *out_bytes, int64_t cap_bytes, int64_t *item_offsets,
                                      int64_t cap_words, int64_t *word_doc_offsets, int64_t *n_words, int64_t *n_out_bytes);
/* Raw text in, word-shingle signatures out: the twins of mhx_minhash_bulk_windows_typed and mhx_hll_bulk_windows.  The corpus goes
 * up once, is normalised on the device, and the normal form goes straight into the windows kernel in token mode (width words per
 * window) and the MinHash / HyperLogLog kernels; the normalised text and its item offsets never visit the host.  The other
 * arguments as in the twins; checked like mhx_words_normalize. */
MHX_API_WORDS int mhx_minhash_bulk_words_typed(mhx_perm *perm, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets,
                                               int64_t n_docs, const uint8_t *table, int64_t width, int hash_dtype,
                                               const uint64_t *init, int64_t init_stride, void *out, int out_dtype);
MHX_API_WORDS int mhx_hll_bulk_words(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                     const uint8_t *table, int64_t width, int32_t hash_bits, int32_t p, const uint8_t *init,
                                     int64_t init_stride, uint8_t *out);

/* ---- Exact overlap of listed pairs: the verification step of deduplication ---------------------------------------------------
 * Not in the reference; datasketch_amd/overlap.py (overlap_counts_host: Python sets) is the definition.  Set i is
 * hv[set_offsets[i] .. set_offsets[i + 1]) of hv_dtype (MHX_U32 / MHX_U64) -- the arrays mhx_minhash_bulk_dev takes; values may
 * repeat and any value may occur, 0 and all ones included.  For pair p = (pairs[2p], pairs[2p + 1]) = (i, j) the call writes three
 * int32 counts of DISTINCT values,
 *   counts[3p .. 3p + 2] = ( |Si n Sj|, |Si|, |Sj| ),
 * from which union = a + b - inter, Jaccard = inter / union and containment = inter / a follow (both 1.0 at 0 / 0 by the
 * convention of overlap.py).  i == j gives (a, a, a); pairs may repeat and come in any order.  Everything is exact on the hashed
 * values: no sketch is involved.  One workgroup per pair (one wave for a pair of up to 512 items) builds a hash set of the pair in
 * LDS (overlap_kernels.hip); a pair of more items than mhx_overlap_limits names builds it in device scratch instead.  n_pairs <
 * 2^31; a set has fewer than 2^31 items.
 *
 * Exported through MHX_API_OVERLAP (the same visibility as MHX_API), bound from _native._PROTOTYPES_OVERLAP; declared = bound =
 * exported is checked in tests/test_overlap_host.py, the argument checks in tests/test_gpu_overlap.py. */
#define MHX_API_OVERLAP __attribute__((visibility("default")))
/* Pure host logic, no device: *lds_max_items = the largest number of items of a pair (both sets, repeats counted) whose table --
 * a 64-byte header, the power of two >= max(64, 2 items) of keys of hv_dtype, two bits per slot -- fits lds_per_block bytes
 * (0: none does).  lds_per_block >= 0. */
MHX_API_OVERLAP int mhx_overlap_limits(int hv_dtype, int64_t lds_per_block, int64_t *lds_max_items);
/* Device arrays, enqueued on the ctx stream, no synchronisation (pair lists and large tables live in the context's scratch, which
 * may grow).  max_set_items, in [0, 2^31 - 1], is the caller's bound on the items of any one named set: it sizes the tables of the
 * large pairs.  A pair with an index outside [0, n_sets) or a set of more than max_set_items items is never followed: its counts
 * are (-1, -1, -1) and it adds one to *d_invalid, an int64 on the device that the caller zeroes (may be NULL).  The offsets are
 * otherwise TRUSTED.  n_pairs == 0 or n_sets == 0 launches nothing and needs no pointers. */
MHX_API_OVERLAP int mhx_overlap_pairs_dev(mhx_ctx *ctx, const void *d_hv, int hv_dtype, const int64_t *d_set_offsets, int64_t n_sets,
                                          int64_t max_set_items, const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts,
                                          int64_t *d_invalid);
/* Host arrays, blocking, checked: set_offsets starts at 0 and never decreases, every pair index is in [0, n_sets) and every named
 * set has fewer than 2^31 items -- MHX_ERR_INVALID otherwise, and nothing is written.  n_pairs == 0 is a no-op. */
MHX_API_OVERLAP int mhx_overlap_pairs(mhx_ctx *ctx, const void *hv, int hv_dtype, const int64_t *set_offsets, int64_t n_sets,
                                      const int64_t *pairs, int64_t n_pairs, int32_t *counts);
/* Text in, counts out: the third sink beside the MinHash and HyperLogLog twins -- the corpus goes up once, is hashed on the device
 * with sha1_hash32 / sha1_hash64 (hash_dtype) and the pair kernels read the hashes where they lie; only the counts come back.
 * A set is the tokens of a `packed=` triple (bytes), the windows of a document (windows) or its w-word shingles (words); the
 * corpus arguments are those of mhx_minhash_bulk_bytes_typed, mhx_minhash_bulk_windows_typed and mhx_minhash_bulk_words_typed and
 * are checked as there; the pairs as in mhx_overlap_pairs, against the number of sets / documents. */
MHX_API_OVERLAP int mhx_overlap_pairs_bytes(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_dtype,
                                            const int64_t *set_offsets, int64_t n_sets, const int64_t *pairs, int64_t n_pairs,
                                            int32_t *counts);
MHX_API_OVERLAP int mhx_overlap_pairs_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                              const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype,
                                              const int64_t *pairs, int64_t n_pairs, int32_t *counts);
MHX_API_OVERLAP int mhx_overlap_pairs_words(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                            const uint8_t *table, int64_t width, int hash_dtype, const int64_t *pairs, int64_t n_pairs,
                                            int32_t *counts);

/* ---- xxHash: a second, cheap token hash for every text path -------------------------------------------------------------------
 * The reference hashes tokens with whatever `hashfunc` the caller passes; SHA-1 is only its default, and at corpus scale the usual
 * choice is a non-cryptographic hash.  datasketch_amd/hashfunc.py (xxh32_hash32, xxh64_hash64: XXH32 / XXH64 with seed 0, the
 * canonical integer values of the published algorithm) is the definition.  hash_kind selects the family, the width argument of
 * the entry selects the function inside it, as it always did for SHA-1:
 *   MHX_HASH_SHA1   MHX_U32 / hash_bits 32: sha1_hash32     MHX_U64 / hash_bits 64: sha1_hash64
 *   MHX_HASH_XXH    MHX_U32 / hash_bits 32: xxh32_hash32    MHX_U64 / hash_bits 64: xxh64_hash64
 * Any other hash_kind is MHX_ERR_INVALID ("unknown hash_kind <value>"), checked before every other argument but the handle.
 * Every entry below takes the arguments of the entry it is named after plus hash_kind -- in front of out_dtype for the two hash
 * entries, directly behind the hash width (hash_dtype / hash_bits) for the nine chains -- and is checked, staged and computed by
 * the same core: with MHX_HASH_SHA1 it IS the older entry, which is now a call of it.  The xxHash kernels (xxh_kernels.hip) read
 * under the rule of the SHA-1 kernels: no byte outside the aligned dwords that hold a byte of a token.
 *
 * Host forms only: a device-pointer form of the two hash entries would have to stand in tests/stream_order_cases.py first.
 *
 * Exported through MHX_API_XXH (the same visibility as MHX_API), bound from _native._PROTOTYPES_XXH; declared = bound = exported
 * is checked in tests/test_xxh_host.py, the argument checks in tests/test_gpu_xxh.py. */
enum { MHX_HASH_SHA1 = 0, MHX_HASH_XXH = 1 };
#define MHX_API_XXH __attribute__((visibility("default")))
/* mhx_sha1_tokens / mhx_sha1_windows with the hash named: one hash per token / window of out_dtype. */
MHX_API_XXH int mhx_hash_tokens(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens, int hash_kind,
                                int out_dtype, void *out);
MHX_API_XXH int mhx_hash_windows(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                 const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_kind, int out_dtype, void *out);
/* The MinHash chains: mhx_minhash_bulk_bytes_typed, mhx_minhash_bulk_windows_typed, mhx_minhash_bulk_words_typed. */
MHX_API_XXH int mhx_minhash_bulk_bytes_typed_hashed(mhx_perm *perm, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens,
                                                    int hash_dtype, int hash_kind, const int64_t *set_offsets, int64_t n_sets,
                                                    const uint64_t *init, int64_t init_stride, uint64_t *out);
MHX_API_XXH int mhx_minhash_bulk_windows_typed_hashed(mhx_perm *perm, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                                      const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype,
                                                      int hash_kind, const uint64_t *init, int64_t init_stride, void *out, int out_dtype);
MHX_API_XXH int mhx_minhash_bulk_words_typed_hashed(mhx_perm *perm, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets,
                                                    int64_t n_docs, const uint8_t *table, int64_t width, int hash_dtype, int hash_kind,
                                                    const uint64_t *init, int64_t init_stride, void *out, int out_dtype);
/* The HyperLogLog chains: mhx_hll_bulk_bytes, mhx_hll_bulk_windows, mhx_hll_bulk_words. */
MHX_API_XXH int mhx_hll_bulk_bytes_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens,
                                          int32_t hash_bits, int hash_kind, const int64_t *set_offsets, int64_t n_sets, int32_t p,
                                          const uint8_t *init, int64_t init_stride, uint8_t *out);
MHX_API_XXH int mhx_hll_bulk_windows_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                            const int64_t *doc_offsets, int64_t n_docs, int64_t width, int32_t hash_bits, int hash_kind,
                                            int32_t p, const uint8_t *init, int64_t init_stride, uint8_t *out);
MHX_API_XXH int mhx_hll_bulk_words_hashed(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets, int64_t n_docs,
                                          const uint8_t *table, int64_t width, int32_t hash_bits, int hash_kind, int32_t p,
                                          const uint8_t *init, int64_t init_stride, uint8_t *out);
/* The overlap chains: mhx_overlap_pairs_bytes, mhx_overlap_pairs_windows, mhx_overlap_pairs_words. */
MHX_API_XXH int mhx_overlap_pairs_bytes_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *byte_offsets, int64_t n_tokens,
                                               int hash_dtype, int hash_kind, const int64_t *set_offsets, int64_t n_sets,
                                               const int64_t *pairs, int64_t n_pairs, int32_t *counts);
MHX_API_XXH int mhx_overlap_pairs_windows_hashed(mhx_ctx *ctx, const uint8_t *bytes, const int64_t *item_offsets, int64_t n_items,
                                                 const int64_t *doc_offsets, int64_t n_docs, int64_t width, int hash_dtype, int hash_kind,
                                                 const int64_t *pairs, int64_t n_pairs, int32_t *counts);
MHX_API_XXH int mhx_overlap_pairs_words_hashed(mhx_ctx *ctx, const uint8_t *bytes, int64_t n_bytes, const int64_t *doc_offsets,
                                               int64_t n_docs, const uint8_t *table, int64_t width, int hash_dtype, int hash_kind,
                                               const int64_t *pairs, int64_t n_pairs, int32_t *counts);

/* ---- Multi-GPU: assemble the signature matrix (RCCL over xGMI) ----------------------------- */
/* 128-byte RCCL unique id, created on rank 0 and distributed by the caller (env, file, socket). */
#define MHX_COMM_ID_BYTES 128
/* RCCL (librccl.so) is bound with dlopen at the first mhx_comm_* call, so libmhx loads on hosts without it. */
MHX_API int mhx_comm_unique_id(uint8_t id[MHX_COMM_ID_BYTES]);
MHX_API int mhx_comm_create(mhx_ctx *ctx, const uint8_t id[MHX_COMM_ID_BYTES], int rank,
                            int world_size, mhx_comm **comm);
MHX_API int mhx_comm_destroy(mhx_comm *comm);
/* What RCCL itself reports for the communicator: ncclCommUserRank, ncclCommCount ("ranks seen"),
 * ncclCommCuDevice and ncclGetVersion.  Any out pointer may be NULL. */
MHX_API int mhx_comm_info(mhx_comm *comm, int *rank, int *world_size, int *device, int *rccl_version);
/* All-gather equal-sized row shards: every rank contributes bytes_per_rank bytes from d_send,
 * d_recv receives world_size*bytes_per_rank bytes in rank order.  Enqueued on the ctx stream. */
MHX_API int mhx_comm_allgather_dev(mhx_comm *comm, const void *d_send, void *d_recv,
                                   size_t bytes_per_rank);
/* All-gather of UNEQUAL row shards, in place: rank q contributes recv_bytes[q] bytes (its own entry from d_send),
 * and every rank receives them at d_recv + recv_offsets[q].  recv_offsets / recv_bytes: host arrays of world_size
 * entries, identical on every rank (shard sizes are common knowledge: SURVEY.md section 8e "AllGatherv-style with
 * per-rank counts").  One grouped launch of ncclBroadcast per root; enqueued on the ctx stream, no host sync. */
MHX_API int mhx_comm_allgatherv_dev(mhx_comm *comm, const void *d_send, void *d_recv,
                                    const uint64_t *recv_offsets, const uint64_t *recv_bytes);
/* A grouped point-to-point exchange (ncclSend / ncclRecv inside one group call, one launch): the BY-BAND exchange of band
 * digests.  The reference's index is one independent hashtable per band (ref: datasketch/lsh.py:199,326-347), so the rank that
 * builds the tables of bands [lo, hi) needs those bands' digests of ALL rows -- [hi - lo, N] uint64 -- and nothing else: every
 * rank digests its own rows band-major ([bands, n_p]) and sends each peer the runs of that peer's bands (at 10M rows x 32 bands
 * on 8 ranks: 0.28 GB received per GPU where the all-gather of the uint32 signature matrix receives 8.96 GB).
 *   message i of the send list: send_bytes[i] bytes at d_send + send_offsets[i] go to rank send_peers[i];
 *   message i of the receive list: recv_bytes[i] bytes from rank recv_peers[i] land at d_recv + recv_offsets[i].
 * Between a pair of ranks messages are matched in list order.  A message a rank sends to itself is a device copy on the stream
 * (its k-th such send pairs with its k-th such receive; sizes must agree).  Messages of zero bytes are dropped on both sides.
 * All lists are host arrays; enqueued on the ctx stream, no host synchronisation.  d_send and d_recv must not overlap. */
MHX_API int mhx_comm_exchange_dev(mhx_comm *comm, const void *d_send, void *d_recv, int32_t n_send, const int32_t *send_peers,
                                  const uint64_t *send_offsets, const uint64_t *send_bytes, int32_t n_recv,
                                  const int32_t *recv_peers, const uint64_t *recv_offsets, const uint64_t *recv_bytes);

#ifdef __cplusplus
}
#endif

/* ---- Weighted Jaccard: pairs, all pairs, thresholded and top-k on WeightedMinHash rows ------------------------------------
 * mhx_weighted_jaccard_pairs, _matrix, _threshold_pairs, _topk and their "_dev" forms: declared in a header of their own. */
#include "mhx_weighted_jaccard.h"

#endif /* MHX_H_ */
