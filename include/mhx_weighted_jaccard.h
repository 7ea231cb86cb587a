/*
 * mhx_weighted_jaccard.h -- the weighted Jaccard entry points of libmhx: WeightedMinHash.jaccard for listed pairs, for every
 * pair of two matrices, thresholded and as top-k.  Part of the C ABI of mhx.h, which includes this file (include either).
 *
 * A weighted signature (ref: datasketch/weighted_minhash.py:11-30, the rows WeightedMinHashGenerator.minhash_many writes) is
 * `samples` pairs (k, t) of int64: a matrix is int64[n, samples, 2], 16 bytes per sample, 8-byte aligned.  Everywhere below
 *     count(x, y) = the number of samples s with x[s][0] == y[s][0] AND x[s][1] == y[s][1],
 * compared on all 64 bits of both values (t is often negative), and the estimate is (double)count / (double)samples (ref:
 * weighted_minhash.py:45-60).  Counts are exact: nothing is hashed down.  The MinHash entry points of mhx.h cannot stand in on a
 * [n, 2 * samples] view of the words: rows with equal k and different t would count one word each.
 *
 * Each entry is the twin of the MinHash entry named beside it and shares its checked core, launcher and kernels' tile: the
 * arguments and the contract are the twin's, word for word, with `samples` in place of num_perm and no sig_dtype.  So: d_b == NULL
 * is the self-join; ldc >= n_b; min_count <= 0 keeps every pair and min_count > samples none; *n_pairs is always the exact total
 * and nothing is written at or past `capacity` entries; pairs come ascending by (i, j); top-k lists are ordered by (count
 * descending, row ascending) and padded with -1; d_b_live_bits masks rows of B; 1 <= k <= MHX_TOPK_MAX; fewer than 2^32 rows per
 * matrix; the "_dev" forms enqueue on the context's stream except the thresholded one, which blocks to read *n_pairs back; scratch
 * (the sort's, the partial top-k lists) stays in the context until mhx_ctx_release_scratch.
 *
 * Exported through MHX_API_WJ (the same visibility as MHX_API) and bound from _native._PROTOTYPES_WJ; declared = bound = exported
 * is checked in tests/test_weighted_jaccard_host.py, the argument checks in tests/test_gpu_weighted_jaccard.py.  The "_dev" forms
 * run on guard-paged, poisoned and far-offset buffers and behind in-flight work in tests/weighted_jaccard_guard_cases.py and
 * tests/weighted_jaccard_sweep_cases.py.
 */
#ifndef MHX_WEIGHTED_JACCARD_H_
#define MHX_WEIGHTED_JACCARD_H_

#include "mhx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MHX_API_WJ __attribute__((visibility("default")))

/* counts[p] = count(row pairs[p][0] of sig_a, row pairs[p][1] of sig_b); pairs int64[n_pairs, 2].  (mhx_jaccard_pairs_dev) */
MHX_API_WJ int mhx_weighted_jaccard_pairs_dev(mhx_ctx *ctx, const int64_t *d_sig_a, const int64_t *d_sig_b, int32_t samples,
                                              const int64_t *d_pairs, int64_t n_pairs, int32_t *d_counts);
/* Host form: both ends of a pair index the n_sigs rows of sig; an index outside [0, n_sigs) is MHX_ERR_INVALID.  (mhx_jaccard_pairs) */
MHX_API_WJ int mhx_weighted_jaccard_pairs(mhx_ctx *ctx, const int64_t *sig, int64_t n_sigs, int32_t samples, const int64_t *pairs,
                                          int64_t n_pairs, int32_t *counts);
/* counts[i * ldc + j] = count(row i of A, row j of B).  (mhx_jaccard_matrix_dev, mhx_jaccard_matrix) */
MHX_API_WJ int mhx_weighted_jaccard_matrix_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b,
                                               int32_t samples, int32_t *d_counts, int64_t ldc);
MHX_API_WJ int mhx_weighted_jaccard_matrix(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b, int32_t samples,
                                           int32_t *counts);
/* Every pair with count >= min_count.  Blocking.  (mhx_jaccard_threshold_pairs_dev, mhx_jaccard_threshold_pairs) */
MHX_API_WJ int mhx_weighted_jaccard_threshold_pairs_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b,
                                                        int32_t samples, int32_t min_count, int64_t *d_pairs, int32_t *d_counts,
                                                        int64_t capacity, int64_t *n_pairs);
MHX_API_WJ int mhx_weighted_jaccard_threshold_pairs(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b,
                                                    int32_t samples, int32_t min_count, int64_t *pairs, int32_t *counts,
                                                    int64_t capacity, int64_t *n_pairs);
/* Per row of A the k rows of B with the largest count.  (mhx_jaccard_topk_dev, mhx_jaccard_topk) */
MHX_API_WJ int mhx_weighted_jaccard_topk_dev(mhx_ctx *ctx, const int64_t *d_a, int64_t n_a, const int64_t *d_b, int64_t n_b,
                                             int32_t samples, const uint32_t *d_b_live_bits, int32_t min_count, int32_t k,
                                             int64_t *d_rows, int32_t *d_counts);
MHX_API_WJ int mhx_weighted_jaccard_topk(mhx_ctx *ctx, const int64_t *a, int64_t n_a, const int64_t *b, int64_t n_b, int32_t samples,
                                         int32_t min_count, int32_t k, int64_t *rows, int32_t *counts);

#ifdef __cplusplus
}
#endif
#endif /* MHX_WEIGHTED_JACCARD_H_ */
