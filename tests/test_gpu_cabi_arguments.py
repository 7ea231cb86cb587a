"""The argument contract of the C ABI (run on an MI355X: python -m pytest tests -m gpu).

One table: (entry point, one argument of a valid call replaced, message of mhx_last_error -- or None for MHX_OK --, and the
values the call leaves in its integer out-parameters).  Every row is a call libmhx answers from its argument checks, before
anything reaches the device: out-of-range scalars, unknown dtype / layout / byte-order codes, bands * r > k, a NULL where a
pointer is required, host offsets that do not grow, host pair and column indices out of range -- and the empty calls
(n == 0 and its kin with NULL data pointers) that succeed without a launch.  The pointers of the valid call the rows start
from are real buffers of 64 KiB for shapes of a few rows, so no row can hand a kernel something it could fault on.

The expected messages are the library's own at the commit before the checks of mhx_api.hip were folded into shared
functions; the strings that change deliberately with that (one wording per condition) are marked `unified`.
"""
import ctypes
import re

import numpy as np
import pytest

from datasketch_amd import _native

pytestmark = pytest.mark.gpu

OK, INVALID = _native.MHX_OK, _native.MHX_ERR_INVALID
CTX, PERM, GEN, DEV, DEV1, HOST = "<ctx>", "<perm>", "<gen>", "<device buffer>", "<device buffer + 1 byte>", "<host buffer>"
OUT64, OUT32 = "<int64 out>", "<int out>"  # integer out-parameters: hold 777 before the call
UNTOUCHED = 777
K, DIM, SAMPLES = 8, 8, 4  # num_perm of PERM; dim and sample_size of GEN
BIG = 1 << 32


def i64(*v):
    return np.array(v, dtype=np.int64)


def i32(*v):
    return np.array(v, dtype=np.int32)


BYTES = np.frombuffer(b"abcd", dtype=np.uint8)

# entry point -> the arguments of a small valid call, in the order of include/mhx.h
VALID = {
    "mhx_device_count": dict(count=OUT32),
    "mhx_ctx_create": dict(device=0, out=HOST),
    "mhx_ctx_destroy": dict(ctx=CTX),
    "mhx_ctx_synchronize": dict(ctx=CTX),
    "mhx_ctx_release_scratch": dict(ctx=CTX),
    "mhx_ctx_device_info": dict(ctx=CTX, name=None, name_len=0, cus=None, hbm_bytes=None),
    "mhx_ctx_set_option": dict(ctx=CTX, key=b"lsh.sort", value=0),
    "mhx_ctx_minhash_mode": dict(ctx=CTX, reset=0, mode=None),
    "mhx_ctx_minhash_flags": dict(ctx=CTX, n_sets=1, flags=HOST),
    "mhx_ctx_counters": dict(ctx=CTX, enable=0, out=None),
    "mhx_debug_guard_alloc": dict(align=0, granule=None, live=None),
    "mhx_debug_poison_alloc": dict(byte_value=-1),
    "mhx_dev_alloc": dict(ctx=CTX, bytes=16, dptr=HOST),
    "mhx_dev_free": dict(ctx=CTX, dptr=None),
    "mhx_host_alloc": dict(ctx=CTX, bytes=16, ptr=HOST),
    "mhx_host_free": dict(ctx=CTX, ptr=None),
    "mhx_memcpy_h2d": dict(ctx=CTX, dst=DEV, src=HOST, bytes=16),
    "mhx_memcpy_d2h": dict(ctx=CTX, dst=HOST, src=DEV, bytes=16),
    "mhx_memcpy_d2d": dict(ctx=CTX, dst=DEV, src=DEV, bytes=16),
    "mhx_memset_dev": dict(ctx=CTX, dst=DEV, byte_value=0, bytes=16),
    "mhx_event_create": dict(ctx=CTX, ev=HOST),
    "mhx_event_record": dict(ev=None),
    "mhx_event_synchronize": dict(ev=None),
    "mhx_event_elapsed_ms": dict(start=None, stop=None, ms=None),
    "mhx_event_destroy": dict(ev=None),
    "mhx_perm_create": dict(ctx=CTX, a=HOST, b=HOST, num_perm=K, out=HOST),
    "mhx_perm_destroy": dict(perm=PERM),
    "mhx_minhash_bulk_dev": dict(perm=PERM, d_hv=DEV, hv_dtype=0, d_offsets=None, fixed_len=4, n_sets=2, total_tokens=8, d_init=None,
                                 init_stride=0, d_out=DEV, out_dtype=0),
    "mhx_minhash_bulk_typed": dict(perm=PERM, hv=HOST, hv_dtype=0, offsets=None, fixed_len=4, n_sets=2, init=None, init_stride=0, out=HOST,
                                   out_dtype=0),
    "mhx_minhash_bulk": dict(perm=PERM, hv=HOST, offsets=None, fixed_len=4, n_sets=2, init=None, init_stride=0, out=HOST),
    "mhx_sha1_tokens_dev": dict(ctx=CTX, d_bytes=DEV, d_byte_offsets=DEV, n_tokens=2, out_dtype=1, d_out=DEV),
    "mhx_sha1_tokens": dict(ctx=CTX, bytes=BYTES, byte_offsets=i64(0, 2, 4), n_tokens=2, out_dtype=1, out=HOST),
    "mhx_minhash_bulk_bytes_typed": dict(perm=PERM, bytes=BYTES, byte_offsets=i64(0, 2, 4), n_tokens=2, hash_dtype=1, set_offsets=i64(0, 1, 2),
                                         n_sets=2, init=None, init_stride=0, out=HOST),
    "mhx_minhash_bulk_bytes": dict(perm=PERM, bytes=BYTES, byte_offsets=i64(0, 2, 4), n_tokens=2, set_offsets=i64(0, 1, 2), n_sets=2, init=None,
                                   init_stride=0, out=HOST),
    "mhx_minhash_update_batch": dict(perm=PERM, hv=HOST, n=4, hashvalues=HOST),
    "mhx_minhash_merge_dev": dict(ctx=CTX, d_x=DEV, d_y=DEV, count=K, d_out=DEV),
    "mhx_minhash_merge": dict(ctx=CTX, x=HOST, y=HOST, count=K, out=HOST),
    "mhx_bbit_num_blocks": dict(num_perm=K, b=4, num_blocks=OUT32),
    "mhx_bbit_pack_dev": dict(ctx=CTX, d_sig=DEV, n=2, k=K, b=4, d_out=DEV),
    "mhx_bbit_pack_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, b=4, d_out=DEV),
    "mhx_bbit_pack": dict(ctx=CTX, sig=HOST, n=2, k=K, b=4, out=HOST),
    "mhx_bbit_unpack_dev": dict(ctx=CTX, d_blocks=DEV, n=2, k=K, b=4, d_out=DEV),
    "mhx_bbit_unpack": dict(ctx=CTX, blocks=HOST, n=2, k=K, b=4, out=HOST),
    "mhx_band_keys_dev": dict(ctx=CTX, d_sig=DEV, n=2, k=K, bands=2, r=4, d_out=DEV),
    "mhx_band_keys": dict(ctx=CTX, sig=HOST, n=2, k=K, bands=2, r=4, out=HOST),
    "mhx_band_digests_dev": dict(ctx=CTX, d_sig=DEV, n=2, k=K, bands=2, r=4, d_out=DEV),
    "mhx_band_digests_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, bands=2, r=4, d_out=DEV),
    "mhx_band_digests_layout_dev": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, bands=2, r=4, layout=0, d_out=DEV),
    "mhx_band_digests": dict(ctx=CTX, sig=HOST, n=2, k=K, bands=2, r=4, out=HOST),
    "mhx_bbit_pack_band_digests_dev": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, b=4, bands=2, r=4, digest_layout=0, d_blocks=DEV,
                                           d_digests=DEV, fused=OUT32),
    "mhx_lsh_sort_bands_dev": dict(ctx=CTX, d_sig=DEV, n=2, k=K, bands=2, r=4, d_sorted_digests=DEV, d_sorted_rows=DEV),
    "mhx_lsh_sort_bands_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, bands=2, r=4, d_sorted_digests=DEV, d_sorted_rows=DEV),
    "mhx_lsh_sort_bands": dict(ctx=CTX, sig=HOST, n=2, k=K, bands=2, r=4, sorted_digests=HOST, sorted_rows=HOST),
    "mhx_lsh_sort_digests_dev": dict(ctx=CTX, d_digests=DEV, n=2, bands=2, d_sorted_digests=DEV, d_sorted_rows=DEV),
    "mhx_lsh_sort_digests_layout_dev": dict(ctx=CTX, d_digests=DEV, n=2, bands=2, layout=0, d_sorted_digests=DEV, d_sorted_rows=DEV),
    "mhx_lsh_candidate_pairs_dev": dict(ctx=CTX, d_sorted_digests=DEV, d_sorted_rows=DEV, n=2, bands=2, d_pairs=DEV, capacity=4, n_pairs=OUT64,
                                        n_raw=OUT64),
    "mhx_lsh_candidate_pairs": dict(ctx=CTX, sig=HOST, n=2, k=K, bands=2, r=4, pairs=HOST, capacity=4, n_pairs=OUT64, n_raw=OUT64),
    "mhx_lsh_query_dev": dict(ctx=CTX, d_sorted_digests=DEV, d_sorted_rows=DEV, n=2, bands=2, r=4, d_query_sig=DEV, d_index_sig=DEV, sig_dtype=0,
                              k=K, m=2, d_pairs=DEV, capacity=4, n_pairs=OUT64),
    # (levels: a list of (d_digests, d_rows, r, bands) that Env.call lays out as mhx_ensemble_level records)
    "mhx_lsh_ensemble_query_dev": dict(ctx=CTX, levels=[(DEV, DEV, 4, 2)], n_levels=1, start=i64(0, 2), n_parts=1, d_index_sig=DEV, sig_dtype=0,
                                       row_words=K, d_query_sig=DEV, n_queries=2, d_choice=DEV, params=i32(0, 2), n_params=1, d_pairs=DEV,
                                       capacity=4, n_pairs=OUT64),
    "mhx_jaccard_pairs_dev": dict(ctx=CTX, d_sig_a=DEV, d_sig_b=DEV, k=K, d_pairs=DEV, n_pairs=1, d_counts=DEV),
    "mhx_jaccard_pairs_dev_typed": dict(ctx=CTX, d_sig_a=DEV, d_sig_b=DEV, sig_dtype=0, k=K, d_pairs=DEV, n_pairs=1, d_counts=DEV),
    "mhx_jaccard_pairs": dict(ctx=CTX, sig=HOST, n=2, k=K, pairs=i64(0, 1), n_pairs=1, counts=HOST),
    "mhx_bbit_jaccard_pairs_dev": dict(ctx=CTX, d_blocks_a=DEV, d_blocks_b=DEV, k=K, b=4, d_pairs=DEV, n_pairs=1, d_counts=DEV),
    "mhx_bbit_jaccard_pairs": dict(ctx=CTX, blocks=HOST, n=2, k=K, b=4, pairs=i64(0, 1), n_pairs=1, counts=HOST),
    "mhx_lean_serialize_dev": dict(ctx=CTX, d_sig=DEV, n=2, k=K, seed=1, d_out=DEV),
    "mhx_lean_serialize_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, k=K, seed=1, byteorder=0, d_out=DEV),
    "mhx_lean_serialize": dict(ctx=CTX, sig=HOST, n=2, k=K, seed=1, out=HOST),
    "mhx_lean_deserialize_dev": dict(ctx=CTX, d_records=DEV, n=2, k=K, byteorder=0, sig_dtype=0, d_sig=DEV, d_seeds=DEV, d_bad=DEV),
    "mhx_lean_deserialize": dict(ctx=CTX, records=HOST, n=2, k=K, byteorder=0, sig=HOST, seeds=HOST),
    "mhx_wgen_create": dict(ctx=CTX, rs=HOST, ln_cs=HOST, betas=HOST, sample_size=SAMPLES, dim=DIM, out=HOST),
    "mhx_wgen_destroy": dict(gen=GEN),
    "mhx_weighted_minhash_many_dev": dict(gen=GEN, d_indptr=DEV, d_indices=DEV, d_values=DEV, values_are_logs=0, n_rows=2, nnz=2, d_out=DEV,
                                          d_nonempty=DEV),
    "mhx_weighted_minhash_many": dict(gen=GEN, indptr=i64(0, 1, 2), indices=i32(0, 1), values=np.ones(2, np.float32), values_are_logs=0, n_rows=2,
                                      out=HOST, nonempty=HOST),
    "mhx_weighted_logf": dict(ctx=CTX, x=HOST, n=4, out=HOST),
    "mhx_weighted_minhash_many_dense_dev": dict(gen=GEN, d_x=DEV, values_are_logs=0, n_rows=2, d_out=DEV, d_nonempty=DEV),
    "mhx_weighted_minhash_many_dense": dict(gen=GEN, x=HOST, values_are_logs=0, n_rows=2, out=HOST, nonempty=HOST),
    "mhx_weighted_dense_begin": dict(gen=GEN, values_are_logs=0, piece_rows=16, feed=HOST),
    "mhx_weighted_dense_feed": dict(feed=None, x=HOST, n_rows=1, out=HOST, nonempty=HOST),
    "mhx_weighted_dense_end": dict(feed=None),
    "mhx_jaccard_matrix_dev": dict(ctx=CTX, d_a=DEV, n_a=2, d_b=DEV, n_b=2, sig_dtype=0, num_perm=K, d_counts=DEV, ldc=2),
    "mhx_jaccard_matrix": dict(ctx=CTX, a=HOST, n_a=2, b=HOST, n_b=2, num_perm=K, counts=HOST),
    "mhx_jaccard_threshold_pairs_dev": dict(ctx=CTX, d_a=DEV, n_a=2, d_b=DEV, n_b=2, sig_dtype=0, num_perm=K, min_count=1, d_pairs=DEV,
                                            d_counts=DEV, capacity=4, n_pairs=OUT64),
    "mhx_jaccard_threshold_pairs": dict(ctx=CTX, a=HOST, n_a=2, b=HOST, n_b=2, num_perm=K, min_count=1, pairs=HOST, counts=HOST, capacity=4,
                                        n_pairs=OUT64),
    "mhx_bbit_jaccard_matrix_dev": dict(ctx=CTX, d_a=DEV, n_a=2, d_b=DEV, n_b=2, num_perm=K, b=4, d_counts=DEV, ldc=2),
    "mhx_bbit_jaccard_matrix": dict(ctx=CTX, a=HOST, n_a=2, b_blocks=HOST, n_b=2, num_perm=K, b=4, counts=HOST),
    "mhx_bbit_jaccard_threshold_pairs_dev": dict(ctx=CTX, d_a=DEV, n_a=2, d_b=DEV, n_b=2, num_perm=K, b=4, min_count=1, d_pairs=DEV,
                                                 d_counts=DEV, capacity=4, n_pairs=OUT64),
    "mhx_bbit_jaccard_threshold_pairs": dict(ctx=CTX, a=HOST, n_a=2, b_blocks=HOST, n_b=2, num_perm=K, b=4, min_count=1, pairs=HOST, counts=HOST,
                                             capacity=4, n_pairs=OUT64),
    "mhx_lsh_bands_merge_dev": dict(ctx=CTX, d_dig_a=DEV, d_rows_a=DEV, n_a=2, d_dig_b=DEV, d_rows_b=DEV, n_b=2, row_offset_b=2, bands=2,
                                    d_dig_out=DEV, d_rows_out=DEV),
    "mhx_lsh_bands_compact_dev": dict(ctx=CTX, d_dig=DEV, d_rows=DEV, n=2, bands=2, d_live_bits=DEV, n_live=1, d_dig_out=DEV, d_rows_out=DEV),
    "mhx_rows_compact_dev": dict(ctx=CTX, d_src=DEV, row_bytes=8, n_rows=2, d_live_bits=DEV, d_dst=DEV, n_kept=OUT64),
    "mhx_lsh_forest_build_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, row_words=K, l=2, tree_words=4, d_order=DEV),
    "mhx_lsh_forest_query_dev_typed": dict(ctx=CTX, d_sig=DEV, sig_dtype=0, n=2, row_words=K, l=2, tree_words=4, w=1, d_order=DEV, d_probes=DEV,
                                           m=2, k=2, d_slots=DEV, d_counts=DEV),
}

# what a NULL handle answers where it is not "<first argument> is NULL"; None: the call succeeds (destroying nothing)
NULL_HANDLE = {
    "mhx_ctx_destroy": None, "mhx_perm_destroy": None, "mhx_wgen_destroy": None, "mhx_host_free": None,
    "mhx_ctx_set_option": "ctx/key is NULL", "mhx_dev_alloc": "ctx/dptr is NULL", "mhx_host_alloc": "ctx/ptr is NULL",
    "mhx_event_create": "ctx/ev is NULL", "mhx_perm_create": "NULL argument", "mhx_wgen_create": "NULL argument",
}
# ... and what it leaves in the out-parameters (default: untouched)
NULL_HANDLE_OUTS = {
    "mhx_bbit_pack_band_digests_dev": dict(fused=0),
    "mhx_bbit_jaccard_threshold_pairs_dev": dict(n_pairs=0),
    "mhx_bbit_jaccard_threshold_pairs": dict(n_pairs=0),
}

GEOMETRY = "bands*r must be in (0, num_perm]"
B_RANGE = "b must be an integer in [0, 32]"
ROWS_32 = "more than 2^32-1 rows per call"
DEVP, HOSTP = "NULL device pointer", "NULL host pointer"

CASES = []  # (entry, {argument: replacement}, message or None, {out-parameter: value after the call})


def case(entry, changes, message, **outs):
    CASES.append((entry, changes, message, outs))


def each(entry, names, message, **outs):
    """One case per name: that argument NULL."""
    for name in names:
        case(entry, {name: None}, message, **outs)


def empty(entry, sizes, **outs):
    """The empty call: the size arguments 0, every data pointer NULL, MHX_OK."""
    changes = {name: None for name, v in VALID[entry].items() if isinstance(v, np.ndarray) or v in (DEV, HOST)}
    changes.update(sizes)
    case(entry, changes, None, **outs)


def geometry(entry, **outs):
    for changes in (dict(bands=0), dict(r=0), dict(bands=-1, r=-4), dict(bands=3), dict(k=7)):
        case(entry, changes, GEOMETRY, **outs)


def sig_dtype(entry, **outs):
    for code in (2, -1, 7):
        case(entry, dict(sig_dtype=code), f"bad sig_dtype {code}", **outs)


# ---- context, memory, events
case("mhx_device_count", dict(count=None), "count is NULL")
case("mhx_ctx_create", dict(out=None), "ctx out pointer is NULL")
case("mhx_ctx_create", dict(device=-1), re.compile(r"device -1 out of range \[0,\d+\)"))
case("mhx_ctx_create", dict(device=1 << 20), re.compile(r"device 1048576 out of range \[0,\d+\)"))
case("mhx_ctx_set_option", dict(key=None), "ctx/key is NULL")
case("mhx_ctx_set_option", dict(key=b"no.such"), "unknown option 'no.such'")
case("mhx_ctx_set_option", dict(key=b"lsh.sort "), "unknown option 'lsh.sort '")
case("mhx_ctx_set_option", dict(key=b""), "unknown option ''")
for v in (1, -8, 12, 32):
    case("mhx_ctx_set_option", dict(key=b"lsh.merge_items", value=v), "lsh.merge_items must be 0, 8 or 16")
case("mhx_ctx_set_option", dict(key=b"debug.cus", value=-1), re.compile(r"debug\.cus must be 0 \(the device's \d+ CUs\) or in \[1, \d+\], got -1"))
case("mhx_ctx_set_option", dict(key=b"debug.cus", value=0), None)
case("mhx_ctx_minhash_flags", dict(n_sets=-1), "NULL flags")
case("mhx_ctx_minhash_flags", dict(flags=None), "NULL flags")
for a in (3, 24, -6, 8192, -8192):
    case("mhx_debug_guard_alloc", dict(align=a), f"guard alignment must be 0 (off) or +-(a power of two <= 4096), got {a}")
for v in (-2, 256):
    case("mhx_debug_poison_alloc", dict(byte_value=v), f"poison byte must be -1 (off) or 0..255, got {v}")
case("mhx_dev_alloc", dict(dptr=None), "ctx/dptr is NULL")
case("mhx_dev_free", {}, None)
case("mhx_host_alloc", dict(ptr=None), "ctx/ptr is NULL")
case("mhx_host_free", {}, None)
for e in ("mhx_memcpy_h2d", "mhx_memcpy_d2h", "mhx_memcpy_d2d", "mhx_memset_dev"):
    case(e, dict(bytes=0, dst=None), None)
case("mhx_event_create", dict(ev=None), "ctx/ev is NULL")
case("mhx_event_record", {}, "event is NULL")
case("mhx_event_synchronize", {}, "event is NULL")
case("mhx_event_elapsed_ms", {}, "event/ms is NULL")
case("mhx_event_destroy", {}, None)

# ---- MinHash
each("mhx_perm_create", ("a", "b", "out"), "NULL argument")
for v in (0, -1):
    case("mhx_perm_create", dict(num_perm=v), f"num_perm must be positive, got {v}")
E = "mhx_minhash_bulk_dev"
case(E, dict(n_sets=-1), "n_sets must be >= 0")
case(E, dict(hv_dtype=7), "bad hv_dtype 7")
case(E, dict(out_dtype=7), "bad out_dtype 7")
case(E, dict(fixed_len=-1), "fixed_len must be >= 0 when offsets is NULL")
case(E, dict(init_stride=K - 1), "init_stride must be 0 or >= num_perm")
case(E, dict(init_stride=-1), "init_stride must be 0 or >= num_perm")
case(E, dict(total_tokens=-1), "total_tokens must be >= 0")
empty(E, dict(n_sets=0, total_tokens=0))
case(E, dict(d_out=None), "d_out is NULL")
case(E, dict(d_hv=None), "d_hv is NULL")
E = "mhx_minhash_bulk_typed"
case(E, dict(n_sets=-1), "n_sets must be >= 0")
case(E, dict(hv_dtype=7), "bad hv_dtype 7")
case(E, dict(out_dtype=7), "bad out_dtype 7")
empty(E, dict(n_sets=0))
case(E, dict(out=None), "out is NULL")
case(E, dict(fixed_len=-1), "fixed_len must be >= 0 when offsets is NULL")
case(E, dict(offsets=i64(-1, 0, 0)), "offsets[0] must be >= 0")
case(E, dict(offsets=i64(0, 3, 2)), "offsets must be non-decreasing (row 1)")
case(E, dict(offsets=i64(2, 1, 1)), "offsets must be non-decreasing (row 0)")
case(E, dict(hv=None), "hv is NULL")
E = "mhx_minhash_bulk"
case(E, dict(n_sets=-1), "n_sets must be >= 0")
empty(E, dict(n_sets=0))
case(E, dict(out=None), "out is NULL")
case(E, dict(offsets=i64(0, 3, 2)), "offsets must be non-decreasing (row 1)")
for E in ("mhx_sha1_tokens_dev", "mhx_sha1_tokens"):
    case(E, dict(n_tokens=-1), "n_tokens must be >= 0")
    case(E, dict(out_dtype=7), "bad out_dtype 7")  # unified: was "out_dtype must be MHX_U32 or MHX_U64"
    empty(E, dict(n_tokens=0))
each("mhx_sha1_tokens_dev", ("d_byte_offsets", "d_out"), DEVP)
E = "mhx_sha1_tokens"
case(E, dict(out=None), "out is NULL")
case(E, dict(byte_offsets=None), "byte_offsets is NULL")
case(E, dict(byte_offsets=i64(1, 2, 4)), "byte_offsets[0] must be 0")
case(E, dict(byte_offsets=i64(0, 3, 2)), "byte_offsets must be non-decreasing (token 1)")
case(E, dict(bytes=None), "bytes is NULL")
E = "mhx_minhash_bulk_bytes_typed"
case(E, dict(hash_dtype=7), "hash_dtype must be MHX_U32 (sha1_hash32) or MHX_U64 (sha1_hash64)")
case(E, dict(n_sets=-1), "n_sets and n_tokens must be >= 0")
case(E, dict(n_tokens=-1), "n_sets and n_tokens must be >= 0")
empty(E, dict(n_sets=0))
each(E, ("out", "set_offsets"), "out/set_offsets is NULL")
case(E, dict(set_offsets=i64(1, 1, 2)), "set_offsets must run from 0 to n_tokens")
case(E, dict(set_offsets=i64(0, 1, 3)), "set_offsets must run from 0 to n_tokens")
case(E, dict(set_offsets=i64(0, 3, 2)), "set_offsets must be non-decreasing (set 1)")
case(E, dict(byte_offsets=None), "byte_offsets is NULL")
case(E, dict(byte_offsets=i64(0, 3, 2)), "byte_offsets must be non-decreasing (token 1)")
case(E, dict(bytes=None), "bytes is NULL")
E = "mhx_minhash_bulk_bytes"
empty(E, dict(n_sets=0))
case(E, dict(n_tokens=-1), "n_sets and n_tokens must be >= 0")
case(E, dict(set_offsets=None), "out/set_offsets is NULL")
E = "mhx_minhash_update_batch"
case(E, dict(n=-1), "n must be >= 0")
empty(E, dict(n=0))
each(E, ("hv", "hashvalues"), "hv/hashvalues is NULL")
for E, names, msg in (("mhx_minhash_merge_dev", ("d_x", "d_y", "d_out"), DEVP), ("mhx_minhash_merge", ("x", "y", "out"), HOSTP)):
    case(E, dict(count=-1), "count must be >= 0")
    empty(E, dict(count=0))
    each(E, names, msg)

# ---- b-bit packing, bands, Lean records
E = "mhx_bbit_num_blocks"
case(E, dict(num_blocks=None), "num_blocks is NULL")
for b in (-1, 33):
    case(E, dict(b=b), B_RANGE, num_blocks=UNTOUCHED)
for k in (0, -1):
    case(E, dict(num_perm=k), "num_perm must be positive", num_blocks=UNTOUCHED)
for b, blocks in ((0, 1), (1, 1), (3, 1), (8, 1), (9, 2), (32, 4)):
    case(E, dict(b=b), None, num_blocks=blocks)
for E, names, msg in (("mhx_bbit_pack_dev", ("d_sig", "d_out"), DEVP), ("mhx_bbit_pack_dev_typed", ("d_sig", "d_out"), DEVP),
                      ("mhx_bbit_pack", ("sig", "out"), HOSTP), ("mhx_bbit_unpack_dev", ("d_blocks", "d_out"), DEVP),
                      ("mhx_bbit_unpack", ("blocks", "out"), HOSTP)):
    for b in (-1, 33):
        case(E, dict(b=b), B_RANGE)  # unified: mhx_bbit_unpack and mhx_bbit_unpack_dev said "b must be in [0, 32]"
    case(E, dict(k=0), "bad shape")  # unified: mhx_bbit_pack said "num_perm must be positive"
    case(E, dict(n=-1), "bad shape")
    empty(E, dict(n=0))
    each(E, names, msg)
sig_dtype("mhx_bbit_pack_dev_typed")
for E, names, msg in (("mhx_band_keys_dev", ("d_sig", "d_out"), DEVP), ("mhx_band_keys", ("sig", "out"), HOSTP),
                      ("mhx_band_digests_dev", ("d_sig", "d_out"), DEVP), ("mhx_band_digests_dev_typed", ("d_sig", "d_out"), DEVP),
                      ("mhx_band_digests_layout_dev", ("d_sig", "d_out"), DEVP), ("mhx_band_digests", ("sig", "out"), HOSTP),
                      ("mhx_lsh_sort_bands_dev", ("d_sig", "d_sorted_digests", "d_sorted_rows"), DEVP),
                      ("mhx_lsh_sort_bands_dev_typed", ("d_sig", "d_sorted_digests", "d_sorted_rows"), DEVP),
                      ("mhx_lsh_sort_bands", ("sig", "sorted_digests", "sorted_rows"), HOSTP)):
    geometry(E)
    case(E, dict(n=-1), "bad shape")
    empty(E, dict(n=0))
    each(E, names, msg)
    if "sig_dtype" in VALID[E]:
        sig_dtype(E)
    if "layout" in VALID[E]:
        for code in (2, -1):
            case(E, dict(layout=code), f"bad layout {code}")
        case(E, dict(layout=1, n=0, d_sig=None, d_out=None), None)
E = "mhx_bbit_pack_band_digests_dev"
sig_dtype(E, fused=0)
for b in (0, -1, 33):
    case(E, dict(b=b), "b must be in [1, 32]", fused=0)
geometry(E, fused=0)
case(E, dict(n=-1), "bad shape", fused=0)
for code in (2, -1):
    case(E, dict(digest_layout=code), f"bad layout {code}", fused=0)
empty(E, dict(n=0), fused=0)
each(E, ("d_sig", "d_blocks", "d_digests"), DEVP, fused=0)
case(E, dict(fused=None, n=-1), "bad shape")
for E in ("mhx_lsh_sort_digests_dev", "mhx_lsh_sort_digests_layout_dev"):
    case(E, dict(n=-1), "bad shape")
    case(E, dict(bands=0), "bad shape")
    empty(E, dict(n=0))
    each(E, ("d_digests", "d_sorted_digests", "d_sorted_rows"), DEVP)
for code in (2, -1):
    case("mhx_lsh_sort_digests_layout_dev", dict(layout=code), f"bad layout {code}")
for E, names, msg in (("mhx_lean_serialize_dev", ("d_sig", "d_out"), DEVP), ("mhx_lean_serialize_dev_typed", ("d_sig", "d_out"), DEVP),
                      ("mhx_lean_serialize", ("sig", "out"), HOSTP), ("mhx_lean_deserialize_dev", ("d_records", "d_sig"), DEVP),
                      ("mhx_lean_deserialize", ("records", "sig"), HOSTP)):
    case(E, dict(k=0), "bad shape")
    case(E, dict(n=-1), "bad shape")
    empty(E, dict(n=0))
    each(E, names, msg)
    if "sig_dtype" in VALID[E]:
        sig_dtype(E)  # unified: was "unknown sig_dtype %d"
    if "byteorder" in VALID[E]:
        for code in (2, -1):
            case(E, dict(byteorder=code), f"unknown byte order {code}")
        case(E, dict(byteorder=1, n=0), None)
case("mhx_lean_deserialize_dev", dict(d_records=DEV1), "records must be 4-byte aligned")

# ---- candidate pairs, bulk query, Jaccard of listed pairs
E = "mhx_lsh_candidate_pairs_dev"
case(E, dict(n_pairs=None), "n_pairs is NULL", n_raw=UNTOUCHED)
for changes in (dict(bands=0), dict(n=-1), dict(capacity=-1)):
    case(E, changes, "bad shape", n_pairs=UNTOUCHED, n_raw=UNTOUCHED)
case(E, dict(n=BIG), ROWS_32, n_pairs=UNTOUCHED, n_raw=UNTOUCHED)  # unified: was "more than 2^32-1 signatures per call"
empty(E, dict(n=0), n_pairs=0, n_raw=0)
case(E, dict(n=0, n_raw=None), None, n_pairs=0)
each(E, ("d_sorted_digests", "d_sorted_rows", "d_pairs"), DEVP, n_pairs=0, n_raw=0)
E = "mhx_lsh_candidate_pairs"
case(E, dict(n_pairs=None), "n_pairs is NULL", n_raw=UNTOUCHED)
geometry(E, n_pairs=UNTOUCHED, n_raw=UNTOUCHED)
for changes in (dict(n=-1), dict(capacity=-1)):
    case(E, changes, "bad shape", n_pairs=UNTOUCHED, n_raw=UNTOUCHED)
empty(E, dict(n=0), n_pairs=0, n_raw=0)
each(E, ("sig", "pairs"), HOSTP, n_pairs=0, n_raw=0)
E = "mhx_lsh_query_dev"
case(E, dict(n_pairs=None), "n_pairs is NULL")
sig_dtype(E, n_pairs=UNTOUCHED)
geometry(E, n_pairs=UNTOUCHED)
for changes in (dict(n=-1), dict(m=-1), dict(capacity=-1)):
    case(E, changes, "bad shape", n_pairs=UNTOUCHED)
for changes in (dict(n=BIG), dict(m=BIG)):
    case(E, changes, ROWS_32, n_pairs=UNTOUCHED)
empty(E, dict(n=0), n_pairs=0)
empty(E, dict(m=0), n_pairs=0)
each(E, ("d_sorted_digests", "d_sorted_rows", "d_query_sig", "d_pairs"), DEVP, n_pairs=0)
E = "mhx_lsh_ensemble_query_dev"
case(E, dict(n_pairs=None), "n_pairs is NULL")
sig_dtype(E, n_pairs=UNTOUCHED)
for changes in (dict(row_words=0), dict(row_words=-16), dict(n_queries=-1), dict(capacity=-1), dict(n_parts=-1)):
    case(E, changes, "bad shape", n_pairs=UNTOUCHED)
for v in (0, 17):
    case(E, dict(n_levels=v), "n_levels must be in [1, 16]", n_pairs=UNTOUCHED)
for v in (0, 65):
    case(E, dict(n_params=v), "n_params must be in [1, 64]", n_pairs=UNTOUCHED)
each(E, ("levels", "start", "params"), HOSTP, n_pairs=UNTOUCHED)
case(E, dict(start=i64(1, 1, 8, 308), n_parts=3), "start[0] must be 0", n_pairs=UNTOUCHED)
case(E, dict(start=i64(0, 9, 8, 308), n_parts=3), "start must ascend", n_pairs=UNTOUCHED)
for changes in (dict(start=i64(0, BIG)), dict(n_queries=BIG)):
    case(E, changes, ROWS_32, n_pairs=UNTOUCHED)
for level in ((DEV, DEV, 3, 6), (DEV, DEV, 0, 5), (DEV, DEV, 4, 0), (DEV, DEV, -4, -1)):  # more words than a row holds; no words; no bands
    case(E, dict(levels=[level]), GEOMETRY, n_pairs=UNTOUCHED)
for b in (3, 17, -1):
    case(E, dict(params=i32(0, b)), f"params row 0: b = {b} is not in [0, 2], the bands of its level", n_pairs=UNTOUCHED)
case(E, dict(levels=[(DEV, DEV, 1, 8), (DEV, DEV, 2, 4), (DEV, DEV, 3, 2)], n_levels=3, params=i32(0, 4, 2, 6), n_params=2),
     "params row 1: b = 6 is not in [0, 2], the bands of its level", n_pairs=UNTOUCHED)
for level in (3, 1, -1):
    case(E, dict(params=i32(level, 1)), f"params row 0 names level {level} of 1", n_pairs=UNTOUCHED)
case(E, dict(n_queries=0, d_query_sig=None, d_choice=None, d_index_sig=None, d_pairs=None, levels=[(None, None, 4, 2)]), None, n_pairs=0)
case(E, dict(start=i64(0, 0), d_query_sig=None, d_choice=None, d_index_sig=None, d_pairs=None, levels=[(None, None, 4, 2)]), None, n_pairs=0)
case(E, dict(n_parts=0, d_query_sig=None, d_choice=None, d_index_sig=None, d_pairs=None), None, n_pairs=0)
for level in ((None, DEV, 4, 2), (DEV, None, 4, 2)):
    case(E, dict(levels=[level]), DEVP, n_pairs=0)
each(E, ("d_index_sig", "d_query_sig", "d_choice", "d_pairs"), DEVP, n_pairs=0)
for E in ("mhx_jaccard_pairs_dev", "mhx_jaccard_pairs_dev_typed", "mhx_bbit_jaccard_pairs_dev"):
    case(E, dict(k=0), "bad shape")
    case(E, dict(n_pairs=-1), "bad shape")
    empty(E, dict(n_pairs=0))
    each(E, [n for n, v in VALID[E].items() if v is DEV], DEVP)
sig_dtype("mhx_jaccard_pairs_dev_typed")
for b in (-1, 33):
    case("mhx_bbit_jaccard_pairs_dev", dict(b=b), B_RANGE)
    case("mhx_bbit_jaccard_pairs", dict(b=b), B_RANGE)
for E, names in (("mhx_jaccard_pairs", ("sig", "pairs", "counts")), ("mhx_bbit_jaccard_pairs", ("blocks", "pairs", "counts"))):
    case(E, dict(k=0), "bad shape")  # unified: mhx_bbit_jaccard_pairs said "num_perm must be positive"
    case(E, dict(n=-1), "bad shape")
    case(E, dict(n_pairs=-1), "bad shape")
    empty(E, dict(n_pairs=0))
    each(E, names, HOSTP)
    case(E, dict(pairs=i64(0, 2)), "pair index 2 out of range [0,2)")
    case(E, dict(pairs=i64(-1, 1)), "pair index -1 out of range [0,2)")
    case(E, dict(n=0), "pair index 0 out of range [0,0)")

# ---- weighted MinHash
each("mhx_wgen_create", ("rs", "ln_cs", "betas", "out"), "NULL argument")
for changes in (dict(sample_size=0), dict(dim=0), dict(dim=-1)):
    case("mhx_wgen_create", changes, "sample_size and dim must be positive")
E = "mhx_weighted_minhash_many_dev"
case(E, dict(n_rows=-1), "bad shape")
case(E, dict(nnz=-1), "bad shape")
empty(E, dict(n_rows=0, nnz=0))
each(E, ("d_indptr", "d_indices", "d_values", "d_out", "d_nonempty"), DEVP)
E = "mhx_weighted_minhash_many"
case(E, dict(n_rows=-1), "bad shape")
empty(E, dict(n_rows=0))
each(E, ("indptr", "indices", "values", "out", "nonempty"), HOSTP)
case(E, dict(indptr=i64(0, 2, 1)), "indptr must be non-decreasing (row 1)")
case(E, dict(indptr=i64(1, 1, 2)), "indptr[0] must be 0")
case(E, dict(indices=i32(0, DIM)), f"column index {DIM} out of range [0,{DIM})")
case(E, dict(indices=i32(-1, 0)), f"column index -1 out of range [0,{DIM})")
for E, names, msg in (("mhx_weighted_logf", ("x", "out"), HOSTP), ("mhx_weighted_minhash_many_dense_dev", ("d_x", "d_out", "d_nonempty"), DEVP),
                      ("mhx_weighted_minhash_many_dense", ("x", "out", "nonempty"), HOSTP)):
    size = "n" if "n" in VALID[E] else "n_rows"
    case(E, {size: -1}, "bad shape")
    empty(E, {size: 0})
    each(E, names, msg)
case("mhx_weighted_dense_begin", dict(feed=None), "feed is NULL")
for v in (0, -1):
    case("mhx_weighted_dense_begin", dict(piece_rows=v), "piece_rows must be positive")
case("mhx_weighted_dense_feed", {}, "feed is NULL")
case("mhx_weighted_dense_end", {}, None)

# ---- all-pairs Jaccard
for E in ("mhx_jaccard_matrix_dev", "mhx_jaccard_matrix", "mhx_bbit_jaccard_matrix_dev", "mhx_bbit_jaccard_matrix",
          "mhx_jaccard_threshold_pairs_dev", "mhx_jaccard_threshold_pairs", "mhx_bbit_jaccard_threshold_pairs_dev",
          "mhx_bbit_jaccard_threshold_pairs"):
    dev, threshold = "_dev" in E, "threshold" in E
    zero = dict(n_pairs=0) if threshold else {}
    a, b = ("d_a", "d_b") if dev else ("a", "b_blocks" if "bbit" in E else "b")
    if threshold:
        case(E, dict(n_pairs=None), "n_pairs is NULL")
        case(E, dict(capacity=-1), "bad capacity", **zero)
        empty(E, dict(n_a=2, n_b=2, min_count=K + 1, capacity=0), **zero)  # more agreeing positions than there are: no pair
    if "sig_dtype" in VALID[E]:
        sig_dtype(E, **zero)
    if "bbit" in E:
        for v in (-1, 33):
            case(E, dict(b=v), B_RANGE, **zero)
    for k in (0, -1):
        case(E, dict(num_perm=k), "num_perm must be positive", **zero)
    for changes in (dict(n_a=-1), dict(n_b=-1)):
        case(E, changes, "bad shape", **zero)
    for changes in (dict(n_a=BIG), dict(n_b=BIG)):
        case(E, changes, ROWS_32, **zero)
    empty(E, dict(n_a=0), **zero)
    case(E, dict(n_b=0), None, **zero)
    empty(E, dict(n_a=0, n_b=0), **zero)
    case(E, {a: None}, DEVP if dev else HOSTP, **zero)
    if threshold:
        for name in (("d_pairs", "d_counts") if dev else ("pairs", "counts")):
            case(E, {name: None}, DEVP if dev else HOSTP, **zero)
        case(E, {"capacity": 0, ("d_pairs" if dev else "pairs"): None, ("d_counts" if dev else "counts"): None, "n_a": 0}, None, **zero)
    else:
        case(E, {("d_counts" if dev else "counts"): None}, DEVP if dev else HOSTP)
        if dev:
            case(E, dict(ldc=1), "ldc must be >= n_b")
            case(E, dict(d_b=None, n_b=0, ldc=1), "ldc must be >= n_b")  # B = A: n_b is n_a

# ---- live index
E = "mhx_lsh_bands_merge_dev"
for v in (0, -1):
    case(E, dict(bands=v), "bands must be positive")
for changes in (dict(n_a=-1), dict(n_b=-1)):
    case(E, changes, "bad shape")
for changes in (dict(n_a=BIG - 2), dict(n_b=BIG)):
    case(E, changes, "more than 2^32-1 entries per band")
empty(E, dict(n_a=0, n_b=0))
each(E, [n for n, v in VALID[E].items() if v is DEV], DEVP)
case(E, dict(n_a=0, d_dig_a=None, d_rows_a=None, d_dig_out=None), DEVP)
E = "mhx_lsh_bands_compact_dev"
case(E, dict(bands=0), "bands must be positive")
for changes in (dict(n=-1), dict(n_live=-1), dict(n_live=3)):
    case(E, changes, "bad shape")
case(E, dict(n=BIG), ROWS_32)
empty(E, dict(n=0, n_live=0))
each(E, [n for n, v in VALID[E].items() if v is DEV], DEVP)
E = "mhx_rows_compact_dev"
case(E, dict(n_kept=None), "n_kept is NULL")
for changes in (dict(row_bytes=0), dict(row_bytes=-8), dict(n_rows=-1)):
    case(E, changes, "bad shape", n_kept=0)
case(E, dict(n_rows=BIG), ROWS_32, n_kept=0)
case(E, dict(row_bytes=1 << 62), "row_bytes * n_rows overflows", n_kept=0)
empty(E, dict(n_rows=0), n_kept=0)
each(E, ("d_src", "d_live_bits", "d_dst"), DEVP, n_kept=0)
for E in ("mhx_lsh_forest_build_dev_typed", "mhx_lsh_forest_query_dev_typed"):
    sig_dtype(E)  # unified: was "sig_dtype must be MHX_U32 or MHX_U64"
    for v in (0, -1, 65536):
        case(E, dict(l=v), "l must be in [1, 65535]")
    for changes in (dict(tree_words=0), dict(row_words=0), dict(tree_words=5), dict(row_words=7)):
        case(E, changes, "l * tree_words must be in [1, row_words]")
    for v in (-1, BIG):
        case(E, dict(n=v), "n_sigs must be in [0, 2^32)")
empty("mhx_lsh_forest_build_dev_typed", dict(n=0))
each("mhx_lsh_forest_build_dev_typed", ("d_sig", "d_order"), DEVP)
E = "mhx_lsh_forest_query_dev_typed"
for changes in (dict(w=0), dict(w=3), dict(w=2, tree_words=3, row_words=6)):
    case(E, changes, "w must be 1 or 2 and divide tree_words")
for v in (0, -1):
    case(E, dict(k=v), "k must be positive")
for v in (-1, 1 << 31):
    case(E, dict(m=v), "m must be in [0, 2^31)")
empty(E, dict(m=0))
each(E, ("d_sig", "d_order", "d_probes", "d_slots", "d_counts"), DEVP)

# ---- a NULL handle, for every entry point that takes one
for E, args in VALID.items():
    first, value = next(iter(args.items()))
    if value is CTX or value is PERM or value is GEN:
        message = NULL_HANDLE.get(E, f"{first} is NULL")
        outs = {n: UNTOUCHED for n, v in args.items() if v is OUT64 or v is OUT32}
        outs.update(NULL_HANDLE_OUTS.get(E, {}))
        case(E, {first: None}, message, **(outs if message else {}))

# every key of mhx_ctx_set_option with the value a fresh context holds
OPTIONS = {
    "minhash.path": 0, "minhash.split": 0, "minhash.packed": 0, "minhash.ties": 0, "minhash.p3": 0, "minhash.share": 0, "minhash.adapt": 0,
    "blocks_per_cu": 0, "minhash.alias": -1, "minhash.prefetch": 1, "weighted.path": 0, "weighted.direct": 0, "weighted.split": 0,
    "weighted.tail": 0, "weighted.debug": 0, "weighted.kernel": 0, "weighted.plan": 0, "weighted.rescue": 0, "weighted.min_dim": 0,
    "host.chunk_bytes": 0, "lsh.sort_bits": 0, "lsh.gather": 0, "lsh.sort": 0, "lsh.levels": 0, "lsh.chunk": 0, "lsh.team": 0, "lsh.bigbins": 0,
    "pack.fused": 0, "weighted.refill": 0, "lsh.prehash": 0, "lsh.merge_items": 0, "hll.split_tokens": 0, "bloom.lanes": 0,
    "jaccard.topk_path": 0, "jaccard.topk_segments": 0,
    "overlap.bins": 0,
    "debug.cus": 0,  # tests only: 0 = the device's own CU count, 1 .. that count = what every launcher sizes its grid from
}


class Env:
    """The handles and buffers the sentinels of VALID stand for."""

    def __init__(self):
        assert _native.gpu_available(), "these tests need an MI355X"
        self.ctx = _native.context()
        self.lib = self.ctx.lib
        self.dev = self.ctx.to_device(np.zeros(8192, dtype=np.uint64))
        self.host = np.zeros(8192, dtype=np.uint64)
        rng = np.random.RandomState(3)
        self.perm = self.ctx.perm_handle((rng.randint(1, 2**31, K).astype(np.uint64), rng.randint(0, 2**31, K).astype(np.uint64)))
        self.gen = self.ctx.wgen_create(*(rng.uniform(0.5, 2.0, (SAMPLES, DIM)).astype(np.float32) for _ in range(3)))
        self.ctx.synchronize()

    def close(self):
        self.ctx.wgen_destroy(self.gen)
        self.dev.free()

    def call(self, entry, changes):
        """-> (status, message, {out-parameter: value after the call})"""
        args = dict(VALID[entry])
        unknown = set(changes) - set(args)
        assert not unknown, f"{entry} has no argument {unknown}"
        args.update(changes)
        outs, keep, argv = {}, [], []
        stand_for = {CTX: self.ctx.handle, PERM: self.perm, GEN: self.gen, DEV: self.dev.ptr, DEV1: self.dev.ptr + 1, HOST: self.host.ctypes.data}
        for (name, v), proto in zip(args.items(), _native._PROTOTYPES[entry]):
            if isinstance(v, np.ndarray):
                keep.append(v)
                v = v.ctypes.data
            elif isinstance(v, list):  # levels
                v = (_native.EnsembleLevel * len(v))(*[_native.EnsembleLevel(stand_for.get(d, d), stand_for.get(w, w), r, b) for d, w, r, b in v])
                keep.append(v)
                v = ctypes.addressof(v)
            elif isinstance(v, str) and v in (OUT64, OUT32):
                obj = outs[name] = (ctypes.c_int64 if v == OUT64 else ctypes.c_int32)(UNTOUCHED)
                v = ctypes.addressof(obj) if proto is ctypes.c_void_p else ctypes.byref(obj)
            elif isinstance(v, str):
                v = stand_for[v]
            if isinstance(v, int) and issubclass(proto, ctypes._Pointer):
                v = ctypes.cast(v, proto)  # (a buffer where the prototype names a typed pointer)
            argv.append(v)
        assert len(argv) == len(_native._PROTOTYPES[entry]), entry
        rc = getattr(self.lib, entry)(*argv)
        return rc, _native.last_error(), {name: v.value for name, v in outs.items()}


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def _id(c):
    entry, changes, message, _ = c
    what = ",".join(f"{k}={'NULL' if v is None else v.tolist() if isinstance(v, np.ndarray) else v}" for k, v in changes.items())
    return f"{entry[4:]}({what})"


def test_the_table_covers_every_bound_entry_point_that_checks_arguments():
    unchecked = {"mhx_last_error", "mhx_version",  # no arguments
                 "mhx_comm_unique_id", "mhx_comm_create", "mhx_comm_destroy", "mhx_comm_info", "mhx_comm_allgather_dev",
                 "mhx_comm_allgatherv_dev", "mhx_comm_exchange_dev"}  # comm.hip: RCCL, tested with its ranks
    assert set(VALID) == set(_native.EXPORTED_SYMBOLS) - unchecked
    assert {c[0] for c in CASES} == set(VALID)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_argument_check(env, c):
    entry, changes, message, outs = c
    rc, got, after = env.call(entry, changes)
    print(f"{_id(c)} -> {rc} {got!r} {after}")
    if message is None:
        assert rc == OK, got
    else:
        assert rc == INVALID
        assert message.fullmatch(got) if isinstance(message, re.Pattern) else got == message, got
    for name, value in outs.items():
        if changes.get(name, 0) is not None:
            assert after[name] == value, f"{name} holds {after[name]} after the call"


def test_every_option_key_is_known(env):
    for key, value in OPTIONS.items():
        assert env.lib.mhx_ctx_set_option(env.ctx.handle, key.encode(), value) == OK, key
    assert env.lib.mhx_ctx_set_option(env.ctx.handle, b"lsh.merge_items", 16) == OK
    assert env.lib.mhx_ctx_set_option(env.ctx.handle, b"lsh.merge_items", 8) == OK
    assert env.lib.mhx_ctx_set_option(env.ctx.handle, b"lsh.merge_items", 0) == OK


def test_debug_cus_takes_zero_to_the_device_count_and_device_info_keeps_the_hardware_count(env):
    """debug.cus: 0 and every value up to the device's CU count are accepted, -1 and the count + 1 are MHX_ERR_INVALID with a
    message that names the key (the option cannot be read back through the C ABI, so what a refused call leaves in it is not
    observable here: the calls after it only show that the context still computes); mhx_ctx_device_info reports the hardware whatever the option holds.
    On a context of its own, so that nothing here reaches the context the other modules share."""
    ctx = _native.Context(env.ctx.device)
    try:
        cus = ctx.info()["compute_units"]
        assert cus == env.ctx.info()["compute_units"] and cus >= 1
        for value in (1, 3 if cus >= 3 else 1, cus, 0):
            assert ctx.lib.mhx_ctx_set_option(ctx.handle, b"debug.cus", value) == OK, value
            assert ctx.info()["compute_units"] == cus, value
        assert ctx.lib.mhx_ctx_set_option(ctx.handle, b"debug.cus", 1) == OK
        for value in (-1, cus + 1, 1 << 40):
            assert ctx.lib.mhx_ctx_set_option(ctx.handle, b"debug.cus", value) == INVALID, value
            assert _native.last_error() == f"debug.cus must be 0 (the device's {cus} CUs) or in [1, {cus}], got {value}"
            assert ctx.info()["compute_units"] == cus
        # after the refused values the context still works, at whatever count it holds and at the device's own
        x = np.arange(70_000, dtype=np.uint64)
        y = x[::-1].copy()
        one = ctx.minhash_merge(x, y)
        assert ctx.lib.mhx_ctx_set_option(ctx.handle, b"debug.cus", 0) == OK
        assert np.array_equal(one, np.minimum(x, y)) and np.array_equal(ctx.minhash_merge(x, y), one)
    finally:
        ctx.close()
