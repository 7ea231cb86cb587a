"""Device entry points with their data past 2^31 / 2^32 elements or 4 GiB (run on an MI355X).

tests/index_width_cases.py describes every case: one large buffer filled by mhx_memset_dev, a few sets / rows / tokens planted
below, across and above a mark, decoys where a 32-bit wrap of the planted indices would land, the call's arguments and the
expected result from the host definitions.  Here the buffers are allocated, the calls made and the named slices downloaded
(never more than 64 MB at a time).  A mismatch that equals a decoy's answer is reported as such: "equals the decoy at index mod
2^32" is a kernel or launcher that formed that index in 32 bits.  Wrong-width reads land inside the same allocation, on the
decoy or the fill, and the wrapped locations of outputs are downloaded too, so a bug shows as a mismatch, not as a fault.

An allocation that fails is a test failure that names the byte count, not a skip: the card has 288 GB and no case holds more
than 64 GiB at a time (tests/test_index_width_host.py).

Every test is named "at_scale": tests/test_guard_pages.py runs the suite once more under mhx_debug_guard_alloc without the tests
of that name, and these belong with them -- that allocator never hands an address range out twice, and this module alone would
reserve more than 600 GB of them.
"""
import numpy as np
import pytest

from datasketch_amd import _native
from datasketch_amd._native import MHX_U32, MHX_U64, check
from oracle import oracle as O
from tests import index_width_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _native.Context(0)
    yield c
    c.close()


def _code(dtype) -> int:
    return MHX_U32 if np.dtype(dtype) == np.uint32 else MHX_U64


def _alloc(ctx, name: str, nbytes: int):
    try:
        return ctx.alloc(max(int(nbytes), 1))
    except (MemoryError, _native.MhxError) as e:
        pytest.fail(f"allocating {name}: {int(nbytes)} bytes failed: {e}", pytrace=False)


def _memset(ctx, buf, byte: int, offset: int = 0, nbytes=None) -> None:
    check(ctx.lib.mhx_memset_dev(ctx.handle, buf.ptr + offset, int(byte), buf.nbytes - offset if nbytes is None else int(nbytes)))


def _fill(ctx, buf, big: C.Big) -> None:
    """The whole buffer set to the model's fill: a byte by mhx_memset_dev, an element no byte fill writes by doubling copies."""
    if big.fill_value is None:
        _memset(ctx, buf, big.fill)
        return
    done = min(big.n, 1 << 22)
    buf.upload(np.full(done, big.fill_elem, dtype=big.dtype))
    z = big.dtype.itemsize
    while done < big.n:
        step = min(done, big.n - done)
        ctx.copy_dev(buf.ptr + done * z, buf.ptr, step * z)
        done += step


def _plant(ctx, buf, big: C.Big, erase: bool = False) -> None:
    z = big.dtype.itemsize
    for start, data in big.plants:
        if erase:
            _memset(ctx, buf, big.fill, start * z, data.nbytes)
        else:
            buf.upload(data, offset=start * z)


# ---- one launcher per entry: (ctx, device pointers by name, case, call) ------------------------------------------------------------
def _minhash(ctx, ptr, bufs, case, call):
    a = call.args
    big = case.bigs["hv"]
    n = case.arrays["offsets"].size - 1
    init = a["init"]
    if init is not None:
        bufs["init"].upload(init)
    ctx.minhash_mode(reset=True)  # every run starts like the first call of a fresh context
    ctx.minhash_bulk_dev(O.np_init_permutations(a["num_perm"], a["seed"]), ptr["hv"], _code(big.dtype), ptr["offsets"], 0, n, big.n,
                         ptr["init"] if init is not None else None, a["num_perm"] if init is not None else 0, ptr["out"], _code(a["out_dtype"]))


def _hll_bulk(ctx, ptr, bufs, case, call):
    big = case.bigs["hv"]
    n = case.arrays["offsets"].size - 1
    _memset(ctx, bufs["overflow"], 0xEE)
    check(ctx.lib.mhx_hll_bulk_dev(ctx.handle, ptr["hv"], _code(big.dtype), ptr["offsets"], 0, n, big.n, call.args["p"], call.args["hash_bits"], None, 0,
                                   ptr["out"], ptr["overflow"]))
    ctx.synchronize()
    assert int(bufs["overflow"].download((1,), np.int64)[0]) == 0


def _sha1_tokens(ctx, ptr, bufs, case, call):
    check(ctx.lib.mhx_sha1_tokens_dev(ctx.handle, ptr["bytes"], ptr["offsets"], case.arrays["offsets"].size - 1, _code(call.args["out_dtype"]), ptr["out"]))


def _overlap(ctx, ptr, bufs, case, call):
    ctx.overlap_pairs_dev(ptr["hv"], _code(case.bigs["hv"].dtype), ptr["offsets"], case.arrays["offsets"].size - 1, call.args["max_set_items"], ptr["pairs"],
                          case.arrays["pairs"].shape[0], ptr["counts"], ptr["invalid"])


def _jaccard_pairs(ctx, ptr, bufs, case, call):
    pairs = call.args["pairs"]
    bufs["pairs"].upload(pairs)
    if "b" in call.args:
        check(ctx.lib.mhx_bbit_jaccard_pairs_dev(ctx.handle, ptr["sig"], ptr["sig"], call.args["num_perm"], call.args["b"], ptr["pairs"], pairs.shape[0],
                                                 ptr["counts"]))
    else:
        ctx.jaccard_pairs_dev(ptr["sig"], ptr["sig"], _code(case.bigs["sig"].dtype), call.args["num_perm"], ptr["pairs"], pairs.shape[0], ptr["counts"])


def _rows_compact(ctx, ptr, bufs, case, call):
    kept = ctx.rows_compact_dev(ptr["src"], call.args["row_bytes"], call.args["n_rows"], ptr["live"], ptr["dst"])
    assert kept == call.args["n_kept"], f"n_kept {kept}, want {call.args['n_kept']}"


def _cc(ctx, ptr, bufs, case, call):
    n = call.args["n"]
    ctx.cc_init_dev(ptr["labels"], n)
    ctx.cc_link_pairs_dev(ptr["labels"], n, ptr["pairs"], case.arrays["pairs"].shape[0], None, 0, ptr["invalid"])
    ctx.cc_finish_dev(ptr["labels"], n)
    ctx.synchronize()
    assert int(bufs["invalid"].download((1,), np.int64)[0]) == 0


def _hll_merge(ctx, ptr, bufs, case, call):
    check(ctx.lib.mhx_hll_merge_dev(ctx.handle, ptr["a"], ptr["b"], call.args["count"]))


def _stream(ctx, ptr, bufs, case, call):
    a = call.args
    fn, n, k, lib, h = a["fn"], a["n"], a["k"], ctx.lib, ctx.handle
    if fn == "mhx_bbit_pack_dev_typed":
        check(lib.mhx_bbit_pack_dev_typed(h, ptr["sig"], MHX_U32, n, k, a["b"], ptr["blocks"]))
    elif fn == "mhx_bbit_unpack_dev":  # on the blocks the call before it wrote
        check(lib.mhx_bbit_unpack_dev(h, ptr["blocks"], n, k, a["b"], ptr["unpacked"]))
    elif fn == "mhx_band_digests_dev_typed":
        check(lib.mhx_band_digests_dev_typed(h, ptr["sig"], MHX_U32, n, k, a["bands"], a["r"], ptr["digests"]))
    elif fn == "mhx_band_digests_layout_dev":
        check(lib.mhx_band_digests_layout_dev(h, ptr["sig"], MHX_U32, n, k, a["bands"], a["r"], a["layout"], ptr["digests"]))
    elif fn == "mhx_bbit_pack_band_digests_dev":
        assert ctx.bbit_pack_band_digests_dev(ptr["sig"], MHX_U32, n, k, a["b"], a["bands"], a["r"], ptr["blocks"], ptr["digests"], a["layout"]), "not the fused kernel"
    elif fn == "mhx_lean_serialize_dev_typed":
        check(lib.mhx_lean_serialize_dev_typed(h, ptr["sig"], MHX_U32, n, k, a["seed"], a["byteorder"], ptr["records"]))
    elif fn == "mhx_lean_deserialize_dev":  # on the records the call before it wrote
        bad = _alloc(ctx, "bad", 4)
        try:
            _memset(ctx, bad, 0)
            check(lib.mhx_lean_deserialize_dev(h, ptr["records"], n, k, a["byteorder"], MHX_U32, ptr["sig2"], ptr["seeds"], bad.ptr))
            ctx.synchronize()
            assert int(bad.download((1,), np.uint32)[0]) == 0
        finally:
            bad.free()
    else:
        raise KeyError(fn)


def _topk(ctx, ptr, bufs, case, call):
    a = call.args
    ctx.jaccard_topk_dev(ptr["probes"], case.arrays["probes"].shape[0], ptr["b"], a["n_b"], MHX_U32, a["k"], None, a["min_count"], a["topk"], ptr["rows"],
                         ptr["counts"])


def _matrix(ctx, ptr, bufs, case, call):
    n = call.args["n"]
    ctx.jaccard_matrix_dev(ptr["a"], n, ptr["b"], n, MHX_U32, call.args["k"], ptr["counts"], n)


def _threshold(ctx, ptr, bufs, case, call):
    a = call.args
    found = ctx.jaccard_threshold_pairs_dev(ptr["a"], a["n"], ptr["b"], a["n"], MHX_U32, a["k"], a["min_count"], ptr["pairs"], ptr["pair_counts"], a["capacity"])
    assert found == a["n_pairs"], f"n_pairs {found}, want {a['n_pairs']}"


def _hll_rows(ctx, ptr, bufs, case, call):
    a = call.args
    if a["fn"] == "mhx_hll_histogram_dev":
        check(ctx.lib.mhx_hll_histogram_dev(ctx.handle, ptr["reg"], a["n"], a["p"], ptr["hist"], ptr["invalid"]))
        ctx.synchronize()
        assert int(bufs["invalid"].download((1,), np.int64)[0]) == 0
    else:
        check(ctx.lib.mhx_hll_union_groups_dev(ctx.handle, ptr["reg"], a["n"], a["p"], ptr["group_offsets"], a["n_groups"], ptr["union"]))


def _bloom(ctx, ptr, bufs, case, call):
    a = call.args
    geometry = (a["k"], a["bands"], a["r"], a["kbits"], a["n_blocks"])
    if a["fn"] == "mhx_bloom_insert_dev":  # the first 64 rows into the zeroed filter
        check(ctx.lib.mhx_bloom_insert_dev(ctx.handle, ptr["sig"], MHX_U32, 64, *geometry, ptr["filter"]))
    elif a["fn"] == "mhx_bloom_query_dev":  # all 128 rows; the filter stays as it is
        check(ctx.lib.mhx_bloom_query_dev(ctx.handle, ptr["sig"], MHX_U32, 128, *geometry, ptr["filter"], ptr["hit"], 0))
    else:  # the zeroed second filter |= the first
        check(ctx.lib.mhx_bloom_union_dev(ctx.handle, ptr["filter2"], ptr["filter"], a["bands"], a["n_blocks"]))


def _sha1_windows(ctx, ptr, bufs, case, call):
    a = call.args
    bufs["set_offsets"].upload(a["set_offsets"])
    ctx.sha1_windows_dev(ptr["bytes"], ptr["item_offsets"] if a["token_mode"] else None, ptr["doc_offsets"], ptr["set_offsets"],
                         case.arrays["doc_offsets"].size - 1, a["n_windows"], a["width"], _code(a["out_dtype"]), ptr["out"])


def _words(ctx, ptr, bufs, case, call):
    a = call.args
    rc, n_words, n_out = ctx.words_normalize_dev(ptr["bytes"], a["n_bytes"], ptr["doc_offsets"], a["n_docs"], a["table"], ptr["out_bytes"], a["n_out_bytes"],
                                                 ptr["item_offsets"], a["n_words"], ptr["word_doc_offsets"])
    assert (rc, n_words, n_out) == (0, a["n_words"], a["n_out_bytes"]), f"status {rc}, {n_words} words, {n_out} bytes; want 0, {a['n_words']}, {a['n_out_bytes']}"


def _weighted(ctx, ptr, bufs, case, call):
    a = call.args
    gen = ctx.wgen_create(*O.np_weighted_params(a["dim"], a["sample_size"], C.WEIGHTED_SEED))
    try:
        if "nnz" in a:
            check(ctx.lib.mhx_weighted_minhash_many_dev(gen, ptr["indptr"], ptr["indices"], ptr["values"], int(a["values_are_logs"]), a["n_rows"], a["nnz"],
                                                        ptr["out"], ptr["nonempty"]))
        else:
            check(ctx.lib.mhx_weighted_minhash_many_dense_dev(gen, ptr["x"], int(a["values_are_logs"]), a["n_rows"], ptr["out"], ptr["nonempty"]))
        ctx.synchronize()
    finally:
        ctx.wgen_destroy(gen)


LAUNCH = {
    "mhx_minhash_bulk_dev": _minhash, "mhx_hll_bulk_dev": _hll_bulk, "mhx_sha1_tokens_dev": _sha1_tokens, "mhx_sha1_windows_dev": _sha1_windows,
    "mhx_overlap_pairs_dev": _overlap, "mhx_jaccard_pairs_dev_typed": _jaccard_pairs, "mhx_bbit_jaccard_pairs_dev": _jaccard_pairs,
    "mhx_rows_compact_dev": _rows_compact, "mhx_cc": _cc, "mhx_hll_merge_dev": _hll_merge, "mhx_hll_rows": _hll_rows, "stream": _stream,
    "mhx_jaccard_topk_dev": _topk, "mhx_jaccard_matrix_dev": _matrix, "mhx_jaccard_threshold_pairs_dev": _threshold, "mhx_bloom": _bloom,
    "mhx_words_normalize_dev": _words, "mhx_weighted_minhash_many_dev": _weighted, "mhx_weighted_minhash_many_dense_dev": _weighted,
}


def run_case(ctx, case: C.Case) -> None:
    bufs = {}
    try:
        for name, big in case.bigs.items():
            bufs[name] = _alloc(ctx, f"{case.id} {name}", big.nbytes)
            _fill(ctx, bufs[name], big)
            _plant(ctx, bufs[name], big)
        for name, arr in case.arrays.items():
            bufs[name] = _alloc(ctx, f"{case.id} {name}", arr.nbytes)
            bufs[name].upload(arr)
        for name, nbytes in case.outputs.items():
            bufs[name] = _alloc(ctx, f"{case.id} {name}", nbytes)
        ptr = {name: b.ptr for name, b in bufs.items()}
        failures = []
        for call in case.calls:
            for name, big in call.bigs.items():
                _plant(ctx, bufs[name], big)
            for name, byte in call.refill.items():
                _memset(ctx, bufs[name], byte)
            LAUNCH[case.entry](ctx, ptr, bufs, case, call)
            ctx.synchronize()
            for chk in call.checks:
                got = bufs[chk.buffer].download(chk.expected.shape, chk.expected.dtype, offset=chk.offset)
                msg = C.describe_mismatch(got, chk)
                if msg:
                    failures.append(f"{case.id} [{call.what}] {msg}")
            for name, big in call.bigs.items():
                _plant(ctx, bufs[name], big, erase=True)
        assert not failures, "\n".join(failures)
    finally:
        ctx.synchronize()
        for b in bufs.values():
            b.free()
        ctx.release_scratch()


def _ids(entry):
    return C.CASE_IDS[entry]


@pytest.mark.parametrize("case_id", _ids("mhx_minhash_bulk_dev"))
def test_at_scale_minhash_bulk_dev_with_offsets_past_the_mark(ctx, case_id):
    """Token types x marks x two shapes -- 12 long sets, which today's launcher splits over waves, and 16 x 256 + 37 tiny ones, which
    it gives a wave or less each -- and inside, num_perm 64 / 128 / 256 into uint32 and uint64 rows, once with d_init.  Only results
    are asserted: which launch a shape takes is the launcher's business."""
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_hll_bulk_dev"))
def test_at_scale_hll_bulk_dev_with_offsets_past_the_mark(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_sha1_tokens_dev"))
def test_at_scale_sha1_tokens_dev_with_byte_offsets_around_4_GiB(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_overlap_pairs_dev"))
def test_at_scale_overlap_pairs_dev_with_sets_at_every_mark(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_jaccard_pairs_dev_typed") + _ids("mhx_bbit_jaccard_pairs_dev"))
def test_at_scale_listed_pairs_of_rows_on_both_sides_of_every_mark(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_rows_compact_dev"))
def test_at_scale_rows_compact_dev_past_4_GiB_of_rows(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_cc"))
def test_at_scale_connected_components_over_the_largest_label_array(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_hll_merge_dev"))
def test_at_scale_hll_merge_dev_past_4_GiB(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("stream"))
def test_at_scale_streaming_over_a_signature_matrix_of_2_to_the_32_elements(ctx, case_id):
    """uint32 [2^24 + 3, 256]: inputs pass element 2^32 (17 GB), the b-bit blocks and band digests pass byte 2^32, the lean records
    byte 2^34; the inverses read what the call before them wrote."""
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_jaccard_topk_dev"))
def test_at_scale_jaccard_topk_dev_against_2_to_the_32_elements(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_jaccard_matrix_dev") + _ids("mhx_jaccard_threshold_pairs_dev"))
def test_at_scale_all_pairs_of_65537_rows_whose_pair_index_passes_2_to_the_32(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_hll_rows"))
def test_at_scale_hll_rows_of_2_to_the_16_registers_past_4_GiB(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_bloom"))
def test_at_scale_bloom_filter_whose_word_index_passes_2_to_the_32(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_sha1_windows_dev"))
def test_at_scale_sha1_windows_dev_of_documents_around_4_GiB(ctx, case_id):
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_words_normalize_dev"))
def test_at_scale_words_normalize_dev_over_4_GiB_of_text_and_spaces(ctx, case_id):
    """The device form only.  mhx_minhash_bulk_words_typed and mhx_hll_bulk_words take the corpus from the host: 4 GiB to build
    there and to stage per call; how long that takes was not measured, and they are not run at this size."""
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_weighted_minhash_many_dev"))
def test_at_scale_weighted_minhash_many_dev_with_indptr_past_the_mark(ctx, case_id):
    """CSR rows on both sides of the walk / entry-by-entry crossover, below and above element 2^31 / 2^32; logs in and values in;
    every row against the C oracle, bit for bit (the rows hold finite positive values: the first rule of
    tests/test_gpu_weighted_small_dims.py::_assert_oracle, and zeros for the empty rows)."""
    run_case(ctx, C.case(case_id))


@pytest.mark.parametrize("case_id", _ids("mhx_weighted_minhash_many_dense_dev"))
def test_at_scale_weighted_minhash_many_dense_dev_past_2_to_the_32_floats(ctx, case_id):
    run_case(ctx, C.case(case_id))
