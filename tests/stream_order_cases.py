"""Every `_dev` entry point of include/mhx.h behind in-flight work on its stream (test infrastructure, run as a script in a
process of its own by tests/test_gpu_stream_order.py; tests/test_stream_order_ledger.py fails when the header declares a `_dev`
entry point that this script does not call).

include/mhx.h promises that a `_dev` entry enqueues on the context's stream and returns without synchronising, that it keeps no
host pointer after it returns, and that the work of calls made one after the other on one context takes effect in call order.
The other tests upload (blocking), call once, download (blocking): a launch on the wrong stream, a copy on the null stream or an
upload that does not wait for the compute stream still finds its inputs ready there.  Here every entry runs as a PLUGGED case:

    dry pass      the entry, synchronised, on its true inputs and on decoys of the same shape (another random draw, valid
                  throughout: the same offsets where the header calls them TRUSTED, indices in range): want_true (checked
                  against the oracle / host path of the entry's guard case) != want_decoy.  Scratch, handles and lazy
                  allocations grow here; the plugged pass allocates and frees nothing.
    plugged pass  I = decoys, O = 0xA5, R = 0x5A; synchronise; t0; then, with no synchronise in between:
                  ev0 | the plug | ev1 | I <- true (d2d) | THE ENTRY | R <- O (d2d) | O <- 0x3C, I <- decoys | t1
                  (host arrays of the call are overwritten the moment it returns); synchronise; R must be want_true bit for bit.
                  Read early: want_decoy.  Written late: 0xA5.  Read after the trailing overwrite: want_decoy.
    armed         a case counts only if the plug (r launches of mhx_minhash_bulk_dev on a resident corpus) was still running
                  when the last call was enqueued: t1 - t0 < ev0.elapsed_ms(ev1) (ev0 sits on a drained stream, so the plug
                  cannot end before t0 + that).  Unarmed: once more with the plug doubled; unarmed twice fails.
    no blocking   an entry the header calls enqueued returned before t0 + plug.  BLOCKING lists the entries that read a total
                  back by design, each with the hipStreamSynchronize that does it; they are armed at entry instead.

Beside the per-entry cases: a `_dev` call in flight followed by the pipelined host calls (mhx_minhash_bulk_typed in pieces,
mhx_weighted_dense_feed: the copy streams start while the compute stream is busy), a counters reset followed at once by a
MinHash call, four chains of the Python classes behind the plug, and the POSITIVE CONTROL: three entries on a second context,
whose stream nothing orders against the first, while the plug and the I <- true copies sit on the first -- they must see the
decoys, exactly.  The decoys are valid inputs: the control computes a wrong answer by design, never a fault.

    python tests/stream_order_cases.py     prints the calibration, "STREAM ORDER CONTROL OK 3 entries, <k> rearmed" and
                                           "STREAM ORDER OK <n> cases, <m> rearmed"; exits 0

Measured on an MI355X (profiles/stream_order.txt): one plug launch 0.37 ms on the device and 0.015 ms to enqueue; the largest
enqueue time of a case 0.36 ms (the ensemble query, which blocks three times); r = 29 launches, a plug of 9 to 10 ms (the floor of
10 ms decides, not the factor ten); 54 cases, none rearmed; 1.1 s from the first allocation to the last line.
"""
import ctypes
import hashlib
import math
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, b_bit_minhash, lsh_bulk  # noqa: E402
from datasketch_amd import hyperloglog as H  # noqa: E402
from datasketch_amd import lsh_bloom as B  # noqa: E402
from datasketch_amd import lshforest as F  # noqa: E402
from datasketch_amd import overlap, shingle  # noqa: E402
from datasketch_amd._native import BAND_MAJOR, MHX_U32, MHX_U64, ROW_MAJOR, check  # noqa: E402
from datasketch_amd.lsh import _HostBands  # noqa: E402
from datasketch_amd.lshensemble import _HostEnsemble  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.guard_cases import _p  # noqa: E402
from tests.jaccard_topk_guard_cases import planted  # noqa: E402
from tests.poison_cases import _clustered, _offsets_to_pairs  # noqa: E402
from tests.test_gpu_lshforest import _corpus  # noqa: E402
from tests.test_gpu_minhash_lsh import _sorted_run  # noqa: E402
from tests.test_lshforest_host import lexsort_order  # noqa: E402
from tests.weighted_dispatch import MI355X_LDS_PER_BLOCK  # noqa: E402

_i64 = ctypes.c_int64
_i32 = ctypes.c_int32

# Entries that block by design: each reads a total or a flag back before it can go on, through the hipStreamSynchronize named.
BLOCKING = {
    "mhx_lsh_sort_bands_dev_typed": "the two-pass bucketing reads its overflow flags back between the passes: hipStreamSynchronize at "
                                    "lsh_kernels.hip:606 (with option lsh.sort = 1, the radix sort, the call only enqueues: tested as such)",
    "mhx_lsh_sort_digests_layout_dev": "the same bucketing from digests: hipStreamSynchronize at lsh_kernels.hip:606 (lsh.sort = 1 only enqueues)",
    "mhx_lsh_candidate_pairs_dev": "the raw and the unique pair counts come back: read_back_u64 (hipStreamSynchronize at device_scan.h:135) from "
                                   "lsh_query_kernels.hip:322 and :288",
    "mhx_lsh_query_dev": "the number of candidates comes back before they are emitted: read_back_u64 (hipStreamSynchronize at device_scan.h:135) "
                         "from lsh_query_kernels.hip:360, and the unique count from :288",
    "mhx_lsh_ensemble_query_dev": "table and bounds are host memory of the call, on the device before anything else is enqueued: hipStreamSynchronize at "
                                  "lsh_query_kernels.hip:428; then the totals come back (read_back_u64 from :437 and :456)",
    "mhx_jaccard_threshold_pairs_dev": "*n_pairs comes back before the sort is sized: hipStreamSynchronize at jaccard_kernels.hip:219",
    "mhx_bbit_jaccard_threshold_pairs_dev": "the same launcher on packed rows: hipStreamSynchronize at jaccard_kernels.hip:219",
    "mhx_lsh_bands_compact_dev": "the live totals come back to be checked against n_live: read_back_u64 (hipStreamSynchronize at device_scan.h:135) "
                                 "from lsh_index_kernels.hip:235 and :245",
    "mhx_rows_compact_dev": "*n_kept comes back: read_back_u64 (hipStreamSynchronize at device_scan.h:135) from lsh_index_kernels.hip:276",
    "mhx_words_normalize_dev": "*n_words and *n_out_bytes come back before the emit: hipStreamSynchronize at words_kernels.hip:259",
}

CASES = 0
REARMED = 0
FAILED = []
# What a case that merely fails raises; the script goes on to the next case and exits 1 at the end.  A RuntimeError (MhxError: a
# HIP call failed) is not among them: after a fault nothing more is started.
FAILS = (AssertionError, ValueError, TypeError, KeyError, IndexError, AttributeError)
VERBOSE = bool(os.environ.get("STREAM_ORDER_VERBOSE"))


def _as(got, dtype, shape=None):
    out = np.ascontiguousarray(got).view(dtype)
    return out if shape is None else out.reshape(shape)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape == want.shape and np.array_equal(got, want):
        return
    if got.shape != want.shape:
        raise AssertionError(f"{what}: shape {got.shape} != {want.shape}")
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    raise AssertionError(f"{what}: {bad.size} of {want.size} elements differ, first at {bad[:4].tolist()}: got "
                         f"{got.reshape(-1)[bad[:4]].tolist()} want {want.reshape(-1)[bad[:4]].tolist()}")


class Case:
    """One entry point on one shape.  ins / inouts: key -> (true array, decoy array); outs: key -> bytes; host(p): the host
    arrays of the call, fresh (key -> numpy array or ctypes object), overwritten when the call has returned; call(ctx, p, h):
    the call, p = key -> device address, returns the host results (a tuple) or None; verify(got, res): want_true against the
    oracle, got = key -> uint8 array of every out and inout; confirm(ctx): after the synchronised call on the true inputs,
    that every internal launch had work (flags, counters).  enqueues: overrides BLOCKING (the radix path of the sorts).
    constant: the entry reads no device memory (its result is a function of its scalar arguments), so there is no decoy."""

    def __init__(self, symbol, name, call, ins=None, inouts=None, outs=None, host=None, verify=None, options=None, confirm=None,
                 enqueues=None, prepare=None, constant=False):
        self.symbol, self.name, self.call = symbol, name, call
        self.ins, self.inouts, self.outs = dict(ins or {}), dict(inouts or {}), dict(outs or {})
        for key, (t, d) in list(self.ins.items()) + list(self.inouts.items()):
            t, d = np.ascontiguousarray(t), np.ascontiguousarray(d)
            assert t.shape == d.shape and t.dtype == d.dtype and t.nbytes > 0, (name, key, t.shape, d.shape)
            (self.ins if key in self.ins else self.inouts)[key] = (t, d)
        self.host, self.verify, self.options, self.confirm = host, verify, dict(options or {}), confirm
        self.blocking = symbol in BLOCKING if enqueues is None else not enqueues
        self.prepare, self.constant = prepare, constant  # prepare(ctx): blocking setup, before the stream is drained
        self.bufs = None

    # -- buffers: allocated once in the dry pass, freed after the final synchronise
    def allocate(self, ctx):
        b = {"I": {}, "S": {}, "D": {}, "O": {}, "R": {}}
        for key, (t, d) in list(self.ins.items()) + list(self.inouts.items()):
            b["I"][key], b["S"][key], b["D"][key] = ctx.alloc(t.nbytes), ctx.to_device(t), ctx.to_device(d)
        for key, nbytes in self.outs.items():
            b["O"][key], b["R"][key] = ctx.alloc(nbytes), ctx.alloc(nbytes)
        for key, (t, _) in self.inouts.items():
            b["R"][key] = ctx.alloc(t.nbytes)
        self.bufs = b

    def results(self):
        """(key, the buffer the entry leaves it in, bytes) of every out and inout."""
        b = self.bufs
        return [(k, b["O"][k], n) for k, n in self.outs.items()] + [(k, b["I"][k], t.nbytes) for k, (t, _) in self.inouts.items()]

    def pointers(self):
        b = self.bufs
        p = {k: buf.ptr for k, buf in b["I"].items()}
        p.update({k: buf.ptr for k, buf in b["O"].items()})
        return p

    def set_options(self, ctx, on):
        for key, v in self.options.items():
            ctx.set_option(key, v if on else 0)

    def load(self, ctx, which):
        """I <- true / decoys, O <- 0xA5, R <- 0x5A (enqueued)."""
        b = self.bufs
        for key, buf in b["I"].items():
            ctx.copy_dev(buf.ptr, b[which][key].ptr, buf.nbytes)
        for buf in b["O"].values():
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(buf), 0xA5, buf.nbytes))
        for buf in b["R"].values():
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(buf), 0x5A, buf.nbytes))

    def sync_run(self, ctx, which):
        """The ordinary synchronised way: (key -> uint8 array of every out and inout, host results)."""
        self.load(ctx, which)
        self.set_options(ctx, True)
        if self.prepare:
            self.prepare(ctx)
        ctx.synchronize()
        h = self.host(self.pointers()) if self.host else {}
        res = self.call(ctx, self.pointers(), h)
        ctx.synchronize()
        self.set_options(ctx, False)
        return {k: buf.download((n,), np.uint8) for k, buf, n in self.results()}, res

    def free(self):
        for group in (self.bufs or {}).values():
            for buf in group.values():
                buf.free()
        self.bufs = None


def _garble(h):
    """Host memory of a call, overwritten the moment the call has returned.  With zeros: an entry that kept the pointer would read
    an empty table, all separators, NULL levels -- a wrong answer, never a wild index."""
    for obj in h.values():
        if isinstance(obj, np.ndarray):
            obj.fill(0)
        else:
            ctypes.memset(ctypes.addressof(obj), 0, ctypes.sizeof(obj))


def _differ(a, b):
    (ga, ra), (gb, rb) = a, b
    return ra != rb or any(not np.array_equal(ga[k], gb[k]) for k in ga)


class Plug:
    """r launches of mhx_minhash_bulk_dev (enqueue-only) on a resident corpus into one output: 128 MiB of uint32 tokens in,
    128 MiB of uint32 signatures out."""

    def __init__(self, ctx, n=1 << 18, t=128, k=128):
        rng = np.random.RandomState(99)
        self.ctx, self.n, self.t = ctx, n, t
        self.perm = ctx.perm_handle(O.np_init_permutations(k, 11))
        self.d_hv = ctx.to_device(rng.randint(0, 2**32, size=(n, t), dtype=np.uint64).astype(np.uint32))
        self.d_out = ctx.alloc(n * k * 4)
        self.ev0, self.ev1 = ctx.event(), ctx.event()

    def enqueue(self, r):
        lib = self.ctx.lib
        for _ in range(r):
            check(lib.mhx_minhash_bulk_dev(self.perm, self.d_hv.ptr, MHX_U32, None, self.t, self.n, self.n * self.t, None, 0, self.d_out.ptr, MHX_U32))

    def begin(self, r):
        """Drain the stream, take t0, enqueue ev0 | plug | ev1: t0."""
        self.ctx.synchronize()
        t0 = time.perf_counter()
        self.ev0.record()
        self.enqueue(r)
        self.ev1.record()
        return t0

    def lasted_ms(self):
        return self.ev0.elapsed_ms(self.ev1)


def _steps_behind(ctx, case):
    """I <- true | the entry | R <- O | O <- 0x3C, I <- decoys, enqueued: (host results, time before the call, after it, at the end)."""
    b = case.bufs
    for key, buf in b["I"].items():
        ctx.copy_dev(buf.ptr, b["S"][key].ptr, buf.nbytes)
    p = case.pointers()
    h = case.host(p) if case.host else {}
    before = time.perf_counter()
    res = case.call(ctx, p, h)
    after = time.perf_counter()
    _garble(h)
    for key, buf, nbytes in case.results():
        ctx.copy_dev(b["R"][key].ptr, buf.ptr, nbytes)
    for buf in b["O"].values():  # the write-after-read and write-after-write hazards behind the call
        check(ctx.lib.mhx_memset_dev(ctx.handle, _p(buf), 0x3C, buf.nbytes))
    for key, buf in b["I"].items():  # (an inout takes the decoys again, not the byte: a launch that read late must find valid rows)
        ctx.copy_dev(buf.ptr, b["D"][key].ptr, buf.nbytes)
    return res, before, after, time.perf_counter()


def plugged(ctx, case, plug, r):
    """One plugged pass: (armed, returned in time, key -> uint8 array of R, host results, milliseconds the plug lasted)."""
    case.load(ctx, "D")
    case.set_options(ctx, True)
    if case.prepare:
        case.prepare(ctx)
    t0 = plug.begin(r)
    res, before, after, t1 = _steps_behind(ctx, case)
    ctx.synchronize()
    case.set_options(ctx, False)
    ms = plug.lasted_ms()
    armed = ((before if case.blocking else t1) - t0) * 1e3 < ms
    in_time = case.blocking or (after - t0) * 1e3 < ms
    got = {k: case.bufs["R"][k].download((n,), np.uint8) for k, _, n in case.results()}
    case.host_ms = (t1 - t0) * 1e3  # from the drained stream to the last enqueue, the plug's own launches included
    return armed, in_time, got, res, ms


def _report(name, err):
    FAILED.append(name)
    print("FAILED", name, "--", type(err).__name__, err, flush=True)


def dry(ctx, case):
    """want_true (checked against the oracle) and want_decoy; they differ."""
    case.allocate(ctx)
    case.want_decoy = case.sync_run(ctx, "D")
    case.want_true = case.sync_run(ctx, "S")
    if case.confirm:
        case.confirm(ctx)
    if case.verify:
        case.verify(*case.want_true)
    assert case.constant or _differ(case.want_true, case.want_decoy), "want_true == want_decoy: the case proves nothing"
    again = case.sync_run(ctx, "S")  # (and the entry is a function of its inputs: the bit-for-bit comparison below means something)
    assert not _differ(case.want_true, again), "two synchronised runs on the same inputs differ"


def unplugged_ms(ctx, case):
    """Host time of enqueueing a case's steps on a drained stream."""
    case.load(ctx, "D")
    case.set_options(ctx, True)
    ctx.synchronize()
    t0 = time.perf_counter()
    _, _, _, t1 = _steps_behind(ctx, case)
    ctx.synchronize()
    case.set_options(ctx, False)
    return (t1 - t0) * 1e3


def run_plugged(ctx, case, plug, r):
    global CASES, REARMED
    for attempt, reps in enumerate((r, 2 * r)):
        armed, in_time, got, res, ms = plugged(ctx, case, plug, reps)
        if VERBOSE:
            print(f"  {case.name}: plug x{reps} lasted {ms:.2f} ms, everything enqueued after {case.host_ms:.2f} ms, armed {armed}, returned in time {in_time}", flush=True)
        if armed:
            break
        if attempt == 0:
            REARMED += 1
    else:
        raise AssertionError(f"unarmed twice: the plug ({2 * r} launches, {ms:.2f} ms) had ended when the last call was enqueued")
    want, want_res = case.want_true
    decoy, _ = case.want_decoy
    for key in want:
        if not np.array_equal(got[key], want[key]):
            kind = ("want_decoy: read early, or after the trailing overwrite" if np.array_equal(got[key], decoy[key]) else
                    "0xA5: written late" if (got[key] == 0xA5).all() else "0x3C: copied late" if (got[key] == 0x3C).all() else
                    "0x5A: never copied" if (got[key] == 0x5A).all() else "a mixture")
            bad = np.flatnonzero(got[key] != want[key])
            raise AssertionError(f"'{key}' differs from want_true in {bad.size} of {want[key].size} bytes, first at {bad[:4].tolist()}: it is {kind}")
    assert res == want_res, f"host results {res} != {want_res} of the dry pass"
    assert in_time, (f"{case.symbol} is enqueue-only by include/mhx.h but returned after the plug had ended "
                     f"({ms:.2f} ms): it blocks")
    CASES += 1


# ---------------------------------------------------------------------------------------------------------------- the cases
def _two(make):
    """(true, decoy) of one generator called with two seeds' RandomState."""
    return make(np.random.RandomState(1)), make(np.random.RandomState(2))


def minhash_cases():
    cases = []
    n, t, k = 97, 77, 128
    perms = O.np_init_permutations(k, 2)
    offsets = (np.arange(n + 1) * t).astype(np.int64)
    odd = [pi for pi in range(k) if int(perms[0][pi]) & 1][:8]

    def close_keys(pi):
        """Three different tokens whose keys under permutation pi are the three smallest of a set and within 32 of each other
        (the recipe of tests/test_gpu_round2.py: the tie-tolerant proof has one candidate too many, the dedup pass drops none)."""
        a_lo, b8 = int(perms[0][pi]) & 0xFFFFFFFF, (int(perms[1][pi]) + 8) & 0xFFFFFFFF
        inv = pow(a_lo, -1, 1 << 32)
        return [((m - b8) * inv) % 2**32 for m in (1000, 1007, 1021)]

    def corpus(rng):
        hv = rng.randint(0, 2**32, size=(n, t), dtype=np.uint64)
        hv[1::3, 5] = hv[1::3, 60]  # one repeated token: the second launch
        hv[2::6, 7] = hv[2::6, 8]
        hv[2::6, 9] = hv[2::6, 8]
        hv[::5] = hv[::5, :1]  # constant sets: the dedup pass leaves one token
        for j, row in enumerate(range(3, n, 7)):  # one candidate too many and nothing to drop: hashed pair by pair by the third
            hv[row, 20:23] = close_keys(odd[j % len(odd)])
        return hv.reshape(-1), rng.randint(0, 2**32, size=(n, k), dtype=np.uint64)
    (hv_t, init_t), (hv_d, init_d) = _two(corpus)

    def call(ctx, p, h):
        ctx.minhash_bulk_dev(perms, p["hv"], MHX_U64, p["off"], 0, n, n * t, p["init"], k, p["out"], MHX_U64)

    def confirm(ctx):
        flags = ctx.minhash_flags(n)
        print(f"  minhash flags of the true corpus: {np.bincount(flags, minlength=3).tolist()} sets with flag 0 / 1 / 2", flush=True)
        assert set(flags.tolist()) == {0, 1, 2}, "the sieve, second and pairwise launches did not all have sets"

    def verify(got, res):
        _same(_as(got["out"], np.uint64, (n, k)), O.c_minhash_bulk(hv_t, offsets, perms[0], perms[1], init=init_t), "minhash bulk")

    cases.append(Case("mhx_minhash_bulk_dev", "minhash bulk csr 97x77 K=128, flags 0 1 2", call, ins={"hv": (hv_t, hv_d), "off": (offsets, offsets), "init": (init_t, init_d)},
                      outs={"out": n * k * 8}, verify=verify, confirm=confirm, prepare=lambda ctx: ctx.minhash_mode(reset=True)))

    # sha1 of byte tokens
    rng = np.random.RandomState(6)
    lens = rng.randint(0, 131, size=333)
    lens[-1] = 77
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    buf_t, buf_d = (r.randint(0, 256, size=int(off[-1]), dtype=np.uint8) for r in (np.random.RandomState(1), np.random.RandomState(2)))

    def sha1_call(ctx, p, h):
        check(ctx.lib.mhx_sha1_tokens_dev(ctx.handle, p["bytes"], p["off"], 333, MHX_U32, p["out"]))

    def sha1_verify(got, res):
        raw = buf_t.tobytes()
        want = np.array([struct.unpack("<I", hashlib.sha1(raw[off[i]:off[i + 1]]).digest()[:4])[0] for i in range(333)], dtype=np.uint32)
        _same(_as(got["out"], np.uint32), want, "sha1 tokens")
    cases.append(Case("mhx_sha1_tokens_dev", "sha1 tokens n=333 len<=130", sha1_call, ins={"bytes": (buf_t, buf_d), "off": (off, off)}, outs={"out": 333 * 4},
                      verify=sha1_verify))

    count = 128 * 33 + 1
    (x_t, y_t), (x_d, y_d) = _two(lambda r: (r.randint(0, 2**32, size=count, dtype=np.uint64), r.randint(0, 2**32, size=count, dtype=np.uint64)))

    def merge_call(ctx, p, h):
        check(ctx.lib.mhx_minhash_merge_dev(ctx.handle, p["x"], p["y"], count, p["out"]))
    cases.append(Case("mhx_minhash_merge_dev", f"merge {count}", merge_call, ins={"x": (x_t, x_d), "y": (y_t, y_d)}, outs={"out": 8 * count},
                      verify=lambda got, res: _same(_as(got["out"], np.uint64), np.minimum(x_t, y_t), "merge")))
    return cases


def weighted_cases(ctx):
    import scipy.sparse as sp

    cases = []
    dim, s, n = 301, 65, 40
    rs_, ln_cs, betas = O.np_weighted_params(dim, s, 4)
    gens = {}  # one generator per context (the control runs nothing of these; a second context would get its own)

    def gen(c):
        if c not in gens:
            gens[c] = c.wgen_create(rs_, ln_cs, betas)
        return gens[c]
    rng = np.random.RandomState(7)
    mask = rng.random_sample((n, dim)) < rng.choice([0.3, 0.5, 0.95], size=(n, 1))
    mask[n // 2] = True  # an empty row

    def rows(r):
        x = r.uniform(0.5, 50, (n, dim)).astype(np.float32)
        x[mask] = 0
        return x
    x_t, x_d = _two(rows)
    csr = sp.csr_matrix(x_t)
    csr.sort_indices()
    csr_d = sp.csr_matrix(x_d)
    csr_d.sort_indices()
    indptr, indices = csr.indptr.astype(np.int64), csr.indices.astype(np.int32)
    assert np.array_equal(indptr, csr_d.indptr) and np.array_equal(indices, csr_d.indices)
    with np.errstate(divide="ignore"):
        want, wn = O.c_weighted_minhash_many(indptr, indices, csr.data, rs_, ln_cs, betas)
        logs_t, logs_d = np.log(x_t), np.log(x_d)
    assert not wn.all() and wn.any()

    def verify(got, res):
        ne = _as(got["ne"], np.uint8).astype(bool)
        out = _as(got["out"], np.int64, (n, s, 2))
        _same(ne, wn, "weighted nonempty")
        _same(out[wn], want[wn], "weighted (k, t)")

    def csr_call(c, p, h):
        check(c.lib.mhx_weighted_minhash_many_dev(gen(c), p["indptr"], p["indices"], p["values"], 1, n, csr.nnz, p["out"], p["ne"]))
    cases.append(Case("mhx_weighted_minhash_many_dev", f"weighted csr dim={dim} S={s} n={n}", csr_call,
                      ins={"indptr": (indptr, indptr), "indices": (indices, indices), "values": (np.log(csr.data), np.log(csr_d.data))},
                      outs={"out": n * s * 16, "ne": n}, verify=verify))

    def dense_call(c, p, h):
        check(c.lib.mhx_weighted_minhash_many_dense_dev(gen(c), p["x"], 1, n, p["out"], p["ne"]))
    cases.append(Case("mhx_weighted_minhash_many_dense_dev", f"weighted dense dim={dim} S={s} n={n}", dense_call, ins={"x": (logs_t, logs_d)},
                      outs={"out": n * s * 16, "ne": n}, verify=verify))
    gen(ctx)
    return cases


def _dup_sig(rng, n, k, dtype=np.uint64):
    sig = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64)
    sig[n // 2:] = sig[: n - n // 2]  # duplicates: buckets with more than one row
    return sig.astype(dtype)


def pack_cases():
    cases = []
    n, k = 777, 128
    sig_t, sig_d = _two(lambda r: _dup_sig(r, n, k))
    s32_t, s32_d = sig_t.astype(np.uint32), sig_d.astype(np.uint32)

    b = 3
    blocks_t, blocks_d = O.c_bbit_pack(sig_t, b), O.c_bbit_pack(sig_d, b)

    def pack_call(ctx, p, h):
        check(ctx.lib.mhx_bbit_pack_dev_typed(ctx.handle, p["sig"], MHX_U32, n, k, b, p["out"]))
    cases.append(Case("mhx_bbit_pack_dev_typed", f"bbit pack n={n} K={k} b={b} uint32", pack_call, ins={"sig": (s32_t, s32_d)}, outs={"out": blocks_t.nbytes},
                      verify=lambda got, res: _same(_as(got["out"], np.uint64, blocks_t.shape), blocks_t, "bbit pack")))

    def unpack_call(ctx, p, h):
        check(ctx.lib.mhx_bbit_unpack_dev(ctx.handle, p["blocks"], n, k, b, p["out"]))
    cases.append(Case("mhx_bbit_unpack_dev", f"bbit unpack n={n} K={k} b={b}", unpack_call, ins={"blocks": (blocks_t, blocks_d)}, outs={"out": n * k * 4},
                      verify=lambda got, res: _same(_as(got["out"], np.uint32, (n, k)), (sig_t & np.uint64(7)).astype(np.uint32), "bbit unpack")))

    (pairs_t, pairs_d) = _two(lambda r: r.randint(0, n, size=(300, 2)).astype(np.int64))

    def bj_call(ctx, p, h):
        check(ctx.lib.mhx_bbit_jaccard_pairs_dev(ctx.handle, p["blocks"], p["blocks"], k, b, p["pairs"], 300, p["out"]))
    cases.append(Case("mhx_bbit_jaccard_pairs_dev", f"bbit jaccard pairs n={n} K={k} b={b}", bj_call, ins={"blocks": (blocks_t, blocks_d), "pairs": (pairs_t, pairs_d)},
                      outs={"out": 4 * 300},
                      verify=lambda got, res: _same(_as(got["out"], np.int32), ((sig_t[pairs_t[:, 0]] & np.uint64(7)) == (sig_t[pairs_t[:, 1]] & np.uint64(7))).sum(axis=1),
                                                    "bbit jaccard pairs")))

    def jp_call(ctx, p, h):
        check(ctx.lib.mhx_jaccard_pairs_dev_typed(ctx.handle, p["sig"], p["sig"], MHX_U32, k, p["pairs"], 300, p["out"]))
    cases.append(Case("mhx_jaccard_pairs_dev_typed", f"jaccard pairs n={n} K={k} uint32", jp_call, ins={"sig": (s32_t, s32_d), "pairs": (pairs_t, pairs_d)},
                      outs={"out": 4 * 300},
                      verify=lambda got, res: _same(_as(got["out"], np.int32), (sig_t[pairs_t[:, 0]] == sig_t[pairs_t[:, 1]]).sum(axis=1), "jaccard pairs")))

    bands, r = 16, 8
    keys = O.c_band_keys(sig_t, bands, r)

    def keys_call(ctx, p, h):
        check(ctx.lib.mhx_band_keys_dev(ctx.handle, p["sig"], n, k, bands, r, p["out"]))
    cases.append(Case("mhx_band_keys_dev", f"band keys n={n} K={k} {bands}x{r}", keys_call, ins={"sig": (sig_t, sig_d)}, outs={"out": keys.nbytes},
                      verify=lambda got, res: _same(_as(got["out"], np.uint64, keys.shape), keys, "band keys")))

    dig_t = lsh_bulk.band_digests(sig_t, bands, r, gpu_mode="disable")
    dig_d = lsh_bulk.band_digests(sig_d, bands, r, gpu_mode="disable")

    def dig_call(ctx, p, h):
        check(ctx.lib.mhx_band_digests_layout_dev(ctx.handle, p["sig"], MHX_U32, n, k, bands, r, BAND_MAJOR, p["out"]))
    cases.append(Case("mhx_band_digests_layout_dev", f"band digests n={n} K={k} {bands}x{r} uint32 band-major", dig_call, ins={"sig": (s32_t, s32_d)},
                      outs={"out": 8 * n * bands}, verify=lambda got, res: _same(_as(got["out"], np.uint64, (bands, n)), dig_t.T, "band digests")))

    # the fused pack: the shape that can fuse
    fn, fk, fb, fbands, fr = 128, 32, 4, 8, 4
    f_t, f_d = _two(lambda r_: _dup_sig(r_, fn, fk))
    f_blocks = b_bit_minhash.pack_matrix(f_t, fb, gpu_mode="disable")
    f_dig = lsh_bulk.band_digests(f_t, fbands, fr, gpu_mode="disable")

    def fused_call(ctx, p, h):
        ctx.bbit_pack_band_digests_dev(p["sig"], MHX_U32, fn, fk, fb, fbands, fr, p["blocks"], p["dig"], ROW_MAJOR)

    def fused_verify(got, res):
        _same(_as(got["blocks"], np.uint64, f_blocks.shape), f_blocks, "fused pack blocks")
        _same(_as(got["dig"], np.uint64, f_dig.shape), f_dig, "fused pack digests")
    cases.append(Case("mhx_bbit_pack_band_digests_dev", f"pack and digests n={fn} K={fk} b={fb} {fbands}x{fr}", fused_call,
                      ins={"sig": (f_t.astype(np.uint32), f_d.astype(np.uint32))}, outs={"blocks": f_blocks.nbytes, "dig": f_dig.nbytes}, verify=fused_verify))

    # sorts: the bucketing (blocks for its flags) and, with lsh.sort = 1, the radix path (enqueue-only)
    order = np.argsort(dig_t.T, axis=1, kind="stable")
    want_rows, want_sorted = order.astype(np.uint32), np.take_along_axis(dig_t.T, order, axis=1)

    def sort_verify(got, res):
        _same(_as(got["rows"], np.uint32, (bands, n)), want_rows, "sorted rows")
        _same(_as(got["dig"], np.uint64, (bands, n)), want_sorted, "sorted digests")

    def sort_call(ctx, p, h):
        ctx.lsh_sort_bands_dev(p["sig"], MHX_U32, n, k, bands, r, p["dig"], p["rows"])

    def sortd_call(layout):
        def call(ctx, p, h):
            check(ctx.lib.mhx_lsh_sort_digests_layout_dev(ctx.handle, p["in"], n, bands, layout, p["dig"], p["rows"]))
        return call
    outs = {"dig": 8 * n * bands, "rows": 4 * n * bands}
    for radix in (0, 1):
        opts, how = ({"lsh.sort": 1}, "radix") if radix else ({}, "bucketing")
        cases.append(Case("mhx_lsh_sort_bands_dev_typed", f"sort bands n={n} {bands}x{r} uint32, {how}", sort_call, ins={"sig": (s32_t, s32_d)}, outs=outs,
                          verify=sort_verify, options=opts, enqueues=True if radix else None))
        layout, src = (BAND_MAJOR, (np.ascontiguousarray(dig_t.T), np.ascontiguousarray(dig_d.T))) if radix else (ROW_MAJOR, (dig_t, dig_d))
        cases.append(Case("mhx_lsh_sort_digests_layout_dev", f"sort digests n={n} bands={bands} layout={layout}, {how}", sortd_call(layout), ins={"in": src},
                          outs=outs, verify=sort_verify, options=opts, enqueues=True if radix else None))

    # candidate pairs from sorted bands
    cb, cr = 8, 4
    c_t, c_d = _two(lambda r_: _dup_sig(r_, 500, 32, np.uint32))
    c_t[:40] = c_t[0]  # one bucket of 40 rows in every band
    sb_t, sb_d = (lsh_bulk.sorted_bands(x, cb, cr, gpu_mode="disable") for x in (c_t, c_d))
    want_pairs = lsh_bulk.candidate_pairs(c_t, cb, cr, gpu_mode="disable")
    cap = max(len(want_pairs), len(lsh_bulk.candidate_pairs(c_d, cb, cr, gpu_mode="disable")))
    assert len(want_pairs) > 500

    def cand_call(ctx, p, h):
        found, raw = _i64(-1), _i64(-1)
        check(ctx.lib.mhx_lsh_candidate_pairs_dev(ctx.handle, p["dig"], p["rows"], 500, cb, p["pairs"], cap, ctypes.byref(found), ctypes.byref(raw)))
        return found.value, raw.value

    def cand_verify(got, res):
        assert res[0] == len(want_pairs) and res[1] >= res[0], res
        _same(_as(got["pairs"], np.int64, (cap, 2))[: res[0]], want_pairs, "candidate pairs")
    cases.append(Case("mhx_lsh_candidate_pairs_dev", f"candidate pairs n=500 {cb}x{cr}: {len(want_pairs)} pairs emitted, sorted, unique", cand_call,
                      ins={"dig": (sb_t[0], sb_d[0]), "rows": (sb_t[1], sb_d[1])}, outs={"pairs": 16 * cap}, verify=cand_verify))

    # lean records
    seed = -77
    rec_t, rec_d = O.c_lean_serialize(sig_t, seed), O.c_lean_serialize(sig_d, seed - 1)

    def ser_call(ctx, p, h):
        check(ctx.lib.mhx_lean_serialize_dev_typed(ctx.handle, p["sig"], MHX_U32, n, k, seed, 0, p["out"]))
    cases.append(Case("mhx_lean_serialize_dev_typed", f"lean serialize n={n} K={k} uint32", ser_call, ins={"sig": (s32_t, s32_d)}, outs={"out": rec_t.nbytes},
                      verify=lambda got, res: _same(got["out"], rec_t.reshape(-1), "lean records")))

    def deser_call(ctx, p, h):
        check(ctx.lib.mhx_lean_deserialize_dev(ctx.handle, p["rec"], n, k, 0, MHX_U64, p["sig"], p["seeds"], p["bad"]))

    def deser_verify(got, res):
        _same(_as(got["sig"], np.uint64, (n, k)), sig_t, "lean deserialize")
        _same(_as(got["seeds"], np.int64), np.full(n, seed, dtype=np.int64), "lean seeds")
        _same(_as(got["bad"], np.uint32), np.zeros(1, dtype=np.uint32), "lean bad records")
    zero = np.zeros(1, dtype=np.uint32)
    cases.append(Case("mhx_lean_deserialize_dev", f"lean deserialize n={n} K={k}", deser_call, ins={"rec": (rec_t.reshape(-1), rec_d.reshape(-1))},
                      inouts={"bad": (zero, zero)}, outs={"sig": n * k * 8, "seeds": n * 8}, verify=deser_verify))
    return cases


def query_cases():
    cases = []
    k, bands, r, n, m = 32, 8, 4, 1000, 100

    def index(seed):
        sig, probes = _clustered(seed, n, m, k, 40)
        sig[100:140] = sig[100]
        dig, rows = lsh_bulk.sorted_bands(sig, bands, r, gpu_mode="disable")
        host = _HostBands(k, bands, r, np.uint32)
        host.append(sig)
        return sig, probes, dig, rows, _offsets_to_pairs(*host.query(probes))
    t, d = index(7), index(8)
    cap = max(len(t[4]), len(d[4]))
    assert len(t[4]) > m

    def call(ctx, p, h):
        found = _i64(-1)
        check(ctx.lib.mhx_lsh_query_dev(ctx.handle, p["dig"], p["rows"], n, bands, r, p["q"], p["sig"], MHX_U32, k, m, p["pairs"], cap, ctypes.byref(found)))
        return (found.value,)

    def verify(got, res):
        assert res[0] == len(t[4]), res
        _same(_as(got["pairs"], np.int64, (cap, 2))[: res[0]], t[4], "bulk query pairs")
    cases.append(Case("mhx_lsh_query_dev", f"bulk query n={n} m={m} {bands}x{r}", call,
                      ins={"sig": (t[0], d[0]), "q": (t[1], d[1]), "dig": (t[2], d[2]), "rows": (t[3], d[3])}, outs={"pairs": 16 * cap}, verify=verify))

    # the ensemble: six partitions (one empty, one of a single row), two levels; table and bounds are host memory of the call
    levels = [(2, 16), (4, 8)]
    sizes = [100, 0, 1, 40, 80, 79]
    start = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    en, n_parts = int(start[-1]), len(sizes)
    params = np.array([[0, 16], [0, 7], [1, 8], [1, 1], [1, 0]], dtype=np.int32)

    def ensemble(seed):
        sig, probes = _clustered(seed, en, 64, k, 12)
        ens = _HostEnsemble(k, np.uint32, levels, start)
        ens.build(sig)
        rng = np.random.RandomState(seed)
        choice = rng.randint(0, params.shape[0] + 1, size=(64, n_parts)).astype(np.uint8)
        choice[choice == params.shape[0]] = 255
        choice[0, 0], choice[-1, -1] = 255, 0
        bufs = ens.level_buffers()
        return sig, probes, choice, bufs, _offsets_to_pairs(*ens.query(probes, choice, params))
    et, ed = ensemble(61), ensemble(62)
    ecap = max(len(et[4]), len(ed[4]))
    parts_hit = np.unique(np.searchsorted(start, et[4][:, 1], side="right") - 1)
    assert len(et[4]) > 0 and parts_hit.size > 1, "the ensemble query's pairs come from one partition only"
    ins = {"sig": (et[0], ed[0]), "q": (et[1], ed[1]), "choice": (et[2], ed[2])}
    for i in range(len(levels)):
        ins[f"dig{i}"] = (et[3][i][0], ed[3][i][0])
        ins[f"rows{i}"] = (et[3][i][1], ed[3][i][1])

    def ens_host(p):
        return {"levels": (_native.EnsembleLevel * len(levels))(*[_native.EnsembleLevel(p[f"dig{i}"], p[f"rows{i}"], lr, lb) for i, (lr, lb) in enumerate(levels)]),
                "start": start.copy(), "params": params.copy()}

    def ens_call(ctx, p, h):
        found = _i64(-1)
        check(ctx.lib.mhx_lsh_ensemble_query_dev(ctx.handle, h["levels"], len(levels), h["start"].ctypes.data_as(ctypes.POINTER(_i64)), n_parts, p["sig"],
                                                 MHX_U32, k, p["q"], 64, p["choice"], h["params"].ctypes.data_as(ctypes.POINTER(_i32)), params.shape[0],
                                                 p["pairs"], ecap, ctypes.byref(found)))
        return (found.value,)

    def ens_verify(got, res):
        assert res[0] == len(et[4]), res
        _same(_as(got["pairs"], np.int64, (ecap, 2))[: res[0]], et[4], "ensemble query pairs")
    cases.append(Case("mhx_lsh_ensemble_query_dev", f"ensemble query n={en} m=64 over partitions {parts_hit.tolist()}", ens_call, ins=ins, outs={"pairs": 16 * ecap},
                      host=ens_host, verify=ens_verify))
    return cases


def matrix_cases():
    cases = []
    counts = lambda a, b: (a[:, None, :] == b[None, :, :]).sum(-1).astype(np.int32)  # noqa: E731
    n_a, n_b, k = 129, 130, 17
    (a_t, b_t), (a_d, b_d) = _two(lambda r: planted(r, n_a, n_b, k, np.uint32))
    want = counts(a_t, b_t)
    ldc = n_b + 3

    def m_call(ctx, p, h):
        ctx.jaccard_matrix_dev(p["a"], n_a, p["b"], n_b, MHX_U32, k, p["out"], ldc)
    cases.append(Case("mhx_jaccard_matrix_dev", f"matrix uint32 {n_a}x{n_b}x{k} ldc=n_b+3", m_call, ins={"a": (a_t, a_d), "b": (b_t, b_d)}, outs={"out": 4 * n_a * ldc},
                      verify=lambda got, res: _same(_as(got["out"], np.int32, (n_a, ldc))[:, :n_b], want, "jaccard matrix")))

    def threshold(symbol, name, caller, w_t, w_d, ins):
        levels = np.unique(w_t)
        min_count = int(levels[len(levels) // 2])
        ij = np.argwhere(w_t >= min_count)
        cap = max(len(ij), int((w_d >= min_count).sum()))
        assert 0 < len(ij) < w_t.size

        def call(ctx, p, h):
            return (caller(ctx, p, min_count, cap),)

        def verify(got, res):
            assert res[0] == len(ij), res
            _same(_as(got["pairs"], np.int64, (cap, 2))[: len(ij)], ij, name + " pairs")
            _same(_as(got["counts"], np.int32)[: len(ij)], w_t[ij[:, 0], ij[:, 1]], name + " counts")
        return Case(symbol, f"{name} min_count={min_count}: {len(ij)} pairs emitted and sorted", call, ins=ins, outs={"pairs": 16 * cap, "counts": 4 * cap}, verify=verify)
    cases.append(threshold("mhx_jaccard_threshold_pairs_dev", f"threshold uint32 {n_a}x{n_b}x{k}",
                           lambda ctx, p, mc, cap: ctx.jaccard_threshold_pairs_dev(p["a"], n_a, p["b"], n_b, MHX_U32, k, mc, p["pairs"], p["counts"], cap),
                           want, counts(a_d, b_d), {"a": (a_t, a_d), "b": (b_t, b_d)}))

    bits, bk = 3, 100
    (v_a, v_b), (w_a, w_b) = _two(lambda r: planted(r, n_a, n_b, bk, np.uint64))
    mask = np.uint64((1 << bits) - 1)
    pk = lambda x: b_bit_minhash.pack_matrix(x, bits, gpu_mode="disable")  # noqa: E731
    bins = {"a": (pk(v_a), pk(w_a)), "b": (pk(v_b), pk(w_b))}
    bwant, bwant_d = counts(v_a & mask, v_b & mask), counts(w_a & mask, w_b & mask)

    def bm_call(ctx, p, h):
        ctx.bbit_jaccard_matrix_dev(p["a"], n_a, p["b"], n_b, bk, bits, p["out"], n_b)
    cases.append(Case("mhx_bbit_jaccard_matrix_dev", f"bbit matrix b={bits} {n_a}x{n_b}x{bk}", bm_call, ins=bins, outs={"out": 4 * n_a * n_b},
                      verify=lambda got, res: _same(_as(got["out"], np.int32, (n_a, n_b)), bwant, "bbit matrix")))
    cases.append(threshold("mhx_bbit_jaccard_threshold_pairs_dev", f"bbit threshold b={bits} {n_a}x{n_b}x{bk}",
                           lambda ctx, p, mc, cap: ctx.bbit_jaccard_threshold_pairs_dev(p["a"], n_a, p["b"], n_b, bk, bits, mc, p["pairs"], p["counts"], cap),
                           bwant, bwant_d, bins))

    # top-k: B cut into three segments, so that the partial lists in scratch[4] are merged
    m, n, kp, topk = 129, 385, 128, 10
    (ta, tb), (da, db) = _two(lambda r: planted(r, m, n, kp, np.uint32))
    live_t, live_d = _two(lambda r: r.random_sample(n) < 0.8)

    def want_topk(a, b, live, min_count):
        rows, cnt = lsh_bulk._topk_from_blocks(lsh_bulk._equal_counts_blocks(a, b), a.shape[0], topk, min_count, False, live)
        return rows, cnt.astype(np.int32)

    def tk_call(ctx, p, h):
        check(ctx.lib.mhx_jaccard_topk_dev(ctx.handle, p["a"], m, p["b"], n, MHX_U32, kp, p["live"], kp // 3, topk, p["rows"], p["counts"]))

    def tk_verify(got, res):
        rows, cnt = want_topk(ta, tb, live_t, kp // 3)
        _same(_as(got["rows"], np.int64, (m, topk)), rows, "topk rows")
        _same(_as(got["counts"], np.int32, (m, topk)), cnt, "topk counts")
    touts = {"rows": 8 * m * topk, "counts": 4 * m * topk}
    cases.append(Case("mhx_jaccard_topk_dev", f"topk uint32 {m}x{n}x{kp} k={topk}, three segments", tk_call,
                      ins={"a": (ta, da), "b": (tb, db), "live": (lsh_bulk.live_bits(live_t), lsh_bulk.live_bits(live_d))}, outs=touts, verify=tk_verify,
                      options={"jaccard.topk_segments": 3}))

    (xa, xb), (ya, yb) = _two(lambda r: planted(r, m, n, kp, np.uint64))
    tbits = 4
    tmask = np.uint64((1 << tbits) - 1)
    pk4 = lambda x: b_bit_minhash.pack_matrix(x, tbits, gpu_mode="disable")  # noqa: E731

    def btk_call(ctx, p, h):
        check(ctx.lib.mhx_bbit_jaccard_topk_dev(ctx.handle, p["a"], m, p["b"], n, kp, tbits, None, 0, topk, p["rows"], p["counts"]))

    def btk_verify(got, res):
        rows, cnt = want_topk(xa & tmask, xb & tmask, None, 0)
        _same(_as(got["rows"], np.int64, (m, topk)), rows, "bbit topk rows")
        _same(_as(got["counts"], np.int32, (m, topk)), cnt, "bbit topk counts")
    cases.append(Case("mhx_bbit_jaccard_topk_dev", f"bbit topk b={tbits} {m}x{n}x{kp} k={topk}, two segments", btk_call, ins={"a": (pk4(xa), pk4(ya)), "b": (pk4(xb), pk4(yb))},
                      outs=touts, verify=btk_verify, options={"jaccard.topk_segments": 2}))
    return cases


def index_cases():
    cases = []
    n_a, n_b, bands = 2049, 2047, 3
    n = n_a + n_b

    def runs(r):
        return _sorted_run(r, n_a, bands, 7) + _sorted_run(r, n_b, bands, 7)
    t, d = _two(runs)

    def m_call(ctx, p, h):
        ctx.lsh_bands_merge_dev(p["da"], p["ra"], n_a, p["db"], p["rb"], n_b, n_a, bands, p["dig"], p["rows"])

    def m_verify(got, res):
        dig = np.concatenate([t[0], t[2]], axis=1)
        rows = np.concatenate([t[1], t[3] + np.uint32(n_a)], axis=1)
        order = np.stack([np.lexsort((rows[j], dig[j])) for j in range(bands)])
        _same(_as(got["dig"], np.uint64, (bands, n)), np.take_along_axis(dig, order, axis=1), "merge digests")
        _same(_as(got["rows"], np.uint32, (bands, n)), np.take_along_axis(rows, order, axis=1), "merge rows")
    cases.append(Case("mhx_lsh_bands_merge_dev", f"bands merge {n_a}+{n_b} rows, {bands} bands", m_call,
                      ins={"da": (t[0], d[0]), "ra": (t[1], d[1]), "db": (t[2], d[2]), "rb": (t[3], d[3])}, outs={"dig": 8 * bands * n, "rows": 4 * bands * n}, verify=m_verify))

    cn = 5001
    (dig_t, rows_t), (dig_d, rows_d) = _two(lambda r: _sorted_run(r, cn, bands, cn // 3))
    live_t = np.random.RandomState(3).rand(cn) >= 0.5
    live_d = live_t[np.random.RandomState(4).permutation(cn)]  # as many live slots: n_live is an argument of the call
    n_live = int(live_t.sum())

    def c_call(ctx, p, h):
        ctx.lsh_bands_compact_dev(p["dig"], p["rows"], cn, bands, p["bits"], n_live, p["odig"], p["orows"])

    def c_verify(got, res):
        remap = (np.cumsum(live_t) - 1).astype(np.uint32)
        keep = live_t[rows_t]
        _same(_as(got["odig"], np.uint64, (bands, n_live)), dig_t[keep].reshape(bands, n_live), "compact digests")
        _same(_as(got["orows"], np.uint32, (bands, n_live)), remap[rows_t[keep]].reshape(bands, n_live), "compact rows")
    cases.append(Case("mhx_lsh_bands_compact_dev", f"bands compact n={cn}, {n_live} live", c_call,
                      ins={"dig": (dig_t, dig_d), "rows": (rows_t, rows_d), "bits": (lsh_bulk.live_bits(live_t), lsh_bulk.live_bits(live_d))},
                      outs={"odig": 8 * bands * n_live, "orows": 4 * bands * n_live}, verify=c_verify))

    row_bytes = 24
    src_t, src_d = _two(lambda r: r.randint(0, 255, (cn, row_bytes // 8)).astype(np.uint64))

    def r_call(ctx, p, h):
        return (ctx.rows_compact_dev(p["src"], row_bytes, cn, p["bits"], p["dst"]),)

    def r_verify(got, res):
        assert res == (n_live,), res
        _same(_as(got["dst"], np.uint64, (n_live, row_bytes // 8)), src_t[live_t], "rows compact")
    cases.append(Case("mhx_rows_compact_dev", f"rows compact n={cn} row_bytes={row_bytes}", r_call,
                      ins={"src": (src_t, src_d), "bits": (lsh_bulk.live_bits(live_t), lsh_bulk.live_bits(live_d))}, outs={"dst": n_live * row_bytes}, verify=r_verify))
    return cases


def forest_cases():
    cases = []
    l, tree_words, w, n, m, k = 8, 16, 1, 257, 65, 10
    width = l * tree_words

    def forest(seed):
        rng = np.random.RandomState(seed)
        sig, bases = _corpus(rng, n, width, 0, np.uint32)
        probes, _ = _corpus(rng, m, width, 0, np.uint32, bases=bases)
        probes[2:23] = sig[rng.randint(n, size=21)]
        return sig, probes, lexsort_order(sig, l, tree_words)
    t, d = forest(1008), forest(1009)

    def b_call(ctx, p, h):
        ctx.lsh_forest_build_dev(p["sig"], MHX_U32, n, width, l, tree_words, p["order"])
    cases.append(Case("mhx_lsh_forest_build_dev_typed", f"forest build l={l} tree_words={tree_words} n={n}", b_call, ins={"sig": (t[0], d[0])}, outs={"order": 4 * l * n},
                      verify=lambda got, res: _same(_as(got["order"], np.uint32, (l, n)), t[2], "forest order")))

    def q_call(ctx, p, h):
        ctx.lsh_forest_query_dev(p["sig"], MHX_U32, n, width, l, tree_words, w, p["order"], p["q"], m, k, p["slots"], p["counts"])

    def q_verify(got, res):
        slots, cnt = F.host_query(t[0], t[2], t[1], l, tree_words // w, w, k)
        assert cnt.max() > 0
        past = np.arange(k)[None, :] >= cnt[:, None]
        _same(_as(got["counts"], np.int32), cnt, "forest counts")
        _same(_as(got["slots"], np.uint32, (m, k)), np.where(past, np.uint32(0xA5A5A5A5), slots), "forest slots")
    cases.append(Case("mhx_lsh_forest_query_dev_typed", f"forest query l={l} n={n} m={m} k={k}", q_call, ins={"sig": (t[0], d[0]), "order": (t[2], d[2]), "q": (t[1], d[1])},
                      outs={"slots": 4 * m * k, "counts": 4 * m}, verify=q_verify))
    return cases


def hll_cases():
    cases = []
    p_, bits = 8, 64
    m = 1 << p_
    lengths = [0, 1, 63, 64, 65, 257, 5000, 0, 3]  # 5000 > hll.split_tokens = 1000: that set is split over workgroups and combined by a max
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ns = len(lengths)

    def corpus(r):
        hv = r.randint(0, 2**32, size=int(offsets[-1]), dtype=np.uint64) >> r.randint(0, 32, size=int(offsets[-1])).astype(np.uint64)
        return hv, r.randint(0, 9, size=(ns, m)).astype(np.uint8)
    (hv_t, init_t), (hv_d, init_d) = _two(corpus)

    def call(ctx, p, h):
        check(ctx.lib.mhx_hll_bulk_dev(ctx.handle, p["hv"], MHX_U64, p["off"], 0, ns, hv_t.size, p_, bits, p["init"], m, p["out"], p["ovf"]))

    def verify(got, res):
        _same(_as(got["out"], np.uint8, (ns, m)), H._registers_host(hv_t, offsets, 0, ns, p_, bits, init_t), "hll registers")
        _same(_as(got["ovf"], np.int64), np.zeros(1, dtype=np.int64), "hll overflow count")
    cases.append(Case("mhx_hll_bulk_dev", f"hll bulk csr p={p_}, a set of 5000 tokens split at 1000", call, ins={"hv": (hv_t, hv_d), "off": (offsets, offsets), "init": (init_t, init_d)},
                      outs={"out": ns * m, "ovf": 8}, verify=verify, options={"hll.split_tokens": 1000}))

    n = 1001

    def regs(r):
        reg = r.randint(0, 64, size=(n, m)).astype(np.uint8)
        reg[-1, m - 1] = 200
        return reg
    reg_t, reg_d = _two(regs)

    def h_call(ctx, p, h):
        check(ctx.lib.mhx_hll_histogram_dev(ctx.handle, p["reg"], n, p_, p["hist"], p["bad"]))

    def h_verify(got, res):
        _same(_as(got["hist"], np.uint32, (n, 64)), np.stack([np.bincount(r[r < 64], minlength=64) for r in reg_t]), "hll histogram")
        _same(_as(got["bad"], np.int64), np.ones(1, dtype=np.int64), "hll histogram invalid count")
    cases.append(Case("mhx_hll_histogram_dev", f"hll histogram p={p_} n={n}", h_call, ins={"reg": (reg_t, reg_d)}, outs={"hist": n * 256, "bad": 8}, verify=h_verify))

    groups = np.array([0, 0, 1, n // 2, n], dtype=np.int64)

    def u_call(ctx, p, h):
        check(ctx.lib.mhx_hll_union_groups_dev(ctx.handle, p["reg"], n, p_, p["groups"], 4, p["out"]))
    cases.append(Case("mhx_hll_union_groups_dev", f"hll union p={p_} n={n}, four groups", u_call, ins={"reg": (reg_t, reg_d), "groups": (groups, groups)}, outs={"out": 4 * m},
                      verify=lambda got, res: _same(_as(got["out"], np.uint8, (4, m)), H.union_groups(reg_t, groups, gpu_mode="disable").view(np.uint8), "hll union")))

    count = 16 * 1000 + 5
    (a_t, b_t), (a_d, b_d) = _two(lambda r: (r.randint(0, 64, size=count).astype(np.uint8), r.randint(0, 64, size=count).astype(np.uint8)))

    def g_call(ctx, p, h):
        check(ctx.lib.mhx_hll_merge_dev(ctx.handle, p["a"], p["b"], count))
    cases.append(Case("mhx_hll_merge_dev", f"hll merge {count} bytes, in place", g_call, ins={"b": (b_t, b_d)}, inouts={"a": (a_t, a_d)},
                      verify=lambda got, res: _same(got["a"], np.maximum(a_t, b_t), "hll merge")))
    return cases


def bloom_cases():
    cases = []
    n, num_perm, b, r, k, nb = 1000, 128, 9, 13, 8, 1001

    def rows(rng):
        sig = rng.randint(0, 2**32, size=(n, num_perm), dtype=np.uint64).astype(np.uint32)
        old = rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x10001)
        B.insert_host(old, sig[: n // 3], r, k)  # a third of the rows are in the filter already
        return sig, old
    (sig_t, old_t), (sig_d, old_d) = _two(rows)

    def i_call(ctx, p, h):
        check(ctx.lib.mhx_bloom_insert_dev(ctx.handle, p["sig"], MHX_U32, n, num_perm, b, r, k, nb, p["filter"]))

    def i_verify(got, res):
        want = old_t.copy()
        B.insert_host(want, sig_t, r, k)
        _same(_as(got["filter"], np.uint32, (b, nb, 16)), want, "bloom insert")
    cases.append(Case("mhx_bloom_insert_dev", f"bloom insert n={n} K={num_perm} b={b} r={r} blocks={nb}", i_call, ins={"sig": (sig_t, sig_d)}, inouts={"filter": (old_t, old_d)},
                      verify=i_verify))

    def q_call(ctx, p, h):
        check(ctx.lib.mhx_bloom_query_dev(ctx.handle, p["sig"], MHX_U32, n, num_perm, b, r, k, nb, p["filter"], p["hit"], 1))

    def q_verify(got, res):
        hit = B.query_host(old_t, sig_t, r, k).view(np.uint8)
        assert 0 < hit.sum() < n
        _same(got["hit"], hit, "bloom query")
        i_verify(got, res)  # then_insert: the second launch
    cases.append(Case("mhx_bloom_query_dev", f"bloom query then insert n={n}", q_call, ins={"sig": (sig_t, sig_d)}, inouts={"filter": (old_t, old_d)}, outs={"hit": n},
                      verify=q_verify))
    other_t, other_d = _two(lambda rng: rng.randint(0, 2**32, size=(b, nb, 16), dtype=np.uint64).astype(np.uint32) & np.uint32(0x01100))

    def u_call(ctx, p, h):
        check(ctx.lib.mhx_bloom_union_dev(ctx.handle, p["dst"], p["src"], b, nb))
    cases.append(Case("mhx_bloom_union_dev", f"bloom union b={b} blocks={nb}", u_call, ins={"src": (other_t, other_d)}, inouts={"dst": (old_t, old_d)},
                      verify=lambda got, res: _same(_as(got["dst"], np.uint32, (b, nb, 16)), old_t | other_t, "bloom union")))
    return cases


def cc_cases():
    """Between init and finish the labels are an opaque parent forest: a link case is the link call and mhx_cc_finish_dev, one
    after the other, on labels as init leaves them (true) or on another valid forest (decoy: labels[i] <= i)."""
    cases = []
    n = 3000
    ident = np.arange(n, dtype=np.uint32)
    twos = ident & ~np.uint32(1)  # a valid forest: every odd row hangs under the even one before it
    # init reads nothing on the device (n is its only input): no decoy can show, a late, early or misplaced write does

    def init_call(ctx, p, h):
        ctx.cc_init_dev(p["labels"], n)
    cases.append(Case("mhx_cc_init_dev", f"cc init n={n}", init_call, outs={"labels": 4 * n}, constant=True,
                      verify=lambda got, res: _same(_as(got["labels"], np.uint32), ident, "cc init")))

    m = 2001
    (pairs_t, cnt_t), (pairs_d, cnt_d) = _two(lambda r: (r.randint(0, n, size=(m, 2)).astype(np.int64), r.randint(0, 17, size=m).astype(np.int32)))
    pairs_t[::50, 0] = n  # invalid edges
    invalid = int(np.count_nonzero(cnt_t[::50] >= 8))
    zero = np.zeros(1, dtype=np.int64)

    def lp_call(ctx, p, h):
        ctx.cc_link_pairs_dev(p["labels"], n, p["pairs"], m, p["counts"], 8, p["bad"])
        ctx.cc_finish_dev(p["labels"], n)

    def lp_verify(got, res):
        keep = (cnt_t >= 8) & (pairs_t < n).all(axis=1)
        _same(_as(got["labels"], np.uint32).astype(np.int64), lsh_bulk.connected_components(pairs_t[keep], n, gpu_mode="disable"), "cc link pairs labels")
        _same(_as(got["bad"], np.int64), np.array([invalid]), "cc link pairs invalid")
    cases.append(Case("mhx_cc_link_pairs_dev", f"cc link pairs + finish n={n} m={m}", lp_call, ins={"pairs": (pairs_t, pairs_d), "counts": (cnt_t, cnt_d)},
                      inouts={"labels": (ident, twos), "bad": (zero, zero + 5)}, verify=lp_verify))

    bands, ns = 3, 2731
    sb_t, sb_d = _two(lambda r: lsh_bulk.sorted_bands(r.randint(0, 900, size=(ns, bands), dtype=np.uint64), bands, 1, gpu_mode="disable"))

    def lb_call(ctx, p, h):
        ctx.cc_link_bands_dev(p["labels"], n, p["dig"], p["rows"], ns, bands, p["bad"])
        ctx.cc_finish_dev(p["labels"], n)

    def lb_verify(got, res):
        edges = np.stack(lsh_bulk._run_edges(*sb_t), axis=1)
        _same(_as(got["labels"], np.uint32).astype(np.int64), lsh_bulk.connected_components(edges, n, gpu_mode="disable"), "cc link bands labels")
        _same(_as(got["bad"], np.int64), np.zeros(1, dtype=np.int64), "cc link bands invalid")
    cases.append(Case("mhx_cc_link_bands_dev", f"cc link bands + finish n={n}, {bands} bands of {ns}", lb_call, ins={"dig": (sb_t[0], sb_d[0]), "rows": (sb_t[1], sb_d[1])},
                      inouts={"labels": (ident, twos), "bad": (zero, zero + 5)}, verify=lb_verify))

    # finish alone: a walk of more than one step for every row (chains of up to 64 rows; the decoy's are of three)
    chain = np.where(ident % 64 == 0, ident, ident - 1).astype(np.uint32)
    chain3 = np.where(ident % 3 == 0, ident, ident - 1).astype(np.uint32)

    def f_call(ctx, p, h):
        ctx.cc_finish_dev(p["labels"], n)
    cases.append(Case("mhx_cc_finish_dev", f"cc finish n={n}, walks of up to 63 steps", f_call, inouts={"labels": (chain, chain3)},
                      verify=lambda got, res: _same(_as(got["labels"], np.uint32), ident - ident % 64, "cc finish")))
    return cases


def text_cases():
    cases = []
    # token windows of w = 2 tokens
    w = 2
    rng = np.random.RandomState(73)
    counts = [w + 1, 0, 1, w, 3 * w, 0, 40, w + 2]
    lens = rng.randint(0, 71, size=sum(counts))
    lens[-1] = 9
    item_offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    doc_offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    buf_t, buf_d = _two(lambda r: r.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8))
    want, set_offsets = shingle.sha1_windows(buf_t, doc_offsets, w, item_offsets=item_offsets, bits=64, gpu_mode="disable")
    n_docs, n_windows = doc_offsets.size - 1, int(set_offsets[-1])

    def win_call(ctx, p, h):
        ctx.sha1_windows_dev(p["bytes"], p["items"], p["docs"], p["sets"], n_docs, n_windows, w, MHX_U64, p["out"])
    cases.append(Case("mhx_sha1_windows_dev", f"sha1 windows of {w} tokens, {n_windows} windows", win_call,
                      ins={"bytes": (buf_t, buf_d), "items": (item_offsets, item_offsets), "docs": (doc_offsets, doc_offsets), "sets": (set_offsets, set_offsets)},
                      outs={"out": want.nbytes}, verify=lambda got, res: _same(_as(got["out"], np.uint64), want, "sha1 windows")))

    # words: count, read the totals back, emit
    alphabet = np.frombuffer(b"aB ,\xc3\xa9", dtype=np.uint8)
    table = shingle.word_table()
    nbytes, docs = 3 * 4096 + 5, 300
    cuts = np.sort(np.random.RandomState(91).randint(0, nbytes + 1, size=docs - 1))
    w_docs = np.concatenate([[0], cuts, [nbytes]]).astype(np.int64)

    def text(r):
        buf = alphabet[r.randint(0, alphabet.size, size=nbytes)].copy()
        buf[0], buf[-1] = ord("a"), ord("B")
        return buf
    txt_t, txt_d = _two(text)
    norm_t, norm_d = (shingle.normalize_words(x, w_docs, table, gpu_mode="disable") for x in (txt_t, txt_d))
    cap_words = max(norm_t[1].size, norm_d[1].size) - 1
    cap_bytes = max(norm_t[0].size, norm_d[0].size)

    def words_call(ctx, p, h):
        return ctx.words_normalize_dev(p["bytes"], nbytes, p["docs"], docs, h["table"], p["text"], cap_bytes, p["items"], cap_words, p["wdocs"])

    def words_verify(got, res):
        assert res == (0, norm_t[1].size - 1, norm_t[0].size), res
        _same(got["text"][: norm_t[0].size], norm_t[0], "words: text")
        _same(_as(got["items"], np.int64)[: norm_t[1].size], norm_t[1], "words: item offsets")
        _same(_as(got["wdocs"], np.int64), norm_t[2], "words: word offsets of the documents")
    cases.append(Case("mhx_words_normalize_dev", f"words normalize {nbytes} bytes, {docs} documents: count, then emit", words_call,
                      ins={"bytes": (txt_t, txt_d), "docs": (w_docs, w_docs)}, outs={"text": cap_bytes, "items": 8 * (cap_words + 1), "wdocs": 8 * (docs + 1)},
                      host=lambda p: {"table": table.copy()}, verify=words_verify))
    return cases


def overlap_cases():
    limit = _native.overlap_limits(32, MI355X_LDS_PER_BLOCK)

    def sets(r):
        pool = r.randint(0, 2**32 - 1, size=2 * limit, dtype=np.int64).astype(np.uint32)
        return [pool[:700], pool[300:1100], pool[: limit // 2], pool[limit // 2: limit], pool[: limit + limit // 2], pool[limit // 2:]]
    s_t, s_d = _two(sets)
    offsets = np.zeros(len(s_t) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in s_t], out=offsets[1:])
    hv_t, hv_d = np.concatenate(s_t), np.concatenate(s_d)
    pairs_t = np.array([[0, 1], [2, 3], [4, 5], [1, 0], [5, 5], [0, 4]], dtype=np.int64)
    pairs_d = np.array([[1, 1], [3, 2], [5, 4], [0, 1], [4, 4], [2, 0]], dtype=np.int64)
    totals = np.diff(offsets)[pairs_t].sum(axis=1)
    assert (totals <= limit).any() and (totals > limit).any(), "one pair in the LDS class and one in the scratch class"
    n_sets, n_pairs, biggest = len(s_t), len(pairs_t), int(np.diff(offsets).max())
    zero = np.zeros(1, dtype=np.int64)

    def call(ctx, p, h):
        ctx.overlap_pairs_dev(p["hv"], MHX_U32, p["off"], n_sets, biggest, p["pairs"], n_pairs, p["counts"], p["bad"])

    def verify(got, res):
        _same(_as(got["counts"], np.int32, (n_pairs, 3)), overlap.overlap_counts_host(hv_t, offsets, pairs_t), "overlap counts")
        _same(_as(got["bad"], np.int64), zero, "overlap invalid")
    return [Case("mhx_overlap_pairs_dev", f"overlap pairs uint32, totals {sorted(set(totals.tolist()))} around the LDS limit {limit}", call,
                 ins={"hv": (hv_t, hv_d), "off": (offsets, offsets), "pairs": (pairs_t, pairs_d)}, inouts={"bad": (zero, zero)}, outs={"counts": 12 * n_pairs}, verify=verify)]


def memset_case(ctx, plug, r):
    """mhx_memset_dev itself (every case above uses it as a tool): O <- 0x77 behind the plug, R <- O, O <- 0x3C.  Its only input
    is the byte, an argument: there is no decoy to read early, a late or reordered write shows as 0xA5 or 0x3C."""
    global CASES, REARMED
    nbytes = 1 << 20
    d_o, d_r = ctx.alloc(nbytes), ctx.alloc(nbytes)
    try:
        for attempt, reps in enumerate((r, 2 * r)):
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(d_o), 0xA5, nbytes))
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(d_r), 0x5A, nbytes))
            t0 = plug.begin(reps)
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(d_o), 0x77, nbytes))
            after = time.perf_counter()
            ctx.copy_dev(d_r.ptr, d_o.ptr, nbytes)
            check(ctx.lib.mhx_memset_dev(ctx.handle, _p(d_o), 0x3C, nbytes))
            t1 = time.perf_counter()
            ctx.synchronize()
            ms = plug.lasted_ms()
            if (t1 - t0) * 1e3 < ms:
                break
            if attempt == 0:
                REARMED += 1
        else:
            raise AssertionError("unarmed twice")
        got = d_r.download((nbytes,), np.uint8)
        assert (got == 0x77).all(), f"R holds {np.unique(got).tolist()}, not 0x77"
        assert (after - t0) * 1e3 < ms, "mhx_memset_dev returned after the plug had ended: it blocks"
        CASES += 1
    finally:
        ctx.synchronize()
        d_o.free()
        d_r.free()


# ------------------------------------------------------------------------------------------- cases beside the per-entry ones
def host_call_cases(ctx, plug, r, front):
    """A `_dev` call still in flight behind the plug, then a pipelined host call: copy_in / copy_out start while the compute
    stream is busy.  Both results must be right.  `front` is a Case that went through the dry pass (its buffers are there)."""
    global CASES, REARMED
    rng = np.random.RandomState(17)
    n, t, k = 2000, 64, 64
    perms = O.np_init_permutations(k, 5)
    hv = rng.randint(0, 2**32, size=(n, t), dtype=np.uint64)
    init = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64)
    want_sig = O.c_minhash_bulk_dense(hv, perms[0], perms[1], init=init)

    def bulk(_):
        return ctx.minhash_bulk(perms, hv, None, t, n, init=init)

    def begin_feed():  # (mhx_weighted_dense_begin allocates the two slots: before the plug)
        return ctx.weighted_dense_feed(gen, s, dim, False, piece)

    dim, s, piece, rows = 64, 32, 64, 200
    rs_, ln_cs, betas = O.np_weighted_params(dim, s, 9)
    gen = ctx.wgen_create(rs_, ln_cs, betas)
    x = rng.uniform(0.5, 50, (rows, dim)).astype(np.float32)
    x[rng.random_sample(x.shape) < 0.5] = 0
    want_w, want_ne = ctx.weighted_minhash_many_dense(gen, s, x, False)

    def feed(f):
        out, ne = np.zeros((rows, s, 2), dtype=np.int64), np.zeros(rows, dtype=np.uint8)
        try:
            for at in range(0, rows, piece):  # four pieces, the last one short
                f.feed(x[at: at + piece], out[at: at + piece], ne[at: at + piece])
        finally:
            f.end()
        return out, ne

    ctx.set_option("host.chunk_bytes", 128 << 10)  # 2000 sets x (512 + 512) bytes: sixteen pieces
    try:
        _same(bulk(None), want_sig, "pipelined host call, unplugged")  # (grows the scratch, creates the copy streams)
        out, ne = feed(begin_feed())
        _same(ne.astype(bool), np.asarray(want_ne).astype(bool), "feed, unplugged: nonempty")
        _same(out, want_w, "feed, unplugged")
        for name, host_call, before_plug, verify in (("mhx_minhash_bulk_typed in sixteen pieces", bulk, lambda: None, lambda got: _same(got, want_sig, "pipelined host call behind a _dev call")),
                                        ("mhx_weighted_dense_feed in four pieces", feed, begin_feed, lambda got: (_same(got[1].astype(bool), np.asarray(want_ne).astype(bool), "feed: nonempty"),
                                                                                                      _same(got[0], want_w, "feed behind a _dev call")))):
            try:
                for attempt, reps in enumerate((r, 2 * r)):
                    front.load(ctx, "D")
                    front.set_options(ctx, True)
                    handle = before_plug()
                    t0 = plug.begin(reps)
                    res, _, _, _ = _steps_behind(ctx, front)
                    entered = time.perf_counter()
                    got_host = host_call(handle)  # blocks: the plug, the _dev call and its own pieces drain
                    ctx.synchronize()
                    front.set_options(ctx, False)
                    ms = plug.lasted_ms()
                    if (entered - t0) * 1e3 < ms:
                        break
                    if attempt == 0:
                        REARMED += 1
                else:
                    raise AssertionError("unarmed twice")
                verify(got_host)
                want, want_res = front.want_true
                for key, _, nb in front.results():
                    _same(front.bufs["R"][key].download((nb,), np.uint8), want[key], f"the _dev call in front of the host call: '{key}'")
                assert res == want_res
                CASES += 1
                print("ok", f"{front.symbol} in flight, then {name}", flush=True)
            except FAILS as e:
                _report(f"{front.symbol} in flight, then {name}", e)
    finally:
        ctx.set_option("host.chunk_bytes", 0)
        ctx.synchronize()
        ctx.wgen_destroy(gen)


def counters_case(ctx, case):
    """mhx_ctx_counters(enable = 1) resets the counters; a MinHash call follows at once, then the counters are read: the counts
    are those of the dry pass (a reset that landed behind the first launch would have eaten some)."""
    global CASES
    case.load(ctx, "S")
    ctx.counters(True)  # (allocates the counters)

    def once():
        ctx.minhash_mode(reset=True)  # the same first launch both times
        ctx.counters(True)
        case.call(ctx, case.pointers(), {})
        return ctx.counters(True)
    first, second = once(), once()
    ctx.counters(False)
    print(f"  counters: {first}", flush=True)
    assert first["sieve_sets_redone"] > 0 and first["pairwise_sets"] > 0, first
    assert first == second, f"counts after a reset differ: {first} then {second}"
    CASES += 1


def python_chains(ctx, plug, r):
    """Four chains of the Python classes on the process context, the plug enqueued in front: equal to the same chain unplugged."""
    global CASES
    from datasketch_amd import MinHash, MinHashLSH

    rng = np.random.RandomState(23)
    sig, probes = _clustered(29, 600, 50, 128, 30, dtype=np.uint64)
    docs = [bytes(rng.choice(np.frombuffer(b"abc de, fg", dtype=np.uint8), size=rng.randint(0, 300))) for _ in range(120)]
    docs[5] = docs[4]
    pairs = rng.randint(0, len(docs), size=(200, 2)).astype(np.int64)

    def lsh_chain():
        index = MinHashLSH(params=(16, 8), num_perm=128, gpu_mode="always")
        index.insert_bulk(list(range(600)), sig)
        a = index.query_bulk(probes)
        for key in (3, 77, 599):
            index.remove(key)
        b = index.query_bulk(probes)
        return [sorted(x) for x in a], [sorted(x) for x in b]

    chains = (("MinHashLSH insert_bulk, query_bulk, remove, query_bulk", lsh_chain),
              ("lsh_bulk.duplicate_clusters", lambda: lsh_bulk.duplicate_clusters(sig, 16, 8, gpu_mode="always")),
              ("MinHash.bulk_signatures(documents, shingle, words)", lambda: MinHash.bulk_signatures(documents=docs, shingle=2, words=True, num_perm=64, seed=3, gpu_mode="always")),
              ("overlap.exact_jaccard_pairs", lambda: overlap.exact_jaccard_pairs(pairs, documents=docs, shingle=3, gpu_mode="always")))
    for name, chain in chains:
        try:
            want = chain()
            ctx.synchronize()
            plug.enqueue(r)
            got = chain()
            ctx.synchronize()
            if isinstance(want, tuple):
                assert want == got, "the chain behind the plug differs from the chain alone"
                assert want[0] != want[1], "removing keys changed no answer"
            else:
                _same(got, want, name)
            CASES += 1
            print("ok", "chain behind the plug:", name, flush=True)
        except FAILS as e:
            _report("chain: " + name, e)


def positive_control(ctx, plug, r, cases):
    """The same three entries on a second context while the plug and the I <- true copies sit on the first: nothing orders the
    second context's stream against the first's, so the entry sees the decoys -- exactly want_decoy, if it was done before the plug."""
    ctx2 = _native.Context(ctx.device)
    rearmed = 0
    try:
        for case in cases:
            # (the second context's own scratch, handles and lazy allocations; and it computes what the first does)
            assert not _differ(case.sync_run(ctx2, "D"), case.want_decoy) and not _differ(case.sync_run(ctx2, "S"), case.want_true), case.name
            for attempt, reps in enumerate((r, 2 * r)):
                case.load(ctx, "D")
                case.set_options(ctx2, True)
                ctx2.synchronize()
                t0 = plug.begin(reps)
                b = case.bufs
                for key, buf in b["I"].items():
                    ctx.copy_dev(buf.ptr, b["S"][key].ptr, buf.nbytes)
                res = case.call(ctx2, case.pointers(), case.host(case.pointers()) if case.host else {})
                ctx2.synchronize()
                done = time.perf_counter()
                ctx.synchronize()
                case.set_options(ctx2, False)
                ms = plug.lasted_ms()
                if (done - t0) * 1e3 < ms:
                    break
                if attempt == 0:
                    rearmed += 1
            else:
                raise AssertionError(f"control unarmed twice: {case.name}")
            # the outputs were written before the plug ended and nothing on the first context writes them; the inputs are the
            # true ones by now, which is the point
            got = {k: buf.download((n,), np.uint8) for k, buf, n in case.results() if k in case.outs}
            for key in got:
                assert np.array_equal(got[key], case.want_decoy[0][key]), (
                    f"control {case.name}: '{key}' is not want_decoy" + (" but want_true: the second context waited for the first" if np.array_equal(got[key], case.want_true[0][key]) else ""))
            assert res == case.want_decoy[1]
            print("ok", "control:", case.name, "on a second context saw the decoys", flush=True)
    finally:
        ctx.synchronize()
        ctx2.synchronize()
        ctx2.close()
    print(f"STREAM ORDER CONTROL OK {len(cases)} entries, {rearmed} rearmed", flush=True)


def main():
    started = time.perf_counter()
    ctx = _native.context()
    cases = (minhash_cases() + weighted_cases(ctx) + pack_cases() + query_cases() + matrix_cases() + index_cases() + forest_cases() + hll_cases() + bloom_cases()
             + cc_cases() + text_cases() + overlap_cases())
    plug = Plug(ctx)
    # -- dry pass: want_true, want_decoy, every allocation
    ready = []
    for case in cases:
        try:
            dry(ctx, case)
            ready.append(case)
        except FAILS as e:
            _report("dry pass: " + case.name, e)
    # -- calibration
    plug.enqueue(2)
    ctx.synchronize()
    t0 = plug.begin(8)
    host_ms = (time.perf_counter() - t0) * 1e3 / 8
    ctx.synchronize()
    unit_ms = plug.lasted_ms() / 8
    enqueue = {case.name: unplugged_ms(ctx, case) for case in ready}
    slowest = max(enqueue, key=enqueue.get)
    # ten times the largest enqueue time, and at least 10 ms: a single sample per case says little about a shared host's worst moment.
    # What the plug's own enqueueing takes (host_ms per launch) is spent before the case's calls and counted against it too
    r = min(4096, int(math.ceil(max(10.0 * enqueue[slowest], 10.0) / max(unit_ms - host_ms, 0.1 * unit_ms))))
    print(f"plug unit {unit_ms:.3f} ms on the device ({host_ms:.3f} ms to enqueue), largest enqueue time {enqueue[slowest]:.3f} ms ({slowest}), "
          f"r = {r}: the plug lasts about {r * unit_ms:.1f} ms", flush=True)
    # -- plugged pass
    for case in ready:
        try:
            run_plugged(ctx, case, plug, r)
            print("ok", case.symbol, "--", case.name, flush=True)
        except FAILS as e:
            _report(case.name, e)
    try:
        memset_case(ctx, plug, r)
        print("ok mhx_memset_dev", flush=True)
    except FAILS as e:
        _report("mhx_memset_dev", e)
    by_symbol = {case.symbol: case for case in ready}
    if "mhx_band_digests_layout_dev" in by_symbol:
        host_call_cases(ctx, plug, r, by_symbol["mhx_band_digests_layout_dev"])
    try:
        counters_case(ctx, by_symbol["mhx_minhash_bulk_dev"])
        print("ok counters reset, MinHash call, counters", flush=True)
    except FAILS as e:
        _report("counters reset followed by a MinHash call", e)
    python_chains(ctx, plug, r)
    # -- positive control: a single-launch entry, MinHash bulk, a multi-launch entry
    try:
        positive_control(ctx, plug, r, [by_symbol[s] for s in ("mhx_band_digests_layout_dev", "mhx_minhash_bulk_dev", "mhx_jaccard_topk_dev")])
    except FAILS as e:
        _report("positive control", e)
    ctx.synchronize()
    for case in cases:
        case.free()
    wall = time.perf_counter() - started
    print(f"total wall time {wall:.1f} s", flush=True)
    if FAILED:
        print(f"STREAM ORDER FAILED: {len(FAILED)} of {CASES + len(FAILED)}: " + "; ".join(FAILED), flush=True)
        sys.exit(1)
    print(f"STREAM ORDER OK {CASES} cases, {REARMED} rearmed", flush=True)


if __name__ == "__main__":
    main()
