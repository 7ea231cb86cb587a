"""The weighted Jaccard device entry points of include/mhx_weighted_jaccard.h in the three sweeps every `_dev` entry of
include/mhx.h goes through (test infrastructure, run by tests/test_gpu_weighted_jaccard_sweeps.py; the helpers of
tests/poison_cases.py, tests/stream_order_cases.py and tests/index_width_cases.py are used as they are):

    python tests/weighted_jaccard_sweep_cases.py poison <byte>   one case per entry on scratch and allocations that hold nothing but
                                                                 the byte; prints "POISON OK <n> cases (weighted_jaccard, byte 0x..)"
    python tests/weighted_jaccard_sweep_cases.py stream          one case per entry behind in-flight work on its stream; prints
                                                                 "WJ STREAM ORDER OK <n> cases, <m> rearmed"

and, imported, WIDTH_BUILDERS: the pair entry with rows past element 2^32 of one allocation (the uint64 words of the rows, as the
MinHash twin counts them) and decoys where a 32-bit index would land; the matrix and the top-k entry with the far rows of B past
byte 2^32 and past 32-bit word 2^32.
"""
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import WeightedMinHash, _native, lsh_bulk  # noqa: E402
from datasketch_amd._native import check  # noqa: E402
from tests import weighted_jaccard_guard_cases as W  # noqa: E402


# ---------------------------------------------------------------------------------------------------------------------- poison
def poison_family(ctx):
    from tests import poison_cases as P
    from tests.guard_cases import _dev, _expect

    rng = np.random.RandomState(51)
    m, n, s = 130, 300, 33
    a, b = W.planted_weighted(rng, m, n, s)
    pairs = np.stack([rng.randint(0, m, size=500), rng.randint(0, n, size=500)], axis=1).astype(np.int64)

    P.begin("weighted pairs")
    d_a, d_b, d_p, d_c = _dev(ctx, a), _dev(ctx, b), _dev(ctx, pairs), P._out(ctx, 500, np.int32)
    check(ctx.lib.mhx_weighted_jaccard_pairs_dev(ctx.handle, d_a.ptr, d_b.ptr, s, d_p.ptr, 500, d_c.ptr))
    _expect(P._taken(d_c, 500, np.int32, "weighted pairs"), W.want_pairs(a, b, pairs), "weighted pairs")

    P.begin("weighted matrix ldc = n_b + 3")
    d_m = P._out(ctx, m * (n + 3), np.int32)
    check(ctx.lib.mhx_weighted_jaccard_matrix_dev(ctx.handle, d_a.ptr, m, d_b.ptr, n, s, d_m.ptr, n + 3))
    got = P._taken(d_m, m * (n + 3), np.int32, "weighted matrix").reshape(m, n + 3)
    _expect(got[:, :n], W.want_matrix(a, b), "weighted matrix")
    assert np.all(got[:, n:].view(np.uint8) == P.PATTERN), "the columns between n_b and ldc"

    floor = s // 3
    want_p, want_c = W.want_threshold(b, None, floor)
    for cap in sorted({len(want_p), len(want_p) // 2}):
        P.begin(f"weighted threshold, self-join, capacity {cap} of {len(want_p)}")
        d_pp, d_cc = P._out(ctx, 2 * cap, np.int64, extra=2 * P.EXTRA), P._out(ctx, cap, np.int32)
        total = ctx.weighted_jaccard_threshold_pairs_dev(d_b.ptr, n, None, 0, s, floor, d_pp.ptr, d_cc.ptr, cap)
        assert total == len(want_p) and 0 < cap, (total, len(want_p))
        p, cc = P._taken(d_pp, 2 * cap, np.int64, "pairs", extra=2 * P.EXTRA).reshape(cap, 2), P._taken(d_cc, cap, np.int32, "counts")
        if cap == len(want_p):
            _expect(p, want_p, "weighted threshold pairs")
            _expect(cc, want_c, "weighted threshold counts")

    live = rng.random_sample(n) < 0.8
    for name, options in (("strip, three segments", {"jaccard.topk_path": 1, "jaccard.topk_segments": 3}), ("stream", {"jaccard.topk_path": 2}),
                          ("the launcher's choice", {})):
        for k, size in ((10, n), (64, 40)):  # (64 of 40 rows: lists with empty entries the merge must still see as empty)
            what = f"weighted topk k={k} of {size} rows, {name}"
            P.begin(what)
            for key, v in options.items():
                ctx.set_option(key, v)
            d_r, d_k = P._out(ctx, m * k, np.int64), P._out(ctx, m * k, np.int32)
            d_l = _dev(ctx, lsh_bulk.live_bits(live[:size]))
            check(ctx.lib.mhx_weighted_jaccard_topk_dev(ctx.handle, d_a.ptr, m, d_b.ptr, size, s, d_l.ptr, floor // 2, k, d_r.ptr, d_k.ptr))
            rows, counts = W.want_topk(a, b[:size], k, floor // 2, live[:size])
            _expect(P._taken(d_r, m * k, np.int64, what).reshape(m, k), rows, what + " rows")
            _expect(P._taken(d_k, m * k, np.int32, what).reshape(m, k), counts, what + " counts")


def poison_main(byte):
    from tests import poison_cases as P

    P.FAMILIES["weighted_jaccard"] = poison_family
    sys.argv = [sys.argv[0], byte, "weighted_jaccard"]
    P.main()


# ---------------------------------------------------------------------------------------------------------------- stream order
def stream_cases():
    from tests.stream_order_cases import Case, _as, _same, _two

    cases = []
    m, n, s = 129, 385, 33
    (a_t, b_t), (a_d, b_d) = _two(lambda r: W.planted_weighted(r, m, n, s))
    ins = {"a": (a_t, a_d), "b": (b_t, b_d)}

    pairs_t, pairs_d = _two(lambda r: np.stack([r.randint(0, m, size=700), r.randint(0, n, size=700)], axis=1).astype(np.int64))
    cases.append(Case("mhx_weighted_jaccard_pairs_dev", f"weighted pairs {m}x{n} S={s}",
                      lambda ctx, p, h: ctx.weighted_jaccard_pairs_dev(p["a"], p["b"], s, p["pairs"], 700, p["out"]),
                      ins=dict(ins, pairs=(pairs_t, pairs_d)), outs={"out": 4 * 700},
                      verify=lambda got, res: _same(_as(got["out"], np.int32), W.want_pairs(a_t, b_t, pairs_t), "weighted pairs")))

    ldc = n + 3
    cases.append(Case("mhx_weighted_jaccard_matrix_dev", f"weighted matrix {m}x{n} S={s} ldc=n_b+3",
                      lambda ctx, p, h: ctx.weighted_jaccard_matrix_dev(p["a"], m, p["b"], n, s, p["out"], ldc),
                      ins=ins, outs={"out": 4 * m * ldc},
                      verify=lambda got, res: _same(_as(got["out"], np.int32, (m, ldc))[:, :n], W.want_matrix(a_t, b_t), "weighted matrix")))

    w_t, w_d = W.want_matrix(a_t, b_t), W.want_matrix(a_d, b_d)
    levels = np.unique(w_t)
    min_count = int(levels[len(levels) // 2])
    ij = np.argwhere(w_t >= min_count)
    cap = max(len(ij), int((w_d >= min_count).sum()))
    assert 0 < len(ij) < w_t.size

    def t_verify(got, res):
        assert res[0] == len(ij), res
        _same(_as(got["pairs"], np.int64, (cap, 2))[: len(ij)], ij, "weighted threshold pairs")
        _same(_as(got["counts"], np.int32)[: len(ij)], w_t[ij[:, 0], ij[:, 1]], "weighted threshold counts")
    # (blocking by design, as its twin: *n_pairs comes back through the launcher's hipStreamSynchronize before the sort is sized)
    cases.append(Case("mhx_weighted_jaccard_threshold_pairs_dev", f"weighted threshold min_count={min_count}: {len(ij)} pairs emitted and sorted",
                      lambda ctx, p, h: (ctx.weighted_jaccard_threshold_pairs_dev(p["a"], m, p["b"], n, s, min_count, p["pairs"], p["counts"], cap),),
                      ins=ins, outs={"pairs": 16 * cap, "counts": 4 * cap}, verify=t_verify, enqueues=False))

    topk = 10
    live_t, live_d = _two(lambda r: r.random_sample(n) < 0.8)

    def tk_verify(got, res):
        rows, cnt = W.want_topk(a_t, b_t, topk, s // 3, live_t)
        _same(_as(got["rows"], np.int64, (m, topk)), rows, "weighted topk rows")
        _same(_as(got["counts"], np.int32, (m, topk)), cnt, "weighted topk counts")
    cases.append(Case("mhx_weighted_jaccard_topk_dev", f"weighted topk {m}x{n} S={s} k={topk}, three segments",
                      lambda ctx, p, h: check(ctx.lib.mhx_weighted_jaccard_topk_dev(ctx.handle, p["a"], m, p["b"], n, s, p["live"], s // 3, topk, p["rows"], p["counts"])),
                      ins=dict(ins, live=(lsh_bulk.live_bits(live_t), lsh_bulk.live_bits(live_d))), outs={"rows": 8 * m * topk, "counts": 4 * m * topk},
                      verify=tk_verify, options={"jaccard.topk_segments": 3}))
    return cases


def stream_main():
    """The dry pass, the calibration and the plugged pass of tests/stream_order_cases.py's main(), for the four cases above."""
    from tests import stream_order_cases as S

    ctx = _native.context()
    cases = stream_cases()
    plug = S.Plug(ctx)
    ready = []
    for case in cases:
        try:
            S.dry(ctx, case)
            ready.append(case)
        except S.FAILS as e:
            S._report("dry pass: " + case.name, e)
    plug.enqueue(2)
    ctx.synchronize()
    t0 = plug.begin(8)
    host_ms = (time.perf_counter() - t0) * 1e3 / 8
    ctx.synchronize()
    unit_ms = plug.lasted_ms() / 8
    enqueue = {case.name: S.unplugged_ms(ctx, case) for case in ready}
    slowest = max(enqueue.values())
    r = min(4096, int(math.ceil(max(10.0 * slowest, 10.0) / max(unit_ms - host_ms, 0.1 * unit_ms))))
    print(f"plug unit {unit_ms:.3f} ms on the device ({host_ms:.3f} ms to enqueue), largest enqueue time {slowest:.3f} ms, r = {r}", flush=True)
    for case in ready:
        try:
            S.run_plugged(ctx, case, plug, r)
            print("ok", case.symbol, "--", case.name, flush=True)
        except S.FAILS as e:
            S._report(case.name, e)
    ctx.synchronize()
    for case in cases:
        case.free()
    if S.FAILED:
        print(f"WJ STREAM ORDER FAILED: {len(S.FAILED)} of {S.CASES + len(S.FAILED)}: " + "; ".join(S.FAILED), flush=True)
        sys.exit(1)
    print(f"WJ STREAM ORDER OK {S.CASES} cases, {S.REARMED} rearmed", flush=True)


# ----------------------------------------------------------------------------------------------------------------- index width
WIDTH_S = 16                             # samples per row of the far-row cases: 64 32-bit words, 256 bytes
WIDTH_N = (1 << 26) + 3                  # rows of B: its 32-bit words pass 2^32, its bytes pass 2^32 at row 2^24


def _samples(words: np.ndarray) -> np.ndarray:
    """[rows, S, 2] int64 view of rows given as uint32 or uint64 words."""
    words = np.ascontiguousarray(words)
    return words.view(np.int64).reshape(words.shape[0], -1, 2)


def _weighted_count(a, b, args):
    return lsh_bulk._equal_samples(_samples(a), _samples(b))


def pair_width_case():
    """mhx_weighted_jaccard_pairs_dev on one allocation of uint64 words whose rows lie around byte 2^32 and elements 2^31 and 2^32,
    with decoys at the wrapped images: tests/index_width_cases.py's _pair_case, counted sample by sample."""
    from tests import index_width_cases as C

    case = C._pair_case("mhx_weighted_jaccard_pairs_dev", "mhx_weighted_jaccard_pairs_dev", np.uint64,
                        [(256, dict(samples=128)), (100, dict(samples=50))], _weighted_count, lambda args: f"S={args['samples']}")

    def definition():
        for call in case.calls:
            big, width, pairs = call.bigs["sig"], call.args["width"], call.args["pairs"]
            rows = {r: WeightedMinHash(1, _samples(big.read(r * width, width)[None])[0]) for r in set(pairs.reshape(-1).tolist())}
            want = [round(rows[i].jaccard(rows[j]) * call.args["samples"]) for i, j in pairs.tolist()]
            np.testing.assert_array_equal(call.checks[0].expected, np.array(want, dtype=np.int32))
            assert 0 < max(want) < call.args["samples"]
    case.definition = definition
    return case


def _far_rows():
    """B as a sparse model (uint32 words, WIDTH_N rows of WIDTH_S samples, filler rows that match nothing), three probes, and the
    planted rows: near-copies of a probe around every mark, and less similar decoys at their wrapped images."""
    from tests import index_width_cases as C

    rng = np.random.RandomState(62)
    k, n = 4 * WIDTH_S, WIDTH_N
    big = C.Big("b", np.uint32, n * k, 0x5A)
    probes = C._rand(rng, 3 * k, np.uint32).reshape(3, k)
    probes[probes == big.fill_elem] ^= np.uint32(1)
    rows = {0, n - 1}
    for u in C.MARKS:
        r = C.mark_elems(u, 4) // k
        rows |= {r - 1, r, r + 1}
    rows = sorted(rows)

    def near(i, keep):
        """`keep` whole samples of probe i; of the others every second one keeps the probe's k and misses its t."""
        row = C._rand(rng, k, np.uint32)
        row[row == big.fill_elem] ^= np.uint32(1)
        at = rng.permutation(WIDTH_S)
        for j, smp in enumerate(at.tolist()):
            if j < keep:
                row[4 * smp: 4 * smp + 4] = probes[i % 3][4 * smp: 4 * smp + 4]
            elif j % 2:
                row[4 * smp: 4 * smp + 2] = probes[i % 3][4 * smp: 4 * smp + 2]
        return row

    for x, r in enumerate(rows):
        big.plant(r * k, near(x, 5 + x))  # every row agrees with its probe in another number of samples
    for x, r in enumerate(rows):
        big.plant_decoys(r * k, k, lambda src, x=x: near(x, 1 + x % 4) if src.size == k else C._rand(rng, src.size, np.uint32))
    planted = sorted({s // k for s, _ in big.plants})
    assert len(rows) == 11 and rows[-1] * k * 4 > 1 << 34
    return big, probes, rows, planted


def topk_width_case():
    from tests import index_width_cases as C

    big, probes, rows, planted = _far_rows()
    k, n = 4 * WIDTH_S, WIDTH_N

    def lists(wrap=None):
        cand = set(planted)
        if wrap is not None:  # the rows whose image is planted read planted data too
            for step in ((1 << 30) // k, (1 << 31) // k, (1 << 32) // k):
                cand |= {q + j * step for q in planted for j in range(1, 5) if q + j * step < n}
        cand = np.array(sorted(cand), dtype=np.int64)
        data = np.stack([big.read(r * k, k) if wrap is None else big.read_wrapped(r * k, k, wrap) for r in cand.tolist()])
        local, counts = lsh_bulk._topk_from_blocks(lsh_bulk._equal_samples_blocks(_samples(probes), _samples(data)), 3, 4, 1, False)
        return np.where(local >= 0, cand[np.maximum(local, 0)], -1).astype(np.int64), counts.astype(np.int32)

    want_rows, want_counts = lists()
    checks = [C.Check("rows", 0, want_rows, "rows", [C.ABOVE] * 3), C.Check("counts", 0, want_counts, "counts", [C.ABOVE] * 3)]
    for name, wrap in C.wraps(4).items():
        r2, c2 = lists(wrap)
        for chk, other in zip(checks, (r2, c2)):
            chk.decoys[name], chk.moved[name] = other, np.ones(3, dtype=bool)
    assert (want_rows >= (1 << 24)).any(axis=1).all(), "every list reaches past byte 2^32"
    first = np.array(rows) * k

    def definition():
        objs = [WeightedMinHash(1, x) for x in _samples(np.stack([big.read(r * k, k) for r in planted]))]
        for i, probe in enumerate(_samples(probes)):
            counts = [round(WeightedMinHash(1, probe).jaccard(o) * WIDTH_S) for o in objs]
            order = sorted((j for j in range(len(planted)) if counts[j] >= 1), key=lambda j: (-counts[j], planted[j]))[:4]
            pad = [-1] * (4 - len(order))
            assert [planted[j] for j in order] + pad == want_rows[i].tolist() and [counts[j] for j in order] + pad == want_counts[i].tolist()

    return C.Case("mhx_weighted_jaccard_topk_dev", "mhx_weighted_jaccard_topk_dev", "unsigned", C.MARKS["unsigned"],
                  C._items(C._roles_of(first, first + k - 1, 1 << 32), first, first + k - 1, 1),
                  [C.Call(dict(n_b=n, samples=WIDTH_S, topk=4, min_count=1), checks, refill={"rows": 0xEE, "counts": 0xEE})], bigs={"b": big},
                  arrays={"probes": probes}, outputs={"rows": 3 * 4 * 8, "counts": 3 * 4 * 4}, elem_bytes=4, definition=definition)


def matrix_width_case():
    """The three probes against all of B: counts[i, r] for every planted row r and its neighbours, downloaded element by element
    (ldc = n_b, so the output's own index i * n_b + r passes 2^27 only: it is the READ of row r that passes the marks)."""
    from tests import index_width_cases as C

    big, probes, rows, planted = _far_rows()
    k, n = 4 * WIDTH_S, WIDTH_N
    p_s = _samples(probes)
    checks = []
    for r in planted:
        want = lsh_bulk._equal_samples(p_s, _samples(big.read(r * k, k)[None])).astype(np.int32)  # [3]
        for i in range(3):
            chk = C.Check("counts", (i * n + r) * 4, want[i: i + 1], f"counts[{i}, {r}]", [C.ABOVE if r * k >= 1 << 32 else C.BELOW])
            for name, wrap in C.wraps(4).items():
                if big.moved(r * k, k, wrap):
                    seen = lsh_bulk._equal_samples(p_s[i: i + 1], _samples(big.read_wrapped(r * k, k, wrap)[None])).astype(np.int32)
                    chk.decoys[name], chk.moved[name] = seen, np.array([True])
            checks.append(chk)
    fillers = [r for r in (1000, (1 << 25) + 1000, n - 1000) if r not in planted]
    assert len(fillers) == 3
    for r in fillers:  # filler rows: nothing agrees
        checks += [C.Check("counts", (i * n + r) * 4, np.zeros(1, dtype=np.int32), f"counts[{i}, {r}] (a filler row)", [C.BELOW]) for i in range(3)]
    first = np.array(rows) * k
    assert any(c.expected[0] > 0 and c.roles == [C.ABOVE] for c in checks)

    def definition():
        for chk in checks[:: 7]:
            i, r = (int(x) for x in chk.what[7:].split("]")[0].split(", "))
            row = WeightedMinHash(1, _samples(big.read(r * k, k)[None])[0])
            assert round(WeightedMinHash(1, p_s[i]).jaccard(row) * WIDTH_S) == int(chk.expected[0]), chk.what

    return C.Case("mhx_weighted_jaccard_matrix_dev", "mhx_weighted_jaccard_matrix_dev", "unsigned", C.MARKS["unsigned"],
                  C._items(C._roles_of(first, first + k - 1, 1 << 32), first, first + k - 1, 1),
                  [C.Call(dict(n_b=n, samples=WIDTH_S), checks, refill={"counts": 0xEE})], bigs={"b": big}, arrays={"probes": probes},
                  outputs={"counts": 3 * n * 4}, elem_bytes=4, definition=definition)


WIDTH_BUILDERS = {"pairs": pair_width_case, "topk": topk_width_case, "matrix": matrix_width_case}


def launch_pairs(ctx, ptr, bufs, case, call):
    pairs = call.args["pairs"]
    bufs["pairs"].upload(pairs)
    ctx.weighted_jaccard_pairs_dev(ptr["sig"], ptr["sig"], call.args["samples"], ptr["pairs"], pairs.shape[0], ptr["counts"])


def launch_topk(ctx, ptr, bufs, case, call):
    a = call.args
    ctx.weighted_jaccard_topk_dev(ptr["probes"], 3, ptr["b"], a["n_b"], a["samples"], None, a["min_count"], a["topk"], ptr["rows"], ptr["counts"])


def launch_matrix(ctx, ptr, bufs, case, call):
    a = call.args
    ctx.weighted_jaccard_matrix_dev(ptr["probes"], 3, ptr["b"], a["n_b"], a["samples"], ptr["counts"], a["n_b"])


WIDTH_LAUNCH = {"mhx_weighted_jaccard_pairs_dev": launch_pairs, "mhx_weighted_jaccard_topk_dev": launch_topk,
                "mhx_weighted_jaccard_matrix_dev": launch_matrix}


if __name__ == "__main__":
    if sys.argv[1] == "poison":
        poison_main(sys.argv[2])
    elif sys.argv[1] == "stream":
        stream_main()
    else:
        raise SystemExit("usage: weighted_jaccard_sweep_cases.py poison <byte> | stream")
