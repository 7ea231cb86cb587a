"""Every device operation of include/mhx.h on scratch and allocations that hold nothing but a poison byte (test infrastructure,
run as a script in a process of its own by tests/test_gpu_poison.py).

    python tests/poison_cases.py <byte> <family>     prints "POISON OK <n> cases (<family>, byte 0x..)" and exits 0
    python tests/poison_cases.py <byte> control      the positive control; prints "POISON CONTROL OK"

<byte> 0 .. 255 goes to mhx_debug_poison_alloc before the first allocation of the process (-1: poison off, for timing a family).
Guard pages stay off.  Before every case mhx_ctx_release_scratch frees the five scratch slots and d_redo, so that the operation
starts on scratch that holds only the byte, and every option the case before set goes back to 0; the name of a case is printed
before it starts.  A case is one call of an entry point; where it goes through a class or a borrowed helper that makes several
calls of the binding, every method of the binding releases the scratch first as well (_install).  Host forms are called through
the C ABI on arrays of this script's own (_host), since the binding allocates most of its outputs itself.  Caller-side outputs are pre-filled with 0xA5 (or the -5 / -7 of the helpers borrowed from the test modules),
the buffers a call may leave partly unwritten have spare elements behind them that must keep the pattern, and every result is
compared for equality with the C / numpy oracle, a gpu_mode="disable" host twin or plain numpy -- never with another GPU path.
"""
import ctypes
import hashlib
import os
import struct
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from datasketch_amd import _native, lsh_bulk  # noqa: E402
from datasketch_amd._native import BAND_MAJOR, MHX_U32, MHX_U64, ROW_MAJOR, check  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import guard_cases as G  # noqa: E402
from tests.guard_cases import _alloc, _dev, _expect, _p  # noqa: E402

_i64 = ctypes.c_int64
EXTRA = 37            # spare elements behind an output the call may leave partly unwritten
PATTERN = 0xA5        # the byte caller-side outputs hold before a call: neither poison byte
CASES = 0
_SET = set()          # options set since the last case began
_FRESH = None


def _install(ctx):
    """Options set through ctx.set_option are remembered; _FRESH() is what happens before every case."""
    global _FRESH
    plain = ctx.set_option

    def set_option(key, value):
        _SET.add(key)
        plain(key, value)

    def fresh():
        ctx.release_scratch()
        for key in sorted(_SET):
            plain(key, 0)
        _SET.clear()

    ctx.set_option = set_option
    _FRESH = fresh

    # A case that goes through a class (an index, a filter, a sketch) makes several calls of the binding, and so do the helpers
    # borrowed from the test modules: every entry point of the binding releases the scratch first, so that each of those calls
    # starts on slots that hold only the byte as well, not on what the call before it left there.  (The calls this script makes
    # through ctx.lib itself come one per case, behind begin().)  Left alone: what allocates or copies for the caller, the knobs,
    # and minhash_mode / minhash_flags, which read what the last MinHash call left in d_redo and the work words.
    plain_methods = {"alloc", "to_device", "event", "info", "set_option", "counters", "minhash_mode", "minhash_flags", "synchronize", "release_scratch",
                     "close", "perm_handle", "wgen_destroy", "pinned_empty", "weighted_dense_feed", "copy_dev", "pack_tokens", "pack_sets", "pack_int_sets"}

    def released_first(method):
        def call(*args, **kwargs):
            ctx.release_scratch()
            return method(*args, **kwargs)
        return call

    for name in dir(type(ctx)):
        if not name.startswith("_") and name not in plain_methods and callable(getattr(ctx, name)):
            setattr(ctx, name, released_first(getattr(ctx, name)))
    # the cases borrowed from the guard scripts count through guard_cases._done: between two of them the scratch is released
    # (the options those functions set around their loops are theirs to put back, and they do)
    # a borrowed case is named only when it is done: the line after it says that the next one has begun, so that the last line
    # of a child that died always names what was running
    G.BETWEEN = lambda name: (print("ok", name, flush=True), ctx.release_scratch(), print("case the borrowed case after", name, flush=True))


def borrowed(name, cases, ctx):
    """The cases of a guard script's function; guard_cases._done counts them and releases the scratch between them."""
    print("case the first borrowed case of", name, flush=True)
    ctx.release_scratch()
    cases(ctx)


def begin(name):
    global CASES
    CASES += 1
    print("case", name, flush=True)
    _FRESH()


def _code(dtype):
    return MHX_U32 if np.dtype(dtype) == np.uint32 else MHX_U64


def _out(ctx, count, dtype, extra=EXTRA):
    return _alloc(ctx, max(1, (count + extra) * np.dtype(dtype).itemsize), fill=PATTERN)


def _taken(buf, count, dtype, what, extra=EXTRA):
    """The first `count` elements; the spare ones behind them must still hold the pattern."""
    size = np.dtype(dtype).itemsize
    raw = buf.download((count + extra) * size, np.uint8)
    if not np.all(raw[count * size:] == PATTERN):
        raise AssertionError(f"{what}: written past the end of the output")
    return raw[: count * size].view(dtype).copy()


def _host_out(shape, dtype):
    out = np.empty(shape, dtype=dtype)
    out.view(np.uint8).fill(PATTERN)
    return out


def _host(what, fn, *args):
    """begin(what), then one host entry point through the C ABI on the caller's own arrays: numpy arrays go as their addresses,
    and the outputs among them are pre-filled by _host_out, so that an element the copy back leaves unwritten shows."""
    begin(what)
    assert all(a.flags.c_contiguous for a in args if isinstance(a, np.ndarray))
    check(fn(*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in args]))


def _csr(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------------- minhash
def _minhash_dev(ctx, perms, hv, offsets, fixed_len, n, want, what, out_dtype=np.uint64, options=None):
    k = len(perms[0])
    begin(what + " _dev")
    for key, v in (options or {}).items():
        ctx.set_option(key, v)
    d_hv = _dev(ctx, hv) if hv.size else ctx.alloc(8)
    d_off = None if offsets is None else _dev(ctx, offsets)
    d_out = _out(ctx, n * k, out_dtype)
    total = int(offsets[-1]) if offsets is not None else n * fixed_len
    ctx.minhash_bulk_dev(perms, d_hv.ptr, _code(hv.dtype), None if d_off is None else d_off.ptr, fixed_len, n, total, None, 0, d_out.ptr, _code(out_dtype))
    ctx.synchronize()
    _expect(_taken(d_out, n * k, out_dtype, what).reshape(n, k), want.astype(out_dtype), what + " _dev")


def _minhash_host(ctx, perms, hv, offsets, fixed_len, n, want, what, out_dtype=np.uint64):
    begin(what + " host")
    got = ctx.minhash_bulk(perms, hv, offsets, fixed_len, n, out=_host_out((n, len(perms[0])), out_dtype))
    _expect(got, want.astype(out_dtype), what + " host")


def minhash_family(ctx):
    rng = np.random.RandomState(101)
    n = 300
    lengths = rng.choice([0, 1, 63, 257, 5000], size=n, p=[0.15, 0.25, 0.3, 0.27, 0.03])
    lengths[:5] = [0, 1, 63, 257, 5000]
    lengths[-1] = 257
    offsets = _csr(lengths)
    for tok_dtype in (np.uint32, np.uint64):
        name = np.dtype(tok_dtype).name
        hv = rng.randint(0, 2**32, size=int(offsets[-1]), dtype=np.uint64)
        if tok_dtype == np.uint64:
            hv[rng.randint(0, hv.size, size=hv.size // 50)] += np.uint64(2**40)
        dense = np.ascontiguousarray(hv[: n * 63].reshape(n, 63))
        for k in (1, 128, 320):
            perms = O.np_init_permutations(k, 3)
            want = O.c_minhash_bulk(hv, offsets, perms[0], perms[1])
            want_dense = O.c_minhash_bulk_dense(dense, perms[0], perms[1])
            ctx.minhash_mode(reset=True)
            _minhash_dev(ctx, perms, hv.astype(tok_dtype), offsets, 0, n, want, f"minhash csr K={k} {name}")  # (300 sets: split over waves)
            _minhash_dev(ctx, perms, hv.astype(tok_dtype), offsets, 0, n, want, f"minhash csr K={k} {name}, a wave per set", options={"minhash.split": 1})
            _minhash_host(ctx, perms, hv.astype(tok_dtype), offsets, 0, n, want, f"minhash csr K={k} {name}")
            _minhash_dev(ctx, perms, dense.astype(tok_dtype), None, 63, n, want_dense, f"minhash dense K={k} {name}", out_dtype=np.uint32)
            _minhash_host(ctx, perms, dense.astype(tok_dtype).reshape(-1), None, 63, n, want_dense, f"minhash dense K={k} {name}")
    # about 10 % repeated tokens: the flagged sets take the second and third launches (d_redo, d_work, the mode word)
    from tests.sieve_rescan_model import sieve_model

    k, t = 128, 256
    perms = O.np_init_permutations(k, 1)
    tok = rng.randint(0, 2**32, (n, t), dtype=np.uint64)
    m = t // 10
    tok[:, t - m:] = np.take_along_axis(tok, rng.randint(0, t - m, (n, m)), axis=1)
    tok[::4] = rng.randint(0, 2**32, (len(tok[::4]), t), dtype=np.uint64)  # every fourth set is clean
    want = O.c_minhash_bulk_dense(tok, perms[0], perms[1])
    begin("minhash repeats, the launcher's choice (300 sets: split over waves, no flags)")
    d_tok, d_out = _dev(ctx, tok), _out(ctx, n * k, np.uint64)
    ctx.minhash_bulk_dev(perms, d_tok.ptr, MHX_U64, None, t, n, n * t, None, 0, d_out.ptr, MHX_U64)
    ctx.synchronize()
    _expect(_taken(d_out, n * k, np.uint64, "repeats").reshape(n, k), want, "minhash repeats, the launcher's choice")
    try:  # the split launches hand no flags over: that they were the ones that ran shows in the flags entry refusing
        ctx.minhash_flags(n)
        raise AssertionError("300 sets of 256 tokens were not split over waves")
    except ValueError:
        pass
    for options in ({"minhash.split": 1}, {"minhash.split": 1, "minhash.adapt": 1}):  # one wave per set: the launches that flag
        what = f"minhash repeats {options}"
        begin(what)
        for key, v in options.items():
            ctx.set_option(key, v)
        ctx.minhash_mode(reset=True)  # a fresh context's first launch: the one-candidate proof
        d_tok, d_out = _dev(ctx, tok), _out(ctx, n * k, np.uint64)
        ctx.minhash_bulk_dev(perms, d_tok.ptr, MHX_U64, None, t, n, n * t, None, 0, d_out.ptr, MHX_U64)
        flags = ctx.minhash_flags(n)
        got = _taken(d_out, n * k, np.uint64, what).reshape(n, k)
        _expect(got, want, what)
        assert set(np.unique(flags).tolist()) <= {0, 1, 2}, (what, np.unique(flags))
        flagged = np.flatnonzero(flags)
        assert flagged.size > 0.2 * n, (what, flagged.size)
        _expect(got[flagged], want[flagged], what + " flagged sets")
        if "minhash.adapt" in options:  # the one-candidate proof first, whatever went before: the launch the numpy model describes
            ok, _ = sieve_model(tok, perms[0], perms[1])
            assert (flags[~ok.all(axis=1)] >= 1).all(), what + ": a set that leaves the proof is not flagged"
        begin(what + " again, by the learned mode")
        for key, v in options.items():
            ctx.set_option(key, v)
        d_out = _out(ctx, n * k, np.uint64)
        ctx.minhash_bulk_dev(perms, d_tok.ptr, MHX_U64, None, t, n, n * t, None, 0, d_out.ptr, MHX_U64)
        assert set(np.unique(ctx.minhash_flags(n)).tolist()) <= {0, 1, 2}
        _expect(_taken(d_out, n * k, np.uint64, what).reshape(n, k), want, what + " again")
        ctx.minhash_mode(reset=True)
    # the dedup and pairwise launches: repeats inside a tile, constant sets
    for k in (64, 128, 256):
        hv = rng.randint(0, 2**32, size=(97, 77), dtype=np.uint64)
        hv[:, 5] = hv[:, 60]
        hv[::3, 7] = hv[::3, 8]
        hv[::3, 9] = hv[::3, 8]
        hv[::5] = hv[::5, :1]
        perms = O.np_init_permutations(k, 2)
        ctx.minhash_mode(reset=True)
        _minhash_dev(ctx, perms, hv, None, 77, 97, O.c_minhash_bulk_dense(hv, perms[0], perms[1]), f"minhash dedup / pairwise K={k}")
        flags = ctx.minhash_flags(97)  # (97 x 77 tokens: a wave per set, the launches that flag)
        assert (flags >= 1).any(), f"K={k}: no set was handed to the launches for the flagged sets"
    # sets split over waves: one huge set, three long ones
    perms = O.np_init_permutations(128, 1)
    one = rng.randint(0, 2**32, (1, 60_000), dtype=np.uint64)
    _minhash_dev(ctx, perms, one, None, 60_000, 1, O.c_minhash_bulk_dense(one, perms[0], perms[1]), "minhash one huge set")
    _minhash_host(ctx, perms, one.reshape(-1), None, 60_000, 1, O.c_minhash_bulk_dense(one, perms[0], perms[1]), "minhash one huge set")
    few = rng.randint(0, 2**32, (3, 5000), dtype=np.uint64)
    _minhash_dev(ctx, perms, few, None, 5000, 3, O.c_minhash_bulk_dense(few, perms[0], perms[1]), "minhash three long sets")
    # minhash.path 1 (the exact fold for every set) and 2
    small = rng.randint(0, 2**32, (67, 100), dtype=np.uint64)
    small[::3, 50:] = small[::3, :50]
    want = O.c_minhash_bulk_dense(small, perms[0], perms[1])
    for path in (1, 2):
        begin(f"minhash.path {path}")
        ctx.set_option("minhash.path", path)
        d_hv, d_out = _dev(ctx, small), _out(ctx, 67 * 128, np.uint64)
        ctx.minhash_bulk_dev(perms, d_hv.ptr, MHX_U64, None, 100, 67, small.size, None, 0, d_out.ptr, MHX_U64)
        ctx.synchronize()
        _expect(_taken(d_out, 67 * 128, np.uint64, "path").reshape(67, 128), want, f"minhash.path {path}")
    # merge
    for count in (1, 127, 128 * 33 + 1):
        x, y = rng.randint(0, 2**32, size=count, dtype=np.uint64), rng.randint(0, 2**32, size=count, dtype=np.uint64)
        begin(f"minhash merge {count} _dev")
        d_x, d_y, d_o = _dev(ctx, x), _dev(ctx, y), _out(ctx, count, np.uint64)
        check(ctx.lib.mhx_minhash_merge_dev(ctx.handle, _p(d_x), _p(d_y), count, _p(d_o)))
        ctx.synchronize()
        _expect(_taken(d_o, count, np.uint64, "merge"), np.minimum(x, y), f"merge {count} _dev")
        out = _host_out(count, np.uint64)
        _host(f"minhash merge {count} host", ctx.lib.mhx_minhash_merge, ctx.handle, x, y, count, out)
        _expect(out, np.minimum(x, y), f"merge {count} host")
    # packed byte tokens through the device SHA-1
    from datasketch_amd import MinHash, sha1_hash64

    sets = [[bytes(rng.randint(0, 256, rng.randint(0, 70), dtype=np.uint8)) for _ in range(rng.randint(0, 60))] for _ in range(50)]
    sets[17] = []
    flat = [tk for s in sets for tk in s]
    buf = np.frombuffer(b"".join(flat), dtype=np.uint8)
    byte_offsets = _csr([len(tk) for tk in flat])
    set_offsets = _csr([len(s) for s in sets])
    for bits, kw in ((32, {}), (64, {"hashfunc": sha1_hash64})):
        fmt, nb, dt = ("<I", 4, np.uint32) if bits == 32 else ("<Q", 8, np.uint64)
        want = np.array([struct.unpack(fmt, hashlib.sha1(tk).digest()[:nb])[0] for tk in flat], dtype=dt)
        out = _host_out(len(flat), dt)
        _host(f"sha1 tokens {bits} bits host", ctx.lib.mhx_sha1_tokens, ctx.handle, buf, byte_offsets, len(flat), _code(dt), out)
        _expect(out, want, f"sha1 {bits} host")
        begin(f"sha1 tokens {bits} bits _dev")
        d_buf, d_off, d_o = _dev(ctx, buf), _dev(ctx, byte_offsets), _out(ctx, len(flat), dt)
        check(ctx.lib.mhx_sha1_tokens_dev(ctx.handle, _p(d_buf), _p(d_off), len(flat), _code(dt), _p(d_o)))
        ctx.synchronize()
        _expect(_taken(d_o, len(flat), dt, "sha1"), want, f"sha1 {bits} _dev")
        begin(f"minhash packed bytes {bits} bits")
        want = MinHash.bulk_signatures(sets, num_perm=128, seed=9, gpu_mode="disable", **kw)
        _expect(MinHash.bulk_signatures(packed=(buf, byte_offsets, set_offsets), num_perm=128, seed=9, gpu_mode="always", **kw), want,
                f"packed bytes {bits} bits")


# ------------------------------------------------------------------------------------------------------------------ weighted
def _weighted_rows(rng, n, dim, densities=(0.02, 0.09, 0.3, 1.0)):
    x = rng.lognormal(0, 2.0, (n, dim)).astype(np.float32)
    dens = rng.choice(densities, size=(n, 1))
    x[rng.random_sample(x.shape) >= dens] = 0
    x[3] = 0
    x[n - 2] = 0
    return x


def _weighted_same(got, ne, want, wn, what):
    _expect(np.asarray(ne).astype(bool), wn, what + " nonempty")
    _expect(got[wn], want[wn], what)
    _expect(got[~wn], np.zeros_like(got[~wn]), what + ": rows that store nothing are zeros")


def weighted_family(ctx):
    import scipy.sparse as sp

    from tests.weighted_dispatch import dense_walk_launch

    rng = np.random.RandomState(202)
    n = 41
    for dim in (64, 1020, 1024, 4096):
        for s in (64, 128):
            rs_, ln_cs, betas = O.np_weighted_params(dim, s, 4)
            begin(f"weighted plan dim={dim} S={s}")
            h = ctx.wgen_create(rs_, ln_cs, betas)
            x = _weighted_rows(rng, n, dim)
            csr = sp.csr_matrix(x)
            csr.sort_indices()
            indptr, indices = csr.indptr.astype(np.int64), csr.indices.astype(np.int32)
            with np.errstate(divide="ignore", invalid="ignore"):
                want, wn = O.c_weighted_minhash_many(indptr, indices, csr.data, rs_, ln_cs, betas)
                want_v, _ = O.c_weighted_minhash_many(indptr, indices, csr.data, rs_, ln_cs, betas, logs=O.c_np_logf(csr.data))
                logs = np.log(x)
            for kernel in (0, 1, 2):
                for is_logs, rows, ref in ((1, logs, want), (0, x, want_v)):
                    # what the option reaches, by the restatement of the launcher that tests/test_weighted_dispatch.py pins: forced
                    # to 1 it is the workgroup-per-row kernel, otherwise the wave-per-row one, and 1 never coincides with the choice
                    launch = {v: dense_walk_launch(dim, s, bool(is_logs), options={"weighted.kernel": v}) for v in (0, 1, 2)}
                    assert launch[1].kernel == "walk_dense" and launch[0].kernel == launch[2].kernel == "walk_wave", (dim, s, launch)
                    what = f"weighted dense dim={dim} S={s} kernel={kernel} logs={is_logs} ({launch[kernel]})"
                    begin(what + " host")
                    ctx.set_option("weighted.kernel", kernel)
                    out, ne = ctx.weighted_minhash_many_dense(h, s, rows, bool(is_logs), out=_host_out((n, s, 2), np.int64), nonempty=_host_out((n,), np.uint8))
                    _weighted_same(out, ne, ref, wn, what + " host")
                    begin(what + " _dev")
                    ctx.set_option("weighted.kernel", kernel)
                    d_x, d_out, d_ne = _dev(ctx, rows), _out(ctx, n * s * 2, np.int64), _out(ctx, n, np.uint8)
                    check(ctx.lib.mhx_weighted_minhash_many_dense_dev(h, _p(d_x), is_logs, n, _p(d_out), _p(d_ne)))
                    ctx.synchronize()
                    _weighted_same(_taken(d_out, n * s * 2, np.int64, what).reshape(n, s, 2), _taken(d_ne, n, np.uint8, what), ref, wn, what + " _dev")
            ctx.wgen_destroy(h)
    # CSR rows on both sides of the cost crossover, rows that store nothing, and a matrix that stores nothing at all
    for dim, s, density in ((1024, 64, 0.1), (4096, 128, 0.09)):
        rs_, ln_cs, betas = O.np_weighted_params(dim, s, 3)
        begin(f"weighted plan (CSR) dim={dim} S={s}")
        h = ctx.wgen_create(rs_, ln_cs, betas)
        n = 120
        x = rng.uniform(0, 100, (n, dim)).astype(np.float32)
        dens = np.clip(density * rng.uniform(0.2, 2.5, n), 0.0, 1.0)
        x[rng.random_sample(x.shape) >= dens[:, None]] = 0
        x[5] = 0
        x[n - 1] = 0
        for name, part in (("mixed", x), ("none walked", x[dens < density * 0.5]), ("all walked", x[dens > density * 1.5]), ("all zero", np.zeros((9, dim), np.float32))):
            m = part.shape[0]
            csr = sp.csr_matrix(part)
            csr.sort_indices()
            indptr, indices, data = csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32)
            with np.errstate(divide="ignore", invalid="ignore"):
                want, wn = O.c_weighted_minhash_many(indptr, indices, data, rs_, ln_cs, betas)
                want_v, _ = O.c_weighted_minhash_many(indptr, indices, data, rs_, ln_cs, betas, logs=O.c_np_logf(data))
            for is_logs, values, ref in ((1, np.log(data), want), (0, data, want_v)):
                what = f"weighted csr dim={dim} S={s} {name} logs={is_logs}"
                out, ne = _host_out((m, s, 2), np.int64), _host_out((m,), np.uint8)
                _host(what + " host", ctx.lib.mhx_weighted_minhash_many, h, indptr, indices, np.ascontiguousarray(values, dtype=np.float32), is_logs, m, out, ne)
                _weighted_same(out, ne, ref, wn, what + " host")
                begin(what + " _dev")
                d_ip, d_ix = _dev(ctx, indptr), _dev(ctx, indices) if indices.size else ctx.alloc(4)
                d_v = _dev(ctx, values) if values.size else ctx.alloc(4)
                d_out, d_ne = _out(ctx, m * s * 2, np.int64), _out(ctx, m, np.uint8)
                check(ctx.lib.mhx_weighted_minhash_many_dev(h, _p(d_ip), _p(d_ix), _p(d_v), is_logs, m, csr.nnz, _p(d_out), _p(d_ne)))
                ctx.synchronize()
                _weighted_same(_taken(d_out, m * s * 2, np.int64, what).reshape(m, s, 2), _taken(d_ne, m, np.uint8, what), ref, wn, what + " _dev")
        ctx.wgen_destroy(h)
    v = rng.lognormal(0, 3.0, 4099).astype(np.float32)
    out = _host_out(v.shape, np.float32)
    _host("weighted logf", ctx.lib.mhx_weighted_logf, ctx.handle, v, v.size, out)
    _expect(out.view(np.uint32), O.c_np_logf(v).view(np.uint32), "weighted logf")


# ------------------------------------------------------------------------------------------------------------------ pack_lsh
def _big_endian(records, n):
    w = records.reshape(n, -1).copy()
    w[:, :8] = w[:, 7::-1]
    w[:, 8:] = w[:, 8:].reshape(n, -1, 4)[:, :, ::-1].reshape(n, -1)
    return w.reshape(records.shape)


def pack_lsh_family(ctx):
    lib = ctx.lib
    rng = np.random.RandomState(303)
    for n in (1, 63, 1001):
        for k, bands, r, takes_fused in ((128, 16, 8, True), (100, 10, 10, False)):
            sig = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64)
            sig[n // 2:] = sig[: n - n // 2]
            shape = f"n={n} K={k}"
            for b in (1, 2, 4, 7, 16, 32):
                want = O.c_bbit_pack(sig, b)
                low = (sig & np.uint64((1 << b) - 1)).astype(np.uint32)
                out = _host_out(want.shape, np.uint64)
                _host(f"bbit pack b={b} {shape} host", lib.mhx_bbit_pack, ctx.handle, sig, n, k, b, out)
                _expect(out, want, f"bbit pack host b={b} {shape}")
                out = _host_out((n, k), np.uint32)
                _host(f"bbit unpack b={b} {shape} host", lib.mhx_bbit_unpack, ctx.handle, want, n, k, b, out)
                _expect(out, low, f"bbit unpack host b={b} {shape}")
                for dt in (np.uint64, np.uint32):
                    begin(f"bbit pack b={b} {shape} {np.dtype(dt).name} _dev")
                    d_sig, d_out = _dev(ctx, sig.astype(dt)), _out(ctx, want.size, np.uint64)
                    check(lib.mhx_bbit_pack_dev_typed(ctx.handle, _p(d_sig), _code(dt), n, k, b, _p(d_out)))
                    ctx.synchronize()
                    _expect(_taken(d_out, want.size, np.uint64, "bbit pack").reshape(want.shape), want, f"bbit pack _dev b={b} {shape}")
                begin(f"bbit unpack b={b} {shape} _dev")
                d_blk, d_out = _dev(ctx, want), _out(ctx, n * k, np.uint32)
                check(lib.mhx_bbit_unpack_dev(ctx.handle, _p(d_blk), n, k, b, _p(d_out)))
                ctx.synchronize()
                _expect(_taken(d_out, n * k, np.uint32, "bbit unpack").reshape(n, k), low, f"bbit unpack _dev b={b} {shape}")
            keys = O.c_band_keys(sig, bands, r)
            dig = lsh_bulk.band_digests(sig, bands, r, gpu_mode="disable")
            out = _host_out(keys.shape, np.uint64)
            _host(f"band keys {shape} host", lib.mhx_band_keys, ctx.handle, sig, n, k, bands, r, out)
            _expect(out, keys, f"band keys host {shape}")
            out = _host_out(dig.shape, np.uint64)
            _host(f"band digests {shape} host", lib.mhx_band_digests, ctx.handle, sig, n, k, bands, r, out)
            _expect(out, dig, f"band digests host {shape}")
            begin(f"band keys {shape} _dev")
            d_sig, d_keys = _dev(ctx, sig), _out(ctx, keys.size, np.uint64)
            check(lib.mhx_band_keys_dev(ctx.handle, _p(d_sig), n, k, bands, r, _p(d_keys)))
            ctx.synchronize()
            _expect(_taken(d_keys, keys.size, np.uint64, "band keys").reshape(keys.shape), keys, f"band keys _dev {shape}")
            for dt in (np.uint64, np.uint32):
                for layout, ref in ((ROW_MAJOR, dig), (BAND_MAJOR, np.ascontiguousarray(dig.T))):
                    what = f"{shape} {np.dtype(dt).name} layout={layout}"
                    begin(f"band digests {what} _dev")
                    d_sig, d_dig = _dev(ctx, sig.astype(dt)), _out(ctx, dig.size, np.uint64)
                    check(lib.mhx_band_digests_layout_dev(ctx.handle, _p(d_sig), _code(dt), n, k, bands, r, layout, _p(d_dig)))
                    ctx.synchronize()
                    _expect(_taken(d_dig, dig.size, np.uint64, "digests").reshape(ref.shape), ref, f"band digests _dev {what}")
                    begin(f"fused pack and digest {what} _dev")
                    blocks = O.c_bbit_pack(sig, 4)
                    d_blk, d_dig = _out(ctx, blocks.size, np.uint64), _out(ctx, dig.size, np.uint64)
                    fused = ctx.bbit_pack_band_digests_dev(d_sig.ptr, _code(dt), n, k, 4, bands, r, d_blk.ptr, d_dig.ptr, layout)
                    ctx.synchronize()
                    assert fused == takes_fused, (what, fused)
                    _expect(_taken(d_blk, blocks.size, np.uint64, "fused blocks").reshape(blocks.shape), blocks, f"fused blocks {what}")
                    _expect(_taken(d_dig, dig.size, np.uint64, "fused digests").reshape(ref.shape), ref, f"fused digests {what}")
            little = O.c_lean_serialize(sig, -77 - n)
            out = _host_out(little.shape, np.uint8)
            _host(f"lean serialize {shape} host", lib.mhx_lean_serialize, ctx.handle, sig, n, k, -77 - n, out)
            _expect(out, little, f"lean serialize host {shape}")
            for big, rec in ((0, little), (1, _big_endian(little, n))):
                back, seeds = _host_out((n, k), np.uint64), _host_out((n,), np.int64)
                _host(f"lean deserialize {shape} big={big} host", lib.mhx_lean_deserialize, ctx.handle, np.ascontiguousarray(rec), n, k, big, back, seeds)
                _expect(back, sig, f"lean deserialize host {shape} big={big}")
                _expect(seeds, np.full(n, -77 - n, dtype=np.int64), f"lean deserialize host seeds {shape} big={big}")
            for big, rec in ((0, little), (1, _big_endian(little, n))):
                for dt in (np.uint64, np.uint32):
                    what = f"{shape} big={big} {np.dtype(dt).name}"
                    begin(f"lean serialize {what} _dev")
                    d_sig, d_rec = _dev(ctx, sig.astype(dt)), _out(ctx, rec.size, np.uint8)
                    check(lib.mhx_lean_serialize_dev_typed(ctx.handle, _p(d_sig), _code(dt), n, k, -77 - n, big, _p(d_rec)))
                    ctx.synchronize()
                    _expect(_taken(d_rec, rec.size, np.uint8, "lean").reshape(rec.shape), rec, f"lean serialize _dev {what}")
                    begin(f"lean deserialize {what} _dev")
                    d_in, d_back, d_seeds, d_bad = _dev(ctx, rec), _out(ctx, n * k, dt), _out(ctx, n, np.int64), _dev(ctx, np.zeros(1, dtype=np.uint32))
                    check(lib.mhx_lean_deserialize_dev(ctx.handle, _p(d_in), n, k, big, _code(dt), _p(d_back), _p(d_seeds), _p(d_bad)))
                    ctx.synchronize()
                    _expect(_taken(d_back, n * k, dt, "lean back").reshape(n, k), sig.astype(dt), f"lean deserialize _dev {what}")
                    _expect(_taken(d_seeds, n, np.int64, "lean seeds"), np.full(n, -77 - n, dtype=np.int64), f"lean deserialize _dev seeds {what}")
                    _expect(d_bad.download((1,), np.uint32), np.zeros(1, dtype=np.uint32), f"lean deserialize _dev bad count {what}")


# ----------------------------------------------------------------------------------------------------------------- bucketing
_SORT_OPTIONS = (("default", {}), ("two_levels", {"lsh.levels": 2}), ("big_bins", {"lsh.bigbins": 2}), ("never_big", {"lsh.bigbins": 1}),
                 ("teams_256", {"lsh.team": 256}), ("teams_1024", {"lsh.team": 1024}), ("radix", {"lsh.sort": 1}),
                 ("radix_gather", {"lsh.sort": 1, "lsh.gather": 1}), ("prehash", {"lsh.prehash": 1}))


def _bucket_plan(n, options):
    """(bits of bins per band, scatter levels, bin capacity) of launch_lsh_bucket_bands (lsh_kernels.hip) for n rows under
    `options`, restated: the library has no counter that names the pass that ran, so what an option or an input reaches is
    asserted from this.  kBinCap 3 072, kBigBinCap 11 264, kOneLevelBits 10, kMaxBinBits 14."""
    levels2, bigbins = options.get("lsh.levels") == 2, options.get("lsh.bigbins", 0)
    bits = 0
    while bits < 14 and (n >> bits) > 2500:
        bits += 1
    big = bigbins != 1 and not levels2 and ((bits > 10 and (n >> 10) <= 11264 * 10 // 11) or (bigbins == 2 and bits >= 2))
    if big:
        bits = bits - 2 if bigbins == 2 and bits <= 10 else 10
    hi_bits = bits // 2 if bits > 10 or (levels2 and bits >= 2) else 0
    return bits, 2 if hi_bits else 1, 11264 if big else 3072


def bucketing_family(ctx):
    lib = ctx.lib
    # what the options reach: at 70 001 rows 32 bins of 3 072 per band in one scatter level; lsh.levels 2 makes it two levels,
    # lsh.bigbins 2 eight bins of 11 264 (at 1 and 2 501 rows there are one and two bins: those options change nothing there, the
    # cases run all the same); lsh.team, lsh.sort, lsh.gather and lsh.prehash choose kernels, not shapes
    assert _bucket_plan(70_001, {}) == (5, 1, 3072) and _bucket_plan(70_001, {"lsh.levels": 2}) == (5, 2, 3072)
    assert _bucket_plan(70_001, {"lsh.bigbins": 2}) == (3, 1, 11264) and _bucket_plan(70_001, {"lsh.bigbins": 1}) == (5, 1, 3072)
    assert _bucket_plan(2501, {"lsh.levels": 2})[:2] == (1, 1) and _bucket_plan(1, {"lsh.bigbins": 2})[:2] == (0, 1)
    bands, r = 4, 2
    k = bands * r
    for n in (1, 2501, 70_001):
        for kind in ("uniform", "cluster"):
            rng = np.random.RandomState(n + len(kind))
            sig = rng.randint(0, 2**32, size=(n, k), dtype=np.uint64).astype(np.uint32)
            if kind == "cluster":
                # band 1: a cluster of equal keys larger than any bin (12 000 > the 11 264 of a big bin; at 2 501 rows nothing can
                # overflow and the cluster is only a long run); band 3: short runs
                sig[rng.randint(0, n, min(n, 12_000) * 2), 2:4] = sig[0, 2:4]
                dup = rng.randint(0, n, n // 3 + 1)
                sig[dup, 6:8] = sig[(dup * 7) % n, 6:8]
            dig = lsh_bulk.band_digests(sig, bands, r, gpu_mode="disable")
            if kind == "cluster" and n > 20_000:  # larger than the bin of every option set: the scatter pass raises its flag
                assert all(np.count_nonzero(dig[:, 1] == dig[0, 1]) > _bucket_plan(n, options)[2] for _, options in _SORT_OPTIONS)
            order = np.argsort(dig.T, axis=1, kind="stable")
            want_rows, want_dig = order.astype(np.uint32), np.take_along_axis(dig.T, order, axis=1)
            dig_bm = np.ascontiguousarray(dig.T)
            for name, options in _SORT_OPTIONS:
                for entry in ("bands", "digests", "digests row-major layout", "digests band-major layout"):
                    what = f"sort {entry} n={n} {kind} {name} (bin bits, levels, capacity {_bucket_plan(n, options)})"
                    begin(what)
                    for key, v in options.items():
                        ctx.set_option(key, v)
                    d_sd, d_sr = _out(ctx, n * bands, np.uint64), _out(ctx, n * bands, np.uint32)
                    if entry == "bands":
                        d_in = _dev(ctx, sig)
                        check(lib.mhx_lsh_sort_bands_dev_typed(ctx.handle, _p(d_in), MHX_U32, n, k, bands, r, _p(d_sd), _p(d_sr)))
                    elif entry == "digests":
                        d_in = _dev(ctx, dig)
                        check(lib.mhx_lsh_sort_digests_dev(ctx.handle, _p(d_in), n, bands, _p(d_sd), _p(d_sr)))
                    else:
                        layout = BAND_MAJOR if "band-major" in entry else ROW_MAJOR
                        d_in = _dev(ctx, dig_bm if layout == BAND_MAJOR else dig)
                        check(lib.mhx_lsh_sort_digests_layout_dev(ctx.handle, _p(d_in), n, bands, layout, _p(d_sd), _p(d_sr)))
                    ctx.synchronize()
                    _expect(_taken(d_sr, n * bands, np.uint32, what).reshape(bands, n), want_rows, what + " rows")
                    _expect(_taken(d_sd, n * bands, np.uint64, what).reshape(bands, n), want_dig, what + " digests")
                    for buf in (d_in, d_sd, d_sr):
                        buf.free()
            got_d, got_r = _host_out((bands, n), np.uint64), _host_out((bands, n), np.uint32)
            _host(f"sort bands n={n} {kind} host form", lib.mhx_lsh_sort_bands, ctx.handle, sig.astype(np.uint64), n, k, bands, r, got_d, got_r)
            _expect(got_r, want_rows, f"host sort n={n} {kind} rows")
            _expect(got_d, want_dig, f"host sort n={n} {kind} digests")


# ------------------------------------------------------------------------------------------------------------------- queries
def _clustered(seed, n, n_probes, k, bases, dtype=np.uint32):
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 2**32, size=(bases, k), dtype=np.uint64)

    def draw(count):
        rows = base[rng.randint(0, bases, size=count)]
        redraw = rng.random_sample(rows.shape) < 0.05
        rows[redraw] = rng.randint(0, 2**32, size=int(redraw.sum()), dtype=np.uint64)
        return rows.astype(dtype)
    return draw(n), draw(n_probes)


def _pairs_call(ctx, call, want_pairs, what):
    """A call that reports `found` (probe, row) or (i, j) pairs and writes them when they fit: with too little room the total is
    exact and nothing is written at or past the capacity; with exactly enough the pairs are the reference's and the spare
    entries keep the pattern."""
    total = len(want_pairs)
    for cap in sorted({0, total // 2, total}):
        begin(f"{what} capacity {cap} of {total}")
        d_pairs = _out(ctx, 2 * cap, np.int64, extra=2 * EXTRA)
        found = call(d_pairs, cap)
        ctx.synchronize()
        assert found == total, (what, cap, found, total)
        raw = d_pairs.download((cap + EXTRA) * 16, np.uint8)
        if cap < total:
            assert np.all(raw[cap * 16:] == PATTERN), f"{what}: written at or past the capacity"
        else:
            _expect(_taken(d_pairs, 2 * cap, np.int64, what, extra=2 * EXTRA).reshape(cap, 2), want_pairs, what)


def _offsets_to_pairs(offsets, rows):
    probe = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    return np.stack([probe, np.asarray(rows, dtype=np.int64)], axis=1).reshape(-1, 2)


def queries_family(ctx):
    from datasketch_amd.lsh import _HostBands
    from datasketch_amd.lshensemble import _HostEnsemble

    lib = ctx.lib
    n, k, bands, r = 3000, 32, 8, 4
    sig, probes = _clustered(7, n, 200, k, 90)
    sig[100:140] = sig[100]  # one bucket of 40 rows in every band
    dig, rows = lsh_bulk.sorted_bands(sig, bands, r, gpu_mode="disable")
    host = _HostBands(k, bands, r, np.uint32)
    host.append(sig)
    want_pairs = lsh_bulk.candidate_pairs(sig, bands, r, gpu_mode="disable")
    assert len(want_pairs) > n

    def candidate_pairs(d_pairs, cap):
        d_dig, d_rows = _dev(ctx, dig), _dev(ctx, rows)
        found, raw = _i64(-1), _i64(-1)
        check(lib.mhx_lsh_candidate_pairs_dev(ctx.handle, _p(d_dig), _p(d_rows), n, bands, _p(d_pairs), cap, ctypes.byref(found), ctypes.byref(raw)))
        assert raw.value >= found.value
        ctx.synchronize()
        return found.value
    _pairs_call(ctx, candidate_pairs, want_pairs, "candidate pairs")
    sig64 = sig.astype(np.uint64)
    for cap in (len(want_pairs) // 2, len(want_pairs)):
        got, found, raw = _host_out((cap + EXTRA, 2), np.int64), _i64(-1), _i64(-1)
        _host(f"candidate pairs host form capacity {cap} of {len(want_pairs)}", lib.mhx_lsh_candidate_pairs, ctx.handle, sig64, n, k, bands, r, got, cap,
              ctypes.byref(found), ctypes.byref(raw))
        assert found.value == len(want_pairs) <= raw.value, (cap, found.value, raw.value)
        assert np.all(got[cap:].view(np.uint8) == PATTERN), "candidate pairs host form: written at or past the capacity"
        if cap == len(want_pairs):
            _expect(got[:cap], want_pairs, "candidate pairs host form")

    rng = np.random.RandomState(8)
    nothing = rng.randint(0, 2**32, size=(50, k), dtype=np.uint64).astype(np.uint32)
    for name, q in (("clustered probes", probes), ("probes that hit nothing", nothing), ("probes that all hit one bucket", np.repeat(sig[100:101], 64, axis=0)),
                    ("one probe", sig[2999:3000])):
        want = _offsets_to_pairs(*host.query(q))
        if "nothing" in name:
            assert len(want) == 0
        if "one bucket" in name:
            assert len(want) >= 64 * 40

        def bulk_query(d_pairs, cap, q=q):
            d_dig, d_rows, d_sig, d_q = _dev(ctx, dig), _dev(ctx, rows), _dev(ctx, sig), _dev(ctx, q)
            found = _i64(-1)
            check(lib.mhx_lsh_query_dev(ctx.handle, _p(d_dig), _p(d_rows), n, bands, r, _p(d_q), _p(d_sig), MHX_U32, k, q.shape[0], _p(d_pairs), cap,
                                        ctypes.byref(found)))
            ctx.synchronize()
            return found.value
        _pairs_call(ctx, bulk_query, want, f"bulk query, {name}")

    # the ensemble's ranges query: two levels, 16 partitions (one empty), level buffers from the host twin
    n_parts = 16
    levels = [(2, 16), (4, 8)]
    start = np.linspace(0, n, n_parts + 1).astype(np.int64)
    start[3] = start[2]
    params = np.array([[0, 16], [0, 7], [1, 8], [1, 1], [1, 0]], dtype=np.int32)
    ens = _HostEnsemble(k, np.uint32, levels, start)
    ens.build(sig)
    for name, q in (("clustered probes", probes), ("probes that hit nothing", nothing), ("one probe", sig[2999:3000])):
        m = q.shape[0]
        choice = np.random.RandomState(12).randint(0, params.shape[0] + 1, size=(m, n_parts)).astype(np.uint8)
        want = _offsets_to_pairs(*ens.query(q, choice, params))

        def ensemble_query(d_pairs, cap, q=q, choice=choice, m=m):
            bufs = [(_dev(ctx, d), _dev(ctx, rw)) for d, rw in ens.level_buffers()]
            c_levels = (_native.EnsembleLevel * len(levels))(*[_native.EnsembleLevel(d.ptr, rw.ptr, lr, lb) for (d, rw), (lr, lb) in zip(bufs, levels)])
            d_sig, d_q, d_choice = _dev(ctx, sig), _dev(ctx, q), _dev(ctx, choice)
            found = _i64(-1)
            check(lib.mhx_lsh_ensemble_query_dev(ctx.handle, c_levels, len(levels), start.ctypes.data_as(ctypes.POINTER(_i64)), n_parts, _p(d_sig), MHX_U32, k,
                                                 _p(d_q), m, _p(d_choice), params.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), params.shape[0], _p(d_pairs),
                                                 cap, ctypes.byref(found)))
            ctx.synchronize()
            return found.value
        _pairs_call(ctx, ensemble_query, want, f"ensemble query, {name}")


# --------------------------------------------------------------------------------------------------------------------- index
def index_family(ctx):
    from datasketch_amd import MinHashLSH
    from datasketch_amd.lsh import _DeviceBands, _HostBands

    k, bands, r = 32, 8, 4
    sig, probes = _clustered(17, 2600, 150, k, 120)
    keys = [f"doc-{i}" for i in range(sig.shape[0])]
    dev, host = (MinHashLSH(num_perm=k, params=(bands, r), gpu_mode=mode) for mode in ("always", "disable"))
    other_dev, other_host = (MinHashLSH(num_perm=k, params=(bands, r), gpu_mode=mode) for mode in ("always", "disable"))

    def same(step, q=probes):
        assert isinstance(dev._backend, _DeviceBands) and isinstance(host._backend, _HostBands)
        got, want = dev.query_bulk(q), host.query_bulk(q)
        assert got == want, f"{step}: query_bulk differs from the numpy back end at probe {next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)}"
        assert sum(map(len, want)) > 0
        (d_dig, d_rows), (h_dig, h_rows) = dev._backend.bands(), host._backend.bands()
        _expect(d_dig, h_dig, step + " band digests")
        _expect(d_rows, h_rows, step + " band rows")
        _expect(dev._backend.matrix(), host._backend.matrix().astype(dev._backend.dtype), step + " matrix")

    for batch in range(3):  # 700, 1 400 (past the 1 024-row capacity: the matrix grows, the bands are merged), 2 100
        begin(f"index insert_bulk batch {batch}")
        part = slice(700 * batch, 700 * (batch + 1))
        for one in (dev, host):
            one.insert_bulk(keys[part], sig[part])
            one.flush()
        same(f"insert_bulk batch {batch}")
    begin("index remove every third key, compact")
    for one in (dev, host):
        for i in range(0, 2100, 3):
            one.remove(keys[i])
        one.compact()
    assert dev._n_dead == 0
    same("remove + compact")
    begin("index merge with a second index")
    for one in (other_dev, other_host):
        one.insert_bulk(keys[2100:], sig[2100:])
        one.flush()
    dev.merge(other_dev)
    host.merge(other_host)
    same("merge")
    begin("index probe that forces widen")
    wide = probes.astype(np.uint64)
    wide[::7, 5] += np.uint64(2**32)
    same("widen", wide)
    assert dev._backend.dtype == np.uint64
    begin("SortedBandsIndex build, query, clusters")
    twin = _HostBands(k, bands, r, np.uint32)
    twin.append(sig)
    index = lsh_bulk.SortedBandsIndex(sig, bands, r)
    offsets, rows = index.query(probes, capacity=1)
    want = twin.query(probes)
    _expect(offsets, want[0], "SortedBandsIndex offsets")
    _expect(rows, want[1], "SortedBandsIndex rows")
    begin("SortedBandsIndex clusters")
    _expect(index.clusters(), lsh_bulk.duplicate_clusters(sig, bands, r, gpu_mode="disable"), "SortedBandsIndex clusters")
    begin("SortedBandsIndex clusters with a threshold")
    _expect(index.clusters(0.93), lsh_bulk.duplicate_clusters(sig, bands, r, threshold=0.93, gpu_mode="disable"), "SortedBandsIndex clusters, threshold")


# ---------------------------------------------------------------------------------------------------------- forest, ensemble
def forest_family(ctx):
    """The sizes of tests/test_gpu_grid_trips.py::test_forest_search_and_build; the build against np.lexsort, the walk against
    lshforest.host_query (inside _query_case), and the class against its numpy back end."""
    from datasketch_amd import MinHashLSHForest
    from tests.test_gpu_lshforest import _build, _corpus, _query_case
    from tests.test_lshforest_host import lexsort_order

    l, tree_words = 8, 4
    width = l * tree_words
    rng = np.random.RandomState(5)
    sig, bases = _corpus(rng, 500, width, 3, np.uint32)
    probes, _ = _corpus(rng, 2100, width, 3, np.uint32, bases=bases)
    probes[:700] = sig[rng.randint(500, size=700)]
    big, _ = _corpus(rng, 2100, width, 3, np.uint32, bases=bases)
    begin("forest build 500 rows")
    d_sig, d_order, order = _build(ctx, sig, l, tree_words)
    _expect(order, lexsort_order(sig, l, tree_words), "forest build 500 rows")
    begin("forest query 1100 probes w=1 k=10")
    _query_case(ctx, sig, d_sig, d_order, order, probes[:1100], l, tree_words, 1, 10)
    begin("forest query 2100 probes w=2 k=3")
    _query_case(ctx, sig, d_sig, d_order, order, probes, l, tree_words, 2, 3)
    begin("forest query one probe k=64")
    _query_case(ctx, sig, d_sig, d_order, order, probes[:1], l, tree_words, 1, 64)
    begin("forest build 2100 rows")
    d_big, d_big_order, big_order = _build(ctx, big, l, tree_words)
    _expect(big_order, lexsort_order(big, l, tree_words), "forest build 2100 rows")
    begin("forest query 300 probes over 2100 rows")
    _query_case(ctx, big, d_big, d_big_order, big_order, probes[:300], l, tree_words, 1, 10)
    begin("MinHashLSHForest class")
    dev, host = (MinHashLSHForest(num_perm=width, l=l, gpu_mode=mode) for mode in ("always", "disable"))
    for one in (dev, host):
        one.add_bulk(list(range(500)), sig)
        one.index()
    assert dev.query_bulk(probes[:200], 10) == host.query_bulk(probes[:200], 10)


def ensemble_family(ctx):
    """The sizes of tests/test_gpu_grid_trips.py::test_lsh_ensemble_query against the numpy back end, and the class."""
    from datasketch_amd import MinHashLSHEnsemble
    from datasketch_amd.lshensemble import _DeviceEnsemble, _HostEnsemble

    n, m, k, n_parts = 800, 600, 64, 16
    sig, probes = _clustered(11, n, m, k, 25)
    levels = [(2, 32), (4, 16)]
    start = np.linspace(0, n, n_parts + 1).astype(np.int64)
    start[3] = start[2]
    params = np.array([[0, 32], [0, 7], [1, 16], [1, 1], [1, 0]], dtype=np.int32)
    choice = np.random.RandomState(12).randint(0, params.shape[0] + 1, size=(m, n_parts)).astype(np.uint8)
    host = _HostEnsemble(k, np.uint32, levels, start)
    host.build(sig)
    begin("ensemble build")
    dev = _DeviceEnsemble(ctx, k, np.uint32, levels, start)
    dev.build(sig)
    for level, ((hd, hr), (dd, dr)) in enumerate(zip(host.level_buffers(), dev.level_buffers())):
        _expect(dd, hd, f"ensemble level {level} digests")
        _expect(dr, hr, f"ensemble level {level} rows")
    want = host.query(probes, choice, params)
    assert int(want[0][-1]) > 0
    for capacity in (None, 1):
        begin(f"ensemble query capacity={capacity}")
        got = dev.query(probes, choice, params, capacity=capacity)
        _expect(got[0], want[0], "ensemble query offsets")
        _expect(got[1], want[1], "ensemble query rows")
    begin("ensemble query one probe")
    got, want = dev.query(probes[:1], choice[:1], params), host.query(probes[:1], choice[:1], params)
    _expect(got[0], want[0], "ensemble query, one probe, offsets")
    _expect(got[1], want[1], "ensemble query, one probe, rows")
    begin("MinHashLSHEnsemble class")
    rng = np.random.RandomState(13)
    sizes = np.minimum((rng.pareto(1.0, n) * 20 + 1).astype(np.int64), 50_000)
    q_sizes = np.exp(rng.uniform(0, np.log(10_000), 100)).astype(np.int64)
    both = [MinHashLSHEnsemble(threshold=0.5, num_perm=k, gpu_mode=mode) for mode in ("always", "disable")]
    for one in both:
        one.index_bulk(list(range(n)), sig, sizes)
    got, want = (one.query_bulk(probes[:100], q_sizes) for one in both)
    assert got == want and sum(map(len, want)) > 0


# ------------------------------------------------------------------------------------------------------------------- jaccard
def _host_threshold(what, fn, front, ij, c):
    """A host threshold entry (front: its arguments up to min_count) with half the room and with exactly enough, a case each:
    the total is exact both times, nothing is written at or past the capacity, and with enough room the list is the reference's."""
    for cap in sorted({len(ij) // 2, len(ij)}):
        pairs, counts, found = _host_out((cap + EXTRA, 2), np.int64), _host_out((cap + EXTRA,), np.int32), _i64(-1)
        _host(f"{what} capacity {cap} of {len(ij)}", fn, *front, pairs, counts, cap, ctypes.byref(found))
        assert found.value == len(ij), (what, cap, found.value, len(ij))
        assert np.all(pairs[cap:].view(np.uint8) == PATTERN) and np.all(counts[cap:].view(np.uint8) == PATTERN), what + ": written at or past the capacity"
        if cap == len(ij):
            _expect(pairs[:cap], ij, what + " pairs")
            _expect(counts[:cap], c, what + " counts")


def jaccard_family(ctx):
    from datasketch_amd import b_bit_minhash
    from tests.test_gpu_jaccard_matrix import _counts, _dev_matrix, _dev_threshold, _planted, _want_pairs

    def threshold(a, b, k, t, counts, what, code=MHX_U32, self_join=False):
        ij, c = _want_pairs(counts, t, self_join)
        for cap in sorted({len(ij), len(ij) // 2}):
            begin(f"{what} t={t} capacity {cap} of {len(ij)}")
            total, p, cc = _dev_threshold(ctx, a, None if self_join else b, k, t, cap, code=code)
            assert total == len(ij), (what, total, len(ij))
            if cap == len(ij):
                _expect(p[:cap], ij, what + " pairs")
                _expect(cc[:cap], c, what + " counts")
            assert np.all(p[cap:] == -5) and np.all(cc[cap:] == -5), what + ": written at or past the capacity"

    for m, n, k in ((65, 129, 64), (130, 200, 3)):
        rng = np.random.RandomState(m * 7 + n + k)
        a, b = _planted(rng, m, n, k)
        counts, self_counts = _counts(a, b), _counts(b, b)  # (the self-join is B's: its rows are planted copies)
        t = max(1, int(np.percentile(counts, 97)))
        for dt in (np.uint32, np.uint64):
            what = f"jaccard {m}x{n}x{k} {np.dtype(dt).name}"
            begin(what + " matrix")
            got = _dev_matrix(ctx, a.astype(dt), b.astype(dt), k, ldc=n + 3, code=_code(dt))
            _expect(got[:, :n], counts, what + " matrix")
            assert np.all(got[:, n:] == -7), what + ": the columns between n_b and ldc"
            begin(what + " self matrix")
            _expect(_dev_matrix(ctx, b.astype(dt), None, k, code=_code(dt)), self_counts, what + " self matrix")
            threshold(a.astype(dt), b.astype(dt), k, t, counts, what + " threshold", code=_code(dt))
            threshold(b.astype(dt), None, k, t, self_counts, what + " self threshold", code=_code(dt), self_join=True)
            # a threshold nothing reaches: column 0 of B holds a value no row of A has, so no pair agrees in all k positions
            b2 = b.copy()
            b2[:, 0] = next(v for v in range(2**31, 2**31 + m + 1) if v not in set(a[:, 0].tolist()))
            begin(what + " a threshold nothing reaches")
            total, p, cc = _dev_threshold(ctx, a.astype(dt), b2.astype(dt), k, k, 16, code=_code(dt))
            assert total == 0, (what, total)
            assert np.all(p == -5) and np.all(cc == -5)
        a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
        out = _host_out((m, n), np.int32)
        _host(f"jaccard {m}x{n}x{k} matrix host form", ctx.lib.mhx_jaccard_matrix, ctx.handle, a64, m, b64, n, k, out)
        _expect(out, counts, "jaccard matrix host form")
        _host_threshold(f"jaccard {m}x{n}x{k} threshold host form", ctx.lib.mhx_jaccard_threshold_pairs, (ctx.handle, a64, m, b64, n, k, t),
                        *_want_pairs(counts, t, False))
        for bits in (1, 2, 8):
            what = f"bbit jaccard {m}x{n}x{k} b={bits}"
            mask = np.uint64((1 << bits) - 1)
            a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
            pa, pb = (b_bit_minhash.pack_matrix(x, bits, gpu_mode="disable") for x in (a64, b64))
            want = _counts(a64 & mask, b64 & mask)
            begin(what + " matrix")
            d_a, d_b, d_c = _dev(ctx, pa), _dev(ctx, pb), _out(ctx, m * (n + 3), np.int32)
            ctx.bbit_jaccard_matrix_dev(d_a.ptr, m, d_b.ptr, n, k, bits, d_c.ptr, n + 3)
            ctx.synchronize()
            got = _taken(d_c, m * (n + 3), np.int32, what).reshape(m, n + 3)
            _expect(got[:, :n], want, what + " matrix")
            assert np.all(got[:, n:].view(np.uint8) == PATTERN)
            tb = max(1, int(np.percentile(want, 97)))
            ij, c = _want_pairs(want, tb, False)
            for cap in sorted({len(ij), len(ij) // 2}):
                begin(f"{what} threshold capacity {cap} of {len(ij)}")
                d_p, d_cc = _out(ctx, 2 * cap, np.int64, extra=2 * EXTRA), _out(ctx, cap, np.int32)
                total = ctx.bbit_jaccard_threshold_pairs_dev(d_a.ptr, m, d_b.ptr, n, k, bits, tb, d_p.ptr, d_cc.ptr, cap)
                assert total == len(ij), (what, total, len(ij))
                p, cc = _taken(d_p, 2 * cap, np.int64, what, extra=2 * EXTRA).reshape(cap, 2), _taken(d_cc, cap, np.int32, what)
                if cap == len(ij):
                    _expect(p, ij, what + " pairs")
                    _expect(cc, c, what + " counts")
            out = _host_out((m, n), np.int32)
            _host(what + " matrix host form", ctx.lib.mhx_bbit_jaccard_matrix, ctx.handle, pa, m, pb, n, k, bits, out)
            _expect(out, want, what + " host matrix")
            _host_threshold(what + " threshold host form", ctx.lib.mhx_bbit_jaccard_threshold_pairs, (ctx.handle, pa, m, pb, n, k, bits, tb), ij, c)


# ---------------------------------------------------------------------------------------------------------------------- topk
def topk_family(ctx):
    from datasketch_amd import b_bit_minhash
    from tests.test_gpu_jaccard_matrix import _counts
    from tests.test_gpu_jaccard_topk import _case, _dev_topk, _tie_at_k, _want

    def same(got, want, what):
        _expect(got[0], want[0], what + " rows")
        _expect(got[1], want[1], what + " counts")

    for m, n, k_perm in ((130, 4097, 64), (3, 4097, 64)):
        a, b, counts = _case(m, n, k_perm)
        for name, options in (("strip, one segment", {"jaccard.topk_path": 1, "jaccard.topk_segments": 1}),
                              ("strip, three segments", {"jaccard.topk_path": 1, "jaccard.topk_segments": 3}),
                              ("stream", {"jaccard.topk_path": 2}), ("the launcher's choice", {})):
            for k in (1, 10, 64):
                what = f"topk {m}x{n}x{k_perm} k={k} {name}"
                assert _tie_at_k(counts, k)
                begin(what)
                for key, v in options.items():
                    ctx.set_option(key, v)
                same(_dev_topk(ctx, a, b, k_perm, k, code=MHX_U32, extra=EXTRA), _want(counts, k), what)
    a, b, counts = _case(130, 4097, 64)
    rng = np.random.RandomState(44)
    live = rng.random_sample(4097) < 0.8
    for name, options in (("strip, three segments", {"jaccard.topk_path": 1, "jaccard.topk_segments": 3}), ("stream", {"jaccard.topk_path": 2})):
        what = f"topk n_b < k, {name}"  # lists with empty entries the merge must still see as empty
        begin(what)
        for key, v in options.items():
            ctx.set_option(key, v)
        same(_dev_topk(ctx, a, b[:40], 64, 64, extra=EXTRA), _want(counts[:, :40], 64), what)
        what = f"topk live-bit map and a floor, {name}"
        begin(what)
        for key, v in options.items():
            ctx.set_option(key, v)
        same(_dev_topk(ctx, a, b, 64, 10, live=live, min_count=20, extra=EXTRA), _want(counts, 10, min_count=20, live=live), what)
        what = f"topk uint64 rows, {name}"
        begin(what)
        for key, v in options.items():
            ctx.set_option(key, v)
        same(_dev_topk(ctx, a.astype(np.uint64), b.astype(np.uint64), 64, 10, code=MHX_U64, extra=EXTRA), _want(counts, 10), what)
        what = f"topk self mode, {name}"
        self_counts = _counts(b[:700], b[:700])
        begin(what)
        for key, v in options.items():
            ctx.set_option(key, v)
        same(_dev_topk(ctx, b[:700], None, 64, 7, live=live[:700], extra=EXTRA), _want(self_counts, 7, self_join=True, live=live[:700]), what)
    a64, b64 = a.astype(np.uint64), b.astype(np.uint64)
    for name, chunk, k in (("three blocks of B", 1400 * 64 * 8, 10), ("one block", 0, 64)):  # 4 097 rows of 512 bytes: 1 400 + 1 400 + 1 297
        rows, cnt = _host_out((130, k), np.int64), _host_out((130, k), np.int32)
        begin(f"topk host form, {name}")
        ctx.set_option("host.chunk_bytes", chunk)
        check(ctx.lib.mhx_jaccard_topk(ctx.handle, a64.ctypes.data, 130, b64.ctypes.data, 4097, 64, 0, k, rows.ctypes.data, cnt.ctypes.data))
        same((rows, cnt), _want(counts, k), f"topk host form, {name}")
    for bits in (2,):
        what = f"topk b-bit rows b={bits}"
        mask = np.uint64((1 << bits) - 1)
        a64, b64 = a.astype(np.uint64), b[:1000].astype(np.uint64)
        pa, pb = (b_bit_minhash.pack_matrix(x, bits, gpu_mode="disable") for x in (a64, b64))
        want = _want(_counts(a64 & mask, b64 & mask), 10)
        begin(what)
        same(_dev_topk(ctx, pa, pb, 64, 10, bbit=bits, extra=EXTRA), want, what)
        rows, cnt = _host_out((130, 10), np.int64), _host_out((130, 10), np.int32)
        _host(what + " host form", ctx.lib.mhx_bbit_jaccard_topk, ctx.handle, pa, 130, pb, 1000, 64, bits, 0, 10, rows, cnt)
        same((rows, cnt), want, what + " host form")


# --------------------------------------------------------------------------------------------------- hll, bloom, clusters
def hll_family(ctx):
    from datasketch_amd import HyperLogLog, prehashed
    from datasketch_amd import hyperloglog as H
    from tests import hll_guard_cases

    borrowed("hll_guard_cases.bulk_cases", hll_guard_cases.bulk_cases, ctx)
    borrowed("hll_guard_cases.matrix_cases", hll_guard_cases.matrix_cases, ctx)
    rng = np.random.RandomState(61)
    for p in (4, 8, 12):
        m = 1 << p
        sets = [rng.randint(0, 2**32, size=c, dtype=np.uint64) for c in (0, 1, m // 2, 2 * m, 3 * m, 40 * m)]
        corpus = (np.concatenate(sets), _csr([s.size for s in sets]))
        begin(f"HyperLogLog bulk registers p={p}")
        reg = HyperLogLog.bulk_registers(corpus, p=p, hashfunc=prehashed, gpu_mode="always")
        want = HyperLogLog.bulk_registers(corpus, p=p, hashfunc=prehashed, gpu_mode="disable")
        _expect(reg, want, f"HyperLogLog bulk registers p={p}")
        groups = np.array([0, 0, 2, 3, len(sets)], dtype=np.int64)
        begin(f"HyperLogLog union p={p}")
        _expect(H.union_groups(want, groups, gpu_mode="always"), H.union_groups(want, groups, gpu_mode="disable"), f"HyperLogLog union p={p}")
        begin(f"HyperLogLog merge p={p}")
        _expect(H.merge_many(want[:3], want[3:], gpu_mode="always"), np.maximum(want[:3], want[3:]), f"HyperLogLog merge p={p}")
        begin(f"HyperLogLog count p={p}")
        on, off = H.count_many(want, gpu_mode="always"), H.count_many(want, gpu_mode="disable")
        assert np.array_equal(on, off, equal_nan=True), (p, on, off)
    begin("HyperLogLog objects: update_batch, union, count")
    tokens = [bytes(rng.randint(0, 256, 9, dtype=np.uint8)) for _ in range(3000)]
    counts = []
    for mode in ("always", "disable"):
        x, y = HyperLogLog(10, gpu_mode=mode), HyperLogLog(10, gpu_mode=mode)
        x.update_batch(tokens[:2000])
        y.update_batch(tokens[1000:])
        u = HyperLogLog.union(x, y)
        counts.append((x.reg.tolist(), u.reg.tolist(), u.count()))
    assert counts[0] == counts[1]


def bloom_family(ctx):
    from datasketch_amd import MinHash
    from tests import bloom_guard_cases
    from tests.test_lsh_bloom_host import quiet

    for lanes in (16, 1, 0):
        ctx.set_option("bloom.lanes", lanes)
        borrowed(f"bloom_guard_cases.filter_cases, bloom.lanes {lanes}", bloom_guard_cases.filter_cases, ctx)
    num_perm = 32
    rng = np.random.RandomState(71)
    sig = rng.randint(0, 2**32, size=(900, num_perm), dtype=np.uint64)
    sig[600:700] = sig[:100]
    args = dict(num_perm=num_perm, n=2000, fp=0.001, params=(8, 4))
    for lanes in (16, 1):
        begin(f"MinHashLSHBloom insert, query, query then insert, lanes={lanes}")
        ctx.set_option("bloom.lanes", lanes)
        dev, host = quiet(gpu_mode="always", **args), quiet(gpu_mode="disable", **args)
        assert dev.on_device and not host.on_device
        for one in (dev, host):
            one.insert_bulk(sig[:300])
            one.insert(MinHash(num_perm, hashvalues=sig[300]))
        _expect(dev.words(), host.words(), f"bloom words after the inserts, lanes={lanes}")
        _expect(dev.query_bulk(sig), host.query_bulk(sig), f"bloom query, lanes={lanes}")
        _expect(dev.query_insert_bulk(sig[300:]), host.query_insert_bulk(sig[300:]), f"bloom query then insert, lanes={lanes}")
        _expect(dev.words(), host.words(), f"bloom words after query then insert, lanes={lanes}")
        other = quiet(gpu_mode="always", **args)
        more = rng.randint(0, 2**32, size=(40, num_perm), dtype=np.uint64)
        other.insert_bulk(more)
        host.insert_bulk(more)
        dev.merge(other)
        _expect(dev.words(), host.words(), f"bloom words after a merge, lanes={lanes}")


def clusters_family(ctx):
    from tests import cc_guard_cases

    borrowed("cc_guard_cases.cases", cc_guard_cases.cases, ctx)
    sig, _ = _clustered(81, 3000, 1, 32, 400)
    for threshold in (None, 0.93):
        begin(f"duplicate_clusters threshold={threshold}")
        got = lsh_bulk.duplicate_clusters(sig, 8, 4, threshold=threshold, gpu_mode="always")
        want = lsh_bulk.duplicate_clusters(sig, 8, 4, threshold=threshold, gpu_mode="disable")
        _expect(got, want, f"duplicate_clusters threshold={threshold}")
        assert 1 < np.unique(want).size < 3000
    from datasketch_amd import MinHashLSH

    begin("MinHashLSH.duplicate_clusters")
    keys = [f"doc-{i}" for i in range(1500)]
    both = [MinHashLSH(num_perm=32, params=(8, 4), gpu_mode=mode) for mode in ("always", "disable")]
    for one in both:
        one.insert_bulk(keys, sig[:1500])
    got, want = (one.duplicate_clusters(0.93) for one in both)
    assert got == want and len(want) > 0


FAMILIES = {"minhash": minhash_family, "weighted": weighted_family, "pack_lsh": pack_lsh_family, "bucketing": bucketing_family,
            "queries": queries_family, "index": index_family, "forest": forest_family, "ensemble": ensemble_family, "jaccard": jaccard_family,
            "topk": topk_family, "hll": hll_family, "bloom": bloom_family, "clusters": clusters_family}


def control(byte):
    """The switch takes effect and can be taken back: a fresh allocation downloaded at once holds the byte; with poison off an
    uploaded buffer comes back as it went up."""
    assert byte >= 0, "the control needs a poison byte"
    ctx = _native.context()
    got = ctx.alloc(100).download(100, np.uint8)
    assert np.all(got == byte), f"a fresh allocation holds {np.unique(got).tolist()}, not {byte}"
    _native.poison_alloc(-1)
    data = np.arange(100, dtype=np.uint8)
    buf = ctx.alloc(100)
    buf.upload(data)
    assert np.array_equal(buf.download(100, np.uint8), data)
    print(f"POISON CONTROL OK (byte 0x{byte:02x})", flush=True)


def main():
    byte, family = int(sys.argv[1], 0), sys.argv[2]
    assert -1 <= byte <= 255 and byte != PATTERN
    assert "MHX_GUARD_ALLOC" not in os.environ, "guard pages stay off: this run is about contents, not extents"
    if byte >= 0:
        _native.poison_alloc(byte)  # before the first allocation of the process
    if family == "control":
        control(byte)
        return
    ctx = _native.context()
    _install(ctx)
    FAMILIES[family](ctx)
    ctx.synchronize()
    _FRESH()
    if G.FAILED:
        print(f"POISON FAILED: {G.FAILED} mismatching cases of {CASES + G.CASES}", flush=True)
        sys.exit(1)
    print(f"POISON OK {CASES + G.CASES} cases ({family}, byte {'off' if byte < 0 else '0x%02x' % byte})", flush=True)


if __name__ == "__main__":
    main()
