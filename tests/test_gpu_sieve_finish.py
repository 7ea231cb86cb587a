"""The sieve's finishes after their redundant work was taken out (csrc/minhash_kernels.hip: the short fold of a proven
candidate, tile rows beyond the block staged without a zero fill, the signature store with a scalar row address), bit
for bit against the C oracle and, for the crafted winners, flag for flag against the numpy model.

  crafted winners  sets whose smallest key under a permutation of the first / the last 64-lane slot is a chosen M
                   (tests/sieve_finish_model.py: winner_sets), every top = s >> 61 for uint64 tokens.  M in {16, 17, 31}: the
                   first launch settles the set (flag 0) wherever the model says the other permutations let it;
                   M in {0, 7, 15}: flagged.  M in {2^32 - 17, 2^32 - 1}: no key can lie 64, or even 32, above these (keys are
                   mod 2^32), so no proof accepts them -- the model says so and they come back flagged too.
  stale tile rows  4 096 sets of 16, 48, 250 and 272 tokens in one CSR call with blocks_per_cu = 1 (every wave walks
                   several sets; a block of 1 or 3 rows follows one of 15 or 16 in the same LDS tile), and each of the four
                   lengths as a fixed-length call (16, 48, 272: SHAPE_PLAIN_FIXED_ROWS; 250: SHAPE_PLAIN_FIXED), through
                   every kernel family: two, three and four permutations per lane,
                   the shared last slot, the packed kernel, both token and output widths, the tie-tolerant first launch
                   after the context has learned it, and the dedup launch on a corpus with 10 % repeated tokens.
  store path       with and without an initial state, empty sets, K = 100 and 136 (lanes of the last slot without a
                   permutation must not store: checked with canaries behind every row and a poisoned output).

Run on an MI355X:  python -m pytest tests/test_gpu_sieve_finish.py -m gpu -q -s
"""
import functools

import numpy as np
import pytest

from datasketch_amd import _native
from oracle import oracle as O
from tests import sieve_finish_model as F
from tests.learned_launch_cases import N_TEACH, initial_state, teaching_prototypes, tiled

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
OPTIONS = ("minhash.split", "minhash.adapt", "minhash.packed", "minhash.ties", "blocks_per_cu")
POISON = 0xA5


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    c = _native.context()
    c.set_option("minhash.split", 1)   # one wave per set: small corpora would go to the split kernels otherwise
    try:
        yield c
    finally:
        for key in OPTIONS:
            c.set_option(key, 0)
        c.minhash_mode(reset=True)


@functools.lru_cache(maxsize=None)
def perms(k):
    return tuple(O.np_init_permutations(k, 4))


def dtype_code(dt):
    return _native.MHX_U32 if dt == U32 else _native.MHX_U64


def run(ctx, k, hv, off, fixed_len, n, tok_dtype, out_dtype, init=None, canary=0):
    """One minhash_bulk_dev call: (signatures as uint64 [n, k], flags, the bytes behind the output).  The output buffer is
    poisoned first and `canary` bytes longer than the signatures."""
    a, b = perms(k)
    item = np.dtype(out_dtype).itemsize
    d_hv = ctx.to_device(hv.astype(tok_dtype))
    d_off = None if off is None else ctx.to_device(off)
    d_init = None if init is None else ctx.to_device(init)
    d_out = ctx.to_device(np.full(n * k * item + canary, POISON, np.uint8))
    ctx.minhash_bulk_dev((a, b), d_hv.ptr, dtype_code(tok_dtype), None if d_off is None else d_off.ptr, fixed_len, n, hv.size,
                         None if d_init is None else d_init.ptr, k if d_init is not None else 0, d_out.ptr, dtype_code(out_dtype))
    flags = ctx.minhash_flags(n)
    raw = d_out.download((n * k * item + canary,), np.uint8)
    return raw[:n * k * item].view(out_dtype).reshape(n, k).astype(U64), flags, raw[n * k * item:]


def differing(got, want):
    return f"rows differing: {np.flatnonzero((got != want).any(axis=1))[:10].tolist()}"


# ---------------------------------------------------------------------------------------------- a. crafted winners
class Winners:
    def __init__(self, k, wide):
        a, b = perms(k)
        self.tok, self.m, self.perm, self.top = F.winner_sets(a, b, wide)
        self.n = len(self.tok)
        self.want = O.c_minhash_bulk_dense(self.tok, a, b)
        self.settled = F.one_candidate_settles(list(self.tok), a, b)
        for arr in (self.tok, self.want, self.settled):
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def winners(k, wide):
    return Winners(k, wide)


@pytest.mark.parametrize("form", ["rows", "csr"])
@pytest.mark.parametrize("k,tok_dtype,out_dtype", [(128, U64, U64), (128, U32, U32), (256, U64, U64), (136, U64, U32), (64, U64, U64)],
                         ids=["k128", "k128_tok32_out32", "k256_four", "k136_shared_out32", "k64_packed"])
def test_crafted_winners(ctx, k, tok_dtype, out_dtype, form):
    """Signatures equal the oracle; flag 0 for every M in {16, 17, 31} set that the model says the first launch settles
    (most of them: asserted), flag >= 1 for every M < 16 and for every set the model says is not settled.  A wave walks one
    set here (a few hundred sets), so no back-off flags a settled set."""
    w = winners(k, tok_dtype == U64)
    if form == "rows":
        got, flags, _ = run(ctx, k, w.tok.reshape(-1), None, F.WINNER_T, w.n, tok_dtype, out_dtype)
    else:
        off = np.arange(w.n + 1, dtype=np.int64) * F.WINNER_T
        got, flags, _ = run(ctx, k, w.tok.reshape(-1), off, 0, w.n, tok_dtype, out_dtype)
    settled_kind = np.isin(w.m, F.SETTLED_M)
    print(f"[finish] winners k={k} {form}: {w.n} sets; settled kinds {int(settled_kind.sum())}, of them settled by the model "
          f"{int((settled_kind & w.settled).sum())}; flags 0/1/2: {np.bincount(flags, minlength=3).tolist()}")
    assert np.array_equal(got, w.want), differing(got, w.want)
    assert (settled_kind & w.settled).sum() >= 0.9 * settled_kind.sum()
    assert not w.settled[~settled_kind].any()   # the guard and the keys next to 2^32: the model refuses every one
    assert (flags[settled_kind & w.settled] == 0).all()
    assert (flags[np.isin(w.m, F.GUARDED_M)] >= 1).all()
    assert (flags[~w.settled] >= 1).all()


# ---------------------------------------------------------------------------------------------- b. stale tile rows
class Mixed:
    """The mixed-length corpus and its oracle per (K, token width, repeats); computed once, never changed."""

    def __init__(self, k, wide, repeats):
        a, b = perms(k)
        sets = F.mixed_length_sets(wide, repeats=repeats)
        self.n = len(sets)
        self.hv, self.off = F.csr(sets)
        self.want = O.c_minhash_bulk(self.hv, self.off, a, b, None)
        for arr in (self.hv, self.off, self.want):
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def mixed(k, wide, repeats=0.0):
    return Mixed(k, wide, repeats)


class Teacher:
    def __init__(self, ctx):
        self.ctx, self.perms = ctx, perms(128)
        protos = teaching_prototypes(*self.perms, "one_tie")
        self.d_tok = ctx.to_device(tiled(protos))
        self.want = tiled(O.c_minhash_bulk_dense(protos, *self.perms))
        self.d_sig = ctx.alloc(N_TEACH * 128 * 8)

    def teach(self):
        self.ctx.minhash_bulk_dev(self.perms, self.d_tok.ptr, _native.MHX_U64, None, 256, N_TEACH, N_TEACH * 256, None, 0, self.d_sig.ptr,
                                  _native.MHX_U64)
        assert np.array_equal(self.d_sig.download((N_TEACH, 128), U64), self.want)
        return self.ctx.minhash_mode()


@pytest.fixture(scope="module")
def teacher(ctx):
    return Teacher(ctx)


STALE_CELLS = [
    ("k128", 128, U64, U64), ("k128_tok32", 128, U32, U64), ("k128_out32", 128, U64, U32), ("k128_tok32_out32", 128, U32, U32),
    ("k136_shared", 136, U64, U64), ("k136_shared_tok32", 136, U32, U64), ("k200_shared", 200, U64, U64), ("k256_four", 256, U64, U64),
    ("k256_tok32", 256, U32, U64), ("k96_packed", 96, U64, U64), ("k48_packed_tok32", 48, U32, U32),
]


@pytest.mark.parametrize("cell", STALE_CELLS, ids=[c[0] for c in STALE_CELLS])
def test_short_blocks_after_long_ones(ctx, cell):
    """The CSR call over the mixed lengths with one workgroup per compute unit."""
    name, k, tok_dtype, out_dtype = cell
    cs = mixed(k, tok_dtype == U64)
    ctx.set_option("blocks_per_cu", 1)
    try:
        got, flags, _ = run(ctx, k, cs.hv, cs.off, 0, cs.n, tok_dtype, out_dtype)
    finally:
        ctx.set_option("blocks_per_cu", 0)
    print(f"[finish] mixed {name}: flags 0/1/2: {np.bincount(flags, minlength=3).tolist()}")
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert (flags == 0).mean() > 0.9   # the first launch did the work


class Fixed:
    """4 096 sets of one length t and their oracle per (K, token width, repeats); computed once, never changed."""

    def __init__(self, k, wide, t, repeats):
        a, b = perms(k)
        rng = np.random.RandomState(1000 + t)
        self.tok = rng.randint(0, 2**32, (F.MIXED_N, t), dtype=U64)
        if wide:
            self.tok |= rng.randint(0, 2**32, self.tok.shape, dtype=U64) << U64(32)
        if repeats:
            for row in self.tok:
                for dst in rng.choice(t, max(1, int(t * repeats)), replace=False):
                    row[dst] = row[rng.randint(0, t)]
        self.n, self.t = len(self.tok), t
        self.want = O.c_minhash_bulk_dense(self.tok, a, b)
        for arr in (self.tok, self.want):
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def fixed(k, wide, t, repeats=0.0):
    return Fixed(k, wide, t, repeats)


@pytest.mark.parametrize("t", F.MIXED_LENGTHS)
@pytest.mark.parametrize("cell", STALE_CELLS, ids=[c[0] for c in STALE_CELLS])
def test_fixed_lengths(ctx, cell, t):
    """The same cells on fixed-length sets of 16 (one row: every row of the tile but row 0 is stale), 48, 250 (15 rows and a
    ragged tail: SHAPE_PLAIN_FIXED) and 272 tokens (a block of 16 rows, then one of 1 in the same tile); 16, 48 and 272 run
    the whole-row kernels (SHAPE_PLAIN_FIXED_ROWS)."""
    name, k, tok_dtype, out_dtype = cell
    cs = fixed(k, tok_dtype == U64, t)
    ctx.set_option("blocks_per_cu", 1)
    try:
        got, flags, _ = run(ctx, k, cs.tok.reshape(-1), None, t, cs.n, tok_dtype, out_dtype)
    finally:
        ctx.set_option("blocks_per_cu", 0)
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert (flags == 0).mean() > 0.9


@pytest.mark.parametrize("t", [0, 16, 250, 272], ids=["csr_mixed", "fixed16", "fixed250", "fixed272"])
@pytest.mark.parametrize("k,tok_dtype", [(128, U64), (200, U64), (136, U32)], ids=["k128", "k200_shared", "k136_shared_tok32"])
def test_learned_tie_tolerant_first_launch(ctx, teacher, k, tok_dtype, t):
    """Mode word 1 (taught by a corpus whose sets all tie once): MODE_SIEVE_TIES walks the mixed lengths in one CSR call, or
    fixed lengths of 16, 250 and 272 tokens, every set with one token occurring twice.  With a single row in a block the
    second row that finish_block_ties reads is a stale one -- read, but used only under row_tie, which needs the record's
    2^32-1 within 32 of the best key's base: about 2^-27 per lane, so no corpus here reaches that use.  That a stale
    second row cannot matter rests on the argument in sieve_range (the proof has failed before the row is consulted); what
    these cases check is everything else that reads the tile in this launch."""
    wide = tok_dtype == U64
    try:
        assert teacher.teach() == 1   # (with its default grid: one workgroup per unit publishes too few tries to write the word)
        ctx.set_option("blocks_per_cu", 1)
        if t == 0:
            cs = mixed(k, wide, 0.004)   # (0.4 % of at most 272 tokens: one copy per set)
            got, flags, _ = run(ctx, k, cs.hv, cs.off, 0, cs.n, tok_dtype, U64)
        else:
            cs = fixed(k, wide, t, 0.004)
            got, flags, _ = run(ctx, k, cs.tok.reshape(-1), None, t, cs.n, tok_dtype, U64)
    finally:
        ctx.set_option("blocks_per_cu", 0)
        ctx.minhash_mode(reset=True)
    print(f"[finish] learned k={k} t={t}: flags 0/1/2: {np.bincount(flags, minlength=3).tolist()}")
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert (flags == 0).mean() > 0.5   # the tie-tolerant launch settles what a one-candidate launch could not


@pytest.mark.parametrize("t", [0, 48, 250], ids=["csr_mixed", "fixed48", "fixed250"])
@pytest.mark.parametrize("k,tok_dtype", [(128, U64), (128, U32), (256, U64)], ids=["k128", "k128_tok32", "k256"])
def test_dedup_launch_on_repeats(ctx, k, tok_dtype, t):
    """10 % of every set's tokens repeat: the first launch flags nearly every set and, with minhash.ties = 1, the second
    launch is the dedup pass alone (finish_block in its PARTIAL form over the compacted tile).  The mixed lengths in one
    CSR call, and fixed lengths of 48 and 250 tokens."""
    cs = mixed(k, tok_dtype == U64, 0.1) if t == 0 else fixed(k, tok_dtype == U64, t, 0.1)
    ctx.set_option("blocks_per_cu", 1)
    ctx.set_option("minhash.ties", 1)
    ctx.set_option("minhash.adapt", 1)
    try:
        if t == 0:
            got, flags, _ = run(ctx, k, cs.hv, cs.off, 0, cs.n, tok_dtype, U64)
        else:
            got, flags, _ = run(ctx, k, cs.tok.reshape(-1), None, t, cs.n, tok_dtype, U64)
    finally:
        for key in ("blocks_per_cu", "minhash.ties", "minhash.adapt"):
            ctx.set_option(key, 0)
    print(f"[finish] repeats k={k}: flags 0/1/2: {np.bincount(flags, minlength=3).tolist()}")
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert (flags >= 1).mean() > 0.5 and (flags == 1).sum() > (flags == 2).sum()


# ---------------------------------------------------------------------------------------------- c. the store
@pytest.mark.parametrize("state", [False, True], ids=["plain", "state"])
@pytest.mark.parametrize("out_dtype", [U64, U32], ids=["out64", "out32"])
@pytest.mark.parametrize("k", [100, 128, 136, 200])
def test_store_path(ctx, k, out_dtype, state):
    """Sets of 0, 16, 33 and 64 tokens in one CSR call (and the non-empty ones as a fixed-length call when there is no
    state): an empty set's row is 2^32 - 1 or its state; nothing is written behind a row's K values (K = 100: 28 lanes of
    the second slot hold no permutation) -- every row is checked against the oracle and 256 canary bytes follow the last."""
    a, b = perms(k)
    rng = np.random.RandomState(k)
    lens = np.tile([0, 16, 33, 64, 0, 64], 100)
    sets = [rng.randint(0, 2**32, t, dtype=U64) | (rng.randint(0, 2**32, t, dtype=U64) << U64(32)) for t in lens]
    hv, off = F.csr(sets)
    init = initial_state(len(sets), k) if state else None
    want = O.c_minhash_bulk(hv, off, a, b, init)
    if out_dtype == U32:
        want = np.minimum(want, U64(0xFFFFFFFF))
    got, flags, behind = run(ctx, k, hv, off, 0, len(sets), U64, out_dtype, init=init, canary=256)
    assert np.array_equal(got, want), differing(got, want)
    assert (behind == POISON).all()
    empty = lens == 0
    assert (flags[empty] == 0).all()
    if state:
        assert np.array_equal(got[empty], np.minimum(init[empty], U64(0xFFFFFFFF)) if out_dtype == U32 else init[empty])
    else:
        assert (got[empty] == 0xFFFFFFFF).all()
        full = np.stack([s for s in sets if len(s) == 64])
        got2, _, behind2 = run(ctx, k, full.reshape(-1), None, 64, len(full), U64, out_dtype, canary=256)
        assert np.array_equal(got2, want[lens == 64]), differing(got2, want[lens == 64])
        assert (behind2 == POISON).all()
