"""The first launch that a context has LEARNED (csrc/minhash_kernels.hip: MODE_SIEVE_TIES, the tie-tolerant proof of
finish_block_ties, chosen on the device from the context's mode word) in every kernel shape it is compiled into, bit
for bit against the C oracle and flag for flag against the numpy model of the proof (tests/sieve_ties_model.py).

Every cell runs its corpus (tests/learned_launch_cases.py: clean sets, one tie, two close keys, triples, three close
keys, rows of keys just below 2^32, every crafted alias / near pair / wrap / guard base, for a permutation of the first and of the last 64-permutation slot)
twice: in mode 1, taught by one K = 128 call over 8 192 sets that all tie once, and after a reset in mode 0.  In mode 1
the flags equal the model's verdict set by set -- the tie-tolerant launch never skips a set -- and every one_tie set has
flag 0; in mode 0 every one_tie set has a flag >= 1.  That difference is the proof that the cell's MODE_SIEVE_TIES
instantiation did the work; each test prints the two counts.

Forms: `rows` fixed 256 tokens (SHAPE_PLAIN_FIXED_ROWS); `ragged` CSR sets of 16 r + tail tokens, empty, one-token and
two- and three-block sets included (SHAPE_GENERAL); `state` fixed 250 tokens with an [n, K] initial state (SHAPE_GENERAL).
The model covers every set of all three forms: whole rows through the proof, the tail through the fast fold's own
"minimum <= 7" test (first_launch_model).

Run on an MI355X:  python -m pytest tests/test_gpu_learned_first_launch.py -m gpu -q -s
"""
import functools

import numpy as np
import pytest

from datasketch_amd import MinHash, _native
from oracle import oracle as O
from tests import learned_launch_cases as C
from tests.sieve_ties_model import first_launch_model

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
OPTIONS = ("minhash.split", "minhash.adapt", "minhash.packed", "minhash.share", "host.chunk_bytes")


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    c = _native.context()
    c.set_option("minhash.split", 1)  # one wave per set: these small corpora would go to the split kernels otherwise
    c.set_option("minhash.adapt", 0)  # the device-side choice of the first launch: what is under test
    try:
        yield c
    finally:
        for key in OPTIONS:
            c.set_option(key, 0)
        c.minhash_mode(reset=True)


# ---------------------------------------------------------------------------------------------- teaching
class Teacher:
    """The three teaching corpora on the device: N_PROTO prototype sets of 256 tokens tiled to N_TEACH rows; the oracle runs
    on the prototypes only.  teach() is one K = 128 call and checks its signatures like any other call."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.perms = tuple(O.np_init_permutations(128, 4))
        self.d_tok, self.want = {}, {}
        for kind in ("clean", "one_tie", "triple"):
            protos = C.teaching_prototypes(*self.perms, kind)
            self.d_tok[kind] = ctx.to_device(C.tiled(protos))
            self.want[kind] = C.tiled(O.c_minhash_bulk_dense(protos, *self.perms))
        self.d_sig = ctx.alloc(C.N_TEACH * 128 * 8)

    def teach(self, kind, n=C.N_TEACH):
        self.ctx.minhash_bulk_dev(self.perms, self.d_tok[kind].ptr, _native.MHX_U64, None, 256, n, n * 256, None, 0, self.d_sig.ptr,
                                  _native.MHX_U64)
        assert np.array_equal(self.d_sig.download((n, 128), U64), self.want[kind][:n]), f"teaching call ({kind})"
        return self.ctx.minhash_mode()


@pytest.fixture(scope="module")
def teacher(ctx):
    return Teacher(ctx)


# ---------------------------------------------------------------------------------------------- corpora, built once
class Case:
    """A corpus in the form the device call takes it, its oracle and the model's verdict; computed once, never changed."""

    def __init__(self, k, wide, form):
        self.a, self.b = O.np_init_permutations(k, 4)
        self.init = None
        if form in ("ragged", "ragged_state"):
            sets, self.kinds = C.ragged_cases(self.a, self.b, wide)
            self.hv, self.off = C.csr(sets)
            self.fixed_len = 0
            if form == "ragged_state":
                self.init = C.initial_state(len(sets), k)
        else:
            t = 256 if form == "rows" else 250
            tok, self.kinds = C.fixed_cases(self.a, self.b, t, wide)
            sets, self.hv, self.off, self.fixed_len = list(tok), tok.reshape(-1), None, t
            if form == "state":
                self.init = C.initial_state(len(tok), k)
        self.n = len(sets)
        off = np.arange(self.n + 1, dtype=np.int64) * self.fixed_len if self.off is None else self.off
        self.want = O.c_minhash_bulk(self.hv, off, self.a, self.b, self.init)
        self.settled = first_launch_model(sets, self.a, self.b)
        for arr in (self.hv, self.want, self.settled, self.kinds):
            arr.setflags(write=False)


@functools.lru_cache(maxsize=None)
def case(k, wide, form):
    return Case(k, wide, form)


def run(ctx, cs, tok_dtype, out_dtype):
    """One minhash_bulk_dev call on the case: (signatures as uint64, flags)."""
    k = len(cs.a)
    d_hv = ctx.to_device(cs.hv.astype(tok_dtype))
    d_off = None if cs.off is None else ctx.to_device(cs.off)
    d_init = None if cs.init is None else ctx.to_device(cs.init)
    d_out = ctx.alloc(cs.n * k * np.dtype(out_dtype).itemsize)
    ctx.minhash_bulk_dev((cs.a, cs.b), d_hv.ptr, _native.MHX_U32 if tok_dtype == U32 else _native.MHX_U64,
                         None if d_off is None else d_off.ptr, cs.fixed_len, cs.n, cs.hv.size, None if d_init is None else d_init.ptr,
                         k if d_init is not None else 0, d_out.ptr, _native.MHX_U32 if out_dtype == U32 else _native.MHX_U64)
    flags = ctx.minhash_flags(cs.n)
    return d_out.download((cs.n, k), out_dtype).astype(U64), flags


def expected(cs, out_dtype):
    """The oracle's signatures as the output type holds them: an initial value >= 2^32 that survives (it lost to no hash: an
    empty set, test_empty_sets_keep_their_state) is clamped to 2^32 - 1 in uint32 output."""
    return np.minimum(cs.want, U64(0xFFFFFFFF)) if out_dtype == U32 else cs.want


def differing(got, want):
    return f"rows differing: {np.flatnonzero((got != want).any(axis=1))[:10].tolist()}"


# ---------------------------------------------------------------------------------------------- a. every instantiation
# (id, K, option, token type, output type): see the table in the docstring of test_every_instantiation
CELLS = [
    ("k64_one_per_lane", 64, "minhash.packed", U64, U64),
    ("k96_two_half_empty_slot_out32", 96, "minhash.packed", U64, U32),
    ("k128_two", 128, None, U64, U64),
    ("k128_two_tok32", 128, None, U32, U64),
    ("k128_two_out32", 128, None, U64, U32),
    ("k128_two_tok32_out32", 128, None, U32, U32),
    ("k136_three_shared_8", 136, None, U64, U64),
    ("k136_three_shared_8_tok32_out32", 136, None, U32, U32),
    ("k136_three_unshared", 136, "minhash.share", U64, U64),
    ("k160_three_shared_32", 160, None, U64, U64),
    ("k192_three_all_lanes", 192, None, U64, U64),
    ("k200_four_shared_8", 200, None, U64, U64),
    ("k224_four_shared_32_out32", 224, None, U64, U32),
    ("k256_four", 256, None, U64, U64),
    ("k256_two_twice_tok32", 256, None, U32, U64),
    ("k300_three_twice", 300, None, U64, U64),
    ("k300_three_twice_tok32_out32", 300, None, U32, U32),
    ("k576_three_thrice", 576, None, U64, U64),
    ("k600_two_five_times", 600, None, U64, U64),
]


@pytest.mark.parametrize("form", ["rows", "ragged", "state"])
@pytest.mark.parametrize("cell", CELLS, ids=[c[0] for c in CELLS])
def test_every_instantiation(ctx, teacher, cell, form):
    """minhash_bulk_kernel<P, TokT, OutT, MODE_SIEVE_TIES, shape, SHARE> by cell and form:
      K 64 / 96 with minhash.packed = 1: one per lane; two with a half-empty second slot.   K 128: two per lane, all four
      token / output types.   K 136 / 160: three, the last slot (8 / 32 permutations) shared among lane groups -- Three records
      through share_last_slot -- and K 136 with minhash.share = 1: not shared.   K 192: three, every lane.   K 200 / 224:
      four, shared (8 / 32).   K 256: four; with uint32 tokens two per lane in two passes.   K 300: three, two passes
      (never shared).   K 576: three, three passes.   K 600: two, five passes.
    `rows` is SHAPE_PLAIN_FIXED_ROWS; `ragged` and `state` are SHAPE_GENERAL."""
    name, k, option, tok_dtype, out_dtype = cell
    cs = case(k, tok_dtype == U64, form)
    want = expected(cs, out_dtype)
    kinds = cs.kinds
    one_tie = kinds == "one_tie"
    if option:
        ctx.set_option(option, 1)
    try:
        assert teacher.teach("one_tie") == 1
        assert ctx.minhash_mode() == 1
        got1, flags1 = run(ctx, cs, tok_dtype, out_dtype)
        assert ctx.minhash_mode(reset=True) == 1  # (a few hundred sets publish fewer than 64 tries: the word stays)
        assert ctx.minhash_mode() == 0
        got0, flags0 = run(ctx, cs, tok_dtype, out_dtype)
    finally:
        if option:
            ctx.set_option(option, 0)
        ctx.minhash_mode(reset=True)
    print(f"[learned] {name} {form}: {cs.n} sets; one_tie {int(one_tie.sum())}: flag 0 in mode 1: {int((flags1[one_tie] == 0).sum())}, "
          f"flag >= 1 in mode 0: {int((flags0[one_tie] >= 1).sum())}; mode 1 flags 0/1/2: {np.bincount(flags1, minlength=3).tolist()}, "
          f"mode 0: {np.bincount(flags0, minlength=3).tolist()}")
    # mode 1: the tie-tolerant first launch
    assert np.array_equal(got1, want), differing(got1, want)
    assert set(np.unique(flags1).tolist()) <= {0, 1, 2}
    # the launch never skips a set (the back-off is the one-candidate launch's): flag 0 exactly where the model's proof accepts
    # every block for every permutation (and the tail's fast fold asks for no redo)
    assert np.array_equal(flags1 == 0, cs.settled), f"sets the model and the launch disagree on: {np.flatnonzero((flags1 == 0) != cs.settled)[:10].tolist()}"
    assert (flags1[kinds == "triple"] >= 1).all()
    assert (flags1[kinds == "three_close"] == 2).all()
    assert one_tie.sum() >= 8 and (flags1[one_tie] == 0).all()
    # mode 0: the one-candidate proof first; a tie defeats it (and a wave's back-off may flag more sets, never fewer)
    assert np.array_equal(got0, want), differing(got0, want)
    assert set(np.unique(flags0).tolist()) <= {0, 1, 2}
    assert (flags0[one_tie] >= 1).all()
    assert (flags0[~cs.settled] >= 1).all()  # what defeats the tie-tolerant proof defeats the one-candidate proof


@pytest.mark.parametrize("out_dtype", [U64, U32], ids=["out64", "out32"])
def test_empty_sets_keep_their_state(ctx, teacher, out_dtype):
    """The ragged corpus with an [n, K] initial state, K = 128, in mode 1: an empty set's row is its state -- values >= 2^32
    as they are in uint64 output, clamped to 2^32 - 1 in uint32 output -- and the flags are the model's as without a state."""
    cs = case(128, True, "ragged_state")
    empty = np.diff(cs.off) == 0
    assert empty.sum() >= 3 and (cs.init[empty] >= 2**32).any() and (cs.want[empty] == cs.init[empty]).all()
    try:
        assert teacher.teach("one_tie") == 1
        got, flags = run(ctx, cs, U64, out_dtype)
        assert ctx.minhash_mode() == 1
    finally:
        ctx.minhash_mode(reset=True)
    want = expected(cs, out_dtype)
    assert np.array_equal(got, want), differing(got, want)
    assert (got[empty].max() > 0xFFFFFFFF) == (out_dtype == U64)
    assert np.array_equal(flags == 0, cs.settled)


# ---------------------------------------------------------------------------------------------- b. the packed kernels
@pytest.mark.parametrize("k", [16, 48])
def test_packed_kernels_ignore_the_word(ctx, teacher, k):
    """K <= 96 with default options: minhash_packed_kernel is the first launch whatever the word says -- the one-candidate
    proof, so a tie is flagged in mode 1 too -- and the results are exact."""
    cs = case(k, True, "rows")
    one_tie = cs.kinds == "one_tie"
    try:
        assert teacher.teach("one_tie") == 1
        got, flags = run(ctx, cs, U64, U64)
        assert ctx.minhash_mode() == 1
    finally:
        ctx.minhash_mode(reset=True)
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert set(np.unique(flags).tolist()) <= {0, 1, 2}
    assert one_tie.sum() >= 8 and (flags[one_tie] >= 1).all()


# ---------------------------------------------------------------------------------------------- c. mode 2
@pytest.mark.parametrize("k", [128, 136, 256])
def test_mode_two_runs_the_one_candidate_launch(ctx, teacher, k):
    """Taught by triples the word reads 2: MODE_SIEVE first again, the second launch's own tie attempt on."""
    cs = case(k, True, "rows")
    one_tie = cs.kinds == "one_tie"
    try:
        assert teacher.teach("triple") == 2
        got, flags = run(ctx, cs, U64, U64)
        assert ctx.minhash_mode() == 2
    finally:
        ctx.minhash_mode(reset=True)
    assert np.array_equal(got, cs.want), differing(got, cs.want)
    assert set(np.unique(flags).tolist()) <= {0, 1, 2}
    assert (flags[one_tie] >= 1).all() and (flags[cs.kinds == "three_close"] == 2).all()


# ---------------------------------------------------------------------------------------------- d. the transition rule
def test_the_word_follows_the_rule(ctx, teacher):
    """The MODE_FULL prologue (minhash_kernels.hip, "the last launch of the call"), from the counts the launches publish:
    t tries of the sampled first-launch waves, f of them "failed", g left unsettled by a tie-tolerant first launch, tt / tf
    the second launch's own tie attempts and failures.  Nothing is written unless t >= 64.  defeated = 4 f > t;
    heavy = 5 g > t in mode 1; otherwise 5 tf > tt when tt >= 64, and "the word was 2" when the second launch published fewer
    than 64 attempts; word = !defeated ? 0 : heavy ? 2 : 1.  Every set of a teaching corpus is of one kind, so the ratios
    are 0 or 1 -- given t >= 64 and tt >= 64.  t: 8 192 sets are 2 048 workgroups of which every 16th publishes its first
    wave's one try, 128, on a device that holds them all at once (a wave that starts after 64 failures were published
    skips and publishes nothing: t stays at 64 or more).  tt: every wave of the second launch publishes, two attempts
    each before its back-off on triples, all of its sets on one_tie: hundreds.  On a much smaller device (fewer resident
    workgroups) a step that fails here should be read against those two counts first.
      clean    f = 0                                   -> 0
      one_tie  f = t; g = 0 (mode 1) or tf = 0         -> 1
      triple   f = t; g = t (mode 1) or tf = tt        -> 2
    whatever the word was before.  Derived from the code, not measured."""
    steps = [("clean", 0), ("one_tie", 1), ("one_tie", 1), ("triple", 2), ("one_tie", 1), ("triple", 2), ("clean", 0), ("triple", 2),
             ("clean", 0)]
    try:
        ctx.minhash_mode(reset=True)
        assert ctx.minhash_mode() == 0
        for i, (kind, want) in enumerate(steps):
            assert teacher.teach(kind) == want, f"step {i}: {kind} after {steps[:i]}"
    finally:
        ctx.minhash_mode(reset=True)


def test_small_and_counted_calls_leave_the_word(ctx, teacher):
    """200 sets: 50 workgroups, 4 of which publish one try each -- fewer than 64, the word is not rewritten, whatever it was
    and whatever the sets would say.  A counted call has no mode word at all: it runs the one-candidate launch (every tied
    set is redone) and writes nothing."""
    n = C.N_TEACH
    try:
        for kind, mode, small in (("clean", 0, "triple"), ("one_tie", 1, "clean"), ("triple", 2, "clean")):
            ctx.minhash_mode(reset=True)
            assert teacher.teach(kind) == mode
            assert teacher.teach(small, n=200) == mode
            ctx.counters(True)
            try:
                assert teacher.teach("one_tie") == mode
            finally:
                c = ctx.counters(False)
            assert c["sieve_sets_redone"] == n, c  # MODE_SIEVE flagged every set; MODE_SIEVE_TIES would have settled them all
            assert ctx.minhash_mode() == mode
    finally:
        ctx.counters(False)
        ctx.minhash_mode(reset=True)


# ---------------------------------------------------------------------------------------------- e. where users meet it
def test_pipelined_host_call_in_mode_one(ctx, teacher):
    """mhx_minhash_bulk in pieces of 4 KiB -- a few sets per device call -- on a ragged corpus where most sets tie once."""
    cs = case(128, True, "ragged")
    every = [cs.hv[cs.off[i]:cs.off[i + 1]] for i in range(cs.n)]
    ties = [s for s, kind in zip(every, cs.kinds) if kind.startswith("one_tie")]
    sets = every[::4] + ties * 8   # (a quarter of the corpus: some 2 000 sets, most of them with a tie, in about 800 pieces)
    hv, off = C.csr(sets)
    want = np.concatenate([cs.want[::4]] + [O.c_minhash_bulk(*C.csr(ties), cs.a, cs.b)] * 8)
    ctx.set_option("host.chunk_bytes", 4096)
    try:
        assert teacher.teach("one_tie") == 1
        got = ctx.minhash_bulk((cs.a, cs.b), hv, off, 0, len(sets))
        assert ctx.minhash_mode() == 1
    finally:
        ctx.set_option("host.chunk_bytes", 0)
        ctx.minhash_mode(reset=True)
    assert np.array_equal(got, want), differing(got, want)


def test_repetitive_text_twice(ctx):
    """8 192 short documents that repeat a five-word phrase: every 5-word shingle occurs several times in its set, so
    the first call teaches the process-wide context and the second one starts from what it learned.  Both equal the host
    arithmetic (gpu_mode='disable'), computed once on the 64 distinct documents."""
    rng = np.random.RandomState(17)
    words = ["alpha", "beta", "gamma", "delta", "epsilon", "zeta", "eta", "theta", "iota", "kappa", "lambda", "mu"]
    protos = [" ".join(list(rng.choice(words, 5, replace=False)) * 10) + f" doc{i}" for i in range(C.N_PROTO)]
    docs = protos * (C.N_TEACH // C.N_PROTO)
    kw = dict(shingle=5, words=True, num_perm=136)
    want = np.tile(MinHash.bulk_signatures(documents=protos, gpu_mode="disable", **kw), (C.N_TEACH // C.N_PROTO, 1))
    try:
        ctx.minhash_mode(reset=True)
        first = MinHash.bulk_signatures(documents=docs, gpu_mode="always", **kw)
        mode = _native.context().minhash_mode()
        second = MinHash.bulk_signatures(documents=docs, gpu_mode="always", **kw)
    finally:
        ctx.minhash_mode(reset=True)
    assert mode in (1, 2), mode
    assert np.array_equal(first, want), differing(first, want)
    assert np.array_equal(second, want), differing(second, want)
