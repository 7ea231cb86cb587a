"""The sieve's rescan of the best row (finish_block in csrc/minhash_kernels.hip: the two smallest tagged keys from a
min3/med3 network), through every kernel it is compiled into, bit for bit against the C oracle.

The crafted sets come from tests/sieve_rescan_model.py: tokens built through the modular inverse of an odd a_lo so
that, for one permutation, the bottom of the hash range holds two keys d apart inside a row or across a row boundary, a
key a multiple of 2^28 above the minimum, or a minimum where the exact value wraps / the smallest key is below 16.
Whatever the proof decides, the signatures must equal the oracle's.

Run on an MI355X:  python -m pytest tests/test_gpu_sieve_rescan.py -m gpu -q
"""
import numpy as np
import pytest

from datasketch_amd import _native
from oracle import oracle as O
from tests.sieve_rescan_model import NEAR_D, crafted_sets, odd_perms, sieve_model, token_for

pytestmark = pytest.mark.gpu

# what the numpy model of the proof flags on the 20 000 random sets of test_flag_rate_on_random_sets (seed 11, permutation
# seed 1), computed on the CPU with sieve_model: 10 sets (10 failed proofs)
MODEL_FLAGGED_SEED_11 = 10


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    c = _native.context()
    # one wave per set (these corpora are small enough for the split kernels otherwise), and the one-candidate proof as
    # the first launch whatever the previous corpus was: the launches under test
    c.set_option("minhash.split", 1)
    c.set_option("minhash.adapt", 1)
    yield c
    for key in ("minhash.split", "minhash.adapt", "minhash.packed", "minhash.share"):
        c.set_option(key, 0)


@pytest.fixture(scope="module")
def headline():
    """(a, b, tok, want) of the K = 128 crafted corpus, shared by the tests that use it."""
    a, b = O.np_init_permutations(128, 4)
    tok = crafted_sets(a, b, 256, n_perms=3)
    return a, b, tok, O.c_minhash_bulk_dense(tok, a, b)


def test_two_per_lane_uint64(ctx, headline):
    """K = 128, 256 tokens: the headline kernel.  Every set on which the model's proof fails is flagged by the first
    launch (a wave that has just seen failures may flag more without trying: its back-off), and it settles some itself."""
    a, b, tok, want = headline
    n = len(tok)
    got = ctx.minhash_bulk((a, b), tok.reshape(-1), None, 256, n)
    flags = ctx.minhash_flags(n)
    assert np.array_equal(got, want)
    ok, _ = sieve_model(tok, a, b)
    assert (flags[~ok.all(axis=1)] >= 1).all()
    assert 0 < (flags == 0).sum() < n


def test_two_per_lane_uint32(ctx):
    a, b = O.np_init_permutations(128, 4)
    tok = crafted_sets(a, b, 256, n_perms=2, wide=False)
    got = ctx.minhash_bulk((a, b), tok.reshape(-1).astype(np.uint32), None, 256, len(tok))
    assert np.array_equal(got, O.c_minhash_bulk_dense(tok, a, b))


@pytest.mark.parametrize("k, option", [(256, None), (136, None), (136, "minhash.share"), (64, "minhash.packed"), (48, None)],
                         ids=["four_per_lane_k256", "three_shared_k136", "three_unshared_k136", "one_per_lane_k64", "packed_k48"])
def test_other_kernels(ctx, k, option):
    """Four permutations per lane; three with the last slot's rows shared among lane groups (and not); one per lane with
    the packed kernels switched off; the packed kernel (several sets per wave, partial rows masked)."""
    a, b = O.np_init_permutations(k, 4)
    perms = odd_perms(a, k)
    tok = crafted_sets(a, b, 256, perms=[perms[0], perms[-1]])  # a permutation of the first slot and one of the last
    want = O.c_minhash_bulk_dense(tok, a, b)
    if option:
        ctx.set_option(option, 1)
    try:
        got = ctx.minhash_bulk((a, b), tok.reshape(-1), None, 256, len(tok))
    finally:
        if option:
            ctx.set_option(option, 0)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k", [128, 48], ids=["wave_per_set", "packed"])
def test_ragged_sets_with_short_tails(ctx, k):
    """CSR sets of 16 r + tail tokens, tail 1..15: the crafted cells sit in the whole rows, the tail goes another way
    (wave per set) or is the masked partial row (packed kernel)."""
    a, b = O.np_init_permutations(k, 4)
    full = crafted_sets(a, b, 272, n_perms=1, seed=5)
    lens = 256 + 1 + np.arange(len(full)) % 15
    lens[::5] = 48 + 1 + np.arange(len(full))[::5] % 15  # short sets: cells beyond them are simply cut off
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hv = np.concatenate([row[:m] for row, m in zip(full, lens)])
    got = ctx.minhash_bulk((a, b), hv, off, 0, len(full))
    assert np.array_equal(got, O.c_minhash_bulk(hv, off, a, b))


@pytest.mark.parametrize("t, distinct", [(40, 37), (250, 243)])
def test_partial_rescan_of_the_dedup_launch(ctx, t, distinct):
    """Sets with repeated tokens, laid out so that the dedup launch's compacted tile is known: `distinct` tokens -- whole
    rows plus a partial one of 5 or 3 tokens -- with the two smallest keys of one permutation d apart in that partial
    row, across its boundary, or in the row before it.  The raw set is [c0, c0, c1, ..., c_last, repeats]: c0 is the
    minimum of another permutation, so its copy makes the first launch's proof fail for certain; the repeats at the end
    are copies of the crafted minimum, which the compaction leaves as stale cells behind the partial row -- unmasked
    they would tie with the minimum and send every set on to the pairwise launch."""
    k = 128
    a, b = O.np_init_permutations(k, 6)
    rng = np.random.RandomState(t)
    last_row, rest = distinct // 16 * 16, distinct % 16
    odd = odd_perms(a, 7)
    sets, far, near = [], [], []
    for pk in odd[:6]:
        for d in NEAR_D[1:]:  # (d = 0 would be one more repeat)
            for p0, p1 in ((last_row, last_row + rest - 1), (last_row + rest - 1, last_row), (last_row - 1, last_row),
                           (last_row - 16, last_row - 1)):
                c = rng.randint(0, 2**32, distinct, dtype=np.uint64)
                c[0] = token_for(a, b, odd[6], 500)
                c[p0], c[p1] = token_for(a, b, pk, 1000), token_for(a, b, pk, 1000 + d)
                sets.append(np.concatenate([c[:1], c, np.full(t - distinct - 1, c[p0], dtype=np.uint64)]))
                far.append(d >= 48)
                near.append(d <= 31)
    tok, far, near = np.stack(sets), np.array(far), np.array(near)
    assert tok.shape[1] == t
    want = O.c_minhash_bulk_dense(tok, a, b)
    ctx.set_option("minhash.ties", 1)  # no tie-tolerant proof in the second launch: the dedup pass takes every flagged set
    try:
        got = ctx.minhash_bulk((a, b), tok.reshape(-1), None, t, len(tok))
        flags = ctx.minhash_flags(len(tok))
    finally:
        ctx.set_option("minhash.ties", 0)
    assert np.array_equal(got, want)
    assert (flags >= 1).all()
    # keys 48 and more apart: settled by the dedup launch (its table misses about one repeat in a thousand, and a random
    # token may come close to another permutation's minimum: nearly all, not all)
    assert (flags[far] == 1).mean() >= 0.9, flags[far]
    assert (flags[near] == 2).mean() >= 0.9, flags[near]  # keys less than 32 apart: left to the pairwise launch


def test_flag_rate_on_random_sets(ctx):
    """20 000 sets of distinct random tokens: the proof fails within the project's bound, and as often as the numpy
    model of the predicate says (same order of magnitude)."""
    n, t, k = 20000, 256, 128
    tok = np.random.RandomState(11).randint(0, 2**32, (n, t), dtype=np.uint64)
    a, b = O.np_init_permutations(k, 1)
    ctx.counters(True)
    got = ctx.minhash_bulk((a, b), tok.reshape(-1), None, t, n)
    c = ctx.counters(False)
    assert np.array_equal(got, O.c_minhash_bulk_dense(tok, a, b))
    assert c["sieve_blocks"] == n and c["sieve_sets_redone"] <= n // 200, c
    assert MODEL_FLAGGED_SEED_11 // 4 <= c["sieve_sets_redone"] <= 4 * MODEL_FLAGGED_SEED_11, c
