"""The numpy model of the tie-tolerant proof (tests/sieve_ties_model.py) against the reference arithmetic, without a GPU:
wherever the model accepts, the smaller exact hash of its (one or two) candidates is the exact minimum
(oracle.c_minhash_bulk_dense) -- on the corpora of tests/learned_launch_cases.py and on random sets -- and the kinds of
those corpora land where they are meant to.  This checks the predicate as modelled and the case builder, not the
kernel's code; the kernel runs the same corpora in tests/test_gpu_learned_first_launch.py."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import learned_launch_cases as C
from tests.sieve_rescan_model import sieve_model, token_for
from tests.sieve_ties_model import first_launch_model, tail_suspicious, ties_model, ties_model_tied


def _check_sound(tok, a, b):
    want = O.c_minhash_bulk_dense(tok, a, b)
    ok, val = ties_model(tok, a, b)
    assert np.array_equal(val[ok], want[ok]), "the proof accepted candidates that do not hold the exact minimum"
    return ok


def test_model_is_sound_on_20000_random_sets():
    """Distinct random tokens, K = 128, 256 tokens, token seed 11 and permutation seed 1 (the corpus of
    test_flag_rate_on_random_sets).  Sets with any ok == False: 4 of 20 000, 0.02 % (the one-candidate model fails on 10
    of them).  No threshold rests on the figure."""
    a, b = O.np_init_permutations(128, 1)
    tok = np.random.RandomState(11).randint(0, 2**32, (20000, 256), dtype=np.uint64)
    ok = _check_sound(tok, a, b)
    print(f"[ties model] random sets with a failed tie-tolerant proof: {int((~ok.all(axis=1)).sum())} of {len(tok)}")


@pytest.mark.parametrize("k, t, wide", [(128, 256, True), (128, 256, False), (136, 256, True), (64, 256, True), (300, 250, True), (600, 256, False)])
def test_model_is_sound_on_the_fixed_corpora_and_the_kinds_land_where_intended(k, t, wide):
    a, b = O.np_init_permutations(k, 4)
    targets = C.target_perms(a)
    tok, kinds = C.fixed_cases(a, b, t, wide, targets)
    body = t // 16 * 16
    ok = _check_sound(tok[:, :body], a, b)
    settled = first_launch_model(list(tok), a, b)
    for kind in ("one_tie", "one_tie_tail"):
        assert settled[kinds == kind].all(), kind
    assert ok[kinds == "one_tie"].all()   # ok everywhere
    # triple and three_close: not ok for the crafted permutation (the builder made half of them for each target)
    for kind in C.DEFEATING_KINDS:
        rows = ok[kinds == kind]
        assert len(rows) and (~rows[:, targets]).any(axis=1).all() and (~rows[:, targets]).any(axis=0).all(), kind
    # a tie is what the one-candidate proof cannot take: every one_tie set fails it in the whole rows
    one = sieve_model(tok[kinds == "one_tie"][:, :body], a, b)[0]
    assert not one.all(axis=1).any()
    # both outcomes among the rest, and every kind present
    assert ok[kinds == "crafted"].all(axis=1).any() and (~ok[kinds == "crafted"]).any()
    assert set(kinds) >= {"clean", "one_tie", "two_close", "triple", "three_close", "crafted"}
    if not wide:
        assert int(tok.max()) < 2**32


def test_model_is_sound_on_the_ragged_corpus_block_by_block():
    """Whole rows of every ragged set (one, two and three blocks, few rows), and the kinds of the ragged form."""
    a, b = O.np_init_permutations(136, 4)
    sets, kinds = C.ragged_cases(a, b, True)
    lens = np.array([len(s) for s in sets])
    assert {0, 1}.issubset(lens.tolist()) and (lens > 512).any() and ((lens > 256) & (lens <= 512)).any()
    assert set((lens[lens >= 16] % 16).tolist()) == set(range(16))
    for m in np.unique(lens // 16 * 16):
        if m:
            _check_sound(np.stack([s[:m] for s, n in zip(sets, lens) if n // 16 * 16 == m]), a, b)
    settled = first_launch_model(sets, a, b)
    for kind in C.SETTLED_KINDS + ("tiny", "near_top_edge"):
        assert (kinds == kind).any() and settled[kinds == kind].all(), kind
    for kind in C.DEFEATING_KINDS + ("near_top",):
        assert (kinds == kind).any() and not settled[kinds == kind].any(), kind
    # blocks of a single row (17 and 33 rows) and sets of a single row are there
    assert {1, 17, 33} <= set((lens // 16).tolist())
    # the copy in another block or in the tail leaves one candidate per block: the one-candidate proof holds there too
    far = [s for s, kd in zip(sets, kinds) if kd == "one_tie_other_block"]
    assert all(sieve_model(s[None, :len(s) // 16 * 16], a, b)[0].all() for s in far)


def test_two_candidates_are_both_hashed():
    """Equal low words, different high words: one key, two exact values -- the smaller one may sit in either cell."""
    a, b = O.np_init_permutations(128, 4)
    k = C.target_perms(a)[0]
    rng = np.random.RandomState(2)
    tok = np.stack([C._one_set("two_close", 0, rng, a, b, k, 256, 256, True) for _ in range(32)])   # variant 0: d = 0
    ok, val, tied = ties_model_tied(tok, a, b)
    assert ok[:, k].all() and tied[:, k].all()
    assert np.array_equal(val[ok], O.c_minhash_bulk_dense(tok, a, b)[ok])


def test_teaching_prototypes_are_of_one_kind():
    a, b = O.np_init_permutations(128, 4)
    clean, one, triple = (C.teaching_prototypes(a, b, kind) for kind in ("clean", "one_tie", "triple"))
    assert clean.shape == one.shape == triple.shape == (C.N_PROTO, 256)
    assert sieve_model(clean, a, b)[0].all()
    assert ties_model(one, a, b)[0].all() and not sieve_model(one, a, b)[0].all(axis=1).any()
    assert not ties_model(triple, a, b)[0].all(axis=1).any() and not sieve_model(triple, a, b)[0].all(axis=1).any()
    assert C.tiled(one).shape == (C.N_TEACH, 256) and np.array_equal(C.tiled(one)[C.N_PROTO], one[0])


def test_fast_fold_of_a_tail_asks_for_a_redo_only_near_zero():
    """tail_suspicious against the fold in Python integers: u = lo32(s + 1) + ((s + 1) >> 61) <= 7, s = tok a + b mod 2^64."""
    a, b = O.np_init_permutations(64, 2)
    k = C.target_perms(a)[0]
    lows = [0, 5, 6, 7, 100, 2**32 - 1, 2**32 - 2, 2**32 - 8]
    tok = np.array([[token_for(a, b, k, s)] for s in lows], dtype=np.uint64)
    bad = tail_suspicious(tok, a, b)
    for i in range(len(lows)):
        for p in range(len(a)):
            s1 = (int(tok[i, 0]) * int(a[p]) + int(b[p]) + 1) % 2**64
            assert bad[i, p] == ((((s1 & 0xFFFFFFFF) + (s1 >> 61)) & 0xFFFFFFFF) <= 7), (i, p)
    assert bad[5, k] and not bad[4, k]   # a low word of 2^32 - 1 always asks for the redo; one of 100 never does
