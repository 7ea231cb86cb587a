"""The numpy model of the sieve's proof and of the rescan's min3/med3 network (tests/sieve_rescan_model.py) against
brute force, without a GPU: the network yields the two smallest tagged keys of any row, and wherever the model's proof
passes, the token it picks has the exact minimum of the reference arithmetic (oracle.c_minhash_bulk_dense) -- on random
sets and on sets crafted to put near keys, keys a multiple of 2^28 apart and the wrap-around guards at the minimum.
This checks the construction and the predicate, not the kernel's code; the kernel runs the same corpora in
tests/test_gpu_sieve_rescan.py."""
import numpy as np

from oracle import oracle as O
from tests.sieve_rescan_model import NEAR_D, crafted_sets, exact_hash, odd_perms, sieve_model, sieve_model_block, token_for


# ---------------------------------------------------------------------------------------------- the tests
def _check_sound(tok, a, b):
    want = O.c_minhash_bulk_dense(tok, a, b)
    ok, val = sieve_model(tok, a, b)
    assert np.array_equal(val[ok], want[ok]), "the proof passed on a token that does not hold the exact minimum"
    return ok


def test_model_is_sound_on_random_sets():
    k = 128
    a, b = O.np_init_permutations(k, 1)
    tok = np.random.RandomState(5).randint(0, 2**32, (1500, 256), dtype=np.uint64)
    ok = _check_sound(tok, a, b)
    # distinct random tokens: the proof almost never fails (about 4 sets in 10^4; 40 times that is far from chance)
    assert (~ok.all(axis=1)).sum() <= 1500 // 60


def test_model_is_sound_on_crafted_sets():
    a, b = O.np_init_permutations(128, 4)
    tok = crafted_sets(a, b, 256, n_perms=2)
    ok = _check_sound(tok, a, b)
    # both outcomes occur: crafted permutations whose proof must fail, and sets that pass everywhere
    assert (~ok).any() and ok.all(axis=1).any()


def test_model_is_sound_on_several_blocks_and_few_rows():
    a, b = O.np_init_permutations(64, 7)
    for t in (48, 64, 512 + 64):
        _check_sound(crafted_sets(a, b, t, n_perms=1, seed=t), a, b)


def test_model_is_sound_on_a_partial_last_row():
    """The compacted tile of the dedup launch: the last row holds 5 tokens, the cells behind them are stale."""
    a, b = O.np_init_permutations(64, 2)
    k = odd_perms(a, 1)[0]
    rng = np.random.RandomState(8)
    cases = []
    for d in NEAR_D:
        for c0, c1 in ((0, 4), (4, 0), (3, 4)):
            row = rng.randint(0, 2**32, 48, dtype=np.uint64)
            row[32 + c0], row[32 + c1] = token_for(a, b, k, 56), token_for(a, b, k, 56 + d)
            row[37:] = token_for(a, b, k, 56)  # stale cells: copies of the minimum, which must not count
            cases.append(row)
    tok = np.stack(cases)
    want = O.c_minhash_bulk_dense(tok[:, :37], a, b)
    ok, pick = sieve_model_block(tok, a, b, partial_cols=5)
    val = exact_hash(np.take_along_axis(tok, pick, axis=1), a, b)
    assert (pick < 37).all()
    assert np.array_equal(val[ok], want[ok])
    assert ok[len(NEAR_D) * 3 - 1, k] and not ok[0, k]  # d = 49 passes, d = 0 does not: the stale copies are masked
