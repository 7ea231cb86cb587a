"""The sieve's finishes with the short fold, as a numpy model, and the corpora of their tests.

The finishes of csrc/minhash_kernels.hip (finish_block, finish_block_ties) hash the candidate their proof picked with
    fold_proven(s) = s_lo + (s >> 61)   (mod 2^32)
instead of fold_exact(s) = (s mod (2^61 - 1)) mod 2^32: a passing proof has the candidate's key M = lo32(s_lo + 8) >= 16,
which leaves no carry and no Mersenne correction.  finish_model / finish_ties_model take the proofs from
tests/sieve_rescan_model.py and tests/sieve_ties_model.py (imported, not restated) and return the SHORT-fold value of
the picked tokens: equal to the reference wherever the proof passes is what tests/test_sieve_finish_host.py asserts.

Corpora (built from fixed seeds, shared by the CPU file and tests/test_gpu_sieve_finish.py):
  winner_sets   sets of 64 tokens whose smallest key under one permutation is a chosen M, the winner's token solved from
                M through the inverse of the odd a_lo (token_for) and, for uint64 tokens, its high word solved so that the
                exact hash has a chosen top = s >> 61 and chosen low 29 bits of s_hi;
  mixed_lengths 4 096 sets of 16, 48, 250 and 272 tokens (1, 3, 15 and 16 + 1 rows per block) ordered so that the sets a
                wave walks with blocks_per_cu = 1 differ in length: a short block follows a long one in its LDS tile.
"""
import numpy as np

from tests.sieve_rescan_model import U32, exact_hash, odd_perms, sieve_model_block, token_for
from tests.sieve_ties_model import tail_suspicious, ties_model_block

U64 = np.uint64
LOW = U64(0xFFFFFFFF)
SETTLED_M = (16, 17, 31)                  # the first launch settles these (given the other 127 permutations behave: the model says)
TOP_M = (2**32 - 17, 2**32 - 1)           # keys are mod 2^32: nothing can lie 64 above these, and a best key >= 2^32 - 32 is
                                          # never 32 below the second (at most 2^32 - 1): refused by every proof, flagged
GUARDED_M = (0, 7, 15)                    # below the guard: flagged
WINNER_T = 64
HI29_EDGES = (0, 1, 2**29 - 2, 2**29 - 1)


def short_fold(tok, a, b):
    """fold_proven of the pairs (tok[n, K], a[K], b[K])."""
    with np.errstate(over="ignore"):
        s = tok * a[None, :] + b[None, :]
    return ((s & LOW) + (s >> U64(61))) & LOW


def finish_model(tok, a, b, chunk=128):
    """The one-candidate finish over sets of whole rows: (ok[n, K], value[n, K]), value the minimum over the blocks of
    the SHORT fold of the picked token (sieve_model with fold_proven in place of the exact hash)."""
    n, t = tok.shape
    ok = np.ones((n, len(a)), bool)
    val = np.full((n, len(a)), 0xFFFFFFFF, U64)
    for i in range(0, n, chunk):
        for blk in range(0, t, 256):
            part = tok[i:i + chunk, blk:blk + 256]
            o, pick = sieve_model_block(part, a, b)
            ok[i:i + chunk] &= o
            val[i:i + chunk] = np.minimum(val[i:i + chunk], short_fold(np.take_along_axis(part, pick, axis=1), a, b))
    return ok, val


def finish_ties_model(tok, a, b, chunk=64):
    """The same for the tie-tolerant finish: both candidates through the short fold."""
    n, t = tok.shape
    ok = np.ones((n, len(a)), bool)
    val = np.full((n, len(a)), 0xFFFFFFFF, U64)
    for i in range(0, n, chunk):
        for blk in range(0, t, 256):
            part = tok[i:i + chunk, blk:blk + 256]
            o, p1, p2, _ = ties_model_block(part, a, b)
            ok[i:i + chunk] &= o
            for p in (p1, p2):
                val[i:i + chunk] = np.minimum(val[i:i + chunk], short_fold(np.take_along_axis(part, p, axis=1), a, b))
    return ok, val


def reference(tok, a, b):
    """min over the tokens of the exact hash: tok[n, T] -> [n, K] (the reference arithmetic, a set at a time)."""
    out = np.empty((len(tok), len(a)), U64)
    for i, row in enumerate(tok):
        out[i] = exact_hash(np.broadcast_to(row[:, None], (len(row), len(a))), a, b).min(axis=0)
    return out


def one_candidate_settles(sets, a, b):
    """settled[n]: the one-candidate first launch (MODE_SIEVE) needs no later launch for the set -- every block of its whole
    rows passes for every permutation and the fast fold of its tail asks for no redo; an empty set is settled."""
    settled = np.ones(len(sets), bool)
    by_len = {}
    for i, s in enumerate(sets):
        by_len.setdefault(len(s), []).append(i)
    for m, idx in by_len.items():
        if m == 0:
            continue
        tok = np.stack([np.asarray(sets[i], dtype=U64) for i in idx])
        whole = m // 16 * 16
        good = np.ones(len(idx), bool)
        if whole:
            good &= finish_model(tok[:, :whole], a, b)[0].all(axis=1)
        if whole < m:
            good &= ~tail_suspicious(tok[:, whole:], a, b).any(axis=1)
        settled[idx] = good
    return settled


# ---------------------------------------------------------------------------------------------- crafted winners
def target_perms(a):
    """An odd permutation of the first 64-lane slot and one of the last."""
    odd = odd_perms(a, len(a))
    last = (len(a) - 1) // 64 * 64
    assert odd[0] < 64 and odd[-1] >= last and odd[0] != odd[-1]
    return [odd[0], odd[-1]]


def _keys(lo, a, b, k):
    """M of 32-bit low words under permutation k."""
    a_lo, b_lo = int(a[k]) & 0xFFFFFFFF, int(b[k]) & 0xFFFFFFFF
    return [(int(x) * a_lo + b_lo + 8) % 2**32 for x in lo]


def _steer_high(lo, a, b, k, top, hi29):
    """The high word of a uint64 token with low word `lo` whose hash s under permutation k has s >> 61 == top and
    (s >> 32) & (2^29 - 1) == hi29: s_hi is linear in the high word with the odd factor a_lo."""
    a_k, b_k = int(a[k]), int(b[k])
    s0_hi = ((lo * a_k + b_k) % 2**64) >> 32
    want = (top << 29) | hi29
    hi = (want - s0_hi) * pow(a_k & 0xFFFFFFFF, -1, 1 << 32) % 2**32
    assert (((hi << 32 | lo) * a_k + b_k) % 2**64) >> 32 == want
    return hi


def winner_sets(a, b, wide, seed=5):
    """(tok[n, 64] uint64, m[n], perm[n], top[n]): for both target permutations, every M of SETTLED_M + TOP_M + GUARDED_M,
    every top 0..7 (uint64 tokens; what the multiplier gives for uint32 ones, one set per M then) and the winner at the
    first cell of the first row or the last cell of the last.  Every other token's key under that permutation is at
    least 64 above M where that is possible; for TOP_M the others take the keys above M round and round (equal keys:
    equal low words, and for uint64 tokens different high words)."""
    rng = np.random.RandomState(seed)
    toks, ms, perms, tops = [], [], [], []
    for k in target_perms(a):
        for m in SETTLED_M + TOP_M + GUARDED_M:
            for top in (range(8) if wide else (None,)):
                for place in (0, WINNER_T - 1):
                    tok = rng.randint(0, 2**32, WINNER_T, dtype=U64)
                    if m in TOP_M:
                        above = list(range(m + 1, 2**32)) or [m]
                        for i in range(WINNER_T):
                            tok[i] = token_for(a, b, k, (above[i % len(above)] - 8) % 2**32)
                    else:
                        while True:  # redraw the fillers within 64 of the winner's key (or wrapped below it)
                            close = [i for i, key in enumerate(_keys(tok, a, b, k)) if key < m + 64]
                            if not close:
                                break
                            tok[close] = rng.randint(0, 2**32, len(close), dtype=U64)
                    lo = token_for(a, b, k, (m - 8) % 2**32)
                    if wide:
                        tok |= rng.randint(0, 2**32, WINNER_T, dtype=U64) << U64(32)
                        hi29 = HI29_EDGES[len(toks) % 4] if len(toks) % 8 < 4 else int(rng.randint(0, 2**29))
                        tok[place] = U64(_steer_high(lo, a, b, k, top, hi29) << 32 | lo)
                    else:
                        tok[place] = U64(lo)
                    assert _keys([int(tok[place]) & 0xFFFFFFFF], a, b, k)[0] == m
                    toks.append(tok)
                    ms.append(m)
                    perms.append(k)
                    tops.append(int((int(tok[place]) * int(a[k]) + int(b[k])) % 2**64 >> 61))
    return np.stack(toks), np.array(ms, dtype=np.int64), np.array(perms), np.array(tops)


# ---------------------------------------------------------------------------------------------- mixed lengths
MIXED_LENGTHS = (16, 48, 250, 272)
MIXED_N = 4096


def mixed_length_sets(wide, repeats=0.0, seed=11, n=MIXED_N):
    """n sets of MIXED_LENGTHS tokens.  A launch of one workgroup per compute unit has 1 024 waves on 256 units, wave w
    walking sets w, w + 1024, ...: the length index (i + (0, 3, 1, 2)[i // 1024]) % 4 gives every wave all four lengths,
    272 -> 16, 272 -> 48, 250 -> 16 and 250 -> 48 among the steps.  (Fewer units: the sets a wave walks still differ in length, since consecutive
    indices do.)  repeats: that share of every set's tokens are copies of other tokens of the set."""
    rng = np.random.RandomState(seed)
    sets = []
    for i in range(n):
        t = MIXED_LENGTHS[(i + (0, 3, 1, 2)[(i // 1024) % 4]) % 4]
        tok = rng.randint(0, 2**32, t, dtype=U64)
        if wide:
            tok |= rng.randint(0, 2**32, t, dtype=U64) << U64(32)
        if repeats:
            for dst in rng.choice(t, max(1, int(t * repeats)), replace=False):
                tok[dst] = tok[rng.randint(0, t)]
        sets.append(tok)
    return sets


def csr(sets, dtype=U64):
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    hv = np.concatenate(sets).astype(dtype) if len(sets) else np.empty(0, dtype)
    return hv, off
