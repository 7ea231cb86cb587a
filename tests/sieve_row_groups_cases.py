"""Corpora for the sieve's row loop, which folds the row minima of uint64 tokens into the two smallest four rows at a time
(Two::add4 in csrc/minhash_kernels.hip) and the remaining rows one at a time.

Shared by tests/test_sieve_row_groups_host.py (CPU) and tests/test_gpu_sieve_row_groups.py.  The reference throughout is the
numpy path, MinHash.bulk_signatures(..., hashfunc=prehashed, gpu_mode="disable"); it is computed once for 256 permutations --
the permutations of a shorter signature with the same seed are its first K (MinHash._init_permutations draws them from one
stream), so its first K columns are that signature.
"""
import functools

import numpy as np

from datasketch_amd import MinHash
from datasketch_amd.hashfunc import prehashed
from tests.sieve_rescan_model import odd_perms

SEED = 1
K_MAX = 256
# rows per set: whole groups of four, every remainder, and a second 16-row block with a short last group
ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 19, 20, 31, 32, 33)
N_SETS = 512
TAILS = (0, 1, 15)  # tokens behind the last whole row in the CSR corpus


def permutations(k):
    a, b = MinHash(num_perm=k, seed=SEED, hashfunc=prehashed).permutations
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def reference(corpus):
    """[n, K_MAX] by the numpy path; corpus: a 2-D array or a (values, offsets) pair."""
    return MinHash.bulk_signatures(corpus, num_perm=K_MAX, seed=SEED, hashfunc=prehashed, gpu_mode="disable")


@functools.lru_cache(maxsize=None)
def tokens(wide):
    """tok[N_SETS, 16 * 33 + 15] of distinct random tokens (uint64): 64-bit ones, or -- not wide -- below 2^32, what a uint32
    array holds.  A set of 16 r + s tokens is a prefix of a row."""
    rng = np.random.RandomState(20 + wide)
    shape = (N_SETS, 16 * max(ROWS) + max(TAILS))
    tok = rng.randint(0, 2**32, shape, dtype=np.uint64)
    if wide:
        tok |= rng.randint(0, 2**32, shape, dtype=np.uint64) << np.uint64(32)
    assert all(len(np.unique(row)) == row.size for row in tok)
    tok.setflags(write=False)
    return tok


@functools.lru_cache(maxsize=None)
def dense_reference(wide, rows):
    want = reference(np.ascontiguousarray(tokens(wide)[:, :16 * rows]))
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def ragged(wide):
    """(values, offsets, want): every row count of ROWS as CSR, set i of a row count with TAILS[i % 3] tokens behind its
    last whole row -- a third of the sets are the dense corpus itself."""
    tok = tokens(wide)
    parts = [tok[i, :16 * rows + TAILS[i % 3]] for rows in ROWS for i in range(N_SETS)]
    offsets = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.int64)
    values = np.concatenate(parts)
    want = reference((values, offsets))
    for a in (values, offsets, want):
        a.setflags(write=False)
    return values, offsets, want


# ------------------------------------------------------------------------------------------------ planted minima
PLANT_K = 128
PLANT_ROWS = 8       # two groups of four
BASE_S = 1000        # s_lo of the smallest planted token: its key is s_lo + 8
GAPS = {"apart": 4096, "close": 8, "tie": 0}
FILLER_FLOOR = 2**28


def places():
    """(row, column) of the smallest and of the second smallest key: every ordered pair of different rows of 0..7 -- both in
    one group, in different groups, every position of a group -- and both in the same row."""
    out = [((i, (3 * i + 1) % 16), (j, (5 * j + 2) % 16)) for i in range(PLANT_ROWS) for j in range(PLANT_ROWS) if i != j]
    out += [((i, 3), (i, 11)) for i in range(PLANT_ROWS)]
    return out


def tokens_for(a, b, k, s_lo):
    """The 32-bit tokens whose hash under permutation k has the low words s_lo (an array): s_lo = lo32(h a_lo + b_lo)."""
    a_lo, b_lo = int(a[k]) & 0xFFFFFFFF, int(b[k]) & 0xFFFFFFFF
    inv = pow(a_lo, -1, 1 << 32)
    return (np.asarray(s_lo, dtype=np.uint64) + np.uint64(2**32 - b_lo)) % np.uint64(2**32) * np.uint64(inv) % np.uint64(2**32)


def sieve_keys(tok, a, b, k):
    """M = lo32(h_lo a_lo + b_lo + 8) of tok[...] under permutation k: what the row loop minimises."""
    a_lo, b8 = np.uint64(int(a[k]) & 0xFFFFFFFF), np.uint64((int(b[k]) + 8) & 0xFFFFFFFF)
    return ((tok & np.uint64(0xFFFFFFFF)) * a_lo + b8) & np.uint64(0xFFFFFFFF)


@functools.lru_cache(maxsize=None)
def planted(kind):
    """(tok[n, 128], k, where): one set per entry of places().  Under permutation k (the first of the seed-1 permutations
    with an odd low multiplier word) the set's smallest key sits at where[i][0] and its second smallest, GAPS[kind] above
    it, at where[i][1]; every other token has a key above 2^28.  Every other set carries random high words in its filler
    (they change the exact values, never a key).  "tie": the same token in both places."""
    a, b = permutations(PLANT_K)
    k = odd_perms(a, 1)[0]
    where = places()
    rng = np.random.RandomState(7)
    n, t = len(where), 16 * PLANT_ROWS
    s_fill = rng.randint(FILLER_FLOOR + 1, 2**32 - 2**20, (n, t), dtype=np.uint64)
    assert all(len(np.unique(row)) == t for row in s_fill)
    tok = tokens_for(a, b, k, s_fill)
    tok[1::2] |= rng.randint(0, 2**32, tok[1::2].shape, dtype=np.uint64) << np.uint64(32)
    first, second = tokens_for(a, b, k, [BASE_S, BASE_S + GAPS[kind]])
    for i, ((r0, c0), (r1, c1)) in enumerate(where):
        tok[i, 16 * r0 + c0] = first
        tok[i, 16 * r1 + c1] = second
    tok.setflags(write=False)
    return tok, k, where
