"""A numpy model of the tie-tolerant proof (finish_block_ties in csrc/minhash_kernels.hip) and of the launch it ends.

The first launch of a bulk MinHash call on a context that has learned "the sets repeat tokens" (mode word 1) is
MODE_SIEVE_TIES: the sieve's row loop with a (smallest, second, third) record per permutation, and per block of up to
256 tokens the proof below.  With the tagged keys of tests/sieve_rescan_model.py,
    key_c = (M_c & ~15) | c,      M_c = lo32(h_c a_lo + b + 8),
`base` is the best tagged ROW key with its low four bits cleared and the "window" the tagged keys below base + 32.  A
block is accepted when
    16 <= base <= 0xFFFFFF00,
    at most two cells are in the window -- two cells of the best row, or the best cells of two rows with one cell each --
    and the third row and the third cell (of the best row; the second cell of the second row) are outside it;
both candidates are hashed exactly and the smaller value kept.  ties_model restates that per block and permutation as
the kernel writes it (the record of three, the unsigned differences, the candidate choice) -- not the kernel's code:
that the kernel decides and computes the same is what tests/test_gpu_learned_first_launch.py checks.

first_launch_model extends it to the sets of the general kernel shape: whole rows through ties_model, the ragged tail
(fewer than 16 tokens) through the fast fold, which asks for a redo when its minimum is <= 7 (fold_fast).

Shared by tests/test_sieve_ties_model.py (CPU), tests/learned_launch_cases.py and the GPU file.
"""
import numpy as np

from tests.sieve_rescan_model import U32, exact_hash

MAXH = U32(0xFFFFFFFF)


def _three_smallest(x):
    """The three smallest of x[..., m] as a multiset (what Three::add leaves), padded with 2^32-1."""
    m = x.shape[-1]
    if m < 3:
        x = np.concatenate([x, np.full(x.shape[:-1] + (3 - m,), MAXH, U32)], axis=-1)
    part = np.sort(np.partition(x, 2, axis=-1)[..., :3], axis=-1)
    return part[..., 0], part[..., 1], part[..., 2]


def _row_keys(lo, rows, a_lo, b8):
    """Tagged keys [n, K, 16] of row rows[n, K] of lo[n, r, 16]."""
    n = lo.shape[0]
    tok = lo[np.arange(n)[:, None], rows]  # [n, K, 16]
    with np.errstate(over="ignore"):
        key = tok * a_lo[None, :, None] + b8[None, :, None]
    return (key & U32(0xFFFFFFF0)) | np.arange(16, dtype=U32)[None, None, :]


def ties_model_block(tok, a, b):
    """One block: tok[n, T], T a multiple of 16, 0 < T <= 256.  Returns (ok[n, K], pick1[n, K], pick2[n, K], tied[n, K]):
    whether the proof accepts, the indices of the two tokens hashed exactly (equal when there is one candidate), and
    whether a second key reaches into the window (the one-candidate proof would have failed)."""
    n, t = tok.shape
    assert t % 16 == 0 and 0 < t <= 256
    r = t // 16
    lo = (tok & np.uint64(0xFFFFFFFF)).astype(U32).reshape(n, r, 16)
    a_lo = (a & np.uint64(0xFFFFFFFF)).astype(U32)
    b8 = ((b + np.uint64(8)) & np.uint64(0xFFFFFFFF)).astype(U32)
    with np.errstate(over="ignore"):
        m = lo[:, None, :, :] * a_lo[None, :, None, None] + b8[None, :, None, None]  # [n, K, r, 16] mod 2^32
        rowmin = m.min(-1)
        del m
        tagged = (rowmin & U32(0xFFFFFFF0)) | np.arange(r, dtype=U32)[None, None, :]
        r1, r2, r3 = _three_smallest(tagged)
        base = r1 & U32(0xFFFFFFF0)
        row_a, row_b = (r1 & U32(15)).astype(np.int64), (r2 & U32(15)).astype(np.int64)  # (r2 = 2^32-1: row 15, never used)
        row_b = np.minimum(row_b, r - 1)
        c1, c2, c3 = _three_smallest(_row_keys(lo, row_a, a_lo, b8))
        o1, o2, _ = _three_smallest(_row_keys(lo, row_b, a_lo, b8))
        row_tie = (r2 - base) < U32(32)
        col_tie = (c2 - base) < U32(32)
        ok = (base >= U32(16)) & (base <= U32(0xFFFFFF00)) & ((r3 - base) >= U32(32)) & ~(row_tie & col_tie) & ((c3 - base) >= U32(32))
        ok &= ~row_tie | ((o2 - base) >= U32(32))
    j1, j2, i1 = (c1 & U32(15)).astype(np.int64), (c2 & U32(15)).astype(np.int64), (o1 & U32(15)).astype(np.int64)
    pick1 = row_a * 16 + j1
    pick2 = np.where(row_tie, row_b * 16 + i1, np.where(col_tie, row_a * 16 + j2, pick1))
    return ok, pick1, pick2, row_tie | col_tie


def ties_model(tok, a, b, chunk=64):
    """Sets of whole rows, any number of 256-token blocks: (ok[n, K], value[n, K]) -- ok where every block's proof
    accepts, value the minimum over the blocks of the exact hashes of the (one or two) candidates."""
    ok, val, _ = ties_model_tied(tok, a, b, chunk)
    return ok, val


def ties_model_tied(tok, a, b, chunk=64):
    """ties_model and tied[n, K]: some block had a second key in the window."""
    n, t = tok.shape
    k = len(a)
    ok, tied = np.ones((n, k), bool), np.zeros((n, k), bool)
    val = np.full((n, k), 0xFFFFFFFF, np.uint64)
    for i in range(0, n, chunk):
        for blk in range(0, t, 256):
            part = tok[i:i + chunk, blk:blk + 256]
            o, p1, p2, td = ties_model_block(part, a, b)
            ok[i:i + chunk] &= o
            tied[i:i + chunk] |= td
            for p in (p1, p2):
                val[i:i + chunk] = np.minimum(val[i:i + chunk], exact_hash(np.take_along_axis(part, p, axis=1), a, b))
    return ok, val, tied


def tail_suspicious(tok, a, b):
    """The fast fold over a ragged tail tok[n, m] (m < 16): u = lo32(s + 1) + ((s + 1) >> 61) with s = tok a + b mod 2^64;
    a permutation whose smallest u is <= 7 sends the set on (sieve_minima).  Returns bad[n, K]."""
    with np.errstate(over="ignore"):
        s1 = tok[:, None, :] * a[None, :, None] + b[None, :, None] + np.uint64(1)
        u = ((s1 & np.uint64(0xFFFFFFFF)) + (s1 >> np.uint64(61))) & np.uint64(0xFFFFFFFF)
    return u.min(-1) <= np.uint64(7)


def first_launch_model(sets, a, b):
    """Which sets the tie-tolerant first launch settles itself, for sets of any length (a list of 1-D uint64 arrays):
    settled[n] -- every block of the whole rows accepted for every permutation and no suspicious tail; an empty set is
    settled (nothing to do).  Sets are grouped by length, so a corpus of few distinct lengths costs few model calls."""
    settled = np.ones(len(sets), bool)
    by_len = {}
    for i, s in enumerate(sets):
        by_len.setdefault(len(s), []).append(i)
    for m, idx in by_len.items():
        if m == 0:
            continue
        tok = np.stack([np.asarray(sets[i], dtype=np.uint64) for i in idx])
        whole = m // 16 * 16
        good = np.ones(len(idx), bool)
        if whole:
            good &= ties_model(tok[:, :whole], a, b)[0].all(axis=1)
        if whole < m:
            good &= ~tail_suspicious(tok[:, whole:], a, b).any(axis=1)
        settled[idx] = good
    return settled
