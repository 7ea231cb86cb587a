"""A numpy model of the sieve's proof with the rescan's min3/med3 network, and the crafted corpora of its tests.

The kernel (csrc/minhash_kernels.hip, finish_block) rescans the best row of a block with the tagged keys
    key_c = (M_c & ~15) | c,      M_c = lo32(h_c a_lo + b + 8),
and, with one or two permutations per lane, takes their two smallest k1 < k2 from a network of v_min3_u32 /
v_med3_u32 over five triples and the 16th key (20 instructions instead of a 16-step (min, med3) fold).  It accepts the
cell behind k1 iff
    the row records are >= 32 apart,  k2 - k1 >= 32  and  k1 >= 16.
network_two_smallest is a numpy re-statement of that network, not the kernel's code: it shows that the construction
yields the two smallest keys (equal keys and the 2^32-1 of masked cells included); that the kernel computes the same
is what tests/test_gpu_sieve_rescan.py checks, bit for bit against the C oracle.  Shared by
tests/test_sieve_rescan_model.py (CPU) and tests/test_gpu_sieve_rescan.py.
"""
import numpy as np


U32 = np.uint32
MERSENNE = np.uint64((1 << 61) - 1)


def exact_hash(tok, a, b):
    """fold((tok * a + b) mod 2^64) for tok[n, K] (uint64), a, b[K]: the reference arithmetic of one pair."""
    with np.errstate(over="ignore"):
        s = tok * a[None, :] + b[None, :]
    return (s % MERSENNE) & np.uint64(0xFFFFFFFF)


def _two_smallest(x):
    part = np.partition(x, 1, axis=-1)
    return part[..., 0], part[..., 1]


def _sort3(x, y, z):
    """(v_min3_u32, v_med3_u32) of three arrays."""
    lo, hi = np.minimum(np.minimum(x, y), z), np.maximum(np.maximum(x, y), z)
    with np.errstate(over="ignore"):
        return lo, (x ^ y ^ z ^ lo ^ hi)


def network_two_smallest(key):
    """The kernel's network over key[..., 16]: five triples give (smallest, middle) each; the two smallest of the row are
    the two smallest of L = {five smallest, key 15} and the middles: k1 = min L, k2 = min(second smallest of L, min middles)."""
    lo, mid = zip(*[_sort3(key[..., 3 * i], key[..., 3 * i + 1], key[..., 3 * i + 2]) for i in range(5)])
    a1, a2 = _sort3(lo[0], lo[1], lo[2])
    b1, b2 = _sort3(lo[3], lo[4], key[..., 15])
    k1 = np.minimum(a1, b1)
    k2 = np.minimum(np.minimum(np.maximum(a1, b1), np.minimum(a2, b2)), np.minimum.reduce(mid))
    return k1, k2


def sieve_model_block(tok, a, b, partial_cols=16):
    """One block: tok[n, T] with T a multiple of 16, T <= 256; the last row holds `partial_cols` tokens (the cells behind
    them are stale and masked, as in the dedup launch's compacted tile).  Returns (ok[n, K], pick[n, K]): whether the
    proof passes and the index of the one token that is then hashed exactly."""
    n, t = tok.shape
    assert t % 16 == 0 and 0 < t <= 256 and 0 < partial_cols <= 16
    r = t // 16
    lo = (tok & np.uint64(0xFFFFFFFF)).astype(U32)
    a_lo = (a & np.uint64(0xFFFFFFFF)).astype(U32)
    b8 = ((b + np.uint64(8)) & np.uint64(0xFFFFFFFF)).astype(U32)
    with np.errstate(over="ignore"):
        m = lo[:, None, :] * a_lo[None, :, None] + b8[None, :, None]  # [n, K, T] mod 2^32
        if partial_cols < 16:
            m[:, :, t - 16 + partial_cols:] = U32(0xFFFFFFFF)
        rowmin = m.reshape(n, -1, r, 16).min(-1)
        tagged = (rowmin & U32(0xFFFFFFF0)) | np.arange(r, dtype=U32)[None, None, :]
        if r == 1:
            r1, r2 = tagged[..., 0], np.full(tagged.shape[:2], 0xFFFFFFFF, U32)
        else:
            r1, r2 = _two_smallest(tagged)
        rows_apart = (r2 - r1) >= U32(32)
        myrow = (r1 & U32(15)).astype(np.int64)
        row_tok = lo.reshape(n, r, 16)[np.arange(n)[:, None], myrow]  # [n, K, 16]
        key = row_tok * a_lo[None, :, None] + b8[None, :, None]
        if partial_cols < 16:
            masked = (myrow == r - 1)[:, :, None] & (np.arange(16) >= partial_cols)[None, None, :]
            key = np.where(masked, U32(0xFFFFFFFF), key)
        key = (key & U32(0xFFFFFFF0)) | np.arange(16, dtype=U32)[None, None, :]
        k1, k2 = network_two_smallest(key)
        s1, s2 = _two_smallest(key)
        assert np.array_equal(k1, s1) and np.array_equal(k2, s2), "the network does not yield the two smallest keys"
        ok = rows_apart & ((k2 - k1) >= U32(32)) & (k1 >= U32(16))
    pick = myrow * 16 + (k1 & U32(15)).astype(np.int64)
    return ok, pick


def sieve_model(tok, a, b, chunk=128):
    """Sets of whole rows, any number of blocks: (ok[n, K], value[n, K]) -- ok where every block's proof passes, value the
    minimum over the blocks of the exact hash of the picked tokens."""
    n, t = tok.shape
    ok = np.ones((n, len(a)), bool)
    val = np.full((n, len(a)), 0xFFFFFFFF, np.uint64)
    for i in range(0, n, chunk):
        for blk in range(0, t, 256):
            part = tok[i:i + chunk, blk:blk + 256]
            o, pick = sieve_model_block(part, a, b)
            ok[i:i + chunk] &= o
            val[i:i + chunk] = np.minimum(val[i:i + chunk], exact_hash(np.take_along_axis(part, pick, axis=1), a, b))
    return ok, val


# ---------------------------------------------------------------------------------------------- crafted sets
ALIAS_J = (1, 8, 15)
ALIAS_DELTA = (0, 1, 15, 16, 47, 48, 49)
NEAR_D = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49)
GUARD_BASE0 = (2**32 - 9, 2**32 - 1, 0, 8, 15, 16, 17)


def odd_perms(a, count):
    """The first `count` permutations whose low multiplier word is odd (invertible mod 2^32)."""
    return [k for k in range(len(a)) if int(a[k]) & 1][:count]


def token_for(a, b, k, s_lo):
    """The 32-bit token whose hash under permutation k has the low word s_lo."""
    a_lo, b_lo = int(a[k]) & 0xFFFFFFFF, int(b[k]) & 0xFFFFFFFF
    return (s_lo - b_lo) * pow(a_lo, -1, 1 << 32) % 2**32


def crafted_cells(a, b, perms, tokens_per_set):
    """A list of placements [(position, token), ...], one per crafted set: the tokens that sit at the bottom of the hash
    range of one permutation.  Positions are < tokens_per_set - 16 and avoid the last row (free for tails and repeats).
      aliases: the minimum at s_lo = 56 + d0 and a token at s_lo = 56 + j 2^28 + d: far above it, yet equal to a near key
               in its low 28 bits.  Nothing in the kernel as it stands treats these specially (a rescan on keys shifted
               left by four bits, which was measured and not kept, would): regression cover; in the minimum's row and
               in another;
      near:    two tokens d apart in one row (columns 0/15, 0/1, 14/15) and across a row boundary (15 | 0);
      guards:  the minimum at s_lo = base0 where the exact value wraps or the key base is below 16."""
    rows = (tokens_per_set - 16) // 16
    assert rows >= 2
    out = []
    for n_k, k in enumerate(perms):
        r0 = n_k % rows
        r1 = (r0 + 1) % rows
        for j in ALIAS_J:
            for d in ALIAS_DELTA:
                for d0 in (0, 3):
                    lo_min, lo_alias = token_for(a, b, k, 56 + d0), token_for(a, b, k, 56 + j * 2**28 + d)
                    out.append([(16 * r0 + 5, lo_min), (16 * r0 + 9, lo_alias)])
                    out.append([(16 * r0 + 9, lo_min), (16 * r0 + 5, lo_alias)])
                    out.append([(16 * r0 + 5, lo_min), (16 * r1 + 9, lo_alias)])
        for d in NEAR_D:
            for base0 in (56, 1000):
                t0, t1 = token_for(a, b, k, base0), token_for(a, b, k, base0 + d)
                for c0, c1 in ((0, 15), (15, 0), (0, 1), (14, 15)):
                    out.append([(16 * r0 + c0, t0), (16 * r0 + c1, t1)])
                lo_r, hi_r = min(r0, r1), max(r0, r1)
                out.append([(16 * lo_r + 15, t0), (16 * hi_r, t1)])
                out.append([(16 * lo_r + 15, t1), (16 * hi_r, t0)])
        for base0 in GUARD_BASE0:
            for d in (None, 1, 40):
                cells = [(16 * r0 + 7, token_for(a, b, k, base0 % 2**32))]
                if d is not None:
                    cells.append((16 * r0 + 8, token_for(a, b, k, (base0 + d) % 2**32)))
                out.append(cells)
    return out


def crafted_sets(a, b, tokens_per_set, n_perms=2, seed=3, wide=True, perms=None):
    """tok[n, tokens_per_set] (uint64): random filler with the crafted cells put in, for the first n_perms odd
    permutations (or those listed in `perms`); with `wide`, every other set carries random high words (they change the
    exact value, never the key)."""
    rng = np.random.RandomState(seed)
    cells = crafted_cells(a, b, odd_perms(a, n_perms) if perms is None else perms, tokens_per_set)
    tok = rng.randint(0, 2**32, (len(cells), tokens_per_set), dtype=np.uint64)
    for i, placed in enumerate(cells):
        for pos, lo in placed:
            tok[i, pos] = lo
    if wide:
        tok[1::2] |= rng.randint(0, 2**32, tok[1::2].shape, dtype=np.uint64) << np.uint64(32)
    return tok
