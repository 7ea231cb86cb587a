"""The corpora of tests/test_gpu_learned_first_launch.py: small sets of known kinds for the first launch that a context
has learned (MODE_SIEVE_TIES, the tie-tolerant proof), and the prototypes that teach a context its mode word.

Kinds (the label of every set; tokens are built through the modular inverse of an odd a_lo, see sieve_rescan_model):
  clean                distinct random tokens
  one_tie              the exact arg-min token of a target permutation occurs twice: in one 16-token row, or in two rows
                       of one 256-token block.  The one-candidate proof fails, the tie-tolerant one holds.
  one_tie_other_block  the copy lies in another 256-token block: every block has one candidate, BOTH proofs hold
  one_tie_tail         the copy lies in the ragged tail (the last len % 16 tokens), which the fast fold takes: both hold
  two_close            two different tokens whose keys are the two smallest and d apart, d in NEAR_D (d = 0: equal low
                       words, different high words -- uint64 tokens only)
  triple               the arg-min token three times: the tie-tolerant proof fails, the dedup pass settles the set
  three_close          three different tokens with keys 1000, 1007, 1021: nothing to drop, the pairwise launch
  crafted              crafted_sets of sieve_rescan_model: aliases, near pairs, wraps, guard bases
  near_top             one row of sixteen tokens whose keys are the largest there are, 8 apart: above the guard on keys near
                       2^32, refused; near_top_edge: 16 apart, the best key's base is the guard's 0xFFFFFF00 itself, accepted
                       with two candidates (ragged form only)
  tiny                 empty, one-token, shorter-than-a-row, one- and two-row sets of random tokens (ragged form only)
Target permutations: one of the first 64-permutation slot and one of the last (the shared slot for K in 129..160 and
193..224).  one_tie* sets are redrawn until the model says the launch settles them (a random third key in the window
is possible, one in 10^5); triple and three_close defeat the proof by construction, which is asserted.
"""
import numpy as np

from tests.sieve_rescan_model import NEAR_D, crafted_sets, exact_hash, odd_perms, sieve_model, token_for
from tests.sieve_ties_model import first_launch_model, ties_model_tied

U64 = np.uint64
LOW = U64(0xFFFFFFFF)
SETTLED_KINDS = ("one_tie", "one_tie_other_block", "one_tie_tail")
DEFEATING_KINDS = ("triple", "three_close")   # (near_top too, in the ragged form: the model says so, the test asserts it)
N_TEACH = 8192   # sets of a teaching call: 2048 workgroups, 128 of them publish their wave 0's count (>= 64 needed)
N_PROTO = 64


def target_perms(a):
    """An odd permutation (odd_perms: invertible low multiplier word) of the first 64-permutation slot and one of the last."""
    odd = odd_perms(a, len(a))
    last = (len(a) - 1) // 64 * 64
    assert odd[0] < 64 and odd[-1] >= last and odd[0] != odd[-1], "no odd multiplier in a slot"
    return [odd[0], odd[-1]]


def _filler(rng, t, wide):
    tok = rng.randint(0, 2**32, t, dtype=U64)
    if wide:
        tok |= rng.randint(0, 2**32, t, dtype=U64) << U64(32)
    return tok


def _with_low(tok, lo):
    """The token with its low word replaced (the key of a token is made of its low word alone)."""
    return (tok & ~LOW) | U64(lo)


class _Place:
    """Where the crafted minimum of a set goes: a random row r0 of a random 256-token block of the whole rows."""

    def __init__(self, rng, body):
        self.rows = body // 16
        self.r0 = int(rng.randint(0, self.rows))
        self.first = self.r0 // 16 * 16
        self.in_block = min(16, self.rows - self.first)   # rows of r0's block (1: the single row of a last block)

    def after(self, i):
        """The i-th row after r0 in its block, going round."""
        return self.first + (self.r0 - self.first + i) % self.in_block


def _argmin_to_r0(tok, a, b, k, body, at):
    """Move the exact arg-min over the whole rows -- what the sieve sees; the tail goes through the fast fold -- to (r0, 3)."""
    src = int(np.argmin(exact_hash(tok[None, :body], a[k:k + 1], b[k:k + 1])[0]))
    dst = 16 * at.r0 + 3
    tok[[src, dst]] = tok[[dst, src]]
    return dst


def _one_tie(tok, variant, rng, a, b, k, body):
    at = _Place(rng, body)
    src = _argmin_to_r0(tok, a, b, k, body, at)
    if variant % 2 and at.in_block >= 2:
        tok[16 * at.after(1 + int(rng.randint(0, at.in_block - 1))) + 7] = tok[src]   # another row of the block
    else:
        tok[16 * at.r0 + 12] = tok[src]                                                # the same row


def _one_tie_other_block(tok, variant, rng, a, b, k, body):
    assert body > 256
    at = _Place(rng, body)
    src = _argmin_to_r0(tok, a, b, k, body, at)
    blocks = [blk for blk in range(-(-body // 256)) if blk != at.r0 // 16]
    blk = blocks[int(rng.randint(0, len(blocks)))]
    tok[256 * blk + int(rng.randint(0, min(256, body - 256 * blk)))] = tok[src]


def _one_tie_tail(tok, variant, rng, a, b, k, body):
    assert len(tok) > body
    src = _argmin_to_r0(tok, a, b, k, body, _Place(rng, body))
    tok[body + int(rng.randint(0, len(tok) - body))] = tok[src]


def _triple(tok, variant, rng, a, b, k, body):
    at = _Place(rng, body)
    src = _argmin_to_r0(tok, a, b, k, body, at)
    if variant % 3 == 1 and at.in_block >= 3:
        dst = [16 * at.after(1) + 1, 16 * at.after(2) + 15]   # three rows, a cell each
    elif variant % 3 == 2 and at.in_block >= 2:
        dst = [16 * at.after(1) + 1, 16 * at.after(1) + 15]   # the best row with one cell, another row with two
    else:
        dst = [16 * at.r0 + 9, 16 * at.r0 + 14]               # three cells of one row
    tok[dst] = tok[src]


def _two_close(tok, variant, rng, a, b, k, body):
    at = _Place(rng, body)
    d = NEAR_D[variant % len(NEAR_D)]
    p0 = 16 * at.r0 + int(rng.randint(0, 16))
    if (variant // len(NEAR_D)) % 2 == 0 or at.in_block < 2:
        p1 = 16 * at.r0 + (p0 + 1 + int(rng.randint(0, 15))) % 16   # the same row
    else:
        p1 = 16 * at.after(1) + int(rng.randint(0, 16))              # two rows of one block
    tok[p0], tok[p1] = _with_low(tok[p0], token_for(a, b, k, 992)), _with_low(tok[p1], token_for(a, b, k, 992 + d))
    if d == 0:   # the same key, another token: uint64 tokens only
        tok[p1] = _with_low(tok[p0] + (U64(1) << U64(32)), token_for(a, b, k, 992))


def _three_close(tok, variant, rng, a, b, k, body):
    """Three neighbours, all in one block (split over two blocks each block would be settled): in one row, the smallest
    alone at the end of a row and two in the next, two and one, or anywhere."""
    inner = [r for r in range(body // 16 - 1) if r % 16 != 15]   # rows followed by a row of the same block
    r = inner[int(rng.randint(0, len(inner)))]
    at = {0: 16 * r + int(rng.randint(0, 14)), 1: 16 * r + 15, 2: 16 * r + 14}.get(variant % 4)
    while at is None or at // 256 != (at + 2) // 256:
        at = int(rng.randint(0, body - 3))
    for i, s_lo in enumerate((992, 999, 1013)):   # keys 1000, 1007, 1021
        tok[at + i] = _with_low(tok[at + i], token_for(a, b, k, s_lo))


def _near_top(tok, variant, rng, a, b, k, body, step=8):
    """One row whose sixteen keys are the largest there are, 8 apart: the best key's base is above the guard's 0xFFFFFF00
    and the 2^32 - 1 that stands for "no second row" is close -- refused."""
    assert body == 16
    order = rng.permutation(16)
    for c in range(16):
        tok[c] = _with_low(tok[c], token_for(a, b, k, (2**32 - 1 - step * int(order[c]) - 8) % 2**32))


def _near_top_edge(tok, variant, rng, a, b, k, body):
    """The same 16 apart: the base IS 0xFFFFFF00, two keys in the window -- accepted."""
    _near_top(tok, variant, rng, a, b, k, body, step=16)


_MAKERS = {"clean": lambda *args: None, "one_tie": _one_tie, "one_tie_other_block": _one_tie_other_block, "one_tie_tail": _one_tie_tail,
           "triple": _triple, "two_close": _two_close, "three_close": _three_close, "near_top": _near_top, "near_top_edge": _near_top_edge}


def _one_set(kind, variant, rng, a, b, k, t, body, wide):
    """One set of `t` tokens whose crafted cells lie in [0, body) (body a multiple of 16: the whole rows); `variant`
    chooses where the companions of the crafted minimum go."""
    tok = _filler(rng, t, wide)
    assert wide or not (kind == "two_close" and NEAR_D[variant % len(NEAR_D)] == 0)
    _MAKERS[kind](tok, variant, rng, a, b, k, body)
    return tok


def _checked(kind, variant, rng, a, b, k, t, body, wide):
    for _ in range(50):
        tok = _one_set(kind, variant, rng, a, b, k, t, body, wide)
        if kind not in SETTLED_KINDS or first_launch_model([tok], a, b)[0]:
            return tok
    raise AssertionError(f"no {kind} set that the model settles in 50 draws")


def kind_sets(a, b, t, body, wide, targets, seed, per_kind=4, near_variants=None, shift=0):
    """[(kind, tokens[t]), ...] of the hand-made kinds for one set length; near_variants: which of the 2 len(NEAR_D)
    two_close variants (distance, then same row / next row) to make, all by default; shift: added to the variant numbers
    of the other kinds (a caller that makes few sets per call goes round the variants with it)."""
    rng = np.random.RandomState(seed)
    near_variants = range(2 * len(NEAR_D)) if near_variants is None else near_variants
    out = [("clean", _one_set("clean", 0, rng, a, b, 0, t, body, wide)) for _ in range(4 * per_kind)]
    for k in targets:
        for v in range(2 * per_kind):
            out.append(("one_tie", _checked("one_tie", v + shift, rng, a, b, k, t, body, wide)))
        if body > 256:
            for v in range(per_kind):
                out.append(("one_tie_other_block", _checked("one_tie_other_block", v, rng, a, b, k, t, body, wide)))
        if t > body:
            for v in range(per_kind):
                out.append(("one_tie_tail", _checked("one_tie_tail", v, rng, a, b, k, t, body, wide)))
        for v in near_variants:
            if NEAR_D[v % len(NEAR_D)] == 0 and not wide:
                continue
            out.append(("two_close", _one_set("two_close", v, rng, a, b, k, t, body, wide)))
        for v in range(max(3, per_kind)):   # (three cells of one row; three rows; one and two)
            out.append(("triple", _one_set("triple", v, rng, a, b, k, t, body, wide)))
        for v in range(per_kind):
            out.append(("three_close", _one_set("three_close", v + shift, rng, a, b, k, t, body, wide)))
    return out


def fixed_cases(a, b, t, wide, targets=None, seed=1):
    """(tok[n, t] uint64, kinds[n]) for sets of one length: the hand-made kinds and every set of crafted_sets for the target
    permutations, crafted cells in the whole rows ([0, t - t % 16))."""
    targets = target_perms(a) if targets is None else targets
    body = t // 16 * 16
    sets = kind_sets(a, b, t, body, wide, targets, seed)
    # crafted_sets keeps its cells below tokens_per_set - 16: a length of body + 16 lets them use every whole row
    crafted = crafted_sets(a, b, body + 16, seed=seed + 2, wide=wide, perms=targets)[:, :t]
    tok = np.concatenate([np.stack([s for _, s in sets]), crafted])
    kinds = np.array([k for k, _ in sets] + ["crafted"] * len(crafted))
    _check_intent([row for row in tok], kinds, a, b)
    return tok, kinds


def ragged_cases(a, b, wide, targets=None, seed=1, full_lengths=(64, 272, 288, 544)):
    """(sets: list of uint64 arrays, kinds[n]): lengths 16 r + tail with tail 0..15 round the kinds -- sets of
    full - 16 + tail tokens for every `full` (48.., 256.., 272.. and 528..: 3, 16, 16 + 1 and 16 + 16 + 1 rows, so two of
    them end in a block of a single row), the crafted cells in the whole rows: the hand-made kinds at four tails and every
    set of crafted_sets at every length, the tails going round so that every member of its alias and near groups (of three
    and six sets) meets every tail -- sets of one row whose keys lie just below 2^32, and empty, one-token, shorter-than-a-row and one- and
    two-row sets."""
    targets = target_perms(a) if targets is None else targets
    rng = np.random.RandomState(seed + 100)
    sets, kinds = [], []
    for full in full_lengths:
        body = full - 16
        for shift, tail in enumerate((0, 1, 8, 15)):   # the hand-made kinds at four tails (every crafted set below, at all sixteen)
            near = [(tail + 3 * j) % (2 * len(NEAR_D)) for j in range(8)]   # the distances and placements go round
            for kind, s in kind_sets(a, b, body + tail, body, wide, targets, seed + 1000 * full + tail, per_kind=1, near_variants=near,
                                     shift=shift):
                sets.append(s)
                kinds.append(kind)
        crafted = crafted_sets(a, b, full, seed=seed + full, wide=wide, perms=targets)
        for i, row in enumerate(crafted):
            # crafted_cells makes its sets in groups of three and six: i // 6 + i moves a member of a group of six on by 7 tails
            # from group to group, one of a group of three by 7 every two groups -- through all sixteen (the 7 guard groups
            # per permutation are too few for that)
            sets.append(row[:body + (i // 6 + i) % 16].copy())
            kinds.append("crafted")
    for k in targets:
        for kind in ("near_top", "near_top_edge"):
            for m in (16, 16, 21, 31):
                sets.append(_one_set(kind, 0, rng, a, b, k, m, 16, wide))
                kinds.append(kind)
    for m in (0, 1, 0, 1, 2, 7, 15, 16, 17, 31, 32, 33, 0):
        sets.append(_filler(rng, m, wide))
        kinds.append("tiny")
    kinds = np.array(kinds)
    _check_intent(sets, kinds, a, b)
    return sets, kinds


def _check_intent(sets, kinds, a, b):
    """The kinds land where they are meant to, according to the model."""
    for kind in DEFEATING_KINDS:
        idx = np.flatnonzero(kinds == kind)
        assert not first_launch_model([sets[i] for i in idx], a, b).any(), kind


def csr(sets, dtype=U64):
    """(hv, offsets) of a list of sets."""
    off = np.concatenate([[0], np.cumsum([len(s) for s in sets])]).astype(np.int64)
    hv = np.concatenate(sets).astype(dtype) if len(sets) else np.empty(0, dtype)
    return hv, off


def initial_state(n, k, seed=9):
    """[n, k] uint64 hashvalues to start from: a third >= 2^32 (the reference's empty value is 2^32 - 1, larger ones clamp to
    it against a hash), a third 2^32 - 1, a third below 2^24 (which win against the minimum of 250 hashes about half the
    time)."""
    rng = np.random.RandomState(seed)
    which = rng.randint(0, 3, (n, k))
    big = rng.randint(2**32, 2**40, (n, k), dtype=U64)
    small = rng.randint(0, 2**24, (n, k), dtype=U64)
    return np.where(which == 0, big, np.where(which == 1, U64(0xFFFFFFFF), small)).astype(U64)


# ---------------------------------------------------------------------------------------------- teaching
def teaching_prototypes(a, b, kind, seed=21):
    """N_PROTO sets of 256 uint64 tokens, all of one kind under the K = 128 permutations (a, b), as the models say:
      clean    the one-candidate proof holds for every permutation (sieve_model)
      one_tie  the one-candidate proof fails (a tie), the tie-tolerant one holds everywhere
      triple   the tie-tolerant proof fails
    so the ratios a teaching call publishes are 0 or 1."""
    rng = np.random.RandomState(seed)
    odd = [p for p in range(len(a)) if int(a[p]) & 1]
    out = []
    while len(out) < N_PROTO:
        k = odd[len(out) % len(odd)]
        tok = _one_set(kind, len(out), rng, a, b, k, 256, 256, True)
        if kind == "clean":
            good = sieve_model(tok[None, :], a, b)[0].all()
        else:
            ok, _, tied = ties_model_tied(tok[None, :], a, b)
            good = (ok.all() and tied.any()) if kind == "one_tie" else not ok.all()
        if good:
            out.append(tok)
    return np.stack(out)


def tiled(protos, n=N_TEACH):
    return np.tile(protos, (-(-n // len(protos)), 1))[:n]
