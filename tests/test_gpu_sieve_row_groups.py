"""The sieve's row loop folds the row minima of uint64 tokens into the two smallest four rows at a time (Two::add4 in
csrc/minhash_kernels.hip; the rows left over, and the kernels that keep it, one at a time): bit for bit against the numpy
path, MinHash.bulk_signatures(..., hashfunc=prehashed, gpu_mode="disable").

Corpora and references come from tests/sieve_row_groups_cases.py; tests/test_sieve_row_groups_host.py checks on the CPU that
the planted sets are what they are meant to be.

Run on an MI355X:  python -m pytest tests/test_gpu_sieve_row_groups.py -m gpu -q
"""
import numpy as np
import pytest

from datasketch_amd import MinHash, _native
from datasketch_amd.hashfunc import prehashed
from tests import sieve_row_groups_cases as C

pytestmark = pytest.mark.gpu

KS = (128, 136, 192, 256)  # two per lane; three with a shared last slot; three; four


@pytest.fixture(scope="module")
def ctx():
    assert _native.gpu_available(), "these tests need an MI355X"
    c = _native.context()
    # one wave per set (these corpora are small enough for the split kernels otherwise), and the one-candidate proof as the
    # first launch whatever the previous corpus was: the launches under test
    c.set_option("minhash.split", 1)
    c.set_option("minhash.adapt", 1)
    yield c
    for key in ("minhash.split", "minhash.adapt"):
        c.set_option(key, 0)


def _device_tokens(tok, wide):
    return np.ascontiguousarray(tok) if wide else np.ascontiguousarray(tok).astype(np.uint32)


@pytest.mark.parametrize("wide", [True, False], ids=["uint64", "uint32"])
@pytest.mark.parametrize("k", KS)
def test_fixed_length_sets_around_the_group_size(ctx, k, wide):
    """512 sets of 16 r distinct random tokens, r = 1 .. 33: whole groups of four rows, every remainder, a second block with
    a short last group (the kernel without tail code)."""
    perms = C.permutations(k)
    for rows in C.ROWS:
        tok = _device_tokens(C.tokens(wide)[:, :16 * rows], wide)
        got = ctx.minhash_bulk(perms, tok.reshape(-1), None, 16 * rows, C.N_SETS)
        assert np.array_equal(got, C.dense_reference(wide, rows)[:, :k]), rows


@pytest.mark.parametrize("wide", [True, False], ids=["uint64", "uint32"])
@pytest.mark.parametrize("k", KS)
def test_csr_sets_with_and_without_tails(ctx, k, wide):
    """The same sets as CSR, a third of them as they are and the others with 1 or 15 tokens behind the last whole row: the
    plain kernel with offsets, and -- counting switched on -- the general one."""
    perms = C.permutations(k)
    values, offsets, want = C.ragged(wide)
    hv = _device_tokens(values, wide)
    n = len(offsets) - 1
    got = ctx.minhash_bulk(perms, hv, offsets, 0, n)
    assert np.array_equal(got, want[:, :k])
    ctx.counters(True)
    try:
        got = ctx.minhash_bulk(perms, hv, offsets, 0, n)
    finally:
        ctx.counters(False)
    assert np.array_equal(got, want[:, :k])


def test_sets_split_over_waves(ctx):
    """K = 128 through the split kernel (slices of whole blocks and of 64 tokens): its row loop is the same one."""
    perms = C.permutations(128)
    ctx.set_option("minhash.split", 2)
    try:
        for rows in (4, 7, 20, 33):
            tok = np.ascontiguousarray(C.tokens(True)[:64, :16 * rows])
            got = ctx.minhash_bulk(perms, tok.reshape(-1), None, 16 * rows, len(tok))
            assert np.array_equal(got, C.dense_reference(True, rows)[:64, :128]), rows
    finally:
        ctx.set_option("minhash.split", 1)


@pytest.mark.parametrize("kind", ["close", "tie"])
def test_planted_sets_through_the_dedup_launch(ctx, kind):
    """The sets whose proof fails, with the tie-tolerant second launch switched off: the dedup launch takes them, and its row
    loop over the compacted tile (8 rows, or 7 and a partial one where the repeat is dropped) folds four rows at a time too."""
    tok, k, where = C.planted(kind)
    want = MinHash.bulk_signatures(tok, num_perm=C.PLANT_K, seed=C.SEED, hashfunc=prehashed, gpu_mode="disable")
    ctx.set_option("minhash.ties", 1)
    try:
        got = ctx.minhash_bulk(C.permutations(C.PLANT_K), np.ascontiguousarray(tok).reshape(-1), None, tok.shape[1], len(tok))
        flags = ctx.minhash_flags(len(tok))
    finally:
        ctx.set_option("minhash.ties", 0)
    assert np.array_equal(got, want)
    assert (flags >= 1).all()


@pytest.mark.parametrize("kind", list(C.GAPS))
def test_the_two_smallest_keys_in_every_pair_of_rows(ctx, kind):
    """One permutation's smallest and second smallest key planted in rows (i, j), every i != j of 0..7 and i = j: 4096 apart
    the proof passes -- the set is settled by the first launch, through the fold --, 8 apart or tied (the same token twice)
    it cannot (a key gap below 32 is never certified) and every such set is redone.  Signatures equal the numpy path's in
    all three."""
    tok, k, where = C.planted(kind)
    want = MinHash.bulk_signatures(tok, num_perm=C.PLANT_K, seed=C.SEED, hashfunc=prehashed, gpu_mode="disable")
    ctx.counters(True)
    try:
        got = MinHash.bulk_signatures(tok, num_perm=C.PLANT_K, seed=C.SEED, hashfunc=prehashed, gpu_mode="always")
    finally:
        c = ctx.counters(False)
    assert np.array_equal(got, want)
    print(kind, c)
    if kind == "apart":
        assert c["sieve_sets_redone"] < len(where), c
    else:
        assert c["sieve_sets_redone"] >= len(where), c
