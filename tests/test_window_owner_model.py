"""The lane-by-lane model of sha1_windows_kernel's window-to-document mapping (tests/window_owner_model.py) against
np.searchsorted, without a GPU: on the corpus shapes that tests/test_gpu_text_shapes.py runs on the device and on a few hundred
random offset arrays.  The shapes are also held to what they claim to reach -- trips of three and more batches, searches of
three and four rounds, a long run of ties in front of a wave's first document -- and two mutations of the model (no further
batch; the first of tied documents instead of the last) must be caught.  This pins the arithmetic of the kernel; that the
kernel's cross-lane operations do the same under its control flow is the GPU test's part."""
import numpy as np
import pytest

from tests import window_owner_model as W

CUS = (W.DEFAULT_CUS, 1)
SEARCH_DEPTH_DOCS = (1, 2, 64, 65, 66, 4096, 4097, 4200)
_DEEP = {}


def _deep():
    if not _DEEP:
        _DEEP["offsets"] = W.set_offsets_of(W.deep_search())
        _DEEP["reports"] = {cus: W.window_owners(_DEEP["offsets"], cus) for cus in CUS}
    return _DEEP["offsets"], _DEEP["reports"]


def _check(counts, cus=W.DEFAULT_CUS):
    offsets = W.set_offsets_of(counts)
    rep = W.window_owners(offsets, cus)
    want = W.reference_owners(offsets)
    assert np.array_equal(rep.owner, want), (cus, np.flatnonzero(rep.owner != want)[:8])
    for base, cur, _, _ in rep.waves:
        assert cur == want[base], (cus, base)
    return rep


def test_launch_plan():
    assert W.launch_plan(1, 256) == (1, 64) and W.launch_plan(257, 256) == (2, 64)
    assert W.launch_plan(20000, 256) == (79, 64)             # every wave takes one trip
    assert W.launch_plan(20000, 1) == (32, 192)              # 128 waves of three trips
    assert W.launch_plan(3 * 2**20, 256) == (8192, 128)      # the capped grid
    for n in (1, 63, 64, 65, 8191, 8192, 8193, 20000, 10**6):
        for cus in (1, 3, 256):
            blocks, per_wave = W.launch_plan(n, cus)
            assert per_wave % 64 == 0 and blocks * 4 * per_wave >= n and 1 <= blocks <= 32 * cus


def test_rounds_of_the_search_derived_from_its_loop():
    """A round turns a range of r = hi - lo documents into one of at most ceil(r / 64) - 1 (fewer where the range is cut at
    its upper end): one round up to r = 64, two up to 65 * 64 = 4160, three up to 4161 * 64 = 266 304 -- that is n_docs = 65,
    4 161 and 266 305.  Window 0 takes them all."""
    def rounds(n_docs):
        r, k = n_docs - 1, 0
        while r > 0:
            r, k = (r + 63) // 64 - 1, k + 1
        return k

    assert [rounds(n) for n in (1, 2, 65, 66, 4161, 4162, 266305, 266306)] == [0, 1, 1, 2, 2, 3, 3, 4]
    for n_docs in (1, 2, 65, 66, 4161, 4162):
        offsets = np.arange(n_docs + 1, dtype=np.int64)  # one window each
        assert W.wave_owner_of(offsets, n_docs, 0) == (0, rounds(n_docs))
        for t in (n_docs // 2, n_docs - 1):
            owner, took = W.wave_owner_of(offsets, n_docs, t)
            assert owner == t and took <= rounds(n_docs)
    assert rounds(W.DEEP_DOCS) == 4


def test_one_window_runs():
    counts = W.one_window_runs()
    runs = W.starts_of_runs(counts, 1)
    assert sorted(length for _, length in runs) == sorted(W.RUN_LENGTHS * 3)
    assert {(start % 64, length) for start, length in runs} == {(o, n) for o in (0, 1, 63) for n in W.RUN_LENGTHS}
    for cus in CUS:
        rep = _check(counts, cus)
        assert rep.max_batches == 2  # 64 windows are at most 65 such documents: the second batch only ends the trip


@pytest.mark.parametrize("edge_run", W.RUN_LENGTHS)
def test_empty_runs(edge_run):
    counts = W.empty_runs(edge_run)
    offsets = W.set_offsets_of(counts)
    assert offsets[-1] == W.EMPTY_RUNS_TOTAL and counts[0] == counts[-1] == 0
    runs = W.starts_of_runs(counts, 0)
    assert sorted(n for _, n in runs) == sorted((edge_run,) * 2 + W.RUN_LENGTHS * 2 + (65, 65))
    assert runs[0][0] == 0 and runs[-1][0] == offsets[-1]
    assert any(start % 64 == 0 and start > 0 for start, _ in runs)
    for cus in CUS:
        rep = _check(counts, cus)
        # a run whose successor starts on the launcher's cut, behind the first wave: the search lands behind >= 64 ties
        assert any(start % rep.per_wave == 0 and start > 0 for start, _ in runs)
        assert rep.max_ties_at_a_first_window >= 64 and any(w[0] > 0 and w[3] >= 64 for w in rep.waves)
    assert W.launch_plan(W.EMPTY_RUNS_TOTAL, 1)[1] > 64 == W.launch_plan(W.EMPTY_RUNS_TOTAL, W.DEFAULT_CUS)[1]


def test_mixed_runs():
    counts = W.mixed_runs()
    for cus in CUS:
        rep = _check(counts, cus)
        assert rep.max_batches >= 4
        base, batches, mixed = rep.trips[-1]  # the corpus's last trip: ends inside a batch
        assert base + 64 >= rep.owner.size and batches >= 3 and mixed


@pytest.mark.parametrize("n_docs", SEARCH_DEPTH_DOCS)
def test_document_counts_around_the_search_depths(n_docs):
    counts = W.random_counts(n_docs, n_docs)
    assert len(counts) == n_docs
    want_rounds = 0 if n_docs == 1 else 1 if n_docs <= 65 else 2 if n_docs <= 4161 else 3
    for cus in CUS:
        rep = _check(counts, cus)
        assert max(rep.rounds) == want_rounds


def test_deep_search():
    offsets, reports = _deep()
    want = W.reference_owners(offsets)
    assert offsets.size - 1 == W.DEEP_DOCS and 20000 <= offsets[-1] <= 32768 and np.count_nonzero(np.diff(offsets)) < 4000
    for cus in CUS:
        rep = reports[cus]
        assert np.array_equal(rep.owner, want)
        assert max(rep.rounds) == 4 and len(rep.waves) >= 100
        assert set(W.deep_search_marks()) <= rep.wave_first_owners()
    assert 3 in _check(W.random_counts(4200, 4200)).rounds


def test_random_offset_arrays():
    reached = set()
    for seed in range(300):
        counts = W.random_runs(seed) if seed % 3 else W.random_counts(seed, 20 + 7 * seed)
        if not sum(counts):
            continue
        rep = _check(counts, CUS[seed % 2])
        reached.add(min(rep.max_batches, 3))
    assert reached >= {1, 2, 3}


# ---------------------------------------------------------------------------------------------- the mutations are caught
def test_a_model_without_further_batches_is_caught():
    for counts in (W.mixed_runs(), W.empty_runs(129), W.deep_search()):
        offsets = W.set_offsets_of(counts)
        rep = W.window_owners(offsets, first_batch_only=True)
        assert not np.array_equal(rep.owner, W.reference_owners(offsets))


def test_a_search_that_takes_the_first_of_tied_documents_is_caught():
    """The search's own answer is wrong wherever a wave's first window follows empty documents.  (The trips behind it load
    offsets again whenever the wave's document has no window, so the final mapping can survive this mutation: the search is
    held to the reference by itself, in _check.)"""
    offsets = W.set_offsets_of(W.empty_runs(65))
    want = W.reference_owners(offsets)
    rep = W.window_owners(offsets, tie="first")
    assert any(cur != want[base] for base, cur, _, _ in rep.waves)
    base, cur, _, ties = next(w for w in W.window_owners(offsets).waves if w[3] >= 64)
    assert W.wave_owner_of(offsets, offsets.size - 1, base, tie="first")[0] == cur - ties
