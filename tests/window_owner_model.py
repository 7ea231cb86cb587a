"""A numpy model of how sha1_windows_kernel (csrc/sha1_kernels.hip) finds the document of every window, and the corpus shapes
of its tests.

The kernel hands every wave `per_wave` consecutive windows, 64 per trip.  The wave finds the document of its first window
once (wave_owner_of: a 64-way search over the set offsets) and then follows the documents trip by trip: where a trip reaches
past the wave's document, the lanes load the offsets of the next 64 documents, one each, every lane counts by a binary search
across the lanes how many of them start at or before its window, and a ballot moves the wave's document on; a trip that spans
more than 64 documents takes further such batches.

This file re-states that lane by lane: `launch_plan` is the launcher's blocks / per_wave arithmetic, `wave_owner_of` the
search (also returning its rounds), `window_owners` the trip loop.  A wave is an array of 64 lanes; every __shfl and readlane
is an index into the 64 values the lanes hold, every __ballot a count over them.  What the model returns is held to
np.searchsorted by tests/test_window_owner_model.py (CPU); that the kernel computes the same is what
tests/test_gpu_text_shapes.py checks, hash by hash against hashlib.  The model also reports what a corpus reaches -- batches
per trip, rounds per search, ties in front of a wave's first document -- so that the shapes below can say what they are for
and the tests can assert it.

A shape is a list of per-document window counts: 0 = an empty document, 1 = a document no longer than the shingle, c > 1 = a
document of width + c - 1 items.  `byte_corpus` and `token_corpus` turn one into a corpus.
"""
import numpy as np


LANES = np.arange(64, dtype=np.int64)
DEFAULT_CUS = 256  # an MI355X; the GPU tests ask the device
RUN_LENGTHS = (63, 64, 65, 127, 128, 129, 200)
LONG = 70  # a document of more windows than a trip


def set_offsets_of(counts):
    out = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64), out=out[1:])
    return out


def reference_owners(set_offsets):
    """The document of every window, by definition: the last one whose first window is <= t."""
    return np.searchsorted(set_offsets[:-1], np.arange(int(set_offsets[-1])), side="right") - 1


# ---------------------------------------------------------------------------------------------- the launcher and the kernel
def launch_plan(n_windows, cus):
    """(blocks, per_wave) of launch_sha1_windows."""
    want = (n_windows + 255) // 256
    blocks = max(1, min(want, cus * 32))
    waves = blocks * 4
    per_wave = ((n_windows + waves - 1) // waves + 63) // 64 * 64
    return blocks, per_wave


def wave_owner_of(set_offsets, n_docs, t, tie="last"):
    """(the document that owns window t, the rounds of the search).  tie='first' is a mutation for the tests: the first of
    the documents that share the owner's offset instead of the last."""
    lo, hi, rounds = 0, n_docs - 1, 0
    while lo < hi:
        step = (hi - lo + 63) // 64
        probe = lo + (LANES + 1) * step
        holds = np.zeros(64, dtype=bool)
        inside = probe <= hi
        holds[inside] = set_offsets[probe[inside]] <= t
        found = lo + int(np.count_nonzero(holds)) * step  # popcount of the ballot
        hi = min(hi, found + step - 1)
        lo = found
        rounds += 1
    if tie == "first":
        while lo > 0 and set_offsets[lo - 1] == set_offsets[lo]:
            lo -= 1
    return lo, rounds


class Report:
    """What window_owners saw: owner[t]; per wave (first window, its document, rounds of the search, tied documents in front
    of it); per trip that loaded offsets (first window, batches, whether a batch held both real and past-the-end documents)."""

    def __init__(self, n_windows, per_wave, blocks):
        self.owner = np.full(n_windows, -1, dtype=np.int64)
        self.per_wave, self.blocks = per_wave, blocks
        self.waves, self.trips = [], []

    @property
    def rounds(self):
        return {w[2] for w in self.waves}

    @property
    def max_batches(self):
        return max([t[1] for t in self.trips], default=0)

    @property
    def max_ties_at_a_first_window(self):
        return max([w[3] for w in self.waves], default=0)

    def wave_first_owners(self):
        return {w[1] for w in self.waves}


def window_owners(set_offsets, cus=DEFAULT_CUS, tie="last", first_batch_only=False):
    """The document sha1_windows_kernel assigns to every window, wave by wave and trip by trip, as a Report.
    tie and first_batch_only are mutations for the tests."""
    set_offsets = np.asarray(set_offsets, dtype=np.int64)
    n_docs, n_windows = set_offsets.size - 1, int(set_offsets[-1])
    if n_windows == 0:
        return Report(0, 0, 0)
    blocks, per_wave = launch_plan(n_windows, cus)
    rep = Report(n_windows, per_wave, blocks)
    for wave in range(blocks * 4):
        base = wave * per_wave
        end = min(base + per_wave, n_windows)
        if base >= end:
            continue
        cur, rounds = wave_owner_of(set_offsets, n_docs, base, tie)
        ties = 0
        while cur - ties > 0 and set_offsets[cur - ties - 1] == set_offsets[cur]:
            ties += 1
        rep.waves.append((base, cur, rounds, ties))
        cur_next = int(set_offsets[cur + 1])
        while base < end:
            last = min(base + 63, n_windows - 1)
            t = base + LANES
            d = np.full(64, cur, dtype=np.int64)
            if last >= cur_next:
                moved, batches, mixed, nxt = 0, 0, False, cur + 1
                while True:
                    j = nxt + LANES
                    rel = np.clip(set_offsets[np.minimum(j, n_docs)] - base, 0, 65)
                    rel_63 = rel[63]  # readlane 63
                    started = np.zeros(64, dtype=np.int64)
                    for s in (32, 16, 8, 4, 2, 1):
                        started += np.where(rel[started + s - 1] <= LANES, s, 0)  # __shfl(rel, started + s - 1)
                    d += np.where(rel_63 <= LANES, 64, started)
                    moved += int(np.count_nonzero((j < n_docs) & (rel <= 64)))  # popcount of the ballot
                    batches += 1
                    mixed = mixed or (j[0] < n_docs < j[63])
                    if rel_63 > 64 or nxt + 63 >= n_docs or first_batch_only:
                        break
                    nxt += 64
                d = np.minimum(d, n_docs - 1)
                cur = min(cur + moved, n_docs - 1)
                cur_next = int(set_offsets[cur + 1])
                rep.trips.append((base, batches, mixed))
            live = t < n_windows
            rep.owner[t[live]] = d[live]
            base += 64
    return rep


# ---------------------------------------------------------------------------------------------- shapes
class Shape:
    """Per-document window counts, built front to back."""

    def __init__(self):
        self.counts = []

    @property
    def windows(self):
        return sum(self.counts)

    def add(self, *counts):
        self.counts += [int(c) for c in counts]
        return self

    def long_to(self, offset, modulus=64):
        """One long document after which the next one starts at a window index = offset (mod modulus)."""
        return self.add(LONG + (offset - self.windows - LONG) % modulus)

    def fill_to(self, total):
        assert total - self.windows >= LONG, (total, self.windows)
        return self.add(total - self.windows)


def one_window_runs():
    """Runs of 63 .. 200 one-window documents that begin at trip offset 0, 1 and 63, a long document on both sides."""
    s = Shape()
    for offset in (0, 1, 63):
        for run in RUN_LENGTHS:
            s.long_to(offset).add(*[1] * run)
    return s.add(LONG + 5).counts


def starts_of_runs(counts, value, at_least=63):
    """(window index at which the run begins, its length) of every run of `value` of at_least documents."""
    counts = np.asarray(counts)
    offsets = set_offsets_of(counts)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], (counts == value).astype(np.int8), [0]])))
    return [(int(offsets[a]), int(b - a)) for a, b in zip(edges[::2], edges[1::2]) if b - a >= at_least]


EMPTY_RUNS_TOTAL = 20000  # windows: under one CU the launcher then hands a wave more than one trip


def empty_runs(edge_run, cus=(DEFAULT_CUS, 1), total=EMPTY_RUNS_TOTAL):
    """Runs of empty documents: `edge_run` of them at the very start and at the very end; every length of RUN_LENGTHS between
    two long documents and between two one-window documents; and, for every CU count of `cus`, one run whose successor starts
    exactly on a multiple of the launcher's per_wave (at the default grid that is a multiple of 64: a trip's first window)."""
    s = Shape().add(*[0] * edge_run)
    for run in RUN_LENGTHS:
        s.add(LONG + run % 7).add(*[0] * run).add(LONG)
        s.add(1, 1).add(*[0] * run).add(1, 1)
    for c in cus:
        s.long_to(0, launch_plan(total, c)[1]).add(*[0] * 65).add(LONG)
    return s.fill_to(total).add(*[0] * edge_run).counts


def mixed_runs():
    """One-window documents with three empty ones behind each: a trip of 64 windows spans 256 documents -- four batches and
    more -- once in the middle of the corpus and once as its last trip, which ends inside a batch."""
    s = Shape().add(LONG).long_to(0).add(*[1, 0, 0, 0] * 70).add(LONG)
    s.long_to(0).add(*[1, 0, 0, 0] * 40).add(1, 0, 0, 0, 0)
    return s.counts


def random_counts(seed, n_docs, weights=(0.45, 0.4, 0.1, 0.04, 0.01)):
    """n_docs window counts out of {0, 1, 2, 70, 130}, documents with windows at both ends."""
    rng = np.random.RandomState(seed)
    counts = rng.choice([0, 1, 2, 70, 130], size=n_docs, p=weights)
    counts[0], counts[-1] = (130, 130) if n_docs < 3 else (1, 2)
    return counts.tolist()


def random_runs(seed):
    """A few hundred to a few thousand documents in runs: long runs of 0 and of 1, short ones of 2, 70 and 130."""
    rng = np.random.RandomState(seed)
    counts = []
    for _ in range(rng.randint(3, 14)):
        value = (0, 1, 2, 70, 130)[rng.randint(5)]
        length = rng.randint(1, 300) if value < 2 else rng.randint(1, 4)
        counts += [value] * length
    return counts


DEEP_DOCS = 270000  # documents: more than a 64-way search settles in three rounds


def deep_search(n_docs=DEEP_DOCS, seed=3):
    """About 270 000 documents of which some 3 000 have a window.  The first and the last document, a document on a probe
    position of the search's first round and its two neighbours have more windows than any wave takes (260: per_wave is at
    most 256 for this total, under one CU too), so each of them owns some wave's first window."""
    rng = np.random.RandomState(seed)
    counts = np.zeros(n_docs, dtype=np.int64)
    some = rng.choice(n_docs, size=3150, replace=False)
    counts[some[:2700]], counts[some[2700:2900]], counts[some[2900:]] = 1, 2, LONG
    for d in deep_search_marks(n_docs):
        counts[d] = 260
    return counts.tolist()


def deep_search_marks(n_docs=DEEP_DOCS):
    probe = 5 * ((n_docs - 1 + 63) // 64)  # lo + (lane + 1) * step of round one, lane 4
    return [0, probe - 1, probe, probe + 1, n_docs - 1]


# ---------------------------------------------------------------------------------------------- shapes as corpora
def byte_corpus(counts, width, seed=0):
    """(buf, doc_offsets): documents of random bytes with these window counts at this width; one-window documents cycle through
    1 .. width bytes."""
    rng = np.random.RandomState(seed)
    counts = np.asarray(counts, dtype=np.int64)
    short = 1 + np.cumsum(counts == 1) % width
    lengths = np.where(counts == 0, 0, np.where(counts == 1, short, counts + width - 1))
    doc_offsets = set_offsets_of(lengths)
    return rng.randint(0, 256, size=int(doc_offsets[-1]), dtype=np.uint8), doc_offsets


def token_corpus(counts, w, seed=0):
    """(buf, item_offsets, doc_offsets): the same in tokens of 0 .. 3 bytes, so that every window fits one SHA-1 block."""
    rng = np.random.RandomState(seed + 1)
    _, doc_offsets = byte_corpus(counts, w, seed)  # the same arithmetic, in tokens
    item_offsets = set_offsets_of(rng.randint(0, 4, size=int(doc_offsets[-1])))
    return rng.randint(0, 256, size=int(item_offsets[-1]), dtype=np.uint8), item_offsets, doc_offsets
