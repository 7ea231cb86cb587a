"""Without a GPU: the short fold of a proven candidate (fold_proven in csrc/minhash_kernels.hip) as a host program, and
the numpy model of the finishes that use it (tests/sieve_finish_model.py) against the reference arithmetic."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from datasketch_amd import MinHash
from datasketch_amd.hashfunc import prehashed
from tests import sieve_finish_model as F
from tests.sieve_rescan_model import crafted_sets, exact_hash
from tests.sieve_ties_model import ties_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 4
U64 = np.uint64


def _perms(k):
    a, b = MinHash(num_perm=k, seed=SEED, hashfunc=prehashed).permutations
    return np.asarray(a, dtype=U64), np.asarray(b, dtype=U64)


def _compilers():
    """(compiler, flags that link the sanitizer runtimes statically), as tests/test_sieve_row_groups_host.py does."""
    out = []
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if cand and os.path.exists(cand):
            out.append((cand, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]))
    for cand in (shutil.which("g++"), shutil.which("c++")):
        if cand:
            out.append((cand, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]))
    return out


def test_short_fold_equals_exact_fold_under_the_guard_on_the_host(tmp_path):
    """tests/proven_fold_check.cpp: fold_exact against s mod (2^61 - 1), and against the short fold for every top, the
    edges of hi29 and s_lo within 40 of both ends (2 592 cases, those with M < 16 exempt), the two ends of the guarded
    range (128) and 10^6 random s with M >= 16; and two listed s with M = 5 and M = 4 where the two differ.  Built with the
    address and undefined-behaviour sanitizers by the first compiler that has their runtimes, plain otherwise."""
    compilers = _compilers()
    assert compilers, "no C++ compiler found"
    src, exe = os.path.join(ROOT, "tests", "proven_fold_check.cpp"), str(tmp_path / "proven_fold_check")
    for cxx, flags in compilers + [(compilers[0][0], [])]:
        p = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + [src, "-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
    assert p.returncode == 0, p.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.split() == ["ok", str(8 * 4 * 81 + 8 * 4 * 4), "1000000"]


def test_short_fold_differs_without_the_guard():
    """The numpy restatement agrees with the host program's listed cases: M = 5 and M = 4 differ, M = 16 does not."""
    one = np.array([1], dtype=U64)
    for s, differs in (((5 << 61) | (0x1FFFFFFF << 32) | 0xFFFFFFFD, True), ((3 << 61) | (0x1FFFFFFF << 32) | 0xFFFFFFFC, True),
                       ((7 << 61) | (0x1FFFFFFF << 32) | 8, False), ((7 << 61) | (0x1FFFFFFF << 32) | 0xFFFFFFF7, False)):
        tok, b = np.array([[0]], dtype=U64), np.array([s], dtype=U64)   # s = 0 * a + b
        assert (int(F.short_fold(tok, one, b)[0, 0]) != int(exact_hash(tok, one, b)[0, 0])) == differs, hex(s)


@pytest.mark.parametrize("wide", [True, False], ids=["tok64", "tok32"])
def test_modelled_finish_equals_the_reference_where_the_proof_passes(wide):
    """Random sets of 64, 256 and 272 + 240 tokens, every crafted set of sieve_rescan_model (aliases, near pairs, wraps,
    guard bases) and the crafted winners: wherever the modelled proof passes -- one candidate or tie-tolerant -- the
    SHORT fold of the picked candidates is the reference value, per permutation; and the proof refuses every winner
    below the guard or next to 2^32."""
    a, b = _perms(128)
    rng = np.random.RandomState(2)
    corpora = []
    for t, n in ((64, 192), (256, 96), (512, 48)):
        tok = rng.randint(0, 2**32, (n, t), dtype=U64)
        if wide:
            tok |= rng.randint(0, 2**32, (n, t), dtype=U64) << U64(32)
        tok[::3, 5] = tok[::3, 1]   # a third of the sets with a repeated token: the tie-tolerant proof has ties to accept
        corpora.append(tok)
    corpora.append(crafted_sets(a, b, 64, wide=wide))
    win, m, perm, top = F.winner_sets(a, b, wide)
    corpora.append(win)
    passed = 0
    for tok in corpora:
        want = F.reference(tok, a, b)
        sig = MinHash.bulk_signatures(np.ascontiguousarray(tok[:4]), num_perm=128, seed=SEED, hashfunc=prehashed, gpu_mode="disable")
        assert np.array_equal(want[:4], sig)   # (the reference here is the library's numpy path)
        for model in (F.finish_model, F.finish_ties_model):
            ok, val = model(tok, a, b)
            assert np.array_equal(val[ok], want[ok])
            passed += int(ok.sum())
        assert np.array_equal(F.finish_ties_model(tok, a, b)[0], ties_model(tok, a, b)[0])
    assert passed > 50000
    # the winners: the target permutation's verdict and value
    ok, val = F.finish_model(win, a, b)
    own = ok[np.arange(len(win)), perm]
    assert own[np.isin(m, F.SETTLED_M)].all() and not own[~np.isin(m, F.SETTLED_M)].any()
    if wide:
        assert sorted(set(top[m == 16].tolist())) == list(range(8))
    # the short fold of a refused winner is indeed wrong for some of them: the guard is needed, not decoration
    low = np.isin(m, F.GUARDED_M)
    picked_short = F.short_fold(win[np.arange(len(win)), np.where(np.arange(len(win)) % 2 == 0, 0, F.WINNER_T - 1)][:, None], a, b)
    picked_exact = exact_hash(win[np.arange(len(win)), np.where(np.arange(len(win)) % 2 == 0, 0, F.WINNER_T - 1)][:, None], a, b)
    differs = picked_short[np.arange(len(win)), perm] != picked_exact[np.arange(len(win)), perm]
    assert not differs[np.isin(m, F.SETTLED_M)].any()
    if wide:
        # s_lo = 2^32 - 1 and top > 0: the sum carries into the high word, and with hi29 = 2^29 - 1 (one of HI29_EDGES) it
        # reaches 2^61 - 1, where the Mersenne correction is due and the short fold is off by one
        assert differs[low & (m == 7) & (top > 0)].any()


def test_mixed_lengths_give_every_wave_every_length():
    sets = F.mixed_length_sets(True)
    lens = np.array([len(s) for s in sets])
    assert sorted(set(lens.tolist())) == list(F.MIXED_LENGTHS)
    walked = lens.reshape(4, 1024)   # wave w of a 1 024-wave launch walks column w
    assert all(sorted(col) == list(F.MIXED_LENGTHS) for col in walked.T)
    for long, short in ((272, 16), (272, 48), (250, 16), (250, 48)):
        assert ((walked[:-1] == long) & (walked[1:] == short)).any(), (long, short)
    rep = F.mixed_length_sets(True, repeats=0.1)
    assert np.mean([len(np.unique(s)) < len(s) for s in rep]) > 0.95
