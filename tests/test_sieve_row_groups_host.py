"""Without a GPU: the four-row fold of the sieve's row minima (Two::add4) as a host program, and the crafted corpora of
tests/test_gpu_sieve_row_groups.py checked against the numpy path."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from datasketch_amd import MinHash
from datasketch_amd.hashfunc import prehashed
from tests import sieve_row_groups_cases as C
from tests.sieve_rescan_model import exact_hash, sieve_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compilers():
    """(compiler, flags that link the sanitizer runtimes statically): a dynamic runtime insists on being the first library
    of the process, which it is not wherever something else is preloaded."""
    out = []
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++")):
        if cand and os.path.exists(cand):
            out.append((cand, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libsan"]))
    for cand in (shutil.which("g++"), shutil.which("c++")):
        if cand:
            out.append((cand, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]))
    return out


def test_add4_equals_four_adds_on_the_host(tmp_path):
    """tests/add4_fold_check.cpp: add4 against four add calls on every sextuple over {0, 1, 2, 2^32-1}, 10^6 random ones
    (equal values and 2^32-1 among them) and whole blocks folded in groups; built with the address and undefined-behaviour
    sanitizers by the first compiler that has their runtimes, plain otherwise."""
    compilers = _compilers()
    assert compilers, "no C++ compiler found"
    src, exe = os.path.join(ROOT, "tests", "add4_fold_check.cpp"), str(tmp_path / "add4_fold_check")
    for cxx, flags in compilers + [(compilers[0][0], [])]:
        p = subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + flags + [src, "-o", exe], capture_output=True, text=True)
        if p.returncode == 0:
            break
    assert p.returncode == 0, p.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert run.stdout.split() == ["ok", str(4096 + 1000000 + 200000)]


def test_shorter_signatures_are_prefixes_of_the_reference():
    """What lets one 256-permutation reference serve K = 128, 136 and 192."""
    a256, b256 = C.permutations(C.K_MAX)
    for k in (128, 136, 192):
        a, b = C.permutations(k)
        assert np.array_equal(a, a256[:k]) and np.array_equal(b, b256[:k])
    tok = np.ascontiguousarray(C.tokens(True)[:8, :80])
    want = MinHash.bulk_signatures(tok, num_perm=136, seed=C.SEED, hashfunc=prehashed, gpu_mode="disable")
    assert np.array_equal(C.reference(tok)[:, :136], want)


@pytest.mark.parametrize("kind", list(C.GAPS))
def test_planted_sets_have_the_intended_gaps(kind):
    """Under the numpy path: permutation k's signature is the exact hash of the planted token; its two smallest keys sit in
    the intended cells, GAPS[kind] apart, everything else above 2^28; and the model of the proof passes permutation k for
    every set of "apart" and fails it for every set of "close" and "tie"."""
    tok, k, where = C.planted(kind)
    a, b = C.permutations(C.PLANT_K)
    assert int(a[k]) & 1 and len(where) == 8 * 7 + 8 and tok.shape == (len(where), 128)
    key = C.sieve_keys(tok, a, b, k)
    order = np.argsort(key, axis=1, kind="stable")
    for i, ((r0, c0), (r1, c1)) in enumerate(where):
        p0, p1 = 16 * r0 + c0, 16 * r1 + c1
        assert {int(order[i, 0]), int(order[i, 1])} == {p0, p1}
        assert int(key[i, p0]) == C.BASE_S + 8 and int(key[i, p1]) - int(key[i, p0]) == C.GAPS[kind]
        assert int(key[i, order[i, 2]]) > C.FILLER_FLOOR
        assert (tok[i, p0] == tok[i, p1]) == (kind == "tie")
    sig = MinHash.bulk_signatures(tok, num_perm=C.PLANT_K, seed=C.SEED, hashfunc=prehashed, gpu_mode="disable")
    planted_tok = np.array([[tok[i, 16 * r0 + c0], tok[i, 16 * r1 + c1]] for i, ((r0, c0), (r1, c1)) in enumerate(where)])
    exact = np.minimum(exact_hash(planted_tok[:, :1], a[k:k + 1], b[k:k + 1]), exact_hash(planted_tok[:, 1:], a[k:k + 1], b[k:k + 1]))
    assert np.array_equal(sig[:, k], exact[:, 0])
    ok, val = sieve_model(tok, a, b)
    assert ok[:, k].all() if kind == "apart" else not ok[:, k].any()
    if kind == "apart":  # nearly every set passes for all 128 permutations: the sets reach the kernel's fold, not its fallback
        assert ok.all(axis=1).mean() > 0.9
        assert np.array_equal(val[ok], sig[ok])
