"""Every device operation on poisoned scratch and allocations (run on an MI355X: python -m pytest tests/test_gpu_poison.py -m gpu).

The rest of the suite shares one process-wide context whose scratch slots are kept as long as they are big enough: a kernel that
reads a word of scratch nobody wrote usually finds there what an earlier call of the same shape left behind, which is often the
right answer.  Fresh hipMalloc memory is zero on a freshly booted board and arbitrary otherwise.  Here every family of
tests/poison_cases.py runs in a process of its own with mhx_debug_poison_alloc set -- every fresh allocation of the library filled
with one byte -- and mhx_ctx_release_scratch before every case, so that every operation starts on scratch that holds nothing but
the byte.  Two bytes: 0xFF (a NaN, a -1, a huge offset -- but also the identity of min and the "empty" pattern of several tables)
and 0x5A (the identity of nothing: a finite float, a plausible count or row number).  Zero is what the rest of the suite runs on.
Guard pages stay off: this run is about contents, not extents (tests/test_guard_pages.py and its siblings are about those).

Never more than one process has the GPU open.  Once a child has died of a signal or a time limit the card is not used further by
this module: every later test fails at once, without starting a process, naming the test that died.
"""
import os
import subprocess
import sys

import pytest

from datasketch_amd import _native

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BYTES = (0xFF, 0x5A)
# Time limit of a child per family, in seconds: five times the family's run with the poison off on an MI355X (the factor covers the
# synchronising fill of every allocation and a cold start), and at least 60 s.  The measured times are in profiles/poison_runs.txt.
LIMITS = {
    "minhash": 60, "weighted": 60, "pack_lsh": 60, "bucketing": 60, "queries": 60, "index": 60, "forest": 60, "ensemble": 60,
    "jaccard": 60, "topk": 60, "hll": 60, "bloom": 60, "clusters": 60,
}
CONTROL_LIMIT = 60

_DIED = None  # the test whose child died of a signal or a time limit: nothing is started after it


def _run(args, what, timeout):
    """One child process; (return code, output).  A child that is killed or runs into its limit closes the module."""
    global _DIED
    if _DIED is not None:
        pytest.fail(f"not started: the child of {_DIED} died of a signal or a time limit, the card is not used further", pytrace=False)
    env = dict(os.environ)
    env.pop("MHX_GUARD_ALLOC", None)
    env.pop("MHX_POISON_ALLOC", None)  # (the script sets the byte itself, as the first call of the process)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    try:
        p = subprocess.run([sys.executable] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _DIED = what
        pytest.fail(f"{what}: no end after {timeout} s:\n" + (e.stdout or b"").decode(errors="replace")[-3000:], pytrace=False)
    out = p.stdout.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _DIED = what
        pytest.fail(f"{what}: the child died, rc={p.returncode}; the last case it names is the one that was running:\n" + out[-3000:], pytrace=False)
    return p.returncode, out


@pytest.mark.parametrize("byte", BYTES, ids=["0xff", "0x5a"])
def test_control_the_switch_takes_effect_and_can_be_taken_back(byte):
    """Runs first; without it a green run below could mean that the switch never took effect.  In a child with the byte set a
    ctx.alloc(100) downloaded at once holds 100 copies of the byte; after poison_alloc(-1) a buffer filled by upload and then
    downloaded is unchanged.  Nothing is read that was not allocated, nothing is launched."""
    assert _native.gpu_available(), "these tests need an MI355X"
    rc, out = _run([os.path.join("tests", "poison_cases.py"), str(byte), "control"], f"control[0x{byte:02x}]", CONTROL_LIMIT)
    assert rc == 0 and f"POISON CONTROL OK (byte 0x{byte:02x})" in out, f"rc={rc}:\n" + out[-3000:]


@pytest.mark.parametrize("family", list(LIMITS))
@pytest.mark.parametrize("byte", BYTES, ids=["0xff", "0x5a"])
def test_family_on_poisoned_scratch_and_allocations(byte, family):
    rc, out = _run([os.path.join("tests", "poison_cases.py"), str(byte), family], f"{family}[0x{byte:02x}]", LIMITS[family])
    assert rc == 0 and "POISON OK" in out and f"({family}, byte 0x{byte:02x})" in out, f"{family} under 0x{byte:02x}: rc={rc}:\n" + out[-4000:]
