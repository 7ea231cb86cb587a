"""The weighted Jaccard device entry points in the sweeps every `_dev` entry goes through (run on an MI355X): on poisoned scratch
and allocations, behind in-flight work on their stream, and with their data past 2^31 / 2^32 elements and byte 2^32.

tests/weighted_jaccard_sweep_cases.py holds the cases and borrows the machinery of tests/poison_cases.py,
tests/stream_order_cases.py and tests/index_width_cases.py unchanged; what those sweeps assert and why is written there.  The
poison and stream-order cases run in a child process each, with a time limit: once a child has died of a signal or a time limit
nothing more is started on the card by this module.  Nothing here provokes a fault: decoys and far rows are valid inputs inside
the caller's own allocations.
"""
import os
import re
import subprocess
import sys

import pytest

from datasketch_amd import _native
from tests import weighted_jaccard_sweep_cases as cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join("tests", "weighted_jaccard_sweep_cases.py")
LIMIT = 120  # seconds: a dozen small synchronised calls per child, a plug of tens of milliseconds per stream-order case

_DIED = None  # the test whose child died of a signal or a time limit: nothing is started after it


def _child(args, what):
    global _DIED
    if _DIED is not None:
        pytest.fail(f"not started: the child of {_DIED} died of a signal or a time limit, the card is not used further", pytrace=False)
    assert _native.gpu_available(), "these tests need an MI355X"
    env = dict(os.environ)
    env.pop("MHX_GUARD_ALLOC", None)
    env.pop("MHX_POISON_ALLOC", None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    try:
        p = subprocess.run([sys.executable, SCRIPT] + args, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _DIED = what
        pytest.fail(f"{what}: no end after {LIMIT} s:\n" + (e.stdout or b"").decode(errors="replace")[-3000:], pytrace=False)
    out = p.stdout.decode(errors="replace")
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _DIED = what
        pytest.fail(f"{what}: the child died, rc={p.returncode}; the last case it names is the one that was running:\n" + out[-3000:], pytrace=False)
    return p.returncode, out


@pytest.mark.parametrize("byte", (0xFF, 0x5A), ids=["0xff", "0x5a"])
def test_the_four_entries_on_poisoned_scratch_and_allocations(byte):
    rc, out = _child(["poison", str(byte)], f"poison[0x{byte:02x}]")
    assert rc == 0 and "POISON OK" in out and f"(weighted_jaccard, byte 0x{byte:02x})" in out, f"rc={rc}:\n" + out[-4000:]
    assert int(re.search(r"POISON OK (\d+) cases", out).group(1)) >= 10  # pairs, matrix, two capacities, six top-k calls


def test_the_four_entries_behind_in_flight_work_on_their_stream():
    rc, out = _child(["stream"], "stream order")
    assert rc == 0, f"the stream-order run died or failed, rc={rc}:\n" + out[-6000:]
    done = re.search(r"^WJ STREAM ORDER OK (\d+) cases, (\d+) rearmed$", out, re.M)
    assert done and int(done.group(1)) == 4, "no final line, or not four cases:\n" + out[-3000:]
    for symbol in _native.EXPORTED_SYMBOLS_WJ:
        assert not symbol.endswith("_dev") or f"ok {symbol} --" in out, symbol
    assert "FAILED" not in out and "unarmed twice" not in out


@pytest.fixture(scope="module")
def width_ctx():
    c = _native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("which", sorted(cases.WIDTH_BUILDERS))
def test_at_scale_weighted_rows_past_element_2_to_the_32_and_byte_2_to_the_32(width_ctx, which):
    """pairs: rows of 2 S uint64 words on both sides of byte 2^32 and of elements 2^31 and 2^32 of one allocation, decoys where a
    32-bit index would land.  matrix, topk: three probes against 2^26 + 3 rows of 256 bytes -- the far rows of B lie past byte 2^32
    and past 32-bit word 2^32 -- whose planted rows have less similar decoys at their wrapped images."""
    from tests import test_gpu_index_width as driver

    if _DIED is not None:
        pytest.fail(f"not started: the child of {_DIED} died of a signal or a time limit, the card is not used further", pytrace=False)
    case = cases.WIDTH_BUILDERS[which]()
    case.definition()
    assert case.live_bytes() <= driver.C.MAX_LIVE_BYTES
    driver.LAUNCH.update(cases.WIDTH_LAUNCH)
    driver.run_case(width_ctx, case)
