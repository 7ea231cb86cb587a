"""Guard pages and poison for the xxHash entry points (run on an MI355X).

tests/xxh_guard_cases.py drives mhx_hash_windows and mhx_hash_tokens -- both kernels, XXH32 and XXH64, window widths 5, 33 and 70,
byte and token mode, byte buffers of every length mod 8 whose first window starts on the first byte and whose last window ends on
the last, which holds for the packed tokens of mhx_hash_tokens too -- and six of the `_hashed` chains on exact-size allocations of mhx_debug_guard_alloc, in a process of its own: an
over-read kills that process, which is the failure.  That the byte past such a buffer is unmapped is shown by
tests/test_guard_pages.py's positive control.  tests/xxh_poison_cases.py runs the same cases with every fresh allocation filled
with 0xFF and with 0x5A and the scratch released before every case: a kernel that reads a word nobody wrote answers wrongly.

These tests show that the kernels stay within their buffers; none of them provokes a fault.  Never more than one process has the
GPU open, every child has a time limit, and once a child has died of a signal or a time limit nothing more is started.
"""
import os
import subprocess

import pytest

from tests.test_guard_pages import _run, vmm  # noqa: F401  (the fixture that checks the virtual-memory API is usable)

pytestmark = pytest.mark.gpu

LIMIT = 120  # seconds per child: about a hundred and fifty small calls and their allocations
_DIED = None  # the test whose child died of a signal or a time limit: nothing is started after it


def _child(args, what, **kwargs):
    global _DIED
    if _DIED is not None:
        pytest.fail(f"not started: the child of {_DIED} died of a signal or a time limit, the card is not used further", pytrace=False)
    try:
        rc, out = _run(args, timeout=LIMIT, **kwargs)
    except subprocess.TimeoutExpired as e:
        _DIED = what
        pytest.fail(f"{what}: no end after {LIMIT} s:\n" + (e.stdout or b"").decode(errors="replace")[-3000:], pytrace=False)
    if rc < 0 or rc in (124, 134, 137, 139):
        _DIED = what
    return rc, out


@pytest.mark.parametrize("align", [16, 4, -16], ids=["tail_rounded_to_16_bytes", "tail_rounded_to_4_bytes", "front"])
def test_xxh_entry_points_on_buffers_that_abut_an_unmapped_page(vmm, align):  # noqa: F811
    rc, out = _child([os.path.join("tests", "xxh_guard_cases.py"), str(align)], f"guard[{align}]", env_extra={"GUARD_VERBOSE": "1"})
    assert rc == 0 and "XXH GUARD OK" in out, f"guard run (align {align}) died or failed, rc={rc}:\n" + out[-4000:]


@pytest.mark.parametrize("byte", [0xFF, 0x5A], ids=["0xff", "0x5a"])
def test_xxh_entry_points_on_poisoned_scratch_and_allocations(byte):
    rc, out = _child([os.path.join("tests", "xxh_poison_cases.py"), str(byte)], f"poison[0x{byte:02x}]")
    assert rc == 0 and "XXH POISON OK" in out and f"(byte 0x{byte:02x})" in out, f"poison run 0x{byte:02x}: rc={rc}:\n" + out[-4000:]
