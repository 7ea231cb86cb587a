"""Every `_dev` entry point behind in-flight work on its stream (run on an MI355X).

include/mhx.h promises that a `_dev` entry enqueues on the context's stream and returns without synchronising, that it keeps no host
pointer after it returns, and that calls made one after the other on one context take effect in call order.  tests/stream_order_cases.py
holds every such entry to it in a process of its own: the entry is enqueued behind a plug of the library's own launches that is still
running when the last call is made, its inputs arrive by a device copy enqueued just in front of it (the buffers hold valid decoys until
then), its outputs leave by a copy enqueued just behind it and are overwritten behind that; the result must be that of the synchronised
call on the true inputs, bit for bit, and an entry that is not listed as blocking must have returned while the plug ran.  The script's
positive control runs three entries on a second context, which nothing orders against the first: they must see the decoys, exactly.

Nothing here provokes a fault: decoys and controls are valid inputs throughout.  One child with a time limit; if it dies of a signal or
the time limit runs out, nothing more is started on the card by this module.
"""
import os
import re
import subprocess

import pytest

from datasketch_amd import _native
from tests.test_guard_pages import _run

pytestmark = pytest.mark.gpu

LIMIT = 240  # seconds: about 50 cases of four small synchronised calls and one plug of tens of milliseconds each, and the CPU oracles
_DIED = None  # the test whose child died of a signal or a time limit: nothing is started after it


def _child(args, what):
    global _DIED
    if _DIED is not None:
        pytest.fail(f"not started: the child of {_DIED} died of a signal or a time limit, the card is not used further", pytrace=False)
    try:
        rc, out = _run(args, timeout=LIMIT)
    except subprocess.TimeoutExpired as e:
        _DIED = what
        pytest.fail(f"{what}: no end after {LIMIT} s:\n" + (e.stdout or b"").decode(errors="replace")[-3000:], pytrace=False)
    if rc < 0 or rc in (124, 134, 137, 139):
        _DIED = what
    return rc, out


def test_every_device_entry_point_behind_in_flight_work_on_its_stream():
    assert _native.gpu_available(), "these tests need an MI355X"
    rc, out = _child([os.path.join("tests", "stream_order_cases.py")], "stream order")
    print(out[-6000:])
    assert rc == 0, f"the stream-order run died or failed, rc={rc}:\n" + out[-6000:]
    done = re.search(r"^STREAM ORDER OK (\d+) cases, (\d+) rearmed$", out, re.M)
    assert done, "no final line:\n" + out[-3000:]
    # 46 per-entry cases and mhx_memset_dev, a _dev call in front of each of the two pipelined host calls, the counters, four chains
    assert int(done.group(1)) >= 54, done.group(0)
    control = re.search(r"^STREAM ORDER CONTROL OK 3 entries, (\d+) rearmed$", out, re.M)
    assert control, "the positive control did not reproduce want_decoy on a second context:\n" + out[-3000:]
    assert "FAILED" not in out and "unarmed twice" not in out
