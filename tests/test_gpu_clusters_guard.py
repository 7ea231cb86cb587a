"""Guard pages behind (and in front of) every buffer of the connected-components device entry points (run on an MI355X).

tests/cc_guard_cases.py drives mhx_cc_init_dev, mhx_cc_link_pairs_dev, mhx_cc_link_bands_dev, mhx_cc_finish_dev and the host form
mhx_cc_pairs -- the path, the star, counts with a floor, hand-made and sorted bands -- on exact-size allocations of
mhx_debug_guard_alloc, in a process of its own: an over-read kills that process, which is the failure.  That the byte past such
a buffer is unmapped is shown by tests/test_guard_pages.py's positive control.
"""
import os

import pytest

from tests.test_guard_pages import _run, vmm  # noqa: F401  (the fixture that checks the virtual-memory API is usable)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("align", [16, 4, -16], ids=["tail_rounded_to_16_bytes", "tail_rounded_to_4_bytes", "front"])
def test_cc_dev_entry_points_on_buffers_that_abut_an_unmapped_page(vmm, align):  # noqa: F811
    rc, out = _run([os.path.join("tests", "cc_guard_cases.py"), str(align)], env_extra={"GUARD_VERBOSE": "1"}, timeout=600)
    assert rc == 0 and "CC GUARD OK" in out, f"guard run (align {align}) died or failed, rc={rc}:\n" + out[-4000:]
