"""Guard pages behind (and in front of) every buffer of the all-pairs Jaccard device entry points (run on an MI355X).

tests/jaccard_matrix_guard_cases.py drives mhx_jaccard_matrix_dev, mhx_jaccard_threshold_pairs_dev and their b-bit twins -- one
row past a tile, one word past a chunk, the triangle, a wider ldc, a pair list of exactly the total and one below it -- on
exact-size allocations of mhx_debug_guard_alloc, in a process of its own: an over-read kills that process, which is the failure.
That the byte past such a buffer is unmapped is shown by tests/test_guard_pages.py's positive control.
"""
import os

import pytest

from tests.test_guard_pages import _run, vmm  # noqa: F401  (the fixture that checks the virtual-memory API is usable)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("align", [16, 4, -16], ids=["tail_rounded_to_16_bytes", "tail_rounded_to_4_bytes", "front"])
def test_matrix_dev_entry_points_on_buffers_that_abut_an_unmapped_page(vmm, align):  # noqa: F811
    rc, out = _run([os.path.join("tests", "jaccard_matrix_guard_cases.py"), str(align)], env_extra={"GUARD_VERBOSE": "1"}, timeout=600)
    assert rc == 0 and "MATRIX GUARD OK" in out, f"guard run (align {align}) died or failed, rc={rc}:\n" + out[-4000:]
