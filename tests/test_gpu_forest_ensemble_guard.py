"""Guard pages behind (and in front of) every buffer of the forest and ensemble device entry points (run on an MI355X).

tests/forest_ensemble_guard_cases.py drives mhx_lsh_forest_build_dev_typed and mhx_lsh_forest_query_dev_typed on rows of exactly
l * tree_words words with probes whose insertion point is position 0 or n of every tree, mhx_lsh_ensemble_query_dev with an
empty partition, a single-row one and one of identical rows, and mhx_lsh_query_dev over identical rows and over one row -- on
exact-size allocations of mhx_debug_guard_alloc, in a process of its own: an over-read kills that process, which is the failure.
That the byte past such a buffer is unmapped is shown by tests/test_guard_pages.py's positive control.
"""
import os

import pytest

from tests.test_guard_pages import _run, vmm  # noqa: F401  (the fixture that checks the virtual-memory API is usable)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("align", [16, 4, -16], ids=["tail_rounded_to_16_bytes", "tail_rounded_to_4_bytes", "front"])
def test_forest_and_ensemble_dev_entry_points_on_buffers_that_abut_an_unmapped_page(vmm, align):  # noqa: F811
    rc, out = _run([os.path.join("tests", "forest_ensemble_guard_cases.py"), str(align)], env_extra={"GUARD_VERBOSE": "1"}, timeout=600)
    assert rc == 0 and "FOREST GUARD OK" in out, f"guard run (align {align}) died or failed, rc={rc}:\n" + out[-4000:]
