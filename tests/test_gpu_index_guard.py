"""Guard pages behind (and in front of) every buffer of the index update and digest layout device entry points (run on an MI355X).

tests/index_guard_cases.py drives mhx_lsh_bands_merge_dev, mhx_lsh_bands_compact_dev, mhx_rows_compact_dev,
mhx_band_digests_layout_dev, mhx_lsh_sort_digests_layout_dev and mhx_bbit_pack_band_digests_dev -- odd counts that put the later
bands on addresses that are no multiple of 16, a bitmap of exactly ceil(n / 32) words, the four access units of a row, both
layouts -- on exact-size allocations of mhx_debug_guard_alloc, in a process of its own: an over-read kills that process, which
is the failure.  That the byte past such a buffer is unmapped is shown by tests/test_guard_pages.py's positive control.
"""
import os

import pytest

from tests.test_guard_pages import _run, vmm  # noqa: F401  (the fixture that checks the virtual-memory API is usable)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("align", [16, 4, -16], ids=["tail_rounded_to_16_bytes", "tail_rounded_to_4_bytes", "front"])
def test_index_dev_entry_points_on_buffers_that_abut_an_unmapped_page(vmm, align):  # noqa: F811
    rc, out = _run([os.path.join("tests", "index_guard_cases.py"), str(align)], env_extra={"GUARD_VERBOSE": "1"}, timeout=600)
    assert rc == 0 and "INDEX GUARD OK" in out, f"guard run (align {align}) died or failed, rc={rc}:\n" + out[-4000:]
