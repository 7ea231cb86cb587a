"""The cases of tests/index_width_cases.py, checked without a device: a case that silently stopped testing anything fails here.

For every case: the touched indices really pass the mark, in the unit stated for the entry; one item really straddles it (from
M - 37 where the layout is free); a decoy never answers like the real data; nothing larger than 64 MB is compared; the compact data
gives the same answer through a second host definition.  Over all cases: no more than 64 GiB are ever allocated at a time, and the
ids the GPU module is parametrised with are the ids the builders make.
"""
import numpy as np
import pytest

from tests import index_width_cases as C

ALL_IDS = [i for ids in C.CASE_IDS.values() for i in ids]
MARKS = {"byte": 2 ** 32, "signed": 2 ** 31, "unsigned": 2 ** 32}  # written out again: a mark edited in the cases module is noticed here


def check_geometry(case: C.Case) -> None:
    """Raises AssertionError when the placement of a case no longer exercises its mark."""
    assert case.mark == MARKS[case.unit], f"{case.id}: its mark is {case.mark}, the {case.unit} mark is {MARKS[case.unit]}"
    roles = {it.role for it in case.items}
    assert {C.BELOW, C.ABOVE} <= roles, f"{case.id}: needs a control below the mark and an item above it, has {sorted(roles)}"
    for it in case.items:
        assert it.first <= it.last
        if it.role == C.BELOW:
            assert it.last < case.mark, f"{case.id}: a 'below' item reaches {it.last} >= {case.mark}"
        elif it.role == C.ABOVE:
            assert it.first >= case.mark, f"{case.id}: an 'above' item starts at {it.first} < {case.mark}"
        else:
            assert it.role == C.ACROSS_ROLE and it.first < case.mark <= it.last, f"{case.id}: the 'across' item [{it.first}, {it.last}] does not straddle {case.mark}"
    assert max(it.last for it in case.items) >= case.mark
    if case.across_first_elem is not None:
        m = MARKS[case.unit] // case.elem_bytes if case.unit == "byte" else MARKS[case.unit]
        assert C.ACROSS_ROLE in roles, f"{case.id}: no item straddles the mark"
        assert case.across_first_elem == m - C.ACROSS, f"{case.id}: the straddling item starts at {case.across_first_elem}, not at M - {C.ACROSS}"
        assert (case.across_first_elem * case.elem_bytes) % 16 != 0  # so that a 16-byte load straddles too


def check_decoys(case: C.Case) -> None:
    """Raises AssertionError when some row that a wrap would move has a decoy that answers like the real data."""
    with_decoys = 0
    for call in case.calls:
        for chk in call.checks:
            assert chk.expected.nbytes <= C.MAX_DOWNLOAD_BYTES, f"{case.id} {chk.what}: compares {chk.expected.nbytes} bytes"
            rows = max(len(chk.roles), 1)
            want = chk.expected.reshape(rows, -1)
            assert set(chk.decoys) == set(chk.moved)
            for name, decoy in chk.decoys.items():
                assert decoy.shape == chk.expected.shape and decoy.dtype == chk.expected.dtype
                moved = np.asarray(chk.moved[name]).reshape(-1)
                assert moved.shape == (rows,) and moved.any()
                same = (decoy.reshape(rows, -1) == want).all(axis=1)
                assert not (same & moved).any(), f"{case.id} {call.what} {chk.what}: the decoy at {name} answers like the real data in rows {np.flatnonzero(same & moved)[:8]}"
                assert same[~moved].all(), f"{case.id} {call.what} {chk.what}: rows that {name} does not move differ from the expected ones"
            if chk.decoys:
                with_decoys += 1
                for r, role in enumerate(chk.roles):  # whatever reaches past the mark has a decoy somewhere
                    if role in (C.ABOVE, C.ACROSS_ROLE):
                        assert any(np.asarray(m).reshape(-1)[r] for m in chk.moved.values()), f"{case.id} {call.what} {chk.what}: row {r} ({role}) has no decoy"
    assert with_decoys or case.no_decoys, f"{case.id}: no check has a decoy"


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_case_passes_its_mark_and_its_decoys_differ(case_id):
    case = C.case(case_id)
    check_geometry(case)
    check_decoys(case)
    assert case.live_bytes() <= C.MAX_LIVE_BYTES


@pytest.mark.parametrize("case_id", ALL_IDS)
def test_compact_data_agrees_with_a_second_host_definition(case_id):
    case = C.case(case_id)
    assert case.definition is not None
    case.definition()


def test_the_ids_of_the_gpu_module_are_the_ids_the_builders_make():
    assert set(C.CASE_IDS) == set(C.BUILDERS)
    for entry, ids in C.CASE_IDS.items():
        assert [c.id for c in C.cases_of(entry)] == ids


def test_no_case_allocates_more_than_64_GiB_at_a_time():
    largest = max(C.all_cases(), key=lambda c: c.live_bytes())
    assert largest.live_bytes() <= 64 * C.GiB, f"{largest.id} allocates {largest.live_bytes()} bytes"
    assert largest.live_bytes() > 16 * C.GiB  # (and the accounting counts the large buffers at all)


def test_the_sparse_model_reads_plants_fill_and_wrapped_images():
    big = C.Big("x", np.uint32, (1 << 32) + 100, 0x5A)
    big.plant((1 << 32) - 3, np.arange(1, 9, dtype=np.uint32))
    big.plant_decoys((1 << 32) - 3, 8, lambda src: np.full(src.size, 7, dtype=np.uint32))
    assert big.read((1 << 32) - 4, 10).tolist() == [0x5A5A5A5A, 1, 2, 3, 4, 5, 6, 7, 8, 0x5A5A5A5A]
    wrap = C.wraps(4)["index mod 2^32"]
    assert big.read_wrapped((1 << 32) - 3, 8, wrap).tolist() == [1, 2, 3, 7, 7, 7, 7, 7]  # the part above the mark comes from the decoy at 0
    assert big.moved((1 << 32) - 3, 8, wrap) and not big.moved((1 << 32) - 3, 3, wrap)
    assert big.read_wrapped((1 << 32) - 3, 3, C.wraps(4)["byte offset mod 2^32"]).tolist() == [7, 7, 7]  # byte 2^34 - 12 wraps to 2^32 - 12
    with pytest.raises(AssertionError):
        big.plant((1 << 32), np.zeros(2, dtype=np.uint32))  # overlaps the first plant


def test_a_mark_shrunk_by_hand_is_noticed():
    """What the geometry check is for: the same case with its mark moved so that nothing straddles must fail."""
    import copy

    case = copy.copy(C.case("mhx_sha1_tokens_dev-byte"))
    case.mark = case.mark + 200  # the straddling token ends below it now
    with pytest.raises(AssertionError):
        check_geometry(case)
    case = copy.copy(C.case("mhx_minhash_bulk_dev-uint32-signed-long"))
    case.across_first_elem += 1
    with pytest.raises(AssertionError):
        check_geometry(case)


def test_a_result_that_equals_a_decoy_is_reported_by_the_name_of_the_wrap():
    """The live test of the comparison, kept: hand it the decoy's answer as the result and the message names the wrap; hand it
    the expected answer and there is no message."""
    chk = C.case("mhx_minhash_bulk_dev-uint32-unsigned-long").calls[0].checks[0]
    assert C.describe_mismatch(chk.expected.copy(), chk) == ""
    name = "index mod 2^32"
    moved = np.flatnonzero(chk.moved[name])
    msg = C.describe_mismatch(chk.decoys[name].copy(), chk)
    assert f"{moved.size} of {len(chk.roles)} rows differ" in msg
    assert f"row {moved[0]} ({chk.roles[moved[0]]}): equals the decoy at {name}" in msg
    other = chk.expected.copy()
    other[moved[0], 0] ^= 1
    assert "equals no decoy" in C.describe_mismatch(other, chk)
