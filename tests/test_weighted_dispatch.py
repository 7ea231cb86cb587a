"""The dispatch mirror of the dense weighted walk (tests/weighted_dispatch.py) on worked cases: launch_weighted_dense_walk
(datasketch_amd/csrc/weighted_kernels.hip) evaluated by hand for an MI355X (256 CUs, 160 KB of LDS per workgroup).  The GPU
tests name their cases and size their grids by the mirror; these pin what it says.  No device needed."""
import pytest

from tests.weighted_dispatch import dense_walk_launch


@pytest.mark.parametrize(
    "dim,s,logs,aligned,options,name,rows_per_turn",
    [
        # 4096 columns, 128 samples: two chunks -> the fetcher / walker split, seven stripes per CU
        (4096, 128, True, True, {}, "walk_wave_NV16_PAIRS_false_FETCH2_SPLIT2", 256 * 7),
        # 4 columns, 1 sample: stripes of 144 bytes beside 10 KB of cached tables, 14 workgroups of eight waves per CU
        (4, 1, True, True, {}, "walk_wave_NV4_PAIRS_true_FETCH0_SPLIT0", 14 * 256 * 8),
        # 1020 columns, 300 samples (five chunks: no split), 4 336-byte stripes: two workgroups per CU
        (1020, 300, True, True, {}, "walk_wave_NV4_PAIRS_true_FETCH0_SPLIT0", 2 * 256 * 8),
        (1020, 300, False, True, {}, "walk_wave_NV4_PAIRS_true_FETCH0_SPLIT0", 2 * 256 * 8),
        # not a multiple of 4: the workgroup-per-row kernel without its 16-byte loads, four workgroups per CU
        (63, 64, True, True, {}, "walk_dense_AHEAD_false", 4 * 256),
        # weighted.kernel 1: the workgroup-per-row kernel always
        (300, 70, True, True, {"weighted.kernel": 1}, "walk_dense_AHEAD_true", 4 * 256),
        # a matrix that does not start on 16 bytes
        (256, 128, False, False, {}, "walk_dense_AHEAD_false", 4 * 256),
        # weighted.min_dim 64: 60 columns go to the workgroup kernel, 64 stay with the wave kernel
        (60, 128, True, True, {"weighted.min_dim": 64}, "walk_dense_AHEAD_true", 4 * 256),
        (64, 128, True, True, {"weighted.min_dim": 64}, "walk_wave_NV4_PAIRS_false_FETCH2_SPLIT2", 256 * 7),
        # six chunks: two rows walked at a time, three stripes, four fetchers (a turn: a row per fetcher)
        (100, 384, False, True, {}, "walk_wave_NV4_PAIRS_false_FETCH2_SPLIT2", 256 * 4),
        # weighted.refill 6 at two chunks: five stripes, six fetchers (a turn: a row per fetcher)
        (16, 128, True, True, {"weighted.refill": 6}, "walk_wave_NV4_PAIRS_false_FETCH2_SPLIT2", 256 * 6),
        # weighted.refill 13: the one-wave-per-row kernel without the split
        (4096, 128, True, True, {"weighted.refill": 13}, "walk_wave_NV16_PAIRS_true_FETCH2_SPLIT0", 256 * 8),
        # values in at 4096 columns: chunk after chunk, non-temporal loads with the early refill
        (4096, 300, False, True, {}, "walk_wave_NV16_PAIRS_false_FETCH3_SPLIT0", 256 * 7),
        (4096, 300, True, True, {}, "walk_wave_NV16_PAIRS_true_FETCH2_SPLIT0", 256 * 7),
        # weighted.kernel 2: chunk after chunk at every width, never the split; 528-byte stripes, six workgroups per CU
        (100, 128, True, True, {"weighted.kernel": 2}, "walk_wave_NV4_PAIRS_false_FETCH0_SPLIT0", 6 * 256 * 8),
        # beyond 4096 columns
        (4100, 128, True, True, {}, "walk_dense_AHEAD_false", 4 * 256),
        (2048, 129, True, True, {}, "walk_wave_NV8_PAIRS_false_FETCH2_SPLIT2", 256 * 5),
    ],
)
def test_dense_walk_dispatch_worked_cases(dim, s, logs, aligned, options, name, rows_per_turn):
    launch = dense_walk_launch(dim, s, logs, aligned, options)
    assert launch.name == name
    assert launch.rows_per_turn == rows_per_turn


def test_dense_walk_dispatch_below_1024_columns():
    """Every width from 4 to 1020 that is a multiple of 4 goes to the wave kernel with NV = 4 (weighted.min_dim 4, round 6);
    2, 3, 4 or 6 chunks of samples to its fetcher / walker form, any other count to the one-wave-per-row form."""
    for dim in range(4, 1024, 4):
        for s in (1, 64, 65, 128, 129, 192, 256, 257, 320, 321, 384, 385, 513):
            launch = dense_walk_launch(dim, s, True)
            assert launch.kernel == "walk_wave" and launch.nv == 4, (dim, s)
            assert launch.split == (2 if (s + 63) // 64 in (2, 3, 4, 6) else 0), (dim, s)
        assert dense_walk_launch(dim + 1, 128, True).name == "walk_dense_AHEAD_false"
        assert dense_walk_launch(dim, 128, True, aligned=False).name == "walk_dense_AHEAD_false"
        assert dense_walk_launch(dim, 128, True, options={"weighted.kernel": 1}).name == "walk_dense_AHEAD_true"
