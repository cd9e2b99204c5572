"""The fine-to-coarse sweep of vx_lod.inl (k_lod_open: cases (a)-(d)) restated in numpy and compared with the least fixed point
of tests/lod_oracle.py, without a GPU.  The device runs the same four cases per node; the GPU tests compare its output with
the oracle, this test checks the sweep itself over every size, level count, camera and range set of tests/test_lod.py."""
import numpy as np
import pytest

from lod_oracle import Selection, dist2, node_boxes, ref_levels
from test_lod import SIZES, cameras, range_sets


def sweep(n, levels, cam, ranges):
    c0, R, T = n // 16, ref_levels(n), levels - 1
    cnt = [c0 >> L for L in range(T + 1)]
    ranges = np.asarray(ranges, np.float32)
    op = [np.zeros((c,) * 3, bool) for c in cnt]
    for L in range(1, T + 1):
        c = cnt[L]
        r = ranges[L]
        o = np.zeros((c,) * 3, bool)
        if r > 0:                                                              # (a) rule 1
            mn, mx = node_boxes(c, L)
            o |= dist2(mn, mx, cam) < np.float32(r * r)
        if L + 1 == R and L == T and (c0 & (c0 - 1)):                           # (d) the level without transitions, odd size
            o[:] = True
        if L >= 2:
            if cnt[L - 2] % 2 == 1 and cnt[L - 1] % 2 == 0:                     # (c) band roots of level L-2
                o[-1, :, :] = o[:, -1, :] = o[:, :, -1] = True
            # (b) children or their outside face neighbours opened: the cross dilation of level L-1 over each 2x2x2 block
            a = np.pad(op[L - 1], 1)
            d = a[1:-1, 1:-1, 1:-1] | a[:-2, 1:-1, 1:-1] | a[2:, 1:-1, 1:-1] | a[1:-1, :-2, 1:-1] | a[1:-1, 2:, 1:-1] \
                | a[1:-1, 1:-1, :-2] | a[1:-1, 1:-1, 2:]
            m = 2 * c
            o |= d[:m, :m, :m].reshape(c, 2, c, 2, c, 2).any((1, 3, 5))
        op[L] = o
    return op


@pytest.mark.parametrize("n", [s for s in SIZES if s < 1000])
def test_sweep_is_the_least_fixed_point(n):
    cases = 0
    for levels in range(1, ref_levels(n) + 1):
        for k, cam in enumerate(cameras(n, n + levels + 7, 5)):
            for j, ranges in enumerate(range_sets(n, cam)):
                want = Selection(n, levels, cam, ranges)
                got = sweep(n, levels, cam, ranges)
                for L in range(1, levels):
                    assert np.array_equal(got[L], want.open[L]), (n, levels, k, j, L)
                cases += 1
    assert cases == ref_levels(n) * 25


def test_sweep_needs_cases_b_c_and_d():
    """Each case of the sweep is needed somewhere: drop one and some selection differs from the fixed point."""
    r = np.zeros(16, np.float32)
    r[1] = 40.0
    # (b): only level 1 split by distance, balance must open everything above it near the camera
    s = Selection(256, 5, np.float32([8, 8, 8]), r)
    assert s.open[3].any() and not any(s.rule1[L].any() for L in (2, 3, 4))
    # (c) and (d): a far camera on an odd size still opens the band edge (208: levels 2 and 3)
    s = Selection(208, 4, np.float32([1e6, 1e6, 1e6]), np.zeros(16, np.float32))
    assert s.open[3].all() and s.open[2][-1, :, :].all() and not s.open[1].any()
