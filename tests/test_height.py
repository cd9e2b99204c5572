"""The height maps without a GPU: the numpy statement of the header's text (tests/height_oracle.py) against answers written by
hand, and both host forms of voxels_amd/csrc/tv_height.h (tests/height/height_host.cpp: the plain loop over columns and the
kernel's tile pipeline, sign summaries given and withheld) against that oracle, byte for byte, over the grids and queries the GPU
test uses."""
import numpy as np
import pytest

import height_oracle as ho
import measure_oracle as mo

TOP, BOTTOM, NONE = ho.HEIGHT_FROM_TOP, ho.HEIGHT_FROM_BOTTOM, ho.HEIGHT_NONE
GRIDS = ho.grids()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


def column_grid(samples, mat=None):
    """16^3 of air (127) with `samples` in column (x, y) = (3, 4), z = 0 upwards"""
    d = np.full((16, 16, 16), 127, np.int8)
    m = np.zeros((16, 16, 16), np.uint8)
    d[:len(samples), 4, 3] = samples
    m[:, 4, 3] = np.arange(16) + 10 if mat is None else mat
    return mo.Grid(d, m, np.zeros((16, 16, 16), np.uint8), np.zeros(1, np.uint8))


COLUMN = ((3, 4, 0), (4, 5, 16))


# ---- the oracle against answers written by hand -----------------------------------------------------------------------------------

@pytest.mark.parametrize("d0,d1,f", [(-1, 127, 2), (-128, 127, 128), (-3, 1, 192), (-128, 0, 256), (-1, 0, 256), (-1, 1, 128), (-127, 127, 128)])
def test_the_fraction_by_hand(d0, d1, f):
    assert ho.fraction(d0, d1) == f
    assert ho.load().hh_value(7, d0, d1, 1, 0) == 7 * 256 + f
    assert ho.load().hh_value(7, d0, d1, 0, 0) == 7 * 256 - f
    assert ho.load().hh_value(7, d0, d1, 1, 1) == ho.load().hh_value(7, d0, d1, 0, 1) == 7 * 256
    # one surface at z = 7 with that pair, from the top (air above) and from the bottom (air below)
    g = column_grid([-5] * 7 + [d0, d1])
    h, m, s, c = ho.heightmap(g, COLUMN, TOP, 2, True)
    assert h[:, 0, 0].tolist() == [7 * 256 + f, NONE] and m[:, 0, 0].tolist() == [17, 0] and s[0, 0] == 1
    g = column_grid([127] * 6 + [d1, d0, -5, -5, -5, -5, -5, -5, -5, -5])
    h, m, s, c = ho.heightmap(g, COLUMN, BOTTOM, 1, True)
    assert h[0, 0, 0] == 7 * 256 - f and m[0, 0, 0] == 17 and int(c["clipped"]) == 0


def test_a_column_by_hand():
    #            z = 0    1    2    3   4   5    6    7   8 ...
    g = column_grid([-10, -10, -3, 1, 0, -128, -128, 0, 127])
    # from the top: surfaces at z = 6 (d0 -128, d1 0 -> 256) and z = 2 (d0 -3, d1 1 -> 192)
    h, m, s, c = ho.heightmap(g, COLUMN, TOP, 3, True)
    assert h[:, 0, 0].tolist() == [6 * 256 + 256, 2 * 256 + 192, NONE]
    assert m[:, 0, 0].tolist() == [16, 12, 0] and s[0, 0] == 2
    assert (int(c["columns"]), int(c["covered"]), int(c["surfaces"]), int(c["max_surfaces"]), int(c["clipped"])) == (1, 1, 2, 2, 0)
    assert int(c["min_height"]) == int(c["max_height"]) == 7 * 256
    # from the bottom: z = 0 is solid at the box's end - clipped, h = 0; then z = 5 with z = 4 air (d0 -128, d1 0 -> 256)
    h, m, s, c = ho.heightmap(g, COLUMN, BOTTOM, 3, True)
    assert h[:, 0, 0].tolist() == [0, 5 * 256 - 256, NONE] and m[:, 0, 0].tolist() == [10, 15, 0]
    assert (int(c["covered"]), int(c["surfaces"]), int(c["clipped"]), int(c["min_height"]), int(c["max_height"])) == (1, 2, 1, 0, 0)
    # a clipped surface from the top: the box ends at z1 = 6 inside the solid run 5..6 -> z = 5 clipped, h = 5 * 256
    h, m, s, c = ho.heightmap(g, ((3, 4, 1), (4, 5, 6)), TOP, 2, True)
    assert h[:, 0, 0].tolist() == [5 * 256, 2 * 256 + 192] and int(c["clipped"]) == 1
    # ... and the number a crossing with d1 = 0 one sample further in gives: the full column's layer 0 at z = 6 is 7 * 256, what
    # a box ending at z1 = 8 over a solid z = 7 would report clipped
    # from the bottom with z0 = 1: z = 1 solid at the box's end -> clipped, h = 256
    h, m, s, c = ho.heightmap(g, ((3, 4, 1), (4, 5, 6)), BOTTOM, 1, False)
    assert h[0, 0, 0] == 256 and int(c["clipped"]) == 1 and int(c["surfaces"]) == 0 and int(c["max_surfaces"]) == 0
    # an empty neighbour column: nothing covered
    h, m, s, c = ho.heightmap(g, ((4, 4, 0), (5, 5, 16)), TOP, 1, True)
    assert h[0, 0, 0] == NONE and m[0, 0, 0] == 0 and s[0, 0] == 0
    assert c.tobytes() == np.array([(1, 0, 0, 0, 0, 0, 0, [0, 0])], ho.HEIGHT_COUNTS_DTYPE)[0].tobytes()
    # layer order and the layout of the outputs: two columns side by side
    h, m, s, c = ho.heightmap(g, ((2, 4, 0), (5, 5, 16)), TOP, 2, True)
    assert h.shape == (2, 1, 3) and h[:, 0, :].tolist() == [[NONE, 7 * 256, NONE], [NONE, 2 * 256 + 192, NONE]]
    assert (int(c["columns"]), int(c["covered"])) == (3, 1)


# ---- both host forms against the oracle ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,g", GRIDS, ids=[k for k, _ in GRIDS])
def test_host_forms_equal_the_oracle(name, g):
    for what, box, direction, layers, flag in ho.cases(g.n):
        want = ho.expected(name, g, box, direction, layers, flag)
        for path, skip in ((0, 0), (1, 0), (1, 1)):
            rc, h, m, s, c, _ = ho.host_heightmap(path, g, box, direction, layers, flag, skip)
            assert rc == 0
            same(h, want[0]); same(m, want[1]); same(c, want[3])
            if flag:
                same(s, want[2])
            else:
                assert s is None


def test_materials_may_be_left_out():
    name, g = GRIDS[1]
    box = ((5, 7, 3), (45, 42, 46))
    want = ho.expected(name, g, box, TOP, 2, False)
    for path in (0, 1):
        rc, h, m, s, c, _ = ho.host_heightmap(path, g, box, TOP, 2, False, materials=False)
        assert rc == 0 and m is None
        same(h, want[0]); same(c, want[3])


def test_the_early_exit_and_the_summaries_save_steps():
    name, g = GRIDS[5]          # 80^3 terrain: 25 tiles, stacks of 5 blocks
    box = ((0, 0, 0), (80, 80, 80))
    walked = {}
    for flag in (False, True):
        for skip in (0, 1):
            rc, h, m, s, c, walked[flag, skip] = ho.host_heightmap(1, g, box, TOP, 1, flag, skip)
            same(h, ho.expected(name, g, box, TOP, 1, flag)[0])
    assert walked[True, 0] == 25 * 5                       # every block of every stack
    assert walked[False, 1] <= walked[False, 0] < walked[True, 0] and walked[True, 1] < walked[True, 0]
    # the heights are the same bytes whichever way the walk went
    assert int(ho.expected(name, g, box, TOP, 1, True)[3]["covered"]) == 80 * 80


def test_every_pair_of_samples():
    g = ho.pairs_grid()
    n = g.n
    box = ((0, 0, 0), (n, n, n))
    y, x = np.mgrid[0:n, 0:n]
    want = (5 * 256 + (256 * (x + 1)) // (y + x + 1)).astype(np.uint32)      # d0 = -(x + 1), d1 = y
    for yy, xx in ((0, 0), (127, 0), (0, 127), (127, 127), (1, 2)):
        assert int(want[yy, xx]) == 5 * 256 + ho.fraction(-(xx + 1), yy)
    h, m, s, c = ho.heightmap(g, box, TOP, 1, True)
    same(h[0], want)
    assert (int(c["covered"]), int(c["surfaces"]), int(c["max_surfaces"]), int(c["clipped"])) == (n * n, n * n, 1, 0)
    assert int(c["min_height"]) == 5 * 256 + 2 and int(c["max_height"]) == 5 * 256 + 256
    for path, skip in ((0, 0), (1, 0), (1, 1)):
        rc, hh, mm, ss, cc, _ = ho.host_heightmap(path, g, box, TOP, 1, True, skip)
        assert rc == 0
        same(hh[0], want); same(mm, m); same(ss, s); same(cc, c)
    # from the bottom the same plane is met from below: z = 5 over air at z = 4 (127)
    hb = ho.heightmap(g, box, BOTTOM, 1, False)[0]
    same(hb[0], (5 * 256 - (256 * (x + 1)) // (127 + x + 1)).astype(np.uint32))
    same(ho.host_heightmap(1, g, box, BOTTOM, 1, False, 1)[1], hb)
