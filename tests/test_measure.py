"""The measurements without a GPU: the numpy statement of the header's text (tests/measure_oracle.py) against answers written by
hand, and the host build of voxels_amd/csrc/tv_measure.h - a plain triple loop and the kernels' pipeline, at several chunk sizes,
with and without the sign-summary shortcuts - against that oracle, byte for byte."""
import numpy as np
import pytest

import brush_oracle as bo
import measure_oracle as mo
import stamp_oracle as sto
import undo_oracle as uo

GRIDS = mo.grids()
DEFAULT_CHUNK = 0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


# ---- the oracle against answers written by hand -----------------------------------------------------------------------------

def hand_grid():
    """16^3 of air (distance 100) with a 3 x 2 x 1 solid bar at x 4..6, y 8..9, z 3: material 5 at y = 8, material 9 at y = 9; the
    voxel beside it at x = 7 has the distance exactly 0 and a material of its own"""
    d = np.full((16, 16, 16), 100, np.int8)
    m = np.zeros((16, 16, 16), np.uint8)
    d[3, 8:10, 4:7] = -1
    m[3, 8, 4:7], m[3, 9, 4:7] = 5, 9
    d[3, 8, 7], m[3, 8, 7] = 0, 77
    return uo.Grid(d, m, np.zeros((16, 16, 16), np.uint8), np.zeros(1, np.uint8))


def test_the_oracle_gives_the_answers_written_by_hand():
    g = hand_grid()
    res, t = mo.measure(g, [((0, 0, 0), (16, 16, 16)), ((5, 0, 0), (16, 9, 16)), ((0, 0, 4), (16, 16, 16)), ((7, 8, 3), (8, 9, 4))])
    whole, cut, air, zero = res
    assert (int(whole["voxels"]), int(whole["solid_voxels"]), int(whole["materials"]), int(whole["reserved"])) == (4096, 6, 2, 0)
    assert whole["min"].tolist() == [4, 8, 3] and whole["max"].tolist() == [6, 9, 3]
    assert int(t[0][5]) == 3 and int(t[0][9]) == 3 and int(t[0][77]) == 0 and int(t[0].sum()) == 6      # zero is air: material 77 is not counted
    # a box that cuts the bar: x 5..6 of the row y = 8
    assert (int(cut["voxels"]), int(cut["solid_voxels"]), int(cut["materials"])) == (11 * 9 * 16, 2, 1)
    assert cut["min"].tolist() == [5, 8, 3] and cut["max"].tolist() == [6, 8, 3] and int(t[1][5]) == 2 and int(t[1].sum()) == 2
    # air only
    for r, k in ((air, 2), (zero, 3)):
        assert int(r["solid_voxels"]) == 0 and int(r["materials"]) == 0 and not r["min"].any() and not r["max"].any() and not t[k].any()
    assert int(air["voxels"]) == 16 * 16 * 12 and int(zero["voxels"]) == 1


def test_the_record_oracle_gives_the_answers_written_by_hand():
    g = hand_grid()
    rec = uo.capture(g, [((0, 0, 0), (16, 16, 16))])
    g.dist[3, 8, 4] = 0                    # removed: material 5
    g.dist[10, 1, 2], g.mat[10, 1, 2] = -7, 33   # added: material 33
    g.mat[3, 9, 6] = 10                    # repainted
    g.mat[0, 0, 0] = 200                   # air before and after: nothing
    delta, removed, added = mo.record_delta(g, rec)
    assert [int(delta[k]) for k in ("removed_voxels", "added_voxels", "repainted_voxels", "blocks")] == [1, 1, 1, 1] and not delta["reserved"].any()
    assert delta["min"].tolist() == [2, 1, 3] and delta["max"].tolist() == [4, 8, 10]
    assert int(removed[5]) == 1 == int(removed.sum()) and int(added[33]) == 1 == int(added.sum())


# ---- the host pipeline and the plain loop against the oracle ----------------------------------------------------------------

_wanted = {}


def wanted(name, g, list_name, bx):
    key = (name, list_name)
    if key not in _wanted:
        _wanted[key] = mo.measure(g, bx)
    return _wanted[key]


@pytest.mark.parametrize("name,g", GRIDS, ids=[k for k, _ in GRIDS])
def test_host_paths_equal_the_oracle(name, g):
    for list_name, bx in mo.box_lists(g.n):
        want, want_t = wanted(name, g, list_name, bx)
        # the invariants of the header's text
        assert np.array_equal(want_t.sum(axis=1), want["solid_voxels"])
        assert np.array_equal(want["voxels"], np.prod(bx["hi"].astype(np.uint64) - bx["lo"], axis=1))
        some = want["solid_voxels"] > 0
        assert (want["min"][some] <= want["max"][some]).all() and (want["min"][some] >= bx["lo"][some]).all() and (want["max"][some] < bx["hi"][some]).all()
        assert not want["min"][~some].any() and not want["max"][~some].any() and not want["materials"][~some].any()
        rc, res, t = mo.host_measure(0, g, bx)
        assert rc == 0
        same(res, want); same(t, want_t)
        for chunk in (1, 7, DEFAULT_CHUNK):
            for skip in (0, 1):
                rc, res, t = mo.host_measure(1, g, bx, chunk, skip)
                assert rc == 0, (list_name, chunk, skip)
                same(res, want); same(t, want_t)
        rc, res, t = mo.host_measure(1, g, bx, 7, 1, tallies=False)
        assert rc == 0 and t is None
        same(res, want)


def test_all_bins_and_the_largest_bin():
    by_name = dict(GRIDS)
    whole = [((0, 0, 0), (48, 48, 48))]
    res, t = wanted("48 noise", by_name["48 noise"], "the whole grid", mo.boxes(whole))
    assert int(res[0]["materials"]) == 256 and (t[0] > 0).all()
    res, t = wanted("48 all solid", by_name["48 all solid"], "the whole grid", mo.boxes(whole))
    assert int(res[0]["solid_voxels"]) == 48 ** 3 == int(t[0][7]) and int(res[0]["materials"]) == 1
    assert res[0]["min"].tolist() == [0, 0, 0] and res[0]["max"].tolist() == [47, 47, 47]
    res, t = wanted("48 all air", by_name["48 all air"], "the whole grid", mo.boxes(whole))
    assert int(res[0]["solid_voxels"]) == 0 and not t.any()


def test_the_merge_is_64_bit():
    # (box, block) partials are 32-bit, at most 4096 each; a whole 2048^3 box sums 2^21 of them to 2^33
    parts = np.full((1 << 21) + 3, 4096, np.uint32)
    assert int(mo.load().mh_merge(parts.ctypes.data, parts.size)) == ((1 << 21) + 3) * 4096 > 1 << 33
    parts = np.full(5, 0xFFFFFFFF, np.uint32)
    assert int(mo.load().mh_merge(parts.ctypes.data, parts.size)) == 5 * 0xFFFFFFFF


def test_count_zero_writes_nothing():
    g = GRIDS[0][1]
    assert mo.load().mh_measure(1, g.n, g.dist.ctypes.data, g.mat.ctypes.data, None, 0, 0, 0, None, None) == 0


# ---- the record delta -------------------------------------------------------------------------------------------------------

def edited(g, brushes):
    a = bo.apply(g.dist, g.mat, g.blend, brushes)
    return uo.Grid(a.dist, a.mat, a.blend, a.flags)


def delta_cases():
    """[(name, grid before, boxes, grid after)] on the 48^3 terrain"""
    g = sto.terrain_grid(48)
    whole = [((0, 0, 0), (48, 48, 48))]
    c = 24.0
    carve = bo.stack([bo.ball((c, c, 10.0), (16.0, 16.0, 16.0), 6.0, 2)])
    build = bo.stack([bo.ball((c + 3.0, c, 26.0), (14.0, 14.0, 14.0), 5.0, 0)])
    ga = g.copy()
    ga.mat[ga.dist >= 0] = 41               # what the air holds: the material of whatever a distance brush adds there
    paint = bo.stack([bo.material((c, c - 2.0, 9.0), (18.0, 10.0, 12.0), 9, True)])
    mixed = bo.stack([carve[0], build[0], paint[0], bo.ball((c + 6.0, c + 2.0, 14.0), (14.0, 14.0, 14.0), 5.0, 2), bo.material((10.0, 30.0, 8.0), (9.0, 9.0, 20.0), 200, True)])
    out = [("a subtracting ball", g, whole, edited(g, carve)), ("an adding ball", ga, whole, edited(ga, build)), ("a material brush", g, whole, edited(g, paint)),
           ("a mixed batch", g, [((8, 8, 0), (40, 41, 33)), ((0, 20, 0), (20, 40, 30))], edited(g, mixed)), ("untouched", g, whole, g.copy())]
    # a stamp pasted over the terrain, by the stamps' oracle
    h = g.copy()
    sto.paste(h, [sto.noise_stamp((20, 21, 22), 5)], sto.pastes([((11, 9, 3), 0, 4, sto.PASTE_REPLACE)]))
    out.append(("a pasted noise stamp", g, whole, h))
    return out


DELTAS = delta_cases()


@pytest.mark.parametrize("case", DELTAS, ids=[c[0] for c in DELTAS])
def test_record_delta_equals_the_oracle(case):
    name, before, bx, after = case
    rec = uo.capture(before, bx)
    want = mo.record_delta(after, rec)
    d = want[0]
    counts = [int(d[k]) for k in ("removed_voxels", "added_voxels", "repainted_voxels")]
    if name == "a subtracting ball":
        assert counts[0] > 0 and counts[1] == 0
    if name == "an adding ball":
        assert counts[0] == 0 and counts[1] > 0 and int(want[2][41]) > 0
    if name == "a material brush":
        assert counts[0] == 0 and counts[1] == 0 and counts[2] > 0
    if name == "a mixed batch":
        assert all(v > 0 for v in counts)
    if name == "untouched":
        assert d.tobytes() == bytes(64) and not want[1].any() and not want[2].any()
    assert int(want[1].sum()) == counts[0] and int(want[2].sum()) == counts[1]
    for path in (0, 1):
        rc, delta, removed, added = mo.host_record(path, after, rec)
        assert rc == 0
        same(delta, want[0]); same(removed, want[1]); same(added, want[2])
    # after the swap the record holds the edited state and the grid the earlier one: removed and added exchange
    g2, r2 = after.copy(), rec.copy()
    uo.swap(g2, r2)
    if len(bx) == 1:                        # (a whole-grid capture)
        assert g2.same_as(before)
    redo = mo.record_delta(g2, r2)
    assert int(redo[0]["removed_voxels"]) == counts[1] and int(redo[0]["added_voxels"]) == counts[0] and int(redo[0]["repainted_voxels"]) == counts[2]
    assert redo[0]["min"].tolist() == d["min"].tolist() and redo[0]["max"].tolist() == d["max"].tolist() and int(redo[0]["blocks"]) == int(d["blocks"])
    for path in (0, 1):
        rc, delta, removed, added = mo.host_record(path, g2, r2)
        assert rc == 0
        same(delta, redo[0]); same(removed, redo[1]); same(added, redo[2])


def test_an_empty_record_gives_zeros():
    g = sto.terrain_grid(48)
    for path in (0, 1):
        rc, delta, removed, added = mo.host_record(path, g, uo.empty_rec())
        assert rc == 0 and delta.tobytes() == bytes(64) and not removed.any() and not added.any()
    d, r, a = mo.record_delta(g, uo.empty_rec())
    assert d.tobytes() == bytes(64) and not r.any() and not a.any()
