"""vx_grid_islands without a GPU: the flood-fill oracle of tests/island/island_host.cpp against answers written by hand, and
the sequential run of the device path's tile pipeline (voxels_amd/csrc/tv_island.h) against that oracle, byte for byte:
labels volume, records, counts, the distance field and the flags after a removal, the dirty box."""
import numpy as np
import pytest

import island_oracle as io

CASES = io.cases()


def both(dist, **kw):
    a, b = io.run("oracle", dist, **kw), io.run("emulate", dist, **kw)
    ok, what = a.same_as(b)
    assert ok, "oracle and emulation differ in " + what
    return a


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_tile_pipeline_equals_the_flood_fill(case):
    _, dist, kw = case
    r = both(dist, **kw)
    assert r.rc == 0
    c = r.counts
    assert c["listed"] == len(r.records) and c["solid_voxels"] == int((r.labels != io.AIR).sum())
    assert np.all(np.diff(r.records["label"].astype(np.int64)) > 0)
    if not kw.get("remove"):
        assert np.array_equal(r.dist, dist) and not r.out_min.any() and not r.out_max.any() and c["removed"] == 0 and c["touched_blocks"] == 0
    else:
        assert c["removed_voxels"] == int((r.dist != dist).sum()) or kw.get("air_value", 127) in dist
        assert np.array_equal(r.flags, io.codec_flags(r.dist))


def test_all_air_all_solid_and_zeros():
    r = both(io.air(16))
    assert r.counts["components"] == 0 and r.counts["solid_voxels"] == 0 and len(r.records) == 0 and (r.labels == io.AIR).all()
    r = both(np.zeros((16, 16, 16), np.int8))
    assert r.counts["components"] == 0 and (r.labels == io.AIR).all()   # zero is air
    solid = np.full((32, 32, 32), io.SOLID, np.int8)
    assert io.codec_flags(solid).all()
    r = both(solid)
    assert r.counts["components"] == 1 and r.counts["detached"] == 0 and (r.labels == 0).all()
    e = r.records[0]
    assert e["label"] == 0 and e["faces"] == 0x3F and e["voxels"] == 32 ** 3 and tuple(e["min"]) == (0, 0, 0) and tuple(e["max"]) == (31, 31, 31)


def test_edge_and_corner_contact_do_not_connect():
    for name in ("edge contact", "corner contact"):
        dist = [c for c in CASES if c[0] == name][0][1]
        r = both(dist)
        assert r.counts["components"] == 2 and r.counts["detached"] == 2
        assert list(r.records["voxels"]) == [64, 64] and list(r.records["faces"]) == [0, 0]
        assert r.records["label"][0] == (4 * 32 + 4) * 32 + 4 and tuple(r.records["min"][0]) == (4, 4, 4) and tuple(r.records["max"][0]) == (7, 7, 7)
        assert tuple(r.records["min"][1])[:2] == (8, 8) and tuple(r.records["max"][1])[:2] == (11, 11)


def test_a_serpentine_is_one_component():
    d = io.serpentine(48)
    r = both(d)
    assert r.counts["components"] == 1 and r.records["voxels"][0] == int((d < 0).sum()) and r.records["label"][0] == 0
    assert (r.labels[(d < 0).ravel()] == 0).all()
    # cut one connector: two pieces, and the second one's label is its own least index
    cut = d.copy()
    cut[17, 46, 0] = io.EMPTY
    assert d[17, 46, 0] < 0
    r = both(cut)
    assert r.counts["components"] == 2 and r.records["label"][1] == (18 * 48 + 0) * 48 + 0
    assert r.records["voxels"].sum() == int((cut < 0).sum())


def test_arms_that_join_outside_the_region_are_two_components():
    u = [c for c in CASES if c[0] == "U whole"][0][1]
    r = both(u)
    assert r.counts["components"] == 1 and r.records["voxels"][0] == 17 + 17 + 11
    r = both(u, box=((0, 0, 8), (32, 32, 32)))
    assert r.counts["components"] == 2 and list(r.records["voxels"]) == [13, 13] and list(r.records["faces"]) == [16, 16]
    assert list(r.records["label"]) == [16 * 32 + 8, 16 * 32 + 20]
    assert tuple(r.records["min"][0]) == (8, 16, 8) and tuple(r.records["max"][1]) == (20, 16, 20)   # grid coordinates
    assert r.counts["detached"] == 0
    r = both(u, box=((0, 0, 8), (32, 32, 32)), anchor_faces=0x2F, detached_only=True)
    assert r.counts["detached"] == 2 and r.counts["listed"] == 2


def test_checkerboard_capacity_and_listed():
    d = [c for c in CASES if c[0] == "checkerboard"][0][1]
    full = both(d)
    assert full.counts["components"] == 16384 and (full.records["voxels"] == 1).all()
    for kind in ("oracle", "emulate"):
        r = io.run(kind, d, capacity=100)
        assert r.rc == -3 and r.counts["listed"] == 16384 and len(r.records) == 100
        assert r.records.tobytes() == full.records[:100].tobytes() and r.labels.tobytes() == full.labels.tobytes()
        r = io.run(kind, d, capacity=0, remove=True, anchor_faces=0)   # removal does not depend on capacity
        assert r.rc == -3 and r.counts["removed"] == 16384 and (r.dist > 0).all() and np.array_equal(r.flags, io.codec_flags(r.dist)) and r.counts["touched_blocks"] == 8
        assert tuple(r.out_min) == (0, 0, 0) and tuple(r.out_max) == (32, 32, 32)
    inner = both(d, detached_only=True)
    assert inner.counts["listed"] == inner.counts["detached"] == int((d[1:-1, 1:-1, 1:-1] < 0).sum())


def test_a_bar_spanning_five_blocks():
    bar = [c for c in CASES if c[0] == "bar over five blocks"][0][1]
    r = both(bar)
    e = r.records[0]
    assert r.counts["components"] == 1 and e["voxels"] == 80 and e["faces"] == 3 and e["label"] == (40 * 80 + 40) * 80
    assert tuple(e["min"]) == (0, 40, 40) and tuple(e["max"]) == (79, 40, 40)


def test_regions_of_one_voxel_and_bad_queries():
    cd = [c for c in CASES if c[0] == "caves 48"][0][1]
    r = both(cd, box=((5, 5, 1), (6, 6, 2)))
    assert cd[1, 5, 5] < 0 and r.counts["components"] == 1 and r.records[0]["faces"] == 0x3F and r.records[0]["voxels"] == 1 and r.labels[0] == 0
    r = both(cd, box=((5, 5, 46), (6, 6, 47)))
    assert cd[46, 5, 5] > 0 and r.counts["components"] == 0 and r.labels[0] == io.AIR
    for kind in ("oracle", "emulate"):
        for bad in (dict(box=((4, 4, 4), (4, 8, 8))), dict(box=((4, 4, 4), (8, 8, 49))), dict(anchor_faces=0x40), dict(remove=True, air_value=0),
                    dict(remove=True, air_value=128), dict(remove=True, air_value=-3)):
            r = io.run(kind, cd, capacity=4, **bad)
            assert r.rc == -1 and np.array_equal(r.dist, cd), bad


def test_anchor_faces_and_max_voxels():
    f = io.floating()
    ground = 10 * 48 * 48 + 20 * 2 * 2
    r = both(f)
    assert r.counts["components"] == 3 and sorted(r.records["voxels"]) == [8, 216, ground] and r.counts["detached"] == 2
    r = both(f, anchor_faces=0x20, detached_only=True)    # only the top anchors: everything hangs
    assert r.counts["detached"] == 3 and r.counts["detached_voxels"] == 8 + 216 + ground
    for limit, gone in ((0, [8, 216]), (7, []), (8, [8]), (215, [8]), (216, [8, 216])):
        for air_value in (1, 127):
            r = both(f, remove=True, max_voxels=limit, air_value=air_value)
            assert r.counts["removed"] == len(gone) and r.counts["removed_voxels"] == sum(gone) and r.counts["components"] == 3
            want = f.copy()
            if 216 in gone:
                want[20:26, 20:26, 20:26] = air_value
            if 8 in gone:
                want[36:38, 36:38, 10:12] = air_value
            assert np.array_equal(r.dist, want)
            if gone == [8]:      # output order (x, z, y): [a, b + 1]
                assert tuple(r.out_min) == (10, 36, 36) and tuple(r.out_max) == (12, 38, 38) and r.counts["touched_blocks"] == 1
            if gone == [8, 216]:
                assert tuple(r.out_min) == (10, 20, 20) and tuple(r.out_max) == (26, 38, 38) and r.counts["touched_blocks"] == 2
            if not gone:
                assert not r.out_max.any() and r.counts["touched_blocks"] == 0
            # the labels describe the grid before the removal
            assert r.labels.tobytes() == both(f).labels.tobytes()


def test_caves_against_scipy_where_it_is_installed():
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    d = io.caves(48, 6)[0]
    r = both(d)
    assert r.counts["components"] > 3 and r.counts["detached"] > 3
    if ndimage is not None:
        lab, count = ndimage.label(d < 0)
        assert count == r.counts["components"]
        assert sorted(np.bincount(lab.ravel())[1:]) == sorted(int(v) for v in r.records["voxels"])
    # the labels volume against the records, without scipy
    solid = r.labels[r.labels != io.AIR]
    ids, sizes = np.unique(solid, return_counts=True)
    assert np.array_equal(ids, r.records["label"]) and np.array_equal(sizes, r.records["voxels"])
    assert (np.minimum.reduceat(np.sort(solid), np.r_[0, np.cumsum(sizes)[:-1]]) == ids).all()
