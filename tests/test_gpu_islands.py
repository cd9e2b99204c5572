"""vx_grid_islands on the MI355X against the flood-fill oracle of tests/island/island_host.cpp, exactly: records, counts, the
labels tensor, the dirty box, and after a removal the packed file of the device grid (distances, untouched materials and
BF_Empty at once) against the pack of the oracle-edited grid.  tests/test_islands.py anchors that oracle to answers written
by hand and runs the same case list through the CPU emulation of the kernels."""
import numpy as np
import pytest

import brush_oracle as bo
import fields
import island_oracle as io
import vxo

pytestmark = pytest.mark.gpu

CASES = io.cases()


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def materials(n):
    return fields.materials_for(n, 3)


def resident(dist, mat=None, blend=None):
    n = dist.shape[0]
    if mat is None:
        mat, blend = materials(n)
    g = vxo.load_port().grid_from_dense(np.ascontiguousarray(dist), mat, blend)
    p = new_poly()
    p.upload_packed(g.pack())
    return p, mat, blend, g


def volume_of(n, box):
    return n ** 3 if box is None else int(np.prod([int(h) - int(l) for l, h in zip(box[0], box[1])]))


def check(p, dist, mat, blend, kw, with_labels=True):
    """one query on the device (grid resident) against the oracle on the dense field -> the oracle's result"""
    import torch
    n = dist.shape[0]
    want = io.run("oracle", dist, **kw)
    assert want.rc == 0
    labels = torch.zeros(volume_of(n, kw.get("box")), dtype=torch.int32, device="cuda:0") if with_labels else None
    recs, counts, mn, mx = p.islands(labels=labels, **kw)
    assert recs.tobytes() == want.records.tobytes()
    assert counts.tobytes() == want.counts.tobytes(), (counts, want.counts)
    assert np.array_equal(mn, want.out_min) and np.array_equal(mx, want.out_max)
    if with_labels:
        torch.cuda.synchronize()
        assert np.array_equal(labels.cpu().numpy().view(np.uint32), want.labels)
    assert np.array_equal(p.pack(), vxo.load_port().grid_from_dense(want.dist, mat, blend).pack())
    return want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_device_equals_the_flood_fill(case):
    _, dist, kw = case
    p, mat, blend, _ = resident(dist)
    before = p.pack()
    want = check(p, dist, mat, blend, kw)
    if not kw.get("remove"):
        assert np.array_equal(p.pack(), before)
    # once more without a labels tensor (the library's own volume), on from the grid the first query left
    again = dict(kw, remove=False)
    check(p, want.dist, mat, blend, again, with_labels=False)


def test_capacity_overflow_and_listed():
    from voxels_amd.binding import VoxelsHipError, ISLAND_DTYPE, ISLAND_COUNTS_DTYPE, island_query
    d = [c for c in CASES if c[0] == "checkerboard"][0][1]
    p, mat, blend, _ = resident(d)
    full = io.run("oracle", d)
    with pytest.raises(VoxelsHipError, match=r"\(-3\)"):
        p.islands(capacity=100)
    q = island_query()
    recs = np.zeros(100, ISLAND_DTYPE)
    counts = np.zeros(1, ISLAND_COUNTS_DTYPE)
    rc = p._lib.vx_grid_islands(p._h, q.ctypes.data, recs.ctypes.data, 100, counts.ctypes.data, None, None, None)
    assert rc == -3 and counts["listed"][0] == 16384 and counts["components"][0] == 16384
    assert recs.tobytes() == full.records[:100].tobytes()
    # removal does not depend on capacity
    q = island_query(remove=True, anchor_faces=0)
    rc = p._lib.vx_grid_islands(p._h, q.ctypes.data, None, 0, counts.ctypes.data, None, None, None)
    want = io.run("oracle", d, remove=True, anchor_faces=0, capacity=0)
    assert rc == -3 and counts[0].tobytes() == want.counts.tobytes()
    assert np.array_equal(p.pack(), vxo.load_port().grid_from_dense(want.dist, mat, blend).pack())


def test_a_caves_terrain_of_208():
    n = 208
    f = fields.terrain_field(n, 4)
    m, b = fields.materials_for(n, 4)
    g = vxo.load_port().grid_from_float(f, m, b)
    d, m, b = g.read_dense()
    p = new_poly()
    p.upload_packed(g.pack())
    want = check(p, d, m, b, {"remove": True, "anchor_faces": 0x1F})
    assert want.counts["components"] >= 1


def test_a_device_terrain_of_336_twice_the_same_bytes():
    import torch
    from voxels_amd import synth
    n = 336
    d, m, b = synth.terrain(n, seed=1337)
    p = new_poly()
    p.create_terrain(n, seed=1337)
    before = p.pack()
    want = io.run("oracle", d)
    got = []
    for _ in range(2):
        labels = torch.zeros(n ** 3, dtype=torch.int32, device="cuda:0")
        recs, counts, mn, mx = p.islands(labels=labels)
        torch.cuda.synchronize()
        got.append((recs.tobytes(), counts.tobytes(), labels.cpu().numpy().tobytes(), mn.tobytes(), mx.tobytes()))
    assert got[0] == got[1]
    assert got[0][0] == want.records.tobytes() and got[0][1] == want.counts.tobytes() and got[0][2] == want.labels.tobytes()
    assert np.array_equal(p.pack(), before)   # a query without a removal leaves the grid alone


def test_invalid_queries_leave_the_grid_untouched():
    import torch
    from voxels_amd.binding import VoxelsHipError, ISLAND_COUNTS_DTYPE, island_query
    d = io.floating()
    p, mat, blend, g = resident(d)
    before = p.pack()
    n = 48
    bad = [dict(box=((4, 4, 4), (4, 8, 8))), dict(box=((4, 4, 4), (8, 8, 49))), dict(box=((9, 4, 4), (8, 8, 8))), dict(anchor_faces=0x40),
           dict(remove=True, air_value=0), dict(remove=True, air_value=128), dict(remove=True, air_value=-1)]
    for kw in bad:
        for labels in (None, torch.zeros(n ** 3, dtype=torch.int32, device="cuda:0")):
            q = island_query(**kw)
            counts = np.zeros(1, ISLAND_COUNTS_DTYPE)
            rc = p._lib.vx_grid_islands(p._h, q.ctypes.data, None, 0, counts.ctypes.data, None if labels is None else labels.data_ptr(), None, None)
            assert rc == -1, kw
            assert np.array_equal(p.pack(), before)
    q = island_query(remove=True)
    q["flags"] |= 4
    counts = np.zeros(1, ISLAND_COUNTS_DTYPE)
    assert p._lib.vx_grid_islands(p._h, q.ctypes.data, None, 0, counts.ctypes.data, None, None, None) == -1
    q = island_query(remove=True)
    assert p._lib.vx_grid_islands(p._h, None, None, 0, counts.ctypes.data, None, None, None) == -1
    assert p._lib.vx_grid_islands(p._h, q.ctypes.data, None, 0, None, None, None, None) == -1
    assert p._lib.vx_grid_islands(p._h, q.ctypes.data, None, 5, counts.ctypes.data, None, None, None) == -1
    assert np.array_equal(p.pack(), before)
    # an attached grid is not the context's own; neither is no grid at all
    dev = torch.device("cuda:0")
    td, tm, tb = (torch.from_numpy(x.copy()).to(dev) for x in (d, mat, blend))
    tf = torch.from_numpy(g.block_flags().copy()).to(dev)
    a = new_poly()
    a.attach(n, 0, n, td.data_ptr(), 0, tm.data_ptr(), tb.data_ptr(), 0, tf.data_ptr())
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        a.islands(remove=True, capacity=8)
    torch.cuda.synchronize()
    assert np.array_equal(td.cpu().numpy(), d)
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        new_poly().islands(capacity=8)


def carve_scene(n=64, seed=12):
    """a pillar built onto the terrain and sawn through: (brushes, dense fields before, oracle of the brushes, oracle of the
    removal on the carved grid)"""
    port = vxo.load_port()
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    g = port.grid_from_float(f, m, b)
    d, m, b = g.read_dense()
    brushes = bo.stack([bo.box((32.0, 32.0, 34.0), (14.0, 14.0, 46.0), (3.0, 3.0, 17.0), 1.0, 0),
                        bo.box((32.0, 32.0, 42.0), (16.0, 16.0, 8.0), (7.0, 7.0, 1.5), 0.5, 2),
                        bo.capsule_stroke((24.0, 32.0, 42.0), (40.0, 32.0, 42.0), 1.5, 2)])
    carved = bo.apply(d, m, b, brushes)
    removal = io.run("oracle", carved.dist, remove=True, detached_only=True)
    return g, brushes, carved, removal, m, b


def test_carve_loose_remove_and_the_incremental_run():
    n = 64
    port = vxo.load_port()
    g, brushes, carved, removal, m, b = carve_scene(n)
    # the cut, chosen on the CPU: exactly one detached component, the top of the pillar
    assert removal.counts["detached"] == 1 and removal.counts["removed"] == 1 and len(removal.records) == 1
    loose = removal.records[0]
    assert loose["voxels"] == int((carved.dist[44:, 24:40, 24:40] < 0).sum()) and loose["voxels"] > 200 and loose["faces"] == 0
    assert io.run("oracle", g.read_dense()[0], detached_only=True).counts["detached"] == 0

    p = new_poly()
    p.upload_packed(g.pack())
    p.execute()
    res, umin, umax, touched = p.inject_brushes(brushes)
    assert touched > 0
    g1 = port.grid_from_dense(carved.dist, carved.mat, carved.blend)
    assert np.array_equal(p.pack(), g1.pack())
    s1 = port.execute(g)             # the surface the oracle's incremental runs go on from
    ref_ids = port.execute_modify(g1, s1, umin, umax)
    got = p.execute_dirty(umin, umax)
    assert np.array_equal(got, ref_ids)

    recs, counts, mn, mx = p.islands(remove=True, detached_only=True)
    assert recs.tobytes() == removal.records.tobytes() and counts.tobytes() == removal.counts.tobytes()
    assert np.array_equal(mn, removal.out_min) and np.array_equal(mx, removal.out_max)
    g2 = port.grid_from_dense(removal.dist, carved.mat, carved.blend)
    assert np.array_equal(p.pack(), g2.pack())
    ref_ids = port.execute_modify(g2, s1, mn, mx)
    got = p.execute_dirty(mn, mx)
    assert np.array_equal(got, ref_ids)
    ok, msg = fields.surface_equal(p.all_levels(), s1.all_levels())
    assert ok, msg
    # level 0, block by block against a fresh full run of the new grid: the box was large enough.  A surface that went through
    # Modifications numbers its rebuilt blocks anew, a fresh run numbers from the start: the blocks are paired by their corner,
    # take the fresh run's id there, and are then compared by id - infos, meshes, transition meshes, byte for byte.  (The
    # upper levels of a modified surface differ from a fresh run's in the reference itself, whatever the box - also after the
    # brushes alone, with their generous box: there the comparison with execute_modify above is the check.)
    fresh = port.execute(g2)
    part, full = p.all_levels()[0], fresh.all_levels()[0]
    assert len(part.infos) == len(full.infos)
    at = {tuple(c): i for c, i in zip(full.infos["min_corner"].tolist(), full.infos["id"])}
    part.infos = part.infos.copy()
    part.infos["id"] = [at[tuple(c)] for c in part.infos["min_corner"].tolist()]
    ok, msg = fields.listed_blocks_equal_by_id(part, full)
    assert ok, msg
    # a full run afterwards: the mirrors followed the removal
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())
