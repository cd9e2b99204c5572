"""vx_grid_walk_field on the MI355X against the Dijkstra oracle of tests/walk/walk_host.cpp, exactly: the field, the direction
bytes and the deterministic counts, with the caller's tensors and with the library's own volume, and the packed file of the
device grid unchanged by the call.  tests/test_walk.py anchors that oracle to answers written by hand, to a brute-force
Bellman-Ford and to the definition's invariants, and runs the same case list through the CPU emulation of the kernels."""
import numpy as np
import pytest

import brush_oracle as bo
import fields
import vxo
import walk_oracle as wo

pytestmark = pytest.mark.gpu

CASES = wo.cases()


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def resident(dist):
    n = dist.shape[0]
    mat, blend = fields.materials_for(n, 3)
    p = new_poly()
    p.upload_packed(vxo.load_port().grid_from_dense(np.ascontiguousarray(dist), mat, blend).pack())
    return p


def dense_of(p):
    """the distances of the resident grid, read back block by block"""
    n, nb = p.n, p.n // 16
    d = np.zeros((n, n, n), np.int8)
    for b in range(nb ** 3):
        bx, by, bz = b % nb, (b // nb) % nb, b // (nb * nb)
        d[bz * 16:bz * 16 + 16, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = p.read_block(b)[0]
    return d


def check(p, dist, kw, tensors=True):
    """one query on the device (grid resident) against the oracle on the dense field"""
    import torch
    want = wo.run("oracle", dist, **kw)
    assert want.rc == 0
    V = want.field.size
    field = torch.full((V,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0") if tensors else None
    dirs = torch.full((V,), 0x5A, dtype=torch.uint8, device="cuda:0") if tensors else None
    counts = p.walk_field(kw.get("box"), kw.get("goals", ()), field=field, dirs=dirs, **{k: v for k, v in kw.items() if k not in ("box", "goals")})
    assert wo.deterministic(counts) == wo.deterministic(want.counts), (counts, want.counts)
    if tensors:
        torch.cuda.synchronize()
        assert np.array_equal(field.cpu().numpy().view(np.uint32), want.field.reshape(-1))
        assert np.array_equal(dirs.cpu().numpy(), want.dirs.reshape(-1))
    return want


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_device_equals_the_oracle(case):
    _, dist, kw = case
    p = resident(dist)
    before = p.pack()
    check(p, dist, kw)
    check(p, dist, kw, tensors=False)   # the library's own volume, no direction bytes: the counts all the same
    assert np.array_equal(p.pack(), before)


def test_only_one_output_each():
    import torch
    _, dist, kw = [c for c in CASES if c[0] == "bridge over a floor"][0]
    p = resident(dist)
    want = wo.run("oracle", dist, **kw)
    field = torch.zeros(want.field.size, dtype=torch.int32, device="cuda:0")
    dirs = torch.zeros(want.field.size, dtype=torch.uint8, device="cuda:0")
    c1 = p.walk_field(None, kw["goals"], field=field)
    c2 = p.walk_field(None, kw["goals"], dirs=dirs)
    torch.cuda.synchronize()
    assert wo.deterministic(c1) == wo.deterministic(want.counts) == wo.deterministic(c2)
    assert np.array_equal(field.cpu().numpy().view(np.uint32), want.field.reshape(-1)) and np.array_equal(dirs.cpu().numpy(), want.dirs.reshape(-1))


def test_the_query_sees_edits_of_the_resident_grid():
    n = 64
    dist = wo.floor(n, 20)
    p = resident(dist)
    kw = dict(box=((4, 4, 8), (60, 60, 40)), goals=[(8, 8, 20)], step_up=2, step_down=2, cost_climb=5)
    flat = check(p, dist, kw)
    p.inject_ball((32.0, 32.0, 20.0), (24.0, 24.0, 24.0), 9.0, 2)   # carve a pit into the floor
    carved = dense_of(p)
    assert not np.array_equal(carved, dist)
    pit = check(p, carved, kw)
    assert not np.array_equal(pit.field, flat.field)
    # a floating slab, then its removal: the field follows again
    p.inject_brushes(bo.stack([bo.box((44.0, 44.0, 30.0), (14.0, 14.0, 8.0), (4.0, 4.0, 1.0), 0.5, 0)]))
    slab = dense_of(p)
    with_slab = check(p, slab, kw)
    assert with_slab.counts["standable"] > pit.counts["standable"]
    _, counts, _, _ = p.islands(remove=True, detached_only=True)
    assert counts["removed"] >= 1
    without = check(p, dense_of(p), kw)
    assert without.counts["standable"] < with_slab.counts["standable"]


def test_working_memory_is_reused_and_grown():
    _, dist, _ = [c for c in CASES if c[0] == "serpentine 48"][0]
    p = resident(dist)
    for box in (((0, 0, 0), (48, 48, 16)), ((5, 5, 3), (20, 20, 7)), None, ((0, 0, 2), (47, 33, 9))):
        check(p, dist, dict(box=box, goals=[(6, 6, 4), (40, 40, 4, 7)]), tensors=False)
    check(p, dist, dict(box=None, goals=[(6, 6, 4)]))


def test_invalid_queries_write_nothing():
    import torch
    from voxels_amd.binding import VoxelsHipError, WALK_COUNTS_DTYPE, WALK_MAX_GOALS, walk_goals, walk_query
    dist = wo.floor(32, 8)
    p = resident(dist)
    before = p.pack()
    V = 32 ** 3
    field = torch.full((V + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    dirs = torch.full((V,), 0x5A, dtype=torch.uint8, device="cuda:0")
    g = walk_goals([(5, 7, 8)])
    many = np.zeros(WALK_MAX_GOALS + 1, g.dtype)
    counts = np.zeros(1, WALK_COUNTS_DTYPE)
    fn, h = p._lib.vx_grid_walk_field, p._h

    def call(q=walk_query(), goals=g, n=1, f=field.data_ptr(), c=counts):
        return fn(h, None if q is None else q.ctypes.data, None if goals is None else goals.ctypes.data, n, f, dirs.data_ptr(), None if c is None else c.ctypes.data)

    assert call() == 0 and counts["reached"][0] == 1024
    field.fill_(0x5A5A5A5A)
    dirs.fill_(0x5A)
    bad = [dict(box=((4, 4, 4), (4, 8, 8))), dict(box=((4, 4, 4), (8, 8, 33))), dict(box=((9, 4, 4), (8, 8, 8))), dict(clearance=0), dict(clearance=33),
           dict(step_up=5), dict(step_down=5), dict(cost_axial=0), dict(cost_axial=65536), dict(cost_diagonal=65536), dict(cost_climb=65536),
           dict(max_cost=(1 << 30) + 1)]
    for kw in bad:
        assert call(q=walk_query(**kw)) == -1, kw
    flagged = walk_query()
    flagged["flags"] = 1
    assert call(q=flagged) == -1
    assert call(q=None) == -1 and call(c=None) == -1
    assert call(goals=None) == -1 and call(goals=many, n=WALK_MAX_GOALS + 1) == -1
    assert call(f=field.data_ptr() + 4) == -1
    # an attached grid is not the context's own; neither is no grid at all
    dev = torch.device("cuda:0")
    mat, blend = fields.materials_for(32, 3)
    td, tm, tb = (torch.from_numpy(x.copy()).to(dev) for x in (dist, mat, blend))
    tf = torch.from_numpy(vxo.load_port().grid_from_dense(dist, mat, blend).block_flags().copy()).to(dev)
    a = new_poly()
    a.attach(32, 0, 32, td.data_ptr(), 0, tm.data_ptr(), tb.data_ptr(), 0, tf.data_ptr())
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        a.walk_field(None, g, field=field[:V], dirs=dirs)
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        new_poly().walk_field(((0, 0, 0), (32, 32, 32)), g, field=field[:V], dirs=dirs)
    torch.cuda.synchronize()
    assert (field.cpu().numpy() == 0x5A5A5A5A).all() and (dirs.cpu().numpy() == 0x5A).all()
    assert np.array_equal(p.pack(), before)
