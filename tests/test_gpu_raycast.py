"""Ray casts on the MI355X (vx_raycast*) against the float64 oracle of tests/test_raycast.py, over the meshes the same context
downloads (Polygonizer.level)."""
import numpy as np
import pytest

import fields
import vxo
from golden_io import Golden
from test_raycast import OracleLevel, camera_rays, compare_hits, make_rays, oracle_cast, random_rays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.init()
    return torch


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def synth_poly(n, seed=1337, style=0):
    from voxels_amd import synth
    d, m, b = synth.terrain(n, seed=seed, style=style)
    p = new_poly()
    p.upload(d, m, b, synth.block_empty_flags(d))
    p.execute()
    return p


def check_level(p, level, rays, label, max_grazing=0.01):
    info = p.raycast_prepare(level)
    assert info["straddling"] == 0, (label, info)
    lvl = OracleLevel(p.level(level))
    assert info["blocks"] == len(lvl.ids) and info["triangles"] == len(lvl.tri), (label, info)
    hits = p.raycast_rays(rays, level)
    compare_hits(lvl, rays, hits, oracle_cast(lvl, rays), max_grazing, label)
    return hits


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat", "caves128"])
def test_raycast_fixtures_and_terrain(torch, name):
    p = new_poly()
    if name == "caves128":
        port = vxo.load_port()
        assert port is not None, "oracle/libvoxels_port.so missing (run __graft_entry__.build())"
        g = port.grid_from_float(fields.terrain_field(128, 5), *fields.materials_for(128, 5))
        p.upload(*g.read_dense(), g.block_flags())
    else:
        gold = Golden(name)
        p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
    p.execute()
    check_level(p, 0, random_rays(20000, p.n, 11), name)
    p.close()


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 48, 80, 336])
def test_raycast_every_level(torch, n):
    p = synth_poly(n, seed=100 + n)
    for level in range(p.info.levels):
        check_level(p, level, random_rays(5000, n, level + n), "n=%d level %d" % (n, level))
    p.close()


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_raycast_is_watertight():
    """Rays aimed at every vertex and edge midpoint on edges shared by two triangles (positions welded across blocks), from
    2 voxels out along the normal: none may miss where the oracle (inclusive edges) hits."""
    n = 64
    p = synth_poly(n, seed=3, style=1)
    level = p.level(0)
    lvl = OracleLevel(level)
    P = lvl.tri.reshape(-1, 3)
    _, weld = np.unique(P, axis=0, return_inverse=True)
    weld = weld.reshape(-1, 3)
    edges = np.sort(np.concatenate([weld[:, [0, 1]], weld[:, [1, 2]], weld[:, [2, 0]]]), axis=1)
    ekey, ecount = np.unique(edges, axis=0, return_counts=True)
    shared = ekey[ecount == 2]
    uniq = np.zeros((weld.max() + 1, 3))
    uniq[weld.reshape(-1)] = P
    tn = np.cross(lvl.tri[:, 1] - lvl.tri[:, 0], lvl.tri[:, 2] - lvl.tri[:, 0])
    vn = np.zeros_like(uniq)
    for j in range(3):
        np.add.at(vn, weld[:, j], tn)
    def unit(v):
        ln = np.linalg.norm(v, axis=1, keepdims=True)
        return v / np.where(ln > 0, ln, 1)
    vn = unit(vn)
    vert_ids = np.unique(shared.reshape(-1))
    pts = np.concatenate([uniq[vert_ids], 0.5 * (uniq[shared[:, 0]] + uniq[shared[:, 1]])])
    nrm = np.concatenate([vn[vert_ids], unit(vn[shared[:, 0]] + vn[shared[:, 1]])])
    keep = (np.linalg.norm(nrm, axis=1) > 0.5) & ((pts > 0) & (pts < n)).all(1)   # open edges lie on the grid's faces
    pts, nrm = pts[keep], nrm[keep]
    rays = make_rays(pts + 2 * nrm, -nrm, 0.0, 4.0)
    hits = p.raycast_rays(rays, 0)
    ref = oracle_cast(lvl, rays)
    missed = np.isfinite(ref["t"]) & ~np.isfinite(hits["t"])
    assert len(rays) > 1000 and np.isfinite(ref["t"]).mean() > 0.95
    assert not missed.any(), "%d of %d rays through shared vertices / edges pass through, e.g. %s" % (missed.sum(), len(rays), rays[missed][:3])
    p.close()


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_raycast_after_edits_and_compaction(torch):
    n = 128
    p = synth_poly(n, seed=21)
    chain = [((40.0, 50.0, 64.0), 6.0, 2), ((80.0, 70.0, 60.0), 7.5, 0), ((60.0, 60.0, 66.0), 5.0, 2), ((90.0, 30.0, 62.0), 6.5, 2)]
    for step, (pos, r, kind) in enumerate(chain):
        mn, mx = p.inject_ball(pos, (16, 16, 16), r, kind)
        p.execute_dirty(mn, mx)
        # rays through the edited region and anywhere
        rays = random_rays(3000, n, 40 + step)
        rays["origin"][:1000] = np.array([pos[0], pos[2], pos[1]], np.float32) + np.random.RandomState(step).uniform(-12, 12, (1000, 3))
        check_level(p, 0, rays, "edit %d" % step)
        check_level(p, 1, random_rays(2000, n, 50 + step), "edit %d level 1" % step)
    p.compact_pools()
    check_level(p, 0, random_rays(3000, n, 60), "compacted")
    p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_pick_then_carve(torch):
    n = 128
    p = synth_poly(n, seed=9)
    ray = make_rays([[61.3, n + 10.0, 67.7]], [[0.0, -1.0, 0.0]])
    first = p.raycast_rays(ray)
    assert np.isfinite(first["t"][0])
    hx, hy, hz = first["pos"][0]
    mn, mx = p.inject_ball((hx, hz, hy), (16, 16, 16), 5.0, 2)       # grid coordinates: y and z swapped
    stale = p.raycast_rays(ray)
    assert stale.tobytes() == first.tobytes(), "before the re-run the old meshes answer"
    p.execute_dirty(mn, mx)
    after = check_level(p, 0, ray, "after the carve", max_grazing=1.0)
    assert after["t"][0] > first["t"][0] + 1.0, (first, after)
    p.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_entry_points(torch):
    from voxels_amd import HIT_DTYPE, RAY_DTYPE
    from voxels_amd.binding import RAY_NONE, VoxelsHipError
    gold = Golden("terrain32_mat")
    p = new_poly()
    with pytest.raises(VoxelsHipError):
        p.raycast([1, 40, 1], [0, -1, 0])                             # no surface yet
    p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
    info = p.execute()
    rays = random_rays(4096, 32, 5)
    want = p.raycast_rays(rays)
    assert np.isfinite(want["t"]).mean() > 0.3
    assert p.raycast_rays(rays).tobytes() == want.tobytes()           # two identical calls, identical bytes
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(rays) * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
    s.synchronize()
    p.set_stream(0)
    assert d_hits.cpu().numpy().tobytes() == want.tobytes()
    # windows
    win = rays.copy()
    win["t_min"] = np.random.RandomState(1).uniform(0, 20, len(win)).astype(np.float32)
    win["t_max"] = win["t_min"] + np.random.RandomState(2).uniform(0, 30, len(win)).astype(np.float32)
    check_level(p, 0, win, "t windows")
    # NaN and zero rays miss; n = 0 does nothing
    bad = make_rays([[5, 40, 5], [np.nan, 40, 5], [5, 40, 5], [5, 40, 5]], [[0, 0, 0], [0, -1, 0], [np.nan, -1, 0], [0, -1, 0]])
    bad["t_min"][3], bad["t_max"][3] = 2.0, 1.0
    h = p.raycast_rays(bad)
    assert np.isinf(h["t"]).all() and (h["entry"] == RAY_NONE).all() and (h["block_id"] == RAY_NONE).all() and (h["tri"] == RAY_NONE).all()
    assert not h["pos"].any() and not h["nrm"].any() and not h["bary"].any()
    assert p.raycast_rays(np.zeros(0, RAY_DTYPE)).size == 0
    p.raycast_device(0, 0, 0)
    # VX_ERR_INVALID cases
    with pytest.raises(VoxelsHipError):
        p.raycast_prepare(info.levels)
    with pytest.raises(VoxelsHipError):
        p.raycast_device(d_rays.data_ptr(), 4, d_hits.data_ptr(), level=info.levels)
    with pytest.raises(VoxelsHipError):
        p.raycast_device(0, 4, d_hits.data_ptr())
    with pytest.raises(VoxelsHipError):
        p.raycast_device(d_rays.data_ptr(), 4, 0)
    rc = p._lib.vx_raycast(p._h, 0, None, 4, None)
    assert rc == -1
    p.close()


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_slab_contexts_merge_to_the_whole_grid(torch):
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world = 256, 2
    d, m, b = synth.terrain(n, seed=77)
    flags = synth.block_empty_flags(d)
    whole = new_poly()
    whole.upload(d, m, b, flags)
    whole.execute()
    rays = random_rays(20000, n, 8)
    want = whole.raycast_rays(rays)
    parts, bufs = [], []
    for r in range(world):
        buf = SlabBuffers(torch, n, r, world, "cuda", axis="y")
        buf.fill_from_full(d, m, b, flags)
        q = new_poly()
        buf.attach(q)
        q.execute(sharded_levels(n, world))
        parts.append(q.raycast_rays(rays))
        bufs.append((buf, q))
    got = np.where(parts[1]["t"] < parts[0]["t"], parts[1], parts[0])
    assert np.array_equal(got["t"], want["t"])
    differ = (got["block_id"] != want["block_id"]) | (got["tri"] != want["tri"])
    assert differ.sum() <= len(rays) // 1000, "%d rays report another triangle" % differ.sum()   # (exact ties only)
    for _, q in bufs:
        q.close()
    whole.close()


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_large_grid(torch):
    n = 1024
    p = new_poly()
    p.create_terrain(n, 1337)
    info = p.execute()
    for level in range(info.levels):
        assert p.raycast_prepare(level)["straddling"] == 0, level
    rays = camera_rays(n, 1024)
    hits = p.raycast_rays(rays)
    assert len(hits) == 1 << 20 and np.isfinite(hits["t"]).mean() > 0.5
    sample = np.random.RandomState(4).choice(len(rays), 4000, replace=False)
    lvl = OracleLevel(p.level(0))
    compare_hits(lvl, rays[sample], hits[sample], oracle_cast(lvl, rays[sample]), 0.01, "1024^3 camera")
    p.close()
