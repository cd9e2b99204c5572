"""Sphere casts and closest points on the MI355X (vx_spherecast*, vx_closest_point*) against the float64 oracle of
tests/test_shapecast.py, over the meshes the same context downloads (Polygonizer.level).  The comparison rules are
compare_sphere_hits and compare_point_hits there."""
import numpy as np
import pytest

import fields
import vxo
from golden_io import Golden
from test_raycast import OracleLevel, make_rays
from test_shapecast import (compare_point_hits, compare_sphere_hits, falling_casts, make_casts, make_queries, oracle_closest,
                            oracle_sphere, queries_near, random_casts, random_queries)

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


def check_level(p, level, casts, queries, label, max_grazing=0.01):
    info = p.raycast_prepare(level)
    assert info["straddling"] == 0, (label, info)
    lvl = OracleLevel(p.level(level))
    sh = None
    if casts is not None:
        sh = p.spherecast_casts(casts, level)
        compare_sphere_hits(lvl, casts, sh, oracle_sphere(lvl, casts), max_grazing, label)
    if queries is not None:
        ph = p.closest_points_queries(queries, level)
        compare_point_hits(lvl, queries, ph, oracle_closest(lvl, queries), label)
    return sh


def cast_batch(n, count, seed, r_lo=0.25, r_hi=12.0):
    c = random_casts(count, n, seed, r_lo, r_hi)
    c["t_max"] = np.minimum(c["t_max"], 0.25 * n)
    return c


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat", "caves128"])
def test_shapecast_fixtures_and_terrain(torch, name):
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
    casts = cast_batch(p.n, 1500, 11)
    hits = check_level(p, 0, casts, random_queries(1500, p.n, 12), name)
    assert np.isfinite(hits["t"]).mean() > 0.2 and (hits["flags"] & 1).any()
    check_level(p, 0, None, random_queries(300, p.n, 13, max_dist=np.inf), name + " max_dist inf")
    p.close()


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 48, 80, 336])
def test_shapecast_every_level(torch, n):
    p = synth_poly(n, seed=100 + n)
    for level in range(p.info.levels):
        check_level(p, level, cast_batch(n, 600, level + n), random_queries(600, n, level + n + 1), "n=%d level %d" % (n, level))
    p.close()


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_tiny_spheres_agree_with_the_ray_casts(torch):
    """radius 1e-3: a sphere touches no later than the ray hits (plus tolerance), and close to it where the ray is not grazing"""
    from test_raycast import random_rays
    n = 128
    p = synth_poly(n, seed=31)
    rays = random_rays(20000, n, 3)
    rh = p.raycast_rays(rays)
    casts = make_casts(rays["origin"], rays["dir"], 1e-3, rays["t_min"], rays["t_max"])
    sh = p.spherecast_casts(casts)
    dlen = np.linalg.norm(rays["dir"].astype(np.float64), axis=1)
    tol = 2e-3 / np.maximum(dlen, 1e-30)
    hit = np.isfinite(rh["t"])
    assert hit.mean() > 0.2
    assert np.all(sh["t"][hit] <= rh["t"][hit] + tol[hit])
    # the sphere may touch a neighbour of the hit triangle first (at a convex edge), by at most r / |dot| along the path
    # for a neighbour that is not grazed (|dot| >= 0.02); against the hit triangle itself by r / |dot| of its own normal
    gap = (rh["t"][hit] - sh["t"][hit]) * dlen[hit]
    assert np.all(gap <= 1e-3 / 0.02 + 2e-3), gap.max()
    dot = np.abs((rays["dir"] / dlen[:, None] * rh["nrm"]).sum(1))[hit]
    steep = dot > 0.1
    close = gap[steep] <= 1e-3 / dot[steep] + 2e-3
    assert close.mean() > 0.99, (close.mean(), gap[steep].max())
    p.close()


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_sphere_casts_and_closest_points_agree_at_1024(torch):
    n = 1024
    p = new_poly()
    p.create_terrain(n, 1337)
    p.execute()
    casts = falling_casts(n, 1 << 18, seed=5, radius=2.0)
    casts["radius"] = np.random.RandomState(6).uniform(0.5, 8.0, len(casts)).astype(np.float32)
    hits = p.spherecast_casts(casts)
    moving = np.isfinite(hits["t"]) & ((hits["flags"] & 1) == 0)
    assert moving.sum() > 10000
    h, c = hits[moving], casts[moving]
    at = p.closest_points(h["center"])
    r = c["radius"].astype(np.float64)
    assert np.all(np.abs(at["dist"] - r) <= 2e-3), np.abs(at["dist"] - r).max()
    for delta in (0.01, 0.25):
        ok = h["t"] >= delta                                      # (earlier than t_min the cast makes no claim)
        before = p.closest_points(h["center"][ok] - delta * c["dir"][ok])
        assert np.all(before["dist"] > r[ok] - 2e-3), (delta, (r[ok] - before["dist"]).max())
    p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_shapecast_after_edits_and_compaction(torch):
    n = 128
    p = synth_poly(n, seed=21)
    chain = [((40.0, 50.0, 64.0), 6.0, 2), ((80.0, 70.0, 60.0), 7.5, 0), ((60.0, 60.0, 66.0), 5.0, 2)]
    for step, (pos, r, kind) in enumerate(chain):
        mn, mx = p.inject_ball(pos, (16, 16, 16), r, kind)
        p.execute_dirty(mn, mx)
        casts = cast_batch(n, 800, 40 + step)
        casts["origin"][:300] = np.array([pos[0], pos[2], pos[1]], np.float32) + np.random.RandomState(step).uniform(-12, 12, (300, 3))
        q = random_queries(800, n, 50 + step)
        q["pos"][:300] = np.array([pos[0], pos[2], pos[1]], np.float32) + np.random.RandomState(step + 9).uniform(-10, 10, (300, 3))
        check_level(p, 0, casts, q, "edit %d" % step)
        check_level(p, 1, cast_batch(n, 400, 60 + step), random_queries(400, n, 70 + step), "edit %d level 1" % step)
    p.compact_pools()
    check_level(p, 0, cast_batch(n, 800, 80), random_queries(800, n, 81), "compacted")
    # a cast through the carved hole: stale until the run, then the new surface
    p2 = synth_poly(n, seed=9)
    c = make_casts([[61.3, n + 10.0, 67.7]], [[0.0, -1.0, 0.0]], 1.5)
    first = p2.spherecast_casts(c)
    assert np.isfinite(first["t"][0])
    cx, cy, cz = first["contact"][0]
    mn, mx = p2.inject_ball((cx, cz, cy), (16, 16, 16), 6.0, 2)
    assert p2.spherecast_casts(c).tobytes() == first.tobytes()
    p2.execute_dirty(mn, mx)
    after = p2.spherecast_casts(c)
    assert after["t"][0] > first["t"][0] + 1.0, (first, after)
    p2.close()
    p.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_slab_contexts_merge_to_the_whole_grid(torch):
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world = 256, 2
    d, m, b = synth.terrain(n, seed=77)
    flags = synth.block_empty_flags(d)
    whole = new_poly()
    whole.upload(d, m, b, flags)
    whole.execute()
    casts = cast_batch(n, 20000, 8, 0.25, 6.0)
    q = random_queries(20000, n, 9)
    want, wantq = whole.spherecast_casts(casts), whole.closest_points_queries(q)
    parts, partq, bufs = [], [], []
    for r in range(world):
        buf = SlabBuffers(torch, n, r, world, "cuda", axis="y")
        buf.fill_from_full(d, m, b, flags)
        s = new_poly()
        buf.attach(s)
        s.execute(sharded_levels(n, world))
        parts.append(s.spherecast_casts(casts))
        partq.append(s.closest_points_queries(q))
        bufs.append((buf, s))
    # merge by least t, then (start contacts) least distance at t_min
    k0 = np.stack([parts[0]["t"], -parts[0]["depth"]], 1)
    k1 = np.stack([parts[1]["t"], -parts[1]["depth"]], 1)
    take1 = (k1[:, 0] < k0[:, 0]) | ((k1[:, 0] == k0[:, 0]) & (k1[:, 1] < k0[:, 1]))
    got = np.where(take1, parts[1], parts[0])
    assert np.array_equal(got["t"], want["t"])
    differ = (got["block_id"] != want["block_id"]) | (got["tri"] != want["tri"])
    assert differ.sum() <= len(casts) // 1000, "%d casts report another triangle" % differ.sum()
    gq = np.where(partq[1]["dist"] < partq[0]["dist"], partq[1], partq[0])
    assert np.array_equal(gq["dist"], wantq["dist"])
    differ = (gq["block_id"] != wantq["block_id"]) | (gq["tri"] != wantq["tri"])
    assert differ.sum() <= len(q) // 1000, "%d queries report another triangle" % differ.sum()
    for _, s in bufs:
        s.close()
    whole.close()


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_entry_points(torch):
    from voxels_amd import POINT_HIT_DTYPE, POINT_QUERY_DTYPE, SPHERE_CAST_DTYPE, SPHERE_HIT_DTYPE
    from voxels_amd.binding import RAY_NONE, VoxelsHipError
    gold = Golden("terrain32_mat")
    p = new_poly()
    with pytest.raises(VoxelsHipError):
        p.spherecast([1, 40, 1], [0, -1, 0], 1.0)                    # no surface yet
    with pytest.raises(VoxelsHipError):
        p.closest_points([1, 20, 1])
    p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
    info = p.execute()
    casts = cast_batch(32, 4096, 5)
    q = random_queries(4096, 32, 6)
    want, wantq = p.spherecast_casts(casts), p.closest_points_queries(q)
    assert np.isfinite(want["t"]).mean() > 0.3 and np.isfinite(wantq["dist"]).mean() > 0.3
    assert p.spherecast_casts(casts).tobytes() == want.tobytes()
    d_c = torch.from_numpy(casts.view(np.uint8).copy()).cuda()
    d_h = torch.zeros(len(casts) * SPHERE_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_q = torch.from_numpy(q.view(np.uint8).copy()).cuda()
    d_qh = torch.zeros(len(q) * POINT_HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.spherecast_device(d_c.data_ptr(), len(casts), d_h.data_ptr())
    p.closest_points_device(d_q.data_ptr(), len(q), d_qh.data_ptr())
    s.synchronize()
    p.set_stream(0)
    assert d_h.cpu().numpy().tobytes() == want.tobytes()
    assert d_qh.cpu().numpy().tobytes() == wantq.tobytes()
    # the Python helpers build the same records
    assert p.spherecast(casts["origin"], casts["dir"], casts["radius"], casts["t_min"], casts["t_max"]).tobytes() == want.tobytes()
    assert p.closest_points(q["pos"], q["max_dist"]).tobytes() == wantq.tobytes()
    # misses
    bad = make_casts([[np.nan, 40, 5], [5, 40, 5], [5, 40, 5], [5, 40, 5], [5, 40, 5], [5, 40, 5]],
                     [[0, -1, 0], [np.nan, -1, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0], [0, -1, 0]],
                     [1.0, 1.0, 0.0, -1.0, np.nan, np.inf])
    bad = np.concatenate([bad, make_casts([[5, 40, 5]], [[0, -1, 0]], 1.0, 2.0, 1.0)])
    h = p.spherecast_casts(bad)
    assert np.isinf(h["t"]).all() and (h["entry"] == RAY_NONE).all() and (h["block_id"] == RAY_NONE).all() and (h["tri"] == RAY_NONE).all()
    assert not h["center"].any() and not h["contact"].any() and not h["nrm"].any() and not h["depth"].any()
    assert not h["flags"].any() and not h["reserved"].any()
    qb = make_queries([[np.nan, 10, 10], [10, 10, 10], [10, 10, 10], [10, 40, 10]], [np.inf, np.nan, -1.0, 0.5])
    hq = p.closest_points_queries(qb)
    assert np.isinf(hq["dist"]).all() and (hq["entry"] == RAY_NONE).all() and (hq["tri"] == RAY_NONE).all()
    assert not hq["point"].any() and not hq["nrm"].any() and not hq["bary"].any()
    # dir = 0: a static overlap test at t_min
    st = p.spherecast_casts(make_casts(want["center"][np.isfinite(want["t"])][:50], [[0, 0, 0]], casts["radius"][np.isfinite(want["t"])][:50] + 0.01, 7.0, 9.0))
    assert (st["t"] == 7.0).all() and (st["flags"] == 1).all()
    # n = 0
    assert p.spherecast_casts(np.zeros(0, SPHERE_CAST_DTYPE)).size == 0
    assert p.closest_points_queries(np.zeros(0, POINT_QUERY_DTYPE)).size == 0
    p.spherecast_device(0, 0, 0)
    p.closest_points_device(0, 0, 0)
    # VX_ERR_INVALID
    for f in (p.spherecast_device, p.closest_points_device):
        with pytest.raises(VoxelsHipError):
            f(d_c.data_ptr(), 4, d_h.data_ptr(), level=info.levels)
        with pytest.raises(VoxelsHipError):
            f(0, 4, d_h.data_ptr())
        with pytest.raises(VoxelsHipError):
            f(d_c.data_ptr(), 4, 0)
    with pytest.raises(VoxelsHipError):
        p.spherecast_casts(casts[:4], level=info.levels)
    assert p._lib.vx_spherecast(p._h, 0, None, 4, None) == -1
    assert p._lib.vx_closest_point(p._h, 0, None, 4, None) == -1
    p.close()


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_large_grid(torch):
    n = 1024
    p = new_poly()
    p.create_terrain(n, 1337)
    p.execute()
    assert p.raycast_prepare(0)["straddling"] == 0
    casts = falling_casts(n, 1 << 20, seed=4)
    hits = p.spherecast_casts(casts)
    hit = np.isfinite(hits["t"])
    assert len(hits) == 1 << 20 and hit.mean() > 0.05
    rng = np.random.RandomState(4)
    sample = np.concatenate([rng.choice(np.nonzero(hit)[0], 2000, replace=False), rng.choice(np.nonzero(~hit)[0], 2000, replace=False)])
    lvl = OracleLevel(p.level(0))
    compare_sphere_hits(lvl, casts[sample], hits[sample], oracle_sphere(lvl, casts[sample]), 0.01, "1024^3 falling")
    q = queries_near(hits["contact"][np.isfinite(hits["t"])], 1 << 20, seed=5)
    qh = p.closest_points_queries(q)
    assert np.isfinite(qh["dist"]).mean() > 0.5
    compare_point_hits(lvl, q[sample], qh[sample], oracle_closest(lvl, q[sample]), "1024^3 near the surface")
    p.close()
