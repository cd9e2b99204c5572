"""vx_scatter / vx_scatter_device on the MI355X against the numpy oracle of tests/scatter_oracle.py, byte for byte, on the block
tables and the mesh pools copied from the same context."""
import ctypes as C

import numpy as np
import pytest

import scatter_oracle as so
import vxo
from golden_io import Golden
from scatter_oracle import scatter_params
from test_scatter import filter_cases

pytestmark = pytest.mark.gpu

INVALID, OVERFLOW = -1, -3
POISON = 0xCD


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


def golden_poly(name):
    gold = Golden(name)
    p = new_poly()
    p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
    p.execute()
    return p


def synth_poly(n, seed):
    from voxels_amd import synth
    d, m, b = synth.terrain(n, seed=seed)
    p = new_poly()
    p.upload(d, m, b, synth.block_empty_flags(d))
    p.execute()
    return p


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def snapshot(p):
    """what the oracle reads: per level the device block table, and the two mesh pools, copied raw from the context"""
    from voxels_amd.binding import LISTED_BLOCK_DTYPE, VERTEX_DTYPE
    hip = _hip()
    tabs = []
    for L in range(p.info.levels):
        tab, nb = p.device_block_table(L)
        t = np.zeros(nb, LISTED_BLOCK_DTYPE)
        assert nb == 0 or hip.hipMemcpy(t.ctypes.data_as(C.c_void_p), C.c_void_p(tab), nb * LISTED_BLOCK_DTYPE.itemsize, 2) == 0
        tabs.append(t)
    dv, di, nv, ni = p.device_meshes()
    verts, idx = np.zeros(nv, VERTEX_DTYPE), np.zeros(ni, np.uint32)
    assert nv == 0 or hip.hipMemcpy(verts.ctypes.data_as(C.c_void_p), C.c_void_p(dv), nv * 48, 2) == 0
    assert ni == 0 or hip.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(di), ni * 4, 2) == 0
    return tabs, verts, idx


def host_form(p, level, prm, capacity=None):
    """vx_scatter -> (rc, points, ranges, counts dict); capacity None = counts first, then the fill"""
    if capacity is None:
        rc, _, _, counts = p.scatter_raw(level, prm, 0)
        assert rc in (0, OVERFLOW)
        capacity = int(counts["points"])
    rc, points, ranges, counts = p.scatter_raw(level, prm, capacity)
    c = {k: int(counts[k]) for k in so.SCATTER_COUNTS_DTYPE.names}
    return rc, points[:min(capacity, c["points"])], ranges, c


def device_form(torch, p, level, prm, capacity, entries, guard=64):
    """vx_scatter_device into poisoned torch tensors on a stream of its own -> (points, ranges, counts dict, guards intact)"""
    d_points = torch.full(((capacity + guard) * 48,), POISON, dtype=torch.uint8, device="cuda")
    d_ranges = torch.full(((entries + guard) * 8,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((32 + guard,), POISON, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.scatter_device(level, prm, capacity, d_points.data_ptr(), d_ranges.data_ptr(), d_counts.data_ptr())
    s.synchronize()
    p.set_stream(0)
    pts, rng, cnt = d_points.cpu().numpy(), d_ranges.cpu().numpy(), d_counts.cpu().numpy()
    counts = cnt[:32].view(so.SCATTER_COUNTS_DTYPE)[0]
    c = {k: int(counts[k]) for k in so.SCATTER_COUNTS_DTYPE.names}
    filled = min(capacity, c["points"])
    intact = bool(np.all(pts[filled * 48:] == POISON) and np.all(rng[entries * 8:] == POISON) and np.all(cnt[32:] == POISON))
    return pts[:filled * 48].view(so.SCATTER_POINT_DTYPE), rng[:entries * 8].view(so.SCATTER_RANGE_DTYPE), c, intact


def check(torch, p, snap, level, prm, label, device=True):
    tabs, verts, idx = snap
    rc, pts, ranges, c = so.scatter(level, prm, tabs[level], verts, idx)
    got = host_form(p, level, prm)
    assert got[3] == c, (label, got[3], c)
    assert got[0] == 0 and got[1].tobytes() == pts.tobytes() and got[2].tobytes() == ranges.tobytes(), label
    if device:
        dpts, dranges, dc, intact = device_form(torch, p, level, prm, c["points"], len(tabs[level]))
        assert dc == c and intact, (label, dc, c, intact)
        assert dpts.tobytes() == pts.tobytes() and dranges.tobytes() == ranges.tobytes(), label
    return pts, ranges, c


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat"])
def test_scatter_matches_the_oracle(torch, name):
    p = golden_poly(name)
    snap = snapshot(p)
    for L in range(p.info.levels):
        for density in (0.25, 1.0, 7.5):
            pts, _, c = check(torch, p, snap, L, scatter_params(seed=1234, density=density), "%s L%d density %g" % (name, L, density))
            assert c["points"] == c["candidates"] > 0 and c["visited_entries"] == c["entries"] == len(snap[0][L])
    p.close()


# 2 -------------------------------------------------------------------------------------------------------------------------
def test_heavy_single_block(torch):
    p = golden_poly("sphere64")
    tabs, verts, idx = snap = snapshot(p)
    assert len(tabs[2]) == 1 and int(tabs[2][0]["i_count"]) // 3 > 256  # several chunks of triangles
    prm = scatter_params(seed=1234, density=64.0)
    P = so.triangles(tabs[2][0], verts, idx)[0]
    ht = so.tri_hash(so.block_hash(1234, 2, tabs[2][0]["coord_id"]), np.arange(len(P), dtype=np.uint32))
    assert so.candidate_counts(P, 64.0, ht)[0].max() > 256  # one triangle's candidates span batches of slots
    pts, ranges, c = check(torch, p, snap, 2, prm, "sphere64 L2 density 64")
    assert c["points"] > 256 * 1024 and ranges.tolist() == [(0, c["points"])]
    p.close()


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_filters(torch):
    p = golden_poly("terrain32_mat")
    snap = snapshot(p)
    n = p.n
    for L in range(p.info.levels):
        for case, kw in filter_cases(n).items():
            pts, ranges, c = check(torch, p, snap, L, scatter_params(seed=77, density=3.0, **kw), "terrain32_mat L%d %s" % (L, case))
            assert 0 < c["points"] < c["candidates"] or "texture" in case
    # a box that cuts through some blocks and misses others
    box = dict(box_min=[2.5, 1.0, 3.0], box_max=[13.75, 30.0, 21.5])
    for kw in (box, dict(min_up=0.4, texture_slot=5, texture_values=[3, 15], **box)):
        pts, ranges, c = check(torch, p, snap, 0, scatter_params(seed=5, density=2.0, **kw), "cutting box")
        assert 0 < c["visited_entries"] < c["entries"] and c["points"] > 0
        missed = [e for e, t in enumerate(snap[0][0]) if not (np.all(t["min_corner"] <= kw["box_max"]) and np.all(t["max_corner"] >= kw["box_min"]))]
        assert len(missed) == c["entries"] - c["visited_entries"] and np.all(ranges["count"][missed] == 0)
    p.close()


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_capacity(torch):
    p = golden_poly("terrain32_mat")
    tabs, verts, idx = snapshot(p)
    prm = scatter_params(seed=9, density=2.0, min_up=0.2)
    rc, pts, ranges, c = so.scatter(0, prm, tabs[0], verts, idx)
    total = c["points"]
    assert total > 1000
    for cap in (0, 1, total - 1, total):
        got = host_form(p, 0, prm, cap)
        assert got[0] == (OVERFLOW if cap < total else 0), cap
        assert got[3] == c and got[2].tobytes() == ranges.tobytes() and got[1].tobytes() == pts[:cap].tobytes(), cap
        dpts, dranges, dc, intact = device_form(torch, p, 0, prm, cap, len(tabs[0]))
        assert dc == c and intact and dranges.tobytes() == ranges.tobytes() and dpts.tobytes() == pts[:cap].tobytes(), cap
    p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def by_coord(table, pts, ranges, blank=("entry", "block_id")):
    """coord_id -> the entry's points with entry and block_id blanked"""
    out = {}
    for e, t in enumerate(table):
        mine = pts[int(ranges[e]["first"]):int(ranges[e]["first"]) + int(ranges[e]["count"])].copy()
        for name in blank:
            mine[name] = 0
        out[int(t["coord_id"])] = mine.tobytes()
    return out


def meshes_by_coord(snap, L):
    """coord_id -> (triangle positions, triangle normals, first vertices' tex bytes) of the block's regular mesh, as bytes"""
    tabs, verts, idx = snap
    return {int(t["coord_id"]): tuple(a.tobytes() for a in so.triangles(t, verts, idx)) for t in tabs[L]}


def test_edits(torch):
    """The same surface gives the same points.  A full run of the edited grid is the same surface as the chain of runs at level
    0, block for block.  At the levels above it is not: a surface that went through an incremental run differs there from a
    fresh full run in the reference itself (tests/test_gpu_smooth.py::test_smoothing_feeds_the_incremental_path has the
    finding), and the library follows the reference byte for byte.  Measured on this very case: level 1, block 0, 9 of 906
    triangles and level 2, block 0, 5 of 1 132 triangles have another Blend byte (tex[1]: 74 against 32, 93 against 82) in
    their first vertex; positions, normals and the order of the triangles are the same.  So above level 0 the comparison is
    block by block: a block whose mesh is the same bytes gives the same bytes of points, and a block whose first vertices
    differ in tex alone gives the same points apart from the tex words, which are copied from those vertices."""
    n = 64
    p = synth_poly(n, seed=21)
    prm = scatter_params(seed=4321, density=1.5, min_up=-0.5)
    before_snap = snapshot(p)
    before = [check(torch, p, before_snap, L, prm, "before L%d" % L, device=False) for L in range(p.info.levels)]
    # near a corner: an incremental run rebuilds a margin of blocks around the box, and some blocks of a 64^3 grid are to stay
    mn, mx = p.inject_ball((10.0, 10.0, 31.0), (5, 5, 5), 4.0, 2)
    assert mx[0] < 32 and mx[2] < 32
    new_ids = set(p.execute_dirty(mn, mx).tolist())
    assert new_ids
    after_snap = snapshot(p)
    after = [check(torch, p, after_snap, L, prm, "after L%d" % L, device=L == 0) for L in range(p.info.levels)]
    kept_blocks = 0
    for L in range(p.info.levels):
        old, new = by_coord(before_snap[0][L], *before[L][:2]), by_coord(after_snap[0][L], *after[L][:2])
        rebuilt = {int(t["coord_id"]) for t in after_snap[0][L] if int(t["id"]) in new_ids} | (set(old) - set(new))
        for coord in set(new) - rebuilt:
            assert new[coord] == old[coord], (L, coord)
            kept_blocks += 1
        if L == 0:
            assert rebuilt and any(old.get(coord) != new.get(coord) for coord in rebuilt)
    assert kept_blocks > 0
    p.compact_pools()
    compact_snap = snapshot(p)
    for L in range(p.info.levels):
        pts, ranges, c = check(torch, p, compact_snap, L, prm, "compacted L%d" % L, device=False)
        assert pts.tobytes() == after[L][0].tobytes() and ranges.tobytes() == after[L][1].tobytes() and c == after[L][2]
    fresh = synth_poly(n, seed=21)  # the same grid and the same edit, then a full run
    fresh.inject_ball((10.0, 10.0, 31.0), (5, 5, 5), 4.0, 2)
    fresh.execute()
    fresh_snap = snapshot(fresh)
    same_upper = 0
    for L in range(p.info.levels):
        pts, ranges, c = check(torch, fresh, fresh_snap, L, prm, "fresh L%d" % L, device=False)
        full, chain = by_coord(fresh_snap[0][L], pts, ranges), by_coord(after_snap[0][L], *after[L][:2])
        full_mesh, chain_mesh = meshes_by_coord(fresh_snap, L), meshes_by_coord(after_snap, L)
        assert set(full) == set(chain), L
        for coord in full:
            if full_mesh[coord] == chain_mesh[coord]:
                assert full[coord] == chain[coord], (L, coord)
                same_upper += L > 0
            else:
                assert L > 0 and full_mesh[coord][:2] == chain_mesh[coord][:2], (L, coord)  # level 0: the same surface, always
                blank = ("entry", "block_id", "tex")
                assert by_coord(fresh_snap[0][L], pts, ranges, blank)[coord] == by_coord(after_snap[0][L], *after[L][:2], blank)[coord], (L, coord)
    assert same_upper > 0
    fresh.close()
    p.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_empty_level(torch):
    n = 32
    p = new_poly()
    p.upload(np.full((n, n, n), 127, np.int8), np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint8), np.ones((n // 16) ** 3, np.uint8))
    p.execute()
    assert p.info.levels >= 1 and p.device_block_table(0)[1] == 0
    prm = np.ascontiguousarray(scatter_params(seed=1), so.SCATTER_PARAMS_DTYPE)
    counts = np.full(32, POISON, np.uint8)
    rc = p._L.lib.vx_scatter(p._h, 0, prm.ctypes.data_as(C.c_void_p), 0, None, None, counts.ctypes.data_as(C.c_void_p))
    assert rc == 0 and not counts.any()
    _, _, dc, intact = device_form(torch, p, 0, prm, 16, 0)
    assert intact and not any(dc.values())
    p.close()


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_validation(torch):
    p = golden_poly("terrain32_mat")
    lib, vp = p._L.lib, C.c_void_p
    nb = p.device_block_table(0)[1]
    cap = 64
    d_points = torch.full((cap * 48 + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_ranges = torch.full((nb * 8 + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((48,), POISON, dtype=torch.uint8, device="cuda")
    points, ranges, counts = np.full(cap * 48, POISON, np.uint8), np.full(nb * 8, POISON, np.uint8), np.full(32, POISON, np.uint8)

    def ptr(a):
        return a.ctypes.data_as(vp)

    def both(label, level, prm, capacity=cap, no_points=False, no_counts=False):
        rec = None if prm is None else np.ascontiguousarray(prm, so.SCATTER_PARAMS_DTYPE)
        rc = lib.vx_scatter(p._h, level, None if rec is None else ptr(rec), capacity, None if no_points else ptr(points), ptr(ranges),
                            None if no_counts else ptr(counts))
        assert rc == INVALID, ("host", label, rc)
        rc = lib.vx_scatter_device(p._h, level, None if rec is None else ptr(rec), capacity, None if no_points else vp(d_points.data_ptr()),
                                   vp(d_ranges.data_ptr()), None if no_counts else vp(d_counts.data_ptr()))
        assert rc == INVALID, ("device", label, rc)

    def changed(**kw):
        prm = scatter_params(seed=1, density=1.0)
        for k, v in kw.items():
            prm[k] = v
        return prm

    good = scatter_params(seed=1, density=1.0)
    nan, inf = float("nan"), float("inf")
    both("level beyond the run", p.info.levels, good)
    both("null params", 0, None)
    both("null counts", 0, good, no_counts=True)
    both("null points with a capacity", 0, good, no_points=True)
    for d in (0.0, -1.0, 64.5, inf, nan):
        both("density %r" % d, 0, changed(density=d))
    for field in ("min_up", "max_up"):
        both("NaN " + field, 0, changed(**{field: nan}))
    for field in ("box_min", "box_max"):
        for a in range(3):
            v = [0.0, 0.0, 0.0] if field == "box_min" else [8.0, 8.0, 8.0]
            v[a] = nan
            both("NaN %s[%d]" % (field, a), 0, changed(**dict(dict(box_min=[0, 0, 0], box_max=[8, 8, 8]), **{field: v})))
    both("min_up > max_up", 0, changed(min_up=0.5, max_up=0.25))
    for a in range(3):
        lo = [0.0, 0.0, 0.0]
        lo[a] = 9.0
        both("box_min > box_max on axis %d" % a, 0, changed(box_min=lo, box_max=[8, 8, 8]))
    both("texture_slot 8", 0, changed(texture_slot=8))
    both("reserved", 0, changed(reserved=1))
    rec = np.ascontiguousarray(good, so.SCATTER_PARAMS_DTYPE)
    for label, off in (("points", (4, 0, 0)), ("ranges", (0, 4, 0)), ("counts", (0, 0, 8))):
        rc = lib.vx_scatter_device(p._h, 0, ptr(rec), cap, vp(d_points.data_ptr() + off[0]), vp(d_ranges.data_ptr() + off[1]), vp(d_counts.data_ptr() + off[2]))
        assert rc == INVALID, ("misaligned " + label, rc)
    empty = new_poly()  # no surface yet
    rc = empty._L.lib.vx_scatter(empty._h, 0, ptr(rec), cap, ptr(points), ptr(ranges), ptr(counts))
    assert rc == INVALID
    rc = empty._L.lib.vx_scatter_device(empty._h, 0, ptr(rec), cap, vp(d_points.data_ptr()), vp(d_ranges.data_ptr()), vp(d_counts.data_ptr()))
    assert rc == INVALID
    empty.close()
    torch.cuda.synchronize()
    for a in (points, ranges, counts, d_points.cpu().numpy(), d_ranges.cpu().numpy(), d_counts.cpu().numpy()):
        assert np.all(a == POISON)
    # and the same buffers are written by a valid call
    assert lib.vx_scatter(p._h, 0, ptr(rec), cap, ptr(points), ptr(ranges), ptr(counts)) == OVERFLOW
    assert not np.all(points == POISON) and not np.all(ranges == POISON) and not np.all(counts == POISON)
    p.close()
