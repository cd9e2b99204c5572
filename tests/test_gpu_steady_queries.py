"""What reads a run's results on the device, behind the steady-state full run (tests/test_gpu_steady.py): the raw block tables
and pools, ray casts, sphere casts and closest points, overlap boxes, scatter and LOD selection - each checked the way its own
GPU test checks it, but behind a one-launch kept run instead of a context's first run.  Behind such a run the tables were not
rewritten, the header is one of three rotating sets whose list totals k_main's last workgroup stored from host copies, and
vx_polygonize has returned on the header flag while the stream may still be busy; the consumers take the tables from
vx_device_block_table, the list counts from the device header, key the ray index on the mesh epoch and size the shared
permutation by the index pool.  A renderer's frame is "kept run, LOD select, ray casts, scatter": the frame loop below.

steady(p) brings a context to that state and states the form of every run through the counters (test_gpu_layout.run), so no
query here runs behind a run that fell back.  Fields: gentle64_nozero (tests/steady_fields.py) and terrain128."""
import ctypes as C

import numpy as np
import pytest

import overlap_oracle as oo
import scatter_oracle as so
import steady_fields as sf
import vxo
import test_gpu_cellmap as cellmap
import test_gpu_lod as glod
import test_gpu_overlap as goverlap
import test_gpu_raycast as gray
import test_gpu_scatter as gscatter
import test_gpu_shapecast as gshape
from scatter_oracle import scatter_params
from test_gpu_layout import HANDS_OUT, KEPT_ONE, KEPT_TWO, hands_on, run, same_tables, tables, warm
from test_gpu_matstore import make_poly
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_slotplan import plan_field
from test_lod import range_sets
from test_raycast import random_rays
from test_shapecast import random_queries

pytestmark = pytest.mark.gpu

HDR_LISTS = 8  # vx_host.inl: the header's list totals, one word per level
FIELDS = ("gentle64_nozero", "terrain128")
LEVELS = {"gentle64_nozero": 3, "terrain128": 4}


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.init()
    return torch


def field(name):
    """(dist, mat, blend, the form of the kept runs)"""
    if name == "terrain128":
        return tuple(plan_field(name)) + (KEPT_ONE,)
    return sf.make(name)


def upload(p, name):
    d, m, b, kept = field(name)
    p.upload(d, m, b, cellmap.flags_of(d))
    return kept


def steady(p, levels=0, kept=KEPT_ONE):
    """behind an upload: the runs that leave plan, store and layout, then one kept run - one launch"""
    warm(p, levels)
    return run(p, kept, levels, "the kept run in front of the queries")


@pytest.fixture(scope="module")
def resident():
    """one context per field, brought to the steady form once; every test that uses it runs one more one-launch run first"""
    made = {}

    def get(name):
        if name not in made:
            p = make_poly()
            assert upload(p, name) == KEPT_ONE
            steady(p)
            made[name] = p
        p = made[name]
        info = run(p, KEPT_ONE, label=name + ": one more one-launch run")
        assert int(info.levels) == LEVELS[name]
        return p

    yield get
    for p in made.values():
        p.close()


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


# ---- raw tables and pools ---------------------------------------------------------------------------------------------------------
def check_resident_meshes(p, label, full_run=True):
    """the body of test_gpu_parity.test_hip_device_resident_meshes on every level, and - behind a full run, which leaves the device
    lists; an incremental run keeps its lists on the host - the header's list totals"""
    from voxels_amd.binding import LISTED_BLOCK_DTYPE
    hip = _hip()
    levels = int(p.info.levels)
    dv, di, nv, ni = p.device_meshes()
    vdt = p.level(0).verts.dtype
    verts, idx = np.zeros(nv, vdt), np.zeros(ni, np.uint32)
    assert nv == 0 or hip.hipMemcpy(verts.ctypes.data_as(C.c_void_p), C.c_void_p(dv), nv * 48, 2) == 0
    assert ni == 0 or hip.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(di), ni * 4, 2) == 0
    counts = []
    for l in range(levels):
        tab, nb = p.device_block_table(l)
        counts.append(nb)
        table = np.zeros(nb, LISTED_BLOCK_DTYPE)
        assert LISTED_BLOCK_DTYPE.itemsize == 156
        assert nb == 0 or hip.hipMemcpy(table.ctypes.data_as(C.c_void_p), C.c_void_p(tab), nb * 156, 2) == 0
        lv, rg = p.level(l), p.level_ranges(l)
        assert nb == lv.infos.size, (label, l)
        for name_t, name_i in (("id", "id"), ("v_count", "n_verts"), ("i_count", "n_idx"), ("tv_count", "n_tverts"), ("ti_count", "n_tidx"),
                               ("min_corner", "min_corner"), ("max_corner", "max_corner")):
            assert np.array_equal(table[name_t], lv.infos[name_i]), (label, l, name_t)
        for name in ("v_off", "i_off", "tv_off", "ti_off"):
            assert np.array_equal(table[name], rg[name]), (label, l, name)
        assert np.all(np.diff(table["coord_id"].astype(np.int64)) > 0), (label, l)
        ov = oi = otv = oti = 0
        for k, info in enumerate(lv.infos):
            assert np.array_equal(verts[rg["v_off"][k]:rg["v_off"][k] + info["n_verts"]], lv.verts[ov:ov + info["n_verts"]]), (label, l, k)
            assert np.array_equal(idx[rg["i_off"][k]:rg["i_off"][k] + info["n_idx"]], lv.idx[oi:oi + info["n_idx"]]), (label, l, k)
            ov += info["n_verts"]; oi += info["n_idx"]
            for f in range(6):
                a, c = info["n_tverts"][f], info["n_tidx"][f]
                assert np.array_equal(verts[rg["tv_off"][k][f]:rg["tv_off"][k][f] + a], lv.tverts[otv:otv + a]), (label, l, k, f)
                assert np.array_equal(idx[rg["ti_off"][k][f]:rg["ti_off"][k][f] + c], lv.tidx[oti:oti + c]), (label, l, k, f)
                otv += a; oti += c
    # (vx_device_block_table has waited for the run: the header on the device is final.  vx_debug_header copies it raw.)
    header = p.debug_header(HDR_LISTS + levels)
    assert not full_run or header[HDR_LISTS:HDR_LISTS + levels].tolist() == counts, "%s: list totals in the device header %s, tables %s" % (label, header[HDR_LISTS:], counts)
    return counts


@pytest.mark.parametrize("name", FIELDS)
def test_tables_pools_and_header_totals(resident, name):
    p = resident(name)
    counts = check_resident_meshes(p, name)
    assert all(c > 0 for c in counts)
    # every one of the rotating header sets
    for k in range(3):
        run(p, KEPT_ONE, label="%s, set %d" % (name, k))
        assert check_resident_meshes(p, "%s, set %d" % (name, k)) == counts


def test_generation_changes_across_a_one_launch_run(resident):
    p = resident("gentle64_nozero")
    before = p.export_meshes()
    run(p, KEPT_ONE, label="one launch")
    after = p.export_meshes()
    assert after["generation"] != before["generation"]  # (a full run rewrites the pools, into the same ranges or not)
    assert (after["n_verts"], after["n_indices"]) == (before["n_verts"], before["n_indices"])


# ---- the consumers, one by one ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_ray_casts(resident, name):
    p = resident(name)
    for level in range(LEVELS[name]):
        hits = gray.check_level(p, level, random_rays(3000, p.n, 11 + level), "%s level %d" % (name, level))  # (blocks and triangles against the download)
        assert np.isfinite(hits["t"]).mean() > 0.1


@pytest.mark.parametrize("name", FIELDS)
def test_sphere_casts_and_closest_points(resident, name):
    p = resident(name)
    for level in (0, LEVELS[name] - 1):
        sh = gshape.check_level(p, level, gshape.cast_batch(p.n, 250, 21 + level), random_queries(250, p.n, 31 + level), "%s level %d" % (name, level))
        assert np.isfinite(sh["t"]).any()


@pytest.mark.parametrize("name", FIELDS)
def test_overlap_boxes(torch, resident, name):
    p = resident(name)
    snap = gscatter.snapshot(p)
    for level in (0, 1):
        assert p.raycast_prepare(level)["straddling"] == 0
        lt = goverlap.level_triangles(snap, level)
        boxes, labels = oo.cases(level, p.n, lt)
        rc, tris, corners, ranges, c = goverlap.check(torch, p, lt, level, boxes, "%s L%d" % (name, level))  # (host and device form)
        assert c["max_per_query"] == len(lt.tri) > 0 and 0 < c["hit_queries"] < len(boxes)


PERMUTED_LUT = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)  # (the table of test_gpu_layout.py, case 3)


@pytest.mark.parametrize("name", FIELDS)
def test_scatter(torch, resident, name):
    p = resident(name)
    snap = gscatter.snapshot(p)
    for level in range(LEVELS[name]):
        pts, _, c = gscatter.check(torch, p, snap, level, scatter_params(seed=1234, density=0.5), "%s L%d" % (name, level))
        assert c["points"] == c["candidates"] > 0 and c["visited_entries"] == c["entries"] == len(snap[0][level])


def test_scatter_texture_filters_follow_a_lut_change_between_one_launch_runs(torch):
    """vx_material_lut keeps plan and layout: the run behind it is one launch that writes other texture bytes into the same pool
    ranges, and a scatter that filters by them answers from the new bytes"""
    name = "gentle64_nozero"
    p = make_poly()
    try:
        upload(p, name)
        first = steady(p)
        before_tables = tables(p, first)
        old_snap = gscatter.snapshot(p)
        slot5 = np.unique(old_snap[1]["tex"][:, 5])
        values = [int(slot5[0]), int(slot5[-1])]
        prm = scatter_params(seed=77, density=1.0, texture_slot=5, texture_values=values)
        old = gscatter.check(torch, p, old_snap, 0, prm, "default map")
        everything = p.scatter(0, scatter_params(seed=77, density=1.0))[2]["points"]
        assert 0 < old[2]["points"] < everything, "the filter passes nothing or everything (a triangle it drops has no candidates)"
        p.set_materials(PERMUTED_LUT)
        info = run(p, KEPT_ONE, label="behind vx_material_lut")
        assert same_tables(tables(p, info), before_tables)
        new_snap = gscatter.snapshot(p)
        assert not np.array_equal(new_snap[1]["tex"], old_snap[1]["tex"]) and np.array_equal(new_snap[1]["pos"], old_snap[1]["pos"])
        for level in range(int(info.levels)):
            new = gscatter.check(torch, p, new_snap, level, prm, "permuted map L%d" % level)
            if level == 0:
                assert new[0].tobytes() != old[0].tobytes() or new[2] != old[2], "the scatter answered from the old texture bytes"
                stale = so.scatter(0, prm, old_snap[0][0], old_snap[1], old_snap[2])
                assert stale[1].tobytes() != new[0].tobytes()
    finally:
        p.set_materials(vxo.default_lut())
        p.close()


@pytest.mark.parametrize("name", FIELDS)
def test_lod_select(resident, name):
    p = resident(name)
    glod.check_many(p, 3, 2, name)  # (2 cameras, every range set, every plane set, on the tables as they are behind the run)


# ---- the frame loop -------------------------------------------------------------------------------------------------------------------
def lod_key(draws):
    """what of a LOD draw record is free of table positions (tests/test_gpu_lod.py, the slab case)"""
    return sorted(zip(draws["level"].tolist(), draws["coord_id"].tolist(), draws["transitions"].tolist(), draws["adjacency"].tolist()))


@pytest.mark.parametrize("name", FIELDS)
def test_frame_loop(torch, resident, name):
    from voxels_amd import lod_ranges
    p = resident(name)
    n = p.n
    cam = np.float32([0.45 * n, 0.6 * n, 0.4 * n])
    planes = glod.frustum(cam, [n / 2, n / 3, n / 2], n)
    rays = random_rays(500, n, 17)
    prm = scatter_params(seed=4321, density=0.5, min_up=-0.5)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros((20, len(rays) * 48), dtype=torch.uint8, device="cuda")  # (a row per frame, zeroed here: nothing to wait for later)
    torch.cuda.synchronize()
    first = None
    for k in range(20):
        info = run(p, KEPT_ONE, label="%s, frame %d" % (name, k))
        # the device form first, queued behind a run that has returned on its header flag and may still be in flight: nothing
        # between the run and this call waits for the stream
        p.raycast_device(d_rays.data_ptr(), len(rays), d_hits[k].data_ptr())
        torch.cuda.synchronize()
        queued = d_hits[k].cpu().numpy().tobytes()
        draws, regular, transition, counts = p.lod_select(cam, lod_ranges(2.0), planes)
        hits = p.raycast_rays(rays, 0)
        assert queued == hits.tobytes(), "%s, frame %d: the rays queued behind the run and the ones behind a wait differ" % (name, k)
        rc, points, ranges, sc = p.scatter_raw(0, prm, 1 << 18)
        assert rc == 0
        points = points[:int(sc["points"])]
        frame = (draws.tobytes(), regular.tobytes(), transition.tobytes(), counts, hits.tobytes(), points.tobytes(), ranges.tobytes(),
                 {f: int(sc[f]) for f in so.SCATTER_COUNTS_DTYPE.names})
        if first is None:
            first, first_tables = frame, tables(p, info)
            assert counts["records"] > 0 and np.isfinite(hits["t"]).any() and len(points) > 0
        else:
            # (records with pool offsets - the draw arguments - included: the layout is kept)
            for i, (a, b) in enumerate(zip(frame, first)):
                assert a == b, "%s, frame %d: answer %d differs from frame 0" % (name, k, i)
        if k in (0, 19):
            assert same_tables(tables(p, info), first_tables)
            glod.check(p, cam, lod_ranges(2.0), planes, "%s, frame %d" % (name, k))
            gray.check_level(p, 0, rays, "%s, frame %d" % (name, k))
            gscatter.check(torch, p, gscatter.snapshot(p), 0, prm, "%s, frame %d" % (name, k), device=False)


# ---- against a context's first run -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIELDS)
def test_answers_equal_those_behind_a_single_first_run(torch, resident, name):
    """The steady context and a fresh context behind ONE execute() hold the same meshes in pools laid out differently (the chain of
    launches reserves in another order).  Compared byte for byte is what is free of pool offsets and table positions - the fields
    the existing tests blank or key by coord_id:
      ray, sphere and point hits   everything but `entry` (a table position; test_gpu_raycast's slab case compares t, block_id, tri)
      scatter                      points per coord_id with entry and block_id blanked (test_gpu_scatter.by_coord)
      overlap boxes                per query (coord_id, tri, corner bytes) (test_gpu_overlap.keyed)
      LOD select                   (level, coord_id, transitions, adjacency) per draw record and the counts (test_gpu_lod, the slab case)
    The draw arguments of LOD select and the ranges are pool offsets: there the oracle is the judge (the tests above)."""
    from voxels_amd import lod_ranges
    p = resident(name)
    fresh = make_poly()
    try:
        upload(fresh, name)
        fresh.execute()
        n = p.n
        rays = random_rays(2000, n, 23)
        casts = gshape.cast_batch(n, 500, 24)
        queries = random_queries(500, n, 25)
        cam = np.float32([0.3 * n, 0.7 * n, 0.55 * n])
        prm = scatter_params(seed=99, density=0.5, max_up=0.9)
        snaps = [gscatter.snapshot(q) for q in (p, fresh)]
        for level in range(LEVELS[name]):
            got = []
            for q in (p, fresh):
                assert q.raycast_prepare(level)["straddling"] == 0
                answers = [q.raycast_rays(rays, level), q.spherecast_casts(casts, level), q.closest_points_queries(queries, level)]
                for a in answers:
                    a["entry"] = 0
                got.append([a.tobytes() for a in answers])
            assert got[0] == got[1], "%s L%d: ray, sphere or point hits" % (name, level)
            pts = [q.scatter(level, prm) for q in (p, fresh)]
            assert pts[0][2] == pts[1][2]
            assert gscatter.by_coord(snaps[0][0][level], pts[0][0], pts[0][1]) == gscatter.by_coord(snaps[1][0][level], pts[1][0], pts[1][1]), (name, level)
            if level < 2:
                lt = goverlap.level_triangles(snaps[0], level)
                boxes, _ = oo.cases(level, n, lt, random_boxes=100)
                ans = [goverlap.host_form(q, level, boxes) for q in (p, fresh)]
                assert ans[0][4] == ans[1][4] and ans[0][3].tobytes() == ans[1][3].tobytes()
                for qi in range(len(boxes)):
                    assert goverlap.keyed(snaps[0][0][level], ans[0], qi) == goverlap.keyed(snaps[1][0][level], ans[1], qi), (name, level, qi)
        sel = [q.lod_select(cam, lod_ranges(2.0), glod.frustum(cam, [n / 2, n / 3, n / 2], n)) for q in (p, fresh)]
        assert sel[0][3] == sel[1][3] and lod_key(sel[0][0]) == lod_key(sel[1][0]) and len(sel[0][0]) > 0
    finally:
        fresh.close()


# ---- form changes under a built index -------------------------------------------------------------------------------------------------------
def every_query(torch, p, label, seed, full_run=True):
    """every consumer once, each against its oracle on the meshes of this moment"""
    from voxels_amd import lod_ranges
    n = p.n
    snap = gscatter.snapshot(p)
    for level in (0, 1):
        gray.check_level(p, level, random_rays(1000, n, seed + level), "%s, rays L%d" % (label, level))
    gshape.check_level(p, 0, gshape.cast_batch(n, 150, seed + 2), random_queries(150, n, seed + 3), label + ", shapes L0")
    lt = goverlap.level_triangles(snap, 0)
    boxes, _ = oo.cases(0, n, lt, random_boxes=100)
    goverlap.check(torch, p, lt, 0, boxes, label + ", overlap L0", device=False)
    for level in (0, 1):
        gscatter.check(torch, p, snap, level, scatter_params(seed=seed, density=0.5), "%s, scatter L%d" % (label, level), device=level == 0)
    cam = np.float32([0.4 * n, 0.65 * n, 0.5 * n])
    glod.check(p, cam, lod_ranges(2.0), glod.frustum(cam, [n / 2, n / 3, n / 2], n), label + ", LOD")
    check_resident_meshes(p, label, full_run)


def test_queries_across_compaction(torch):
    """query, vx_compact_pools (moves the meshes, rewrites every offset, drops the layout), a kept run of two launches, query, a
    one-launch run, query"""
    p = make_poly()
    try:
        upload(p, "gentle64_nozero")
        steady(p)
        every_query(torch, p, "steady", 40)
        p.compact_pools()
        every_query(torch, p, "compacted", 40)
        run(p, KEPT_TWO, label="first run behind vx_compact_pools")
        every_query(torch, p, "behind the two-launch run", 40)
        run(p, KEPT_ONE, label="second run behind vx_compact_pools")
        every_query(torch, p, "behind the one-launch run", 40)
    finally:
        p.close()


def test_queries_across_an_incremental_run(torch, port):
    """query, carve, incremental run, query, full run (hands out its slots), query, kept run, query"""
    p = make_poly()
    try:
        upload(p, "gentle64_nozero")
        steady(p)
        every_query(torch, p, "steady", 50)
        before = p.raycast_rays(random_rays(1000, p.n, 50), 0)
        mn, mx = p.inject_ball((30.0, 33.5, 31.25), (8, 8, 8), 5.0, 2)
        assert len(p.execute_dirty(mn, mx))
        every_query(torch, p, "behind the incremental run", 50, full_run=False)
        assert p.raycast_rays(random_rays(1000, p.n, 50), 0).tobytes() != before.tobytes(), "the carve changed no answer"
        d_now = port.grid_load(p.pack()).read_dense()[0]
        assert all(c.max() <= sf.LARGE_THRESHOLD for c in sf.per_level(d_now))
        kept = KEPT_TWO if hands_on(d_now) else KEPT_ONE  # (the ball leaves zeros wherever x^2 + y^2 + z^2 = r^2 has lattice solutions)
        run(p, HANDS_OUT, label="full run behind the incremental one")
        every_query(torch, p, "behind the full run", 50)
        run(p, kept, label="kept run behind it")
        every_query(torch, p, "behind the kept run", 50)
    finally:
        p.close()


# ---- grids without a surface, and the single block ----------------------------------------------------------------------------------------
def test_queries_on_a_grid_without_a_surface(torch):
    from voxels_amd import lod_ranges
    from voxels_amd.binding import RAY_NONE
    p = make_poly()
    try:
        assert upload(p, "empty64") == KEPT_ONE
        info = steady(p)
        n, levels = p.n, int(info.levels)
        assert levels == 3 and check_resident_meshes(p, "empty64") == [0, 0, 0]
        assert p.device_meshes()[2:] == (0, 0)
        cam = np.float32([20, 30, 40])
        for k, ranges in enumerate(range_sets(n, cam)):
            glod.check(p, cam, ranges, None, "empty64 ranges %d" % k)
        draws, regular, transition, counts = p.lod_select(cam, lod_ranges(), glod.frustum(cam, [n / 2, n / 3, n / 2], n))
        assert len(draws) == len(regular) == len(transition) == 0 and counts["records"] == 0 and counts["meshed_leaves"] == 0
        for level in range(levels):
            prep = p.raycast_prepare(level)
            assert prep["blocks"] == prep["triangles"] == prep["straddling"] == 0
            h = p.raycast_rays(random_rays(500, n, 3), level)
            assert np.isinf(h["t"]).all() and (h["entry"] == RAY_NONE).all() and (h["tri"] == RAY_NONE).all()
            sh = p.spherecast_casts(gshape.cast_batch(n, 200, 4), level)
            assert np.isinf(sh["t"]).all() and (sh["entry"] == RAY_NONE).all()
            ph = p.closest_points_queries(random_queries(200, n, 5), level)
            assert np.isinf(ph["dist"]).all() and (ph["entry"] == RAY_NONE).all()
            boxes = oo.overlap_boxes([[0, 0, 0], [-np.inf] * 3], [[n, n, n], [np.inf] * 3])
            rc, tris, crn, ranges, c = p.overlap_boxes_raw(level, boxes, 0)
            assert rc == 0 and not any(oo.counts_dict(c)[f] for f in ("triangles", "pairs", "hit_queries", "max_per_query")) and not ranges.view(np.uint32).any()
            tris, crn, dranges, dc, intact = goverlap.device_form(torch, p, level, boxes, 16)
            assert intact and not any(dc[f] for f in ("triangles", "pairs", "hit_queries", "max_per_query")) and len(tris) == 0
            rc, points, ranges, sc = p.scatter_raw(level, scatter_params(seed=1), 0)
            assert rc == 0 and int(sc["points"]) == int(sc["candidates"]) == int(sc["entries"]) == 0
            _, _, dc, intact = gscatter.device_form(torch, p, level, scatter_params(seed=1), 16, 0)
            assert intact and not any(dc.values())
    finally:
        p.close()


def test_queries_on_the_single_block_grid(torch):
    """16^3: one level, so every run is the chain of launches (steady_fields.py) - three runs of that form, then every consumer"""
    from voxels_amd import lod_ranges
    p = make_poly()
    try:
        assert upload(p, "terrain16") == HANDS_OUT
        info = steady(p, kept=HANDS_OUT)
        n = p.n
        assert int(info.levels) == 1 and check_resident_meshes(p, "terrain16") == [1]
        snap = gscatter.snapshot(p)
        hits = gray.check_level(p, 0, random_rays(2000, n, 6), "terrain16 rays")
        assert np.isfinite(hits["t"]).any()
        gshape.check_level(p, 0, gshape.cast_batch(n, 200, 7, 0.25, 3.0), random_queries(200, n, 8), "terrain16 shapes")
        lt = goverlap.level_triangles(snap, 0)
        boxes, _ = oo.cases(0, n, lt, random_boxes=100)
        goverlap.check(torch, p, lt, 0, boxes, "terrain16 overlap")
        pts, ranges, c = gscatter.check(torch, p, snap, 0, scatter_params(seed=5, density=2.0), "terrain16 scatter")
        assert c["points"] > 0 and ranges.tolist() == [(0, c["points"])]
        glod.check_many(p, 3, 2, "terrain16")
        draws = p.lod_select(np.float32([8, 8, 8]), lod_ranges())[0]
        assert len(draws) == 1 and int(draws["level"][0]) == 0
    finally:
        p.close()
