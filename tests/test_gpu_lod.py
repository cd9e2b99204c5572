"""LOD selection on the MI355X (vx_lod_select*) against the numpy oracle of tests/lod_oracle.py, on the block tables the same
context left on the device."""
import ctypes as C

import numpy as np
import pytest

import fields
import vxo
from golden_io import Golden
from lod_oracle import ADJ_BIT, Selection, face_axis, ref_levels, select
from test_lod import cameras, range_sets

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


def synth_poly(n, seed=1337, style=0, levels=0):
    from voxels_amd import synth
    d, m, b = synth.terrain(n, seed=seed, style=style)
    p = new_poly()
    p.upload(d, m, b, synth.block_empty_flags(d))
    p.execute(levels)
    return p


def tables(p):
    """the context's device block tables, copied raw"""
    from voxels_amd.binding import LISTED_BLOCK_DTYPE
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    out = []
    for L in range(p.info.levels):
        tab, nb = p.device_block_table(L)
        t = np.zeros(nb, LISTED_BLOCK_DTYPE)
        assert nb == 0 or hip.hipMemcpy(t.ctypes.data_as(C.c_void_p), C.c_void_p(tab), nb * LISTED_BLOCK_DTYPE.itemsize, 2) == 0
        out.append(t)
    return out


def frustum(eye, target, n, fov=60.0, aspect=1.5, near=0.5, far=None):
    """six planes (a, b, c, d), inside where a x + b y + c z + d >= 0, of a perspective view in mesh space"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, [0.0, 1.0, 0.0])
    if np.linalg.norm(r) < 1e-6:
        r = np.cross(f, [1.0, 0.0, 0.0])
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    tv = np.tan(np.radians(fov) / 2)
    th = tv * aspect
    far = 4.0 * n if far is None else far
    normals = [f, -f, f * th - r, f * th + r, f * tv - u, f * tv + u]
    ds = [-np.dot(f, eye + f * near), np.dot(f, eye + f * far)] + [-np.dot(nn, eye) for nn in normals[2:]]
    return np.array([list(nn) + [d] for nn, d in zip(normals, ds)], np.float32)


def plane_sets(n, cam):
    return [None, frustum(cam, [n / 2, n / 3, n / 2], n), frustum([-10, n / 2, n / 2], [-100, n / 2, n / 2], n, far=50)]


def check(p, cam, ranges, planes, label, tabs=None, sel=None):
    tabs = tables(p) if tabs is None else tabs
    sel = Selection(p.n, p.info.levels, cam, ranges) if sel is None else sel
    draws, regular, transition, counts = p.lod_select(cam, ranges, planes)
    want = select(sel, tabs, () if planes is None else planes)
    assert counts == want[3], (label, counts, want[3])
    assert counts["leaf_volume"] == (p.n // 16) ** 3, label
    assert draws.tobytes() == want[0].tobytes(), label
    assert regular.tobytes() == want[1].tobytes(), label
    assert transition.tobytes() == want[2].tobytes(), label
    return draws, counts


def check_many(p, seed, count, label, all_planes=True):
    tabs = tables(p)
    for k, cam in enumerate(cameras(p.n, seed, count)):
        for j, ranges in enumerate(range_sets(p.n, cam)):
            sel = Selection(p.n, p.info.levels, cam, ranges)
            for i, planes in enumerate(plane_sets(p.n, cam) if all_planes else [None]):
                check(p, cam, ranges, planes, "%s cam %d ranges %d planes %d" % (label, k, j, i), tabs, sel)


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat", "caves128", "synth256"])
def test_lod_matches_the_oracle(torch, name):
    p = new_poly()
    if name == "caves128":
        port = vxo.load_port()
        assert port is not None, "oracle/libvoxels_port.so missing (run __graft_entry__.build())"
        g = port.grid_from_float(fields.terrain_field(128, 5), *fields.materials_for(128, 5))
        p.upload(*g.read_dense(), g.block_flags())
        p.execute()
    elif name == "synth256":
        p.close()
        p = synth_poly(256, seed=7)
    else:
        gold = Golden(name)
        p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
        p.execute()
    check_many(p, 3, 4, name)
    p.close()


def test_lod_1024(torch):
    p = new_poly()
    p.create_terrain(1024, 1337)
    info = p.execute()
    assert info.levels == 7
    tabs = tables(p)
    for k, cam in enumerate([np.float32([512, 300, 512]), np.float32([100, 700, 900]), np.float32([-200, 400, 1300])]):
        for j, ranges in enumerate(range_sets(1024, cam)[:3]):
            sel = Selection(1024, 7, cam, ranges)
            for i, planes in enumerate(plane_sets(1024, cam)):
                _, counts = check(p, cam, ranges, planes, "1024 cam %d ranges %d planes %d" % (k, j, i), tabs, sel)
    p.close()


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [48, 80, 112, 208, 336])
def test_lod_odd_sizes_every_level_limit(torch, n):
    for levels in range(1, ref_levels(n) + 1):
        p = synth_poly(n, seed=30 + n, levels=levels)
        assert p.info.levels == levels
        check_many(p, n + levels, 3, "n=%d levels=%d" % (n, levels), all_planes=levels == ref_levels(n))
        p.close()


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_adjacency_bits_from_the_meshes(torch):
    """Transition mesh f lies on face f of its block; a regular vertex with bit ADJ_BIT[f] of sec[3] lies on face f's plane:
    that pins both the face order of `transitions` and the mapping to `adjacency` (the same order: bit b is face b)."""
    n = 256
    p = synth_poly(n, seed=5, style=1)
    seen, marked = np.zeros(6, int), np.zeros(6, int)
    for L in range(1, ref_levels(n) - 1):
        lv = p.level(L)
        s = np.float32(16 << L)
        sec3 = lv.verts["sec"][:, 3].copy().view(np.uint32)
        ov = otv = 0
        for info in lv.infos:
            mn, mx = info["min_corner"], info["max_corner"]
            assert np.allclose(mx - mn, s)
            pos = lv.verts["pos"][ov:ov + info["n_verts"]]
            bits = sec3[ov:ov + info["n_verts"]]
            ov += info["n_verts"]
            for f in range(6):
                a, d = face_axis(f)
                m = (0, 2, 1)[a]                              # mesh axis of internal axis a
                plane = mx[m] if d > 0 else mn[m]
                tv = lv.tverts["pos"][otv:otv + info["n_tverts"][f]]
                otv += info["n_tverts"][f]
                if len(tv):
                    seen[f] += 1
                    assert (tv >= mn - 1e-3).all() and (tv <= mx + 1e-3).all(), (L, f)
                    assert (np.abs(tv[:, m] - plane) <= (1 << L) + 1e-3).all(), (L, f)
                on = (bits & (1 << ADJ_BIT[f])) != 0
                assert (np.abs(pos[on, m] - plane) <= 1e-3).all(), (L, f)
                marked[f] += int(on.sum())
    assert (seen > 0).all() and (marked > 0).all(), (seen, marked)
    p.close()


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_lod_after_edits_compaction_and_a_full_run(torch):
    from voxels_amd import DRAW_INDEXED_DTYPE, LOD_COUNTS_DTYPE, LOD_DRAW_DTYPE, lod_params, lod_ranges
    n = 128
    p = synth_poly(n, seed=21)
    cam = np.float32([60, 70, 50])
    check(p, cam, lod_ranges(), None, "first run")
    for step, (pos, r, kind) in enumerate([((40.0, 50.0, 64.0), 6.0, 2), ((80.0, 70.0, 60.0), 7.5, 0)]):
        mn, mx = p.inject_ball(pos, (16, 16, 16), r, kind)
        p.execute_dirty(mn, mx)
        check(p, cam, lod_ranges(), None, "edit %d" % step)
        check(p, cam, lod_ranges(2.0), frustum(cam, [64, 40, 64], n), "edit %d frustum" % step)
    p.compact_pools()
    check(p, cam, lod_ranges(), None, "compacted")
    p.execute()
    want = check(p, cam, lod_ranges(), frustum(cam, [64, 40, 64], n), "full run")
    # the device variant on a torch stream
    draws, regular, transition, counts = p.lod_select(cam, lod_ranges(), frustum(cam, [64, 40, 64], n))
    cap, tcap = len(draws) + 5, len(transition) + 5
    d_draws = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda")
    d_reg = torch.zeros((cap * 20 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_tr = torch.zeros((tcap * 20 + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(32, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.lod_select_device(lod_params(cam, lod_ranges(), frustum(cam, [64, 40, 64], n)), cap, tcap, d_draws.data_ptr(),
                        d_reg.data_ptr(), d_tr.data_ptr(), d_cnt.data_ptr())
    s.synchronize()
    p.set_stream(0)
    got = d_cnt.cpu().numpy().view(LOD_COUNTS_DTYPE)[0]
    assert {k: int(got[k]) for k in LOD_COUNTS_DTYPE.names} == counts
    assert d_draws.cpu().numpy()[:len(draws) * 32].tobytes() == draws.tobytes()
    assert d_reg.cpu().numpy()[:len(regular) * 20].tobytes() == regular.tobytes()
    assert d_tr.cpu().numpy()[:len(transition) * 20].tobytes() == transition.tobytes()
    assert want[1] == counts
    p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_lod_slab_contexts_union_to_the_whole_grid(torch):
    from voxels_amd import lod_ranges, synth
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world = 256, 2
    assert sharded_levels(n, world) == 4
    d, m, b = synth.terrain(n, seed=77)
    flags = synth.block_empty_flags(d)
    whole = new_poly()
    whole.upload(d, m, b, flags)
    whole.execute(4)
    key = lambda dr: sorted(zip(dr["level"].tolist(), dr["coord_id"].tolist(), dr["transitions"].tolist(), dr["adjacency"].tolist()))
    bufs = []
    for cam in (np.float32([100, 90, 60]), np.float32([200, 140, 230])):
        want = whole.lod_select(cam, lod_ranges(3.0))[0]
        got = []
        for r in range(world):
            buf = SlabBuffers(torch, n, r, world, "cuda", axis="y")
            buf.fill_from_full(d, m, b, flags)
            q = new_poly()
            buf.attach(q)
            q.execute(sharded_levels(n, world))
            got += key(q.lod_select(cam, lod_ranges(3.0))[0])
            bufs.append((buf, q))
        assert sorted(got) == key(want)
    for _, q in bufs:
        q.close()
    whole.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_lod_errors_and_overflow(torch):
    from voxels_amd import LOD_COUNTS_DTYPE, LOD_DRAW_DTYPE, DRAW_INDEXED_DTYPE, lod_params, lod_ranges
    from voxels_amd.binding import VoxelsHipError, _ptr
    p = new_poly()
    with pytest.raises(VoxelsHipError):
        p.lod_select([1, 1, 1])                                           # no surface
    p.close()
    p = synth_poly(128, seed=4)
    assert p.execute_from(0, 1).first_meshed_level == 1
    with pytest.raises(VoxelsHipError):
        p.lod_select([1, 1, 1])                                           # levels left unmeshed
    p.execute()
    lib = p._lib
    cnt = np.zeros(1, LOD_COUNTS_DTYPE)
    for bad in ([np.nan, 1, 1], lod_ranges()), ([1, 1, 1], np.float32([0, np.nan] + [0] * 14)):
        with pytest.raises(VoxelsHipError):
            p.lod_select(*bad)
    prm = lod_params([1, 1, 1], lod_ranges(), np.float32([[0, 1, 0, np.nan]]))
    assert lib.vx_lod_select(p._h, _ptr(prm), 0, 0, None, None, None, _ptr(cnt)) == -1
    prm = lod_params([1, 1, 1])
    prm["n_planes"] = 7
    assert lib.vx_lod_select(p._h, _ptr(prm), 0, 0, None, None, None, _ptr(cnt)) == -1
    prm = lod_params([60, 60, 60], lod_ranges(1.0))
    assert lib.vx_lod_select(p._h, _ptr(prm), 4, 0, None, None, None, _ptr(cnt)) == -1
    assert lib.vx_lod_select(p._h, _ptr(prm), 0, 4, None, None, None, _ptr(cnt)) == -1
    assert lib.vx_lod_select(p._h, _ptr(prm), 0, 0, None, None, None, None) == -1
    # overflow: counts in full, the first `capacity` entries equal to the oracle's
    sel = Selection(128, p.info.levels, np.float32([60, 60, 60]), lod_ranges(1.0))
    want = select(sel, tables(p))
    assert want[3]["records"] > 8 and want[3]["transition"] > 4
    draws, regular, tr = np.zeros(8, LOD_DRAW_DTYPE), np.zeros(8, DRAW_INDEXED_DTYPE), np.zeros(4, DRAW_INDEXED_DTYPE)
    rc = lib.vx_lod_select(p._h, _ptr(prm), 8, 4, _ptr(draws), _ptr(regular), _ptr(tr), _ptr(cnt))
    assert rc == -3
    assert {k: int(cnt[k][0]) for k in LOD_COUNTS_DTYPE.names} == want[3]
    assert draws.tobytes() == want[0][:8].tobytes() and regular.tobytes() == want[1][:8].tobytes()
    assert tr.tobytes() == want[2][:4].tobytes()
    # zero capacities: counts only
    assert lib.vx_lod_select(p._h, _ptr(prm), 0, 0, None, None, None, _ptr(cnt)) == -3
    assert int(cnt["records"][0]) == want[3]["records"]
    p.close()
