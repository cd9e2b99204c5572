"""Ray casts against the regular meshes of a level (include/voxels_hip.h, vx_raycast*): the ABI, the binding, and the float64
oracle the GPU tests (tests/test_gpu_raycast.py) and tools/raycast_bench.py compare the device with.

The oracle shares no code with the library: Moeller-Trumbore in float64 over a level as Polygonizer.level(L) downloads it,
both faces, inclusive edges, prefiltered with the blocks' boxes."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TIE_T = 1e-6         # hits within this of the nearest t are ties
GRAZE_MARGIN = 1e-5  # barycentric margin below which a ray counts as grazing
GRAZE_DOT = 0.02     # |dot(unit dir, unit normal)| below which a ray counts as grazing


class OracleLevel:
    """The regular triangles of one downloaded level, in float64: tri[k] = 3 x 3 vertex positions, ent[k] / ord[k] = its
    table entry and ordinal in the block's mesh, boxes[entry] = the block's corners."""

    def __init__(self, level):
        infos = level.infos
        vo = np.concatenate([[0], np.cumsum(infos["n_verts"].astype(np.int64))])
        io = np.concatenate([[0], np.cumsum(infos["n_idx"].astype(np.int64))])
        pos = level.verts["pos"].astype(np.float64)
        tris, ent, ords = [], [], []
        for e in range(len(infos)):
            ix = level.idx[io[e]:io[e + 1]].astype(np.int64).reshape(-1, 3)
            tris.append(pos[vo[e] + ix])
            ent.append(np.full(len(ix), e, np.int64))
            ords.append(np.arange(len(ix), dtype=np.int64))
        self.ids = infos["id"].astype(np.int64)
        self.lo = infos["min_corner"].astype(np.float64)
        self.hi = infos["max_corner"].astype(np.float64)
        self.tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.ent = np.concatenate(ent) if ent else np.zeros(0, np.int64)
        self.ord = np.concatenate(ords) if ords else np.zeros(0, np.int64)
        self.first = np.concatenate([[0], np.cumsum([len(t) for t in tris])]).astype(np.int64)

    @classmethod
    def from_triangles(cls, tris):
        """One block holding the given triangles (hand-made cases)."""
        self = cls.__new__(cls)
        self.tri = np.asarray(tris, np.float64).reshape(-1, 3, 3)
        self.ent = np.zeros(len(self.tri), np.int64)
        self.ord = np.arange(len(self.tri), dtype=np.int64)
        self.ids = np.zeros(1, np.int64)
        self.lo = self.tri.reshape(-1, 3).min(0)[None] - 1.0
        self.hi = self.tri.reshape(-1, 3).max(0)[None] + 1.0
        self.first = np.array([0, len(self.tri)], np.int64)
        return self

    def normal(self, entry, tri):
        t = self.tri[self.first[entry] + tri]
        n = np.cross(t[1] - t[0], t[2] - t[0])
        return n / np.linalg.norm(n)


def oracle_cast(lvl, rays, near=GRAZE_MARGIN):
    """For each ray: t (inf = miss), the tied (entry, tri) pairs, the winner's barycentric margin, its unit normal and hit
    point, and `near_miss`: a triangle missed by less than `near` (barycentric) at t <= the winner's (or with no winner)."""
    o = np.stack([rays["origin"][:, a].astype(np.float64) for a in range(3)], 1)
    d = np.stack([rays["dir"][:, a].astype(np.float64) for a in range(3)], 1)
    tmin, tmax = rays["t_min"].astype(np.float64), rays["t_max"].astype(np.float64)
    n = len(rays)
    bad = ~np.isfinite(o).all(1) | np.isnan(d).any(1) | ~(np.abs(d) > 0).any(1)
    hits = [[] for _ in range(n)]   # (t, entry, tri, margin)
    nearest_near = np.full(n, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        for e in range(len(lvl.first) - 1):
            if lvl.first[e] == lvl.first[e + 1]:
                continue
            # rays whose line segment [tmin, tmax] meets the block's box (slab test, zero components on the origin alone)
            ta = (lvl.lo[e] - 1e-6 - o) * inv
            tb = (lvl.hi[e] + 1e-6 - o) * inv
            lo = np.where(d == 0, np.where((o >= lvl.lo[e] - 1e-6) & (o <= lvl.hi[e] + 1e-6), -np.inf, np.inf), np.minimum(ta, tb))
            hi = np.where(d == 0, np.where((o >= lvl.lo[e] - 1e-6) & (o <= lvl.hi[e] + 1e-6), np.inf, -np.inf), np.maximum(ta, tb))
            t0 = np.maximum(lo.max(1), tmin)
            t1 = np.minimum(hi.min(1), tmax)
            sel = np.nonzero((t0 <= t1) & ~bad)[0]
            if not len(sel):
                continue
            T = lvl.tri[lvl.first[e]:lvl.first[e + 1]]                        # (m, 3, 3)
            A, e1, e2 = T[:, 0], T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]
            D, O = d[sel][:, None, :], o[sel][:, None, :]                       # (r, 1, 3)
            p = np.cross(D, e2[None])                                            # (r, m, 3)
            det = np.einsum("rmk,mk->rm", p, e1)
            s = O - A[None]
            q = np.cross(s, e1[None])
            u = np.einsum("rmk,rmk->rm", s, p) / det
            v = np.einsum("rmk,rmk->rm", np.broadcast_to(D, q.shape), q) / det
            t = np.einsum("rmk,mk->rm", q, e2) / det
            margin = np.minimum(np.minimum(u, v), 1.0 - u - v)
            inrange = (det != 0) & (t >= tmin[sel][:, None]) & (t <= tmax[sel][:, None])
            hit = inrange & (margin >= 0)
            nm = inrange & (margin < 0) & (margin > -near)
            for r, k in zip(*np.nonzero(hit)):
                hits[sel[r]].append((t[r, k], e, k, margin[r, k]))
            if nm.any():
                tn = np.where(nm, t, np.inf).min(1)
                nearest_near[sel] = np.minimum(nearest_near[sel], tn)
    out_t = np.full(n, np.inf)
    margin = np.full(n, np.inf)
    nrm = np.zeros((n, 3))
    pos = np.zeros((n, 3))
    ties = [set() for _ in range(n)]
    for r in range(n):
        if not hits[r]:
            continue
        h = sorted(hits[r])
        best = h[0][0]
        out_t[r] = best
        for (t, e, k, m) in h:
            if t - best > TIE_T:
                break
            ties[r].add((int(e), int(k)))
        margin[r] = h[0][3]
        nrm[r] = lvl.normal(h[0][1], h[0][2])
        pos[r] = o[r] + best * d[r]
    near_miss = np.isfinite(nearest_near) & (nearest_near <= np.where(np.isfinite(out_t), out_t + TIE_T, np.inf))
    return {"t": out_t, "ties": ties, "margin": margin, "nrm": nrm, "pos": pos, "near_miss": near_miss}


def compare_hits(lvl, rays, hits, ref, max_grazing=0.01, label=""):
    """The comparison rule of the ray casts: grazing rays (oracle margin < 1e-5, |dot(d, n)| < 0.02, or a near miss) at most
    `max_grazing` of the batch and left out; every other ray agrees on hit / miss, reports a tied (entry, tri) with that
    entry's block id, its hit point within 1e-3 voxels and the triangle's normal within 1e-5.  Returns the grazing count."""
    from voxels_amd.binding import RAY_NONE
    n = len(rays)
    d = np.stack([rays["dir"][:, a].astype(np.float64) for a in range(3)], 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        dn = d / np.linalg.norm(d, axis=1, keepdims=True)
    dot = np.abs((dn * ref["nrm"]).sum(1))
    hit = np.isfinite(ref["t"])
    grazing = ref["near_miss"] | (hit & ((ref["margin"] < GRAZE_MARGIN) | (dot < GRAZE_DOT)))
    assert grazing.sum() <= max_grazing * n, "%s: %d of %d rays graze" % (label, grazing.sum(), n)
    errors = []
    for r in np.nonzero(~grazing)[0]:
        h = hits[r]
        if not hit[r]:
            if np.isfinite(h["t"]) or h["entry"] != RAY_NONE or h["block_id"] != RAY_NONE or h["tri"] != RAY_NONE:
                errors.append((r, "device hit (entry %d, tri %d, t %g), oracle miss" % (h["entry"], h["tri"], h["t"])))
            continue
        if not np.isfinite(h["t"]):
            errors.append((r, "device miss, oracle t %g %s" % (ref["t"][r], sorted(ref["ties"][r])[:3])))
            continue
        key = (int(h["entry"]), int(h["tri"]))
        if key not in ref["ties"][r]:
            errors.append((r, "device (entry, tri) %s at t %.9g, oracle %s at t %.9g" % (key, h["t"], sorted(ref["ties"][r])[:3], ref["t"][r])))
            continue
        if int(h["block_id"]) != int(lvl.ids[key[0]]):
            errors.append((r, "block id %d, table says %d" % (h["block_id"], lvl.ids[key[0]])))
        if np.abs(h["pos"].astype(np.float64) - ref["pos"][r]).max() > 1e-3:
            errors.append((r, "pos %s vs %s" % (h["pos"], ref["pos"][r])))
        if np.abs(h["nrm"].astype(np.float64) - lvl.normal(*key)).max() > 1e-5:
            errors.append((r, "nrm %s vs %s" % (h["nrm"], lvl.normal(*key))))
    assert not errors, "%s: %d of %d rays disagree with the oracle, e.g. %s" % (label, len(errors), n, errors[:5])
    return int(grazing.sum())


def make_rays(origins, dirs, t_min=0.0, t_max=np.inf):
    from voxels_amd.binding import RAY_DTYPE
    origins, dirs = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(dirs, np.float32).reshape(-1, 3)
    r = np.zeros(max(len(origins), len(dirs)), RAY_DTYPE)
    r["origin"], r["dir"], r["t_min"], r["t_max"] = origins, dirs, t_min, t_max
    return r


def random_rays(n_rays, size, seed):
    """Rays inside and outside [0, size]^3 in random directions, a share of them axis-aligned or with zero components."""
    rng = np.random.RandomState(seed)
    o = rng.uniform(-0.25 * size, 1.25 * size, (n_rays, 3))
    inside = rng.rand(n_rays) < 0.5
    o[inside] = rng.uniform(0, size, (inside.sum(), 3))
    d = rng.normal(size=(n_rays, 3))
    d *= rng.uniform(0.1, 4.0, (n_rays, 1))           # not unit length
    kind = rng.randint(0, 10, n_rays)
    axis = rng.randint(0, 3, n_rays)
    sign = np.where(rng.rand(n_rays) < 0.5, -1.0, 1.0)
    ax = kind == 0                                     # axis-aligned
    d[ax] = 0
    d[ax, axis[ax]] = sign[ax]
    zc = kind == 1                                     # one zero component
    d[zc, axis[zc]] = 0
    # rays from far outside aimed into the grid
    aim = kind == 2
    target = rng.uniform(0.2 * size, 0.8 * size, (aim.sum(), 3))
    d[aim] = target - o[aim]
    return make_rays(o, d)


def camera_rays(n, res=1024, tile=8):
    """A res x res pinhole camera above the n^3 terrain (ground near y = n / 2), looking along +z and tilted 45 degrees
    down, 60 degree field of view; lanes ordered in tile x tile pixel tiles (neighbouring lanes, neighbouring pixels)."""
    eye = np.array([0.5 * n, 0.9 * n, -0.05 * n])
    fwd = np.array([0.0, -1.0, 1.0]) / np.sqrt(2.0)
    right = np.array([1.0, 0.0, 0.0])
    up = np.cross(fwd, right)
    half = np.tan(np.radians(30.0))
    ty, tx, py, px = np.meshgrid(np.arange(res // tile), np.arange(res // tile), np.arange(tile), np.arange(tile), indexing="ij")
    y = (ty * tile + py).reshape(-1)
    x = (tx * tile + px).reshape(-1)
    sx = ((x + 0.5) / res * 2 - 1) * half
    sy = (1 - (y + 0.5) / res * 2) * half
    d = fwd[None] + sx[:, None] * right[None] + sy[:, None] * up[None]
    return make_rays(np.broadcast_to(eye, d.shape), d)


def horizontal_rays(n, count, seed=0):
    """Long walks at mid height: from the x = 0 face across the whole grid, nearly along +x, around the terrain's ground."""
    rng = np.random.RandomState(seed)
    o = np.stack([np.zeros(count), rng.uniform(0.45 * n, 0.6 * n, count), rng.uniform(0, n, count)], 1)
    d = np.stack([np.ones(count), rng.uniform(-0.02, 0.02, count), rng.uniform(-0.2, 0.2, count)], 1)
    return make_rays(o, d)


# ---- ABI and binding (no GPU) -------------------------------------------------------------------------------------------

def _header_struct_offsets():
    """Field offsets of vx_ray / vx_ray_hit as a C compiler lays them out from include/voxels_hip.h."""
    import subprocess
    import tempfile
    src = r"""
#include <stddef.h>
#include <stdio.h>
#include "voxels_hip.h"
#define F(s, f) printf("%s.%s %zu\n", #s, #f, offsetof(s, f));
int main(void) {
  printf("vx_ray %zu\nvx_ray_hit %zu\n", sizeof(vx_ray), sizeof(vx_ray_hit));
  F(vx_ray, origin) F(vx_ray, t_min) F(vx_ray, dir) F(vx_ray, t_max)
  F(vx_ray_hit, t) F(vx_ray_hit, pos) F(vx_ray_hit, nrm) F(vx_ray_hit, bary) F(vx_ray_hit, entry) F(vx_ray_hit, block_id) F(vx_ray_hit, tri)
  F(vx_ray_index_info, triangles) F(vx_ray_index_info, bytes) F(vx_ray_index_info, blocks) F(vx_ray_index_info, straddling) F(vx_ray_index_info, build_ms)
  printf("vx_ray_index_info %zu\n", sizeof(vx_ray_index_info));
  return 0;
}
"""
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "o.c"), os.path.join(tmp, "o")
        open(c, "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, c])
        out = subprocess.check_output([exe], text=True)
    return dict((k, int(v)) for k, v in (l.split() for l in out.splitlines()))


def test_ray_dtypes_match_the_header():
    from voxels_amd import HIT_DTYPE, RAY_DTYPE
    from voxels_amd.binding import RayIndexInfo
    off = _header_struct_offsets()
    assert RAY_DTYPE.itemsize == off["vx_ray"] == 32
    assert HIT_DTYPE.itemsize == off["vx_ray_hit"] == 48
    for f in RAY_DTYPE.names:
        assert RAY_DTYPE.fields[f][1] == off["vx_ray." + f], f
    for f in HIT_DTYPE.names:
        assert HIT_DTYPE.fields[f][1] == off["vx_ray_hit." + f], f
    assert C.sizeof(RayIndexInfo) == off["vx_ray_index_info"]
    for f, _ in RayIndexInfo._fields_:
        assert getattr(RayIndexInfo, f).offset == off["vx_ray_index_info." + f], f


def test_hip_library_exports_the_ray_casts():
    from voxels_amd import build
    lib = C.CDLL(build.build_hip())
    for name in ("vx_raycast_prepare", "vx_raycast_device", "vx_raycast"):
        assert hasattr(lib, name), name
    from voxels_amd.binding import HipLibrary
    assert HipLibrary().has_raycast


def test_emulation_library_still_loads_through_the_binding():
    """tests/emu compiles vx_host.inl against its own backend: no ray casts there, and the binding must not require them."""
    from emu_lib import emu_library
    from voxels_amd import Polygonizer
    from voxels_amd.binding import VoxelsHipError
    lib = emu_library()
    assert not lib.has_raycast
    p = Polygonizer(device=0, library=lib)
    with pytest.raises(VoxelsHipError):
        p.raycast([0, 0, 0], [1, 0, 0])
    p.close()


# ---- the oracle on hand-made triangles -----------------------------------------------------------------------------------

# two triangles sharing the edge (1,0,0)-(0,1,0) in the plane z = 1, and a third one behind them at z = 3
QUAD = [[[0, 0, 1], [1, 0, 1], [0, 1, 1]], [[1, 0, 1], [1, 1, 1], [0, 1, 1]], [[0, 0, 3], [4, 0, 3], [0, 4, 3]]]


def test_oracle_shared_edge_and_vertex_report_both_triangles():
    lvl = OracleLevel.from_triangles(QUAD)
    ref = oracle_cast(lvl, make_rays([[0.5, 0.5, 0], [1, 0, 0], [0.25, 0.25, 0]], [[0, 0, 1]] * 3))
    assert np.allclose(ref["t"], 1.0)
    assert ref["ties"][0] == {(0, 0), (0, 1)}          # on the shared edge
    assert ref["ties"][1] == {(0, 0), (0, 1)}          # on the shared vertex
    assert ref["ties"][2] == {(0, 0)}
    assert ref["margin"][0] == pytest.approx(0.0, abs=1e-12) and ref["margin"][2] == pytest.approx(0.25)
    assert np.allclose(ref["nrm"][2], [0, 0, 1]) and np.allclose(ref["pos"][2], [0.25, 0.25, 1])


def test_oracle_both_faces_and_not_unit_directions():
    lvl = OracleLevel.from_triangles(QUAD)
    ref = oracle_cast(lvl, make_rays([[0.25, 0.25, 5], [0.25, 0.25, 0]], [[0, 0, -2], [0, 0, 0.5]]))
    assert ref["t"][0] == pytest.approx(1.0)           # the back face of the z = 3 triangle, t in units of |dir|
    assert ref["t"][1] == pytest.approx(2.0)
    assert np.allclose(ref["pos"], [[0.25, 0.25, 3], [0.25, 0.25, 1]])


def test_oracle_parallel_rays_and_degenerate_rays_miss():
    lvl = OracleLevel.from_triangles(QUAD)
    ref = oracle_cast(lvl, make_rays([[0.25, 0.25, 1], [-1, 0.5, 1], [0.25, 0.25, 0], [np.nan, 0, 0], [0.25, 0.25, 0]],
                                     [[1, 0, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [np.nan, 0, 1]]))
    assert np.isinf(ref["t"]).all()


def test_oracle_t_windows():
    lvl = OracleLevel.from_triangles(QUAD)
    o, d = [[0.25, 0.25, 0]] * 4, [[0, 0, 1]] * 4
    rays = make_rays(o, d)
    rays["t_min"] = [0.0, 1.5, 0.0, 3.0]
    rays["t_max"] = [np.inf, np.inf, 0.5, 3.0]
    ref = oracle_cast(lvl, rays)
    assert ref["t"][0] == pytest.approx(1.0) and ref["t"][1] == pytest.approx(3.0)
    assert np.isinf(ref["t"][2]) and ref["t"][3] == pytest.approx(3.0)   # both ends of the window count


def test_oracle_near_misses_count_as_grazing():
    lvl = OracleLevel.from_triangles(QUAD[2:])
    ref = oracle_cast(lvl, make_rays([[4.000001, 0.0, 0], [2.0, 2.0 - 1e-7, 0]], [[0, 0, 1]] * 2))
    assert np.isinf(ref["t"][0]) and ref["near_miss"][0]
    assert np.isfinite(ref["t"][1]) and ref["margin"][1] < GRAZE_MARGIN
