"""The rule of vx_occlusion (include/voxels_hip.h, "ambient occlusion") stated again in numpy, from the header's text and not
from voxels_amd/csrc/tv_occlusion.h: arrays over the vertices, one pass per direction and step; test-only access to the host
build of that header (tests/occlusion/occlusion_host.cpp); and the grids and the case list the CPU and the GPU tests share.
Dense fields are indexed [z, y, x] (internal axes, Z up); vertex positions and normals are mesh space (Y up), as in the pool."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import (OCCLUSION_COUNTS_DTYPE, OCCLUSION_MAX_STEPS, OCCLUSION_PARAMS_DTYPE, OCCLUSION_TRANSITIONS,  # noqa: E402,F401
                                VERTEX_DTYPE, occlusion_params)

SO = os.path.join(ROOT, "tests", "measure", "libvoxels_measure_host.so")   # (one host library for the measurements, the height maps and the occlusion)

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.oh_check.argtypes = [u32, u32, u32, u32, vp, u32, u64, u64]
        lib.oh_bake.argtypes = [u32, u32, vp, u32, u32, vp, u32, vp, u32, u32, vp, vp, vp]
        lib.oh_quantise.argtypes = [vp, vp, u32, vp]
        lib.oh_quantise.restype = u32
        lib.oh_dir.argtypes = [u32, vp]
        lib.oh_dir.restype = None
        lib.oh_layout.argtypes = [u32, vp]
        lib.oh_layout.restype = u32
        lib.oh_limit.argtypes = [u32]
        lib.oh_limit.restype = u32
        for name in ("oh_check", "oh_bake"):
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


# ---- the header's text ------------------------------------------------------------------------------------------------------

def directions():
    """the 98 step vectors S, int64 [98, 3] (x, y, z), by the rule - in float64"""
    rows = []
    for dz in range(-2, 3):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if max(abs(dx), abs(dy), abs(dz)) == 2:
                    d = np.array([dx, dy, dz], np.float64)
                    rows.append(np.floor(256.0 * d / np.sqrt((d * d).sum()) + 0.5).astype(np.int64))
    return np.array(rows)


DIRS = directions()
assert DIRS.shape == (98, 3)


def quantise(pos, nrm, level):
    """pos, nrm float32 [k, 3], mesh axes -> (P int64 [k, 3], N int64 [k, 3], baked bool [k]), grid axes"""
    f32 = np.float32
    g = np.ascontiguousarray(pos, f32).reshape(-1, 3)[:, [0, 2, 1]]
    m = np.ascontiguousarray(nrm, f32).reshape(-1, 3)[:, [0, 2, 1]]
    with np.errstate(all="ignore"):
        baked = np.all(np.isfinite(g) & ~(np.abs(g) > f32(4096.0)), axis=1)
        scale = f32(256.0) / f32(1 << level)
        p = np.floor(np.where(baked[:, None], g, f32(0)) * scale + f32(0.5))           # float32, one rounding per operation
        f = np.floor(m * f32(127.0) + f32(0.5))
        f = np.where(np.isfinite(m), np.clip(f, f32(-127.0), f32(127.0)), f32(0))
    assert p.dtype == f32 and f.dtype == f32
    return p.astype(np.int64), f.astype(np.int64), baked


def bake(dist, level, steps, pos, nrm, part=None):
    """-> (bytes uint8 [k], baked bool [k]): 255 where a vertex is not baked.  part = (n, (x0, y0, z0)): `dist` is the part of a
    grid of edge n that starts at this sample, a multiple of the level's stride per axis; a probe that reads a sample of the grid
    outside the part is an error"""
    dist = np.asarray(dist)
    s = 1 << level
    n, first = (dist.shape[0], (0, 0, 0)) if part is None else part
    assert all(v % s == 0 for v in first)
    lattice = dist[::s, ::s, ::s] < 0                      # lattice point c = grid sample c * s; its extent is every c with c * s < n
    lim = -(-n // s)
    c0, held = np.array(first, np.int64) // s, np.array(lattice.shape[::-1], np.int64)
    P, N, baked = quantise(pos, nrm, level)
    O = P + 2 * N
    tot, occ = np.zeros(len(P), np.int64), np.zeros(len(P), np.int64)
    for S in DIRS:
        w = np.maximum(0, (N @ S) >> 8)
        alive = (w > 0) & baked
        tot += np.where(baked, w, 0)
        for j in range(1, steps + 1):
            if not alive.any():
                break
            c = (O + j * S + 128) >> 8
            alive &= np.all((c >= 0) & (c < lim), axis=1)   # the first c outside the grid: unoccluded
            cl = c - c0
            assert np.all((cl >= 0) & (cl < held) | ~alive[:, None]), "a probe leaves the part of the grid that was given"
            cc = np.clip(cl, 0, held - 1)
            hit = alive & lattice[cc[:, 2], cc[:, 1], cc[:, 0]]
            occ += np.where(hit, w * (steps + 1 - j), 0)
            alive &= ~hit
    tot *= steps
    ao = np.where(tot > 0, 255 - (255 * occ) // np.maximum(tot, 1), 255)
    assert ao.min(initial=255) >= 0 and ao.max(initial=0) <= 255
    return np.where(baked, ao, 255).astype(np.uint8), baked


def check(whole_grid, have_surface, levels_run, level, prm, has_array, capacity, n_verts):
    """what vx_occlusion returns for its arguments alone: 0, or -1 (VX_ERR_INVALID)"""
    if not whole_grid or not have_surface or level >= levels_run or prm is None:
        return -1
    p = np.asarray(prm, OCCLUSION_PARAMS_DTYPE).reshape(-1)[0]
    if not 1 <= int(p["steps"]) <= OCCLUSION_MAX_STEPS or int(p["flags"]) & ~OCCLUSION_TRANSITIONS or p["reserved"].any():
        return -1
    if np.isnan(p["box_min"]).any() or np.isnan(p["box_max"]).any() or (p["box_min"] > p["box_max"]).any():
        return -1
    if not has_array or capacity < n_verts:
        return -1
    return 0


def entry_vertices(t, transitions):
    """pool indices of the vertices of table entry t that a call bakes"""
    parts = [np.arange(int(t["v_off"]), int(t["v_off"]) + int(t["v_count"]))]
    if transitions:
        parts += [np.arange(int(t["tv_off"][f]), int(t["tv_off"][f]) + int(t["tv_count"][f])) for f in range(6)]
    return np.concatenate(parts).astype(np.int64)


def visited(table, prm):
    p = np.asarray(prm, OCCLUSION_PARAMS_DTYPE).reshape(-1)[0]
    return np.array([bool(np.all(t["min_corner"] <= p["box_max"]) and np.all(t["max_corner"] >= p["box_min"])) for t in table], bool)


# ---- the host build of tv_occlusion.h -----------------------------------------------------------------------------------------

def vertices(pos, nrm):
    v = np.zeros(len(pos), VERTEX_DTYPE)
    v["pos"], v["nrm"] = np.asarray(pos, np.float32), np.asarray(nrm, np.float32)
    return v


def host_bake(path, dist, level, steps, verts, block=(0, 0, 0), reach=None, skip=0):
    """path 0: the plain loop, 1: the kernel's pipeline for the block at `block` (its coordinate at the level) -> (rc, bytes,
    counts record, samples read from the grid instead of the staged masks)"""
    d = np.ascontiguousarray(dist, np.int8)
    v = np.ascontiguousarray(verts, VERTEX_DTYPE)
    out = np.full(len(v), 0xA5, np.uint8)
    counts = np.zeros(1, OCCLUSION_COUNTS_DTYPE)
    b = np.asarray(block, np.uint32)
    outside = C.c_uint64()
    rc = load().oh_bake(path, d.shape[0], _ptr(d), level, steps, _ptr(v), len(v), _ptr(b), steps + 2 if reach is None else reach, skip, _ptr(out), _ptr(counts),
                        C.byref(outside))
    return rc, out, counts[0], int(outside.value)


def host_quantise(pos, nrm, level):
    p, m, out = np.asarray(pos, np.float32).copy(), np.asarray(nrm, np.float32).copy(), np.zeros(6, np.int32)
    ok = load().oh_quantise(_ptr(p), _ptr(m), level, _ptr(out))
    return bool(ok), out[:3].copy(), out[3:].copy()


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

LEVELS = (0, 1, 2)
STEPS = (1, 5, 12)

_grids = {}


def grids():
    """{name: dist int8 [n, n, n]} shared, read-only: a 32^3 sphere, a 48^3 terrain (level 2 covers only a prefix of each axis)
    and 64^3 cave noise, from tests/fields.py"""
    if not _grids:
        import fields
        z, y, x = np.meshgrid(*([np.arange(32, dtype=np.float32)] * 3), indexing="ij")
        _grids["sphere32"] = fields.quantize_full_range(np.sqrt((x - 15.3) ** 2 + (y - 16.1) ** 2 + (z - 14.7) ** 2) - np.float32(10.4), 12.0)
        _grids["terrain48"] = fields.quantize_full_range(fields.terrain_field(48, 11), 6.0)
        _grids["caves64"] = fields.quantize_full_range(fields.smooth_noise(64, 23, scale=8, amp=6.0, octaves=2), 12.0)
        for d in _grids.values():
            d.setflags(write=False)
    return _grids


def surface_vertices(dist, level, block, count, seed):
    """`count` seeded vertices near the surface inside the span of block `block` of the level (what a mesh's vertices are to
    the rule: positions on crossing edges, any normal) -> VERTEX_DTYPE; a block without a crossing gives random positions"""
    rng = np.random.RandomState(seed)
    n, s = dist.shape[0], 1 << level
    lo = np.array(block, np.int64) * 16 * s                                  # grid axes (x, y, z)
    hi = np.minimum(lo + 16 * s, n - 1)
    sub = dist[lo[2]:hi[2] + 1:s, lo[1]:hi[1] + 1:s, lo[0]:hi[0] + 1:s] < 0
    cz, cy, cx = np.nonzero(sub[:-1] != sub[1:]) if sub.shape[0] > 1 else (np.zeros(0, np.int64),) * 3
    if len(cz):
        pick = rng.randint(0, len(cz), count)
        g = np.stack([lo[0] + cx[pick] * s, lo[1] + cy[pick] * s, lo[2] + (cz[pick] + rng.uniform(0, 1, count)) * s], axis=1)
    else:
        g = lo[None, :] + rng.uniform(0, 1, (count, 3)) * (hi - lo)[None, :]
    g = g.astype(np.float32)
    m = rng.normal(size=(count, 3))
    m /= np.linalg.norm(m, axis=1)[:, None]
    return vertices(g[:, [0, 2, 1]], m[:, [0, 2, 1]])


def face_blocks(n, level):
    """block coordinates of the level at every face of the grid: the corners and the middle"""
    cnt = max(1, -(-n // (16 << level)))
    picks = sorted({0, cnt // 2, cnt - 1})
    return [(bx, by, bz) for bz in picks for by in picks for bx in picks]
