"""Test-only access to the host oracle of vx_grid_inject_brushes (tests/brush/brush_host.cpp) and the brush lists the brush
tests share.  The oracle applies a BRUSH_DTYPE array one Grid::InjectSurface / InjectMaterial call at a time on the host
grid class; all it shares with the device path are the sample functions of voxels_amd/csrc/tv_brush.h."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import (BRUSH_BALL, BRUSH_BOX, BRUSH_CAPSULE, BRUSH_DTYPE, BRUSH_MATERIAL,  # noqa: E402,F401
                                BRUSH_RESULT_DTYPE, capsule_stroke)

SO = os.path.join(ROOT, "tests", "brush", "libvoxels_brush_host.so")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


_lib = None


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
        lib.bh_apply.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, sz, vp]
        lib.bh_apply.restype = C.c_int
        lib.bh_sample.argtypes = [u32, u32, vp, vp, vp, vp, vp]
        lib.bh_sample.restype = None
        _lib = lib
    return _lib


class Applied:
    pass


def apply(dist, mat, blend, brushes):
    """The brushes applied in array order to copies of the dense fields -> fields, codec flags, blocks touched by a distance
    brush, per-brush boxes and block counts, the packed file."""
    lib = load()
    n = dist.shape[0]
    nb = n // 16
    brushes = np.ascontiguousarray(brushes, BRUSH_DTYPE)
    r = Applied()
    r.dist, r.mat, r.blend = dist.copy(), mat.copy(), blend.copy()
    r.flags = np.zeros(nb ** 3, np.uint8)
    r.dist_touched = np.zeros(nb ** 3, np.uint8)
    r.boxes = np.zeros((brushes.size, 6), np.float32)
    r.touched = np.zeros(brushes.size, np.uint32)
    cap = 64 + 3 * n ** 3 + 40 * nb ** 3
    pack = np.zeros(cap, np.uint8)
    size = C.c_size_t()
    rc = lib.bh_apply(n, _ptr(r.dist), _ptr(r.mat), _ptr(r.blend), _ptr(brushes), brushes.size, _ptr(r.flags), _ptr(r.dist_touched),
                      _ptr(r.boxes), _ptr(r.touched), _ptr(pack), cap, C.byref(size))
    assert rc == 0 and size.value <= cap
    r.pack = pack[:size.value].copy()
    return r


def sample(shape, p, a, b, radius):
    p = np.ascontiguousarray(p, np.float32); a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    radius = np.ascontiguousarray(radius, np.float32)
    out = np.zeros(len(p), np.float32)
    load().bh_sample(int(shape), len(p), _ptr(p), _ptr(a), _ptr(b), _ptr(radius), _ptr(out))
    return out


def brush(shape, pos, ext, type=0, radius=0.0, a=(0, 0, 0), b=(0, 0, 0), material=0):
    r = np.zeros(1, BRUSH_DTYPE)
    r["position"] = pos; r["extents"] = ext; r["shape"] = shape; r["type"] = type
    r["radius"] = radius; r["a"] = a; r["b"] = b; r["material"] = material
    return r[0]


def ball(pos, ext, radius, type):
    return brush(BRUSH_BALL, pos, ext, type, radius)


def material(pos, ext, mat, add):
    return brush(BRUSH_MATERIAL, pos, ext, 1 if add else 0, material=mat)


def box(pos, ext, half, rounding, type):
    return brush(BRUSH_BOX, pos, ext, type, rounding, a=half)


def stack(items):
    return np.array(list(items), BRUSH_DTYPE)


def anywhere_balls(n, count, seed):
    """`count` ball brushes in the manner of check_brushes_anywhere (tests/test_emu.py): inside the grid, across its sides,
    outside it, of zero extent, on block boundaries, at fractional positions; all three injection types."""
    fn = float(n)
    fixed = [((16.0, 16.0, 16.0), (16.0, 16.0, 16.0), 5.0), ((0.0, 0.0, 0.0), (10.0, 10.0, 10.0), 6.0), ((fn, fn, fn), (8.0, 8.0, 8.0), 5.0),
             ((24.0, 24.0, 24.0), (0.0, 0.0, 0.0), 3.0), ((-30.0, 20.0, 20.0), (10.0, 10.0, 10.0), 4.0), ((20.0, 200.0, 20.0), (12.0, 12.0, 12.0), 4.0),
             ((31.999, 32.0, 32.001), (0.001, 16.0, 15.999), 7.0), ((fn - 0.5, 0.5, 23.0), (3.0, 3.0, 40.0), 9.0),
             ((32.0, 32.0, 32.0), (32.0, 32.0, 32.0), 13.0), ((fn / 2, fn / 2, fn / 2), (2 * fn, 2 * fn, 2 * fn), fn / 3)]
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        if k < len(fixed) and count > 2:
            pos, ext, r = fixed[k]
        else:
            pos = tuple(float(x) for x in rng.uniform(-10, n + 10, 3).round(3))
            ext = tuple(float(x) for x in rng.choice([0.5, 3.0, 8.0, 17.0, 40.0], 3))
            r = float(rng.uniform(1, 12))
        out.append(ball(pos, ext, r, (2, 0, 1)[k % 3]))
    return stack(out)


def scattered_balls(n, count, seed, r_lo=2.0, r_hi=7.0):
    """`count` crater-like balls anywhere in the grid (some reach across its sides), types mixed."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        r = float(rng.uniform(r_lo, r_hi))
        pos = tuple(float(x) for x in rng.uniform(-2, n + 2, 3).round(2))
        out.append(ball(pos, (2 * r + 4,) * 3, r, (2, 2, 0, 1)[k % 4]))
    return stack(out)


def sequential(grid, brushes):
    """The ball / material brushes through a tests/vxo.py grid, one call per brush -> boxes [count, 6]."""
    boxes = np.zeros((len(brushes), 6), np.float32)
    for i, b in enumerate(brushes):
        if b["shape"] == BRUSH_BALL:
            mn, mx = grid.inject_ball(b["position"], b["extents"], float(b["radius"]), int(b["type"]))
        else:
            assert b["shape"] == BRUSH_MATERIAL
            mn, mx = grid.inject_material(b["position"], b["extents"], int(b["material"]), bool(b["type"]))
        boxes[i, :3], boxes[i, 3:] = mn, mx
    return boxes


def union_box(boxes, touched):
    """What vx_grid_inject_brushes hands back as union_min / union_max."""
    hit = touched > 0
    if not hit.any():
        return np.zeros(3, np.float32), np.zeros(3, np.float32)
    return boxes[hit, :3].min(axis=0), boxes[hit, 3:].max(axis=0)
