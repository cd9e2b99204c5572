"""The specification of the height maps (include/voxels_hip.h, "height maps") stated again in numpy, from the header's text and
not from voxels_amd/csrc/tv_height.h: slices, shifts along the scan axis and a running count of surfaces, Python integers for the
fraction f; test-only access to the host build of that header (tests/height/height_host.cpp); and the grids and the query list
the CPU and the GPU tests share.  Dense fields are indexed [z, y, x] (internal axes, Z up); a grid is an undo_oracle.Grid."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import measure_oracle as mo  # noqa: E402
from voxels_amd.binding import (HEIGHT_COUNT_SURFACES, HEIGHT_COUNTS_DTYPE, HEIGHT_FROM_BOTTOM, HEIGHT_FROM_TOP, HEIGHT_MAX_LAYERS,  # noqa: E402,F401
                                HEIGHT_NONE, HEIGHT_QUERY_DTYPE, height_query)

SO = os.path.join(ROOT, "tests", "measure", "libvoxels_measure_host.so")   # (one host library for the measurements and the height maps)

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        lib.hh_check.argtypes = [u32, vp, u32, u32]
        lib.hh_heightmap.argtypes = [u32, u32, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        lib.hh_value.argtypes = [u32, i32, i32, u32, u32]
        lib.hh_value.restype = u32
        lib.hh_layout.argtypes = [u32, vp]
        lib.hh_layout.restype = u32
        lib.hh_limit.argtypes = [u32]
        lib.hh_limit.restype = u32
        for name in ("hh_check", "hh_heightmap"):
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


# ---- the header's text ------------------------------------------------------------------------------------------------------

# f = (256 * -d0) / (d1 - d0) in integer division, for -d0 = 1..128 and d1 = 0..127, in Python integers
_F = np.array([[(256 * a) // (b + a) if a else 0 for b in range(128)] for a in range(129)], np.uint32)


def fraction(d0, d1):
    assert -128 <= d0 <= -1 and 0 <= d1 <= 127
    return (256 * -d0) // (d1 - d0)


def check(n, q, heights=True, surfaces=False):
    """what vx_grid_heightmap returns for the query and the presence of the arrays alone: 0, or -1 (VX_ERR_INVALID)"""
    if q is None or not heights:
        return -1
    q = np.asarray(q, HEIGHT_QUERY_DTYPE).reshape(-1)[0]
    lo, hi = [int(v) for v in q["box"]["lo"]], [int(v) for v in q["box"]["hi"]]
    if not all(lo[k] < hi[k] <= n for k in range(3)):
        return -1
    if int(q["direction"]) > 1 or not 1 <= int(q["layers"]) <= HEIGHT_MAX_LAYERS:
        return -1
    if int(q["flags"]) & ~HEIGHT_COUNT_SURFACES or q["reserved"].any():
        return -1
    if surfaces and not int(q["flags"]) & HEIGHT_COUNT_SURFACES:
        return -1
    return 0


def heightmap(g, box, direction=HEIGHT_FROM_TOP, layers=1, count_surfaces=False):
    """-> (heights uint32 [layers, H, W], materials uint8 [layers, H, W], surfaces uint16 [H, W] (always: the caller drops it
    where the flag is not set), the HEIGHT_COUNTS_DTYPE record)"""
    (x0, y0, z0), (x1, y1, z1) = [int(v) for v in box[0]], [int(v) for v in box[1]]
    top = direction == HEIGHT_FROM_TOP
    d, m = g.dist[z0:z1, y0:y1, x0:x1], g.mat[z0:z1, y0:y1, x0:x1]
    if top:
        d, m = d[::-1], m[::-1]                            # axis 0 in scan order: k = 0 is the sample at the box's end
    solid = d < 0                                          # zero is air
    before = np.zeros_like(solid)                          # the sample in the scan direction's back: air at the box's end
    before[1:] = solid[:-1]
    surf = solid & ~before
    nth = np.cumsum(surf, axis=0)                          # a surface's place in its column's order, from 1
    total = nth[-1]
    depth, h, w = d.shape
    heights = np.full((layers, h, w), HEIGHT_NONE, np.uint32)
    mats = np.zeros((layers, h, w), np.uint8)
    k, y, x = np.nonzero(surf & (nth <= layers))
    layer = nth[k, y, x] - 1
    z = (z1 - 1 - k) if top else (z0 + k)
    clipped = k == 0                                       # its air neighbour is the box's end
    d0 = d[k, y, x].astype(np.int64)
    d1 = np.where(clipped, 0, d[np.maximum(k, 1) - 1, y, x]).astype(np.int64)
    assert (d0 < 0).all() and (d1 >= 0).all()
    f = _F[-d0, d1].astype(np.int64)
    value = np.where(clipped, z * 256, z * 256 + f if top else z * 256 - f)
    heights[layer, y, x] = value.astype(np.uint32)
    mats[layer, y, x] = m[k, y, x]
    counts = np.zeros(1, HEIGHT_COUNTS_DTYPE)[0]
    covered = total > 0
    counts["columns"] = w * h
    counts["covered"] = int(covered.sum())
    if covered.any():
        counts["min_height"] = heights[0][covered].min()
        counts["max_height"] = heights[0][covered].max()
    first = np.zeros((h, w), bool)
    first[y[layer == 0], x[layer == 0]] = clipped[layer == 0]
    counts["clipped"] = int(first.sum())
    if count_surfaces:
        counts["surfaces"] = int(total.sum())
        counts["max_surfaces"] = int(total.max())
    return heights, mats, total.astype(np.uint16), counts


_expected = {}


def expected(name, g, box, direction, layers, count_surfaces):
    """heightmap() of a shared grid through a cache: the walk is done once per (grid, box, direction) with all eight layers and
    cut down to what a query asks for -> (heights, materials, surfaces or None, counts)"""
    key = (name, tuple(map(tuple, box)), direction)
    if key not in _expected:
        _expected[key] = heightmap(g, box, direction, HEIGHT_MAX_LAYERS, True)
        for a in _expected[key][:3]:
            a.setflags(write=False)
    heights, mats, total, counts = _expected[key]
    counts = counts.copy()
    if not count_surfaces:
        counts["surfaces"] = 0
        counts["max_surfaces"] = 0
    return heights[:layers], mats[:layers], total if count_surfaces else None, counts


# ---- the host build of tv_height.h --------------------------------------------------------------------------------------------

def host_heightmap(path, g, box, direction=HEIGHT_FROM_TOP, layers=1, count_surfaces=False, skip=0, materials=True, query=None):
    """path 0: the plain loop over columns, 1: the kernel's tile pipeline -> (rc, heights, materials, surfaces, counts, steps walked)"""
    q = height_query(box, direction, layers, count_surfaces) if query is None else query
    w, h = (max(int(q["box"]["hi"][0][k]) - int(q["box"]["lo"][0][k]), 1) for k in (0, 1))   # (room for something where the query is a bad one)
    shape = (max(int(q["layers"][0]), 1), h, w)
    heights = np.full(shape, 0xA5A5A5A5, np.uint32)
    mats = np.full(shape, 0xA5, np.uint8) if materials else None
    surfaces = np.full(shape[1:], 0xA5A5, np.uint16) if count_surfaces else None
    counts = np.zeros(1, HEIGHT_COUNTS_DTYPE)
    walked = C.c_uint64()
    rc = load().hh_heightmap(path, g.n, _ptr(g.dist), _ptr(g.mat), _ptr(q), skip, _ptr(heights), _ptr(mats), _ptr(surfaces), _ptr(counts), C.byref(walked))
    return rc, heights, mats, surfaces, counts[0], int(walked.value)


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

_grids = []


def grids():
    """[(name, Grid)]: shared, read-only - one block, 48^3 terrain, 48^3 white noise (a dozen surfaces per column), all solid, all
    air, and the 80^3 terrain"""
    if not _grids:
        _grids.extend(mo.grids() + [("80 terrain", mo.terrain_grid(80))])
    return list(_grids)


def pairs_grid():
    """edge 128: plane z = 5 holds -(x + 1), plane z = 6 holds y, air elsewhere - every pair (d0, d1) once, from the top"""
    n = 128
    d = np.full((n, n, n), 127, np.int8)
    d[5] = -(np.arange(n, dtype=np.int16) + 1)[None, :].astype(np.int8)
    d[6] = np.arange(n, dtype=np.int8)[:, None]
    m = np.zeros((n, n, n), np.uint8)
    m[5] = (np.arange(n)[None, :] ^ np.arange(n)[:, None]).astype(np.uint8)
    return mo.Grid(d, m, np.zeros((n, n, n), np.uint8), mo._flags(d))


def boxes(n):
    """[(name, (lo, hi))] for a grid of edge n: the cases of the issue that fit it"""
    k = n // 2
    out = [("the whole grid", ((0, 0, 0), (n, n, n))),
           ("one column", ((7, 9, 0), (8, 10, n))),
           ("one voxel", ((7, 9, 5), (8, 10, 6))),
           ("a z range inside one block", ((0, 0, 3), (n, n, 12))),
           ("z1 = 16", ((0, 0, 0), (n, n, 16))),
           ("a z range of one sample", ((0, 0, k), (n, n, k + 1)))]
    if n > 16:
        out += [("unaligned edges across block borders", ((5, 7, 3), (n - 3, n - 6, n - 2))),
                ("z0 = 16", ((0, 0, 16), (n, n, n))),
                ("z1 = 32", ((0, 0, 5), (n, n, 32))),
                ("a partial tile in a corner", ((n - 19, n - 17, 14), (n - 2, n, 35)))]
    return out


LAYERS = (1, 2, 8)
DIRECTIONS = (HEIGHT_FROM_TOP, HEIGHT_FROM_BOTTOM)


def cases(n):
    """[(name, box, direction, layers, count_surfaces)]: every box with layers 1, 2 and 8, both directions, both walks"""
    return [(name, box, direction, layers, flag) for name, box in boxes(n) for direction in DIRECTIONS for layers in LAYERS for flag in (False, True)]
