"""The specification of the measurements (include/voxels_hip.h, "measurements") stated again in numpy, from the header's text and
not from voxels_amd/csrc/tv_measure.h: slices, np.bincount and np.argwhere; test-only access to the host build of that header
(tests/measure/measure_host.cpp); and the grids and box lists the CPU and the GPU tests share.  Dense fields are indexed [z, y, x]
(internal axes, Z up); a grid is an undo_oracle.Grid, a record an undo_oracle.Rec."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from undo_oracle import Grid  # noqa: E402
from voxels_amd.binding import BOX_DTYPE, MEASURE_DTYPE, MEASURE_MAX_BOXES, RECORD_DELTA_DTYPE, boxes  # noqa: E402,F401

SO = os.path.join(ROOT, "tests", "measure", "libvoxels_measure_host.so")

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.mh_check.argtypes = [u32, vp, u32, vp]
        lib.mh_measure.argtypes = [u32, u32, vp, vp, vp, u32, u64, u32, vp, vp]
        lib.mh_record.argtypes = [u32, u32, vp, vp, u32, u32, u32, vp, vp, vp, vp, vp, vp]
        lib.mh_merge.argtypes = [vp, u64]
        lib.mh_merge.restype = u64
        lib.mh_layout.argtypes = [u32, vp]
        lib.mh_layout.restype = u32
        lib.mh_limit.argtypes = [u32]
        lib.mh_limit.restype = u32
        for name in ("mh_check", "mh_measure", "mh_record"):
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


# ---- the header's text ------------------------------------------------------------------------------------------------------

def check(n, bx):
    """what vx_grid_measure returns for the box array alone: 0, or -1 (VX_ERR_INVALID)"""
    bx = boxes(bx)
    if bx.size > MEASURE_MAX_BOXES:
        return -1
    for b in bx:
        if not all(int(b["lo"][k]) < int(b["hi"][k]) <= n for k in range(3)):
            return -1
    return 0


def measure(g, bx):
    """-> (the MEASURE_DTYPE array, uint64[count, 256]): every box on its own"""
    bx = boxes(bx)
    res = np.zeros(bx.size, MEASURE_DTYPE)
    tallies = np.zeros((bx.size, 256), np.uint64)
    for r, t, b in zip(res, tallies, bx):
        (x0, y0, z0), (x1, y1, z1) = [int(v) for v in b["lo"]], [int(v) for v in b["hi"]]
        d, m = g.dist[z0:z1, y0:y1, x0:x1], g.mat[z0:z1, y0:y1, x0:x1]
        solid = d < 0                                       # zero is air
        r["voxels"] = d.size
        r["solid_voxels"] = int(solid.sum())
        t[:] = np.bincount(m[solid], minlength=256)
        r["materials"] = int((t != 0).sum())
        if solid.any():
            at = np.argwhere(solid)                         # (z, y, x) inside the box
            r["min"] = [x0 + at[:, 2].min(), y0 + at[:, 1].min(), z0 + at[:, 0].min()]
            r["max"] = [x0 + at[:, 2].max(), y0 + at[:, 1].max(), z0 + at[:, 0].max()]
    return res, tallies


def record_delta(g, rec):
    """-> (the RECORD_DELTA_DTYPE record, removed uint64[256], added uint64[256]): the held blocks of `rec` beside grid g"""
    delta = np.zeros(1, RECORD_DELTA_DTYPE)[0]
    removed, added = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    nb = g.n // 16
    moved = []
    blocks = 0
    for i, bid in enumerate(rec.ids):
        bid = int(bid)
        d, m, _ = g.block(bid)
        was, now = rec.dist[i] < 0, d < 0
        gone, new = was & ~now, now & ~was
        painted = was & now & (rec.mat[i] != m)
        removed += np.bincount(rec.mat[i][gone], minlength=256).astype(np.uint64)     # by the material the record holds
        added += np.bincount(m[new], minlength=256).astype(np.uint64)                 # by the material the grid holds now
        delta["removed_voxels"] += int(gone.sum())
        delta["added_voxels"] += int(new.sum())
        delta["repainted_voxels"] += int(painted.sum())
        blocks += int(gone.any() or new.any() or painted.any())
        if (gone | new).any():
            org = np.array([bid // (nb * nb) * 16, (bid // nb) % nb * 16, bid % nb * 16])
            moved.append(np.argwhere(gone | new) + org)
    delta["blocks"] = blocks
    if moved:
        at = np.concatenate(moved)                          # (z, y, x)
        delta["min"] = [at[:, 2].min(), at[:, 1].min(), at[:, 0].min()]
        delta["max"] = [at[:, 2].max(), at[:, 1].max(), at[:, 0].max()]
    return delta, removed, added


# ---- the host build of tv_measure.h -------------------------------------------------------------------------------------------

def host_measure(path, g, bx, chunk=0, skip=0, tallies=True):
    """path 0: the plain triple loop, 1: the kernels' pipeline -> (rc, results, tallies)"""
    bx = boxes(bx)
    res = np.zeros(bx.size, MEASURE_DTYPE)
    t = np.zeros((bx.size, 256), np.uint64) if tallies else None
    rc = load().mh_measure(path, g.n, _ptr(g.dist), _ptr(g.mat), _ptr(bx) if bx.size else None, bx.size, chunk, skip,
                           _ptr(res) if bx.size else None, _ptr(t) if tallies and bx.size else None)
    return rc, res, t


def host_record(path, g, rec, rec_n=None, has_record=1, null_delta=False):
    """-> (rc, delta, removed, added)"""
    delta = np.zeros(1, RECORD_DELTA_DTYPE)
    removed, added = np.zeros(256, np.uint64), np.zeros(256, np.uint64)
    ids = np.ascontiguousarray(rec.ids, np.uint32)
    rc = load().mh_record(path, g.n, _ptr(g.dist), _ptr(g.mat), has_record, g.n if rec_n is None else rec_n, rec.blocks, _ptr(ids) if rec.blocks else None,
                          _ptr(np.ascontiguousarray(rec.dist)), _ptr(np.ascontiguousarray(rec.mat)), None if null_delta else _ptr(delta), _ptr(removed), _ptr(added))
    return rc, delta[0], removed, added


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

def _flags(d):
    import island_oracle
    return island_oracle.codec_flags(d)


def terrain_grid(n):
    import stamp_oracle
    return stamp_oracle.terrain_grid(n)


def noise_grid(n, seed=5):
    """white noise in the distances and full-range materials: all 256 bins are hit"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-128, 128, (n, n, n), dtype=np.int8)
    return Grid(d, rng.integers(0, 256, (n, n, n), dtype=np.uint8), rng.integers(0, 256, (n, n, n), dtype=np.uint8), _flags(d))


def constant_grid(n, value, mat):
    d = np.full((n, n, n), value, np.int8)
    return Grid(d, np.full((n, n, n), mat, np.uint8), np.zeros((n, n, n), np.uint8), _flags(d))


def small_grid():
    """16^3, one block: noise with a zero plane (zero is air) and a few materials"""
    rng = np.random.default_rng(3)
    d = rng.integers(-128, 128, (16, 16, 16), dtype=np.int8)
    d[5] = 0
    return Grid(d, rng.integers(0, 5, (16, 16, 16), dtype=np.uint8), np.zeros((16, 16, 16), np.uint8), _flags(d))


def layered_grid(n, seed=8):
    """noise between a solid slab below and air above, materials in bands with noise between: blocks that are all solid, all air
    and mixed, rows of one material and rows of sixteen"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-128, 128, (n, n, n), dtype=np.int8)
    d[:n // 3] = -100
    d[2 * n // 3:] = 50
    m = rng.integers(0, 256, (n, n, n), dtype=np.uint8)
    m[:n // 4] = (np.arange(n // 4) // 7 + 1).astype(np.uint8)[:, None, None]
    return Grid(d, m, np.zeros((n, n, n), np.uint8), _flags(d))


_grids = {}


def grids():
    """[(name, Grid)]: shared, read-only"""
    if not _grids:
        _grids["16 one block"] = small_grid()
        _grids["48 terrain"] = terrain_grid(48)
        _grids["48 noise"] = noise_grid(48)
        _grids["48 all solid"] = constant_grid(48, -100, 7)
        _grids["48 all air"] = constant_grid(48, 0, 7)
    return list(_grids.items())


def random_boxes(n, count, seed, largest=None):
    """`count` boxes anywhere in a grid of edge n, clipped to it, of extents up to `largest` (default: n) per axis"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, n, (count, 3))
    hi = np.minimum(lo + 1 + rng.integers(0, largest or n, (count, 3)) // rng.integers(1, 5, (count, 1)), n)
    b = np.zeros(count, BOX_DTYPE)
    b["lo"], b["hi"] = lo, hi
    return b


def box_lists(n, randoms=300):
    """[(name, BOX_DTYPE array)] for a grid of edge n"""
    e = n - 1
    a = min(15, n - 3)                      # a row of three voxels: across a block border where the grid has one
    k = n // 2
    out = [("single voxels", boxes([((0, 0, 0), (1, 1, 1)), ((e, e, e), (n, n, n))])),
           ("a row across a block border", boxes([((a, 9, 9), (a + 3, 10, 10))])),
           ("a plane", boxes([((0, 0, k), (n, n, k + 1)), ((k, 0, 0), (k + 1, n, n)), ((0, k - 1, 0), (n, k, n))])),
           ("the whole grid", boxes([((0, 0, 0), (n, n, n))])),
           ("inside one block", boxes([((3, 4, 5), (9, 12, 14))])),
           ("lo not aligned, hi = n", boxes([((5, 7, n - 11), (n, n, n))])),
           ("identical and overlapping", boxes([((2, 3, 4), (n - 3, n - 2, n - 1)), ((2, 3, 4), (n - 3, n - 2, n - 1)), ((0, 0, 0), (k + 3, k + 2, k + 1)), ((k - 2, k - 3, k - 4), (n, n, n))])),
           ("%d random" % randoms, random_boxes(n, randoms, 11))]
    return out
