"""The specification of the stamps (include/voxels_hip.h, "stamps") stated again in numpy, from the header's text and not from
voxels_amd/csrc/tv_stamp.h: a sequential paste by the index formulas of the orientation table, the flag rule through
island_oracle.codec_flags, the result boxes and the counts; test-only access to the host build of tv_stamp.h
(tests/stamp/stamp_host.cpp); and the case list the CPU and the GPU tests share.  Dense fields are indexed [z, y, x] (internal
axes, Z up); a grid is an undo_oracle.Grid; a stamp is an St of dist / mat / blend of shape [sz, sy, sx]."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from undo_oracle import Grid  # noqa: E402
from voxels_amd.binding import (BOX_DTYPE, PASTE_COUNTS_DTYPE, PASTE_DTYPE, PASTE_MAX_COUNT, PASTE_MAX_STAMPS, PASTE_PAINT, PASTE_REPLACE,  # noqa: E402,F401
                                PASTE_RESULT_DTYPE, PASTE_SUBTRACT, PASTE_UNION, STAMP_INFO_DTYPE, STAMP_MAX_EDGE, STAMP_MAX_VOXELS, pastes)

SO = os.path.join(ROOT, "tests", "stamp", "libvoxels_stamp_host.so")
MODES = (PASTE_REPLACE, PASTE_UNION, PASTE_SUBTRACT, PASTE_PAINT)

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        lib.sh_check.argtypes = [vp, u32, vp, u32]
        lib.sh_check_size.argtypes = [vp]
        lib.sh_check_box.argtypes = [u32, vp]
        lib.sh_paste.argtypes = [u32, u32, vp, vp, vp, vp, vp, vp, u32, vp, u32, u32, u64, vp, vp]
        lib.sh_paste_box.argtypes = [vp, vp, u32, vp]
        lib.sh_layout.argtypes = [u32, vp]
        lib.sh_layout.restype = u32
        lib.sh_limit.argtypes = [u32]
        lib.sh_limit.restype = u32
        for name in ("sh_check", "sh_check_size", "sh_check_box", "sh_paste", "sh_paste_box"):
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


class St:
    def __init__(self, dist, mat=None, blend=None):
        self.dist = np.ascontiguousarray(dist, np.int8).copy()
        self.mat = np.zeros(self.dist.shape, np.uint8) if mat is None else np.ascontiguousarray(mat, np.uint8).copy()
        self.blend = np.zeros(self.dist.shape, np.uint8) if blend is None else np.ascontiguousarray(blend, np.uint8).copy()
        assert self.dist.ndim == 3 and self.mat.shape == self.dist.shape == self.blend.shape

    @property
    def size(self):
        return tuple(int(v) for v in self.dist.shape[::-1])   # (sx, sy, sz)


def capture(g, box):
    """the stamp of box = (lo, hi) of grid g"""
    (x0, y0, z0), (x1, y1, z1) = box
    s = (slice(z0, z1), slice(y0, y1), slice(x0, x1))
    return St(g.dist[s], g.mat[s], g.blend[s])


# ---- the header's text ------------------------------------------------------------------------------------------------------

def oriented(orient, sx, sy, i, j):
    """the oriented coordinates (u, v) of stamp coordinates (i, j) (integers or arrays): the header's table"""
    ip = sx - 1 - i if orient & 4 else i
    q = orient & 3
    if q == 0:
        return ip, j
    if q == 1:
        return sy - 1 - j, ip
    if q == 2:
        return sx - 1 - ip, sy - 1 - j
    return j, sx - 1 - ip


def oriented_size(orient, size):
    return (size[1], size[0], size[2]) if orient & 1 else tuple(size)


def targets(paste, size, n):
    """per stamp voxel [k, j, i]: the grid coordinates (int64 arrays x, y, z) and whether they lie inside the grid"""
    sx, sy, sz = size
    k, j, i = np.indices((sz, sy, sx), dtype=np.int64)
    u, v = oriented(int(paste["orient"]), sx, sy, i, j)
    x, y, z = (int(paste["origin"][0]) + u, int(paste["origin"][1]) + v, int(paste["origin"][2]) + k)
    inside = (x >= 0) & (x < n) & (y >= 0) & (y < n) & (z >= 0) & (z < n)
    return x, y, z, inside


def paste_box(paste, size, n):
    """-> (1 or 0, the BOX_DTYPE record): the clipped box, from the corner arithmetic of the header's text in Python integers"""
    out = np.zeros(1, BOX_DTYPE)[0]
    os_ = oriented_size(int(paste["orient"]), size)
    lo = [max(int(paste["origin"][k]), 0) for k in range(3)]
    hi = [min(int(paste["origin"][k]) + int(os_[k]), n) for k in range(3)]
    if any(l >= h for l, h in zip(lo, hi)):
        return 0, out
    out["lo"], out["hi"] = lo, hi
    return 1, out


def blocks_of_box(box, n):
    """the ids of the blocks a BOX_DTYPE record intersects, ascending"""
    nb = n // 16
    held = np.zeros((nb, nb, nb), bool)
    lo, hi = [int(v) // 16 for v in box["lo"]], [(int(v) - 1) // 16 for v in box["hi"]]
    held[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return np.flatnonzero(held.reshape(-1))


def check(ps, sizes):
    """what vx_grid_paste returns for the arrays alone: 0, or -1 (VX_ERR_INVALID); sizes[i] = None: a null entry"""
    if ps.size > PASTE_MAX_COUNT or len(sizes) > PASTE_MAX_STAMPS:
        return -1
    for p in ps:
        if int(p["stamp"]) >= len(sizes) or sizes[int(p["stamp"])] is None or int(p["orient"]) > 7 or int(p["mode"]) > 3 or p["reserved"].any():
            return -1
    return 0


def paste(g, stamps, ps):
    """applies the PASTE_DTYPE array ps to g in place, one paste after the other -> (results, counts)"""
    import island_oracle
    ps = pastes(ps)
    n, nb = g.n, g.n // 16
    before = g.copy()
    results = np.zeros(ps.size, PASTE_RESULT_DTYPE)
    counts = np.zeros(1, PASTE_COUNTS_DTYPE)[0]
    touched, carved = np.zeros(nb ** 3, bool), np.zeros(nb ** 3, bool)
    for r, p in zip(results, ps):
        st = stamps[int(p["stamp"])]
        x, y, z, inside = targets(p, st.size, n)
        if not inside.any():
            continue
        x, y, z = x[inside], y[inside], z[inside]
        r["box"]["lo"], r["box"]["hi"] = (x.min(), y.min(), z.min()), (x.max() + 1, y.max() + 1, z.max() + 1)
        ids = blocks_of_box(r["box"], n)
        r["touched_blocks"] = ids.size
        touched[ids] = True
        sd, sm, sb = st.dist[inside], st.mat[inside], st.blend[inside]
        d, m, b = g.dist[z, y, x], g.mat[z, y, x], g.blend[z, y, x]
        mode = int(p["mode"])
        if mode != PASTE_PAINT:
            carved[ids] = True
        if mode == PASTE_REPLACE:
            d, m, b = sd, sm, sb
        elif mode == PASTE_UNION:
            take = sd < d
            d, m, b = np.where(take, sd, d), np.where(take, sm, m), np.where(take, sb, b)
        elif mode == PASTE_SUBTRACT:
            c = np.where(sd == -128, 127, -sd.astype(np.int16)).astype(np.int8)
            d = np.where(c > d, c, d)
        else:
            take = sd < 0
            m, b = np.where(take, sm, m), np.where(take, sb, b)
        g.dist[z, y, x], g.mat[z, y, x], g.blend[z, y, x] = d, m, b
    if carved.any():
        g.flags[carved] = np.asarray(island_oracle.codec_flags(g.dist), np.uint8).reshape(-1)[carved]
    diff = (g.dist != before.dist) | (g.mat != before.mat) | (g.blend != before.blend)
    if diff.any():
        z, y, x = np.nonzero(diff)
        lo, hi = (x.min(), y.min(), z.min()), (x.max(), y.max(), z.max())
        counts["out_min"] = [min(int(lo[k]), n) for k in (0, 2, 1)]          # output order: x, then the internal z, then the internal y
        counts["out_max"] = [min(int(hi[k]) + 1, n) for k in (0, 2, 1)]
    block_diff = diff.reshape(nb, 16, nb, 16, nb, 16).any(axis=(1, 3, 5)).reshape(-1)
    flag_diff = g.flags != before.flags
    counts["changed_voxels"], counts["changed_blocks"], counts["flag_changes"] = int(diff.sum()), int((block_diff | flag_diff).sum()), int(flag_diff.sum())
    counts["touched_blocks"] = int(touched.sum())
    return results, counts


def touched_blocks(stamps, ps, n):
    """the ascending ids of the blocks a batch touches, from the voxels the pastes reach"""
    nb = n // 16
    held = np.zeros(nb ** 3, bool)
    for p in pastes(ps):
        x, y, z, inside = targets(p, stamps[int(p["stamp"])].size, n)
        if inside.any():
            box = np.zeros(1, BOX_DTYPE)[0]
            box["lo"], box["hi"] = (x[inside].min(), y[inside].min(), z[inside].min()), (x[inside].max() + 1, y[inside].max() + 1, z[inside].max() + 1)
            held[blocks_of_box(box, n)] = True
    return np.flatnonzero(held)


# ---- the host build of tv_stamp.h ---------------------------------------------------------------------------------------------

def _sizes(stamps):
    s = np.zeros((max(len(stamps), 1), 3), np.uint32)
    for k, st in enumerate(stamps):
        if st is not None:
            s[k] = st.size
    return s


def host_paste(path, g, stamps, ps, list_cap=0, seed=0):
    """path 0: the plain loop, 1: the kernels' pipeline; applies in place -> (rc, results, counts)"""
    ps = pastes(ps)
    flat = [None if st is None else np.concatenate([st.dist.view(np.uint8).reshape(-1), st.mat.reshape(-1), st.blend.reshape(-1)]) for st in stamps]
    bases = (C.c_void_p * max(len(stamps), 1))(*[None if f is None else f.ctypes.data for f in flat])
    sizes = _sizes(stamps)
    results = np.zeros(ps.size, PASTE_RESULT_DTYPE)
    counts = np.zeros(1, PASTE_COUNTS_DTYPE)
    rc = load().sh_paste(path, g.n, _ptr(g.dist), _ptr(g.mat), _ptr(g.blend), _ptr(g.flags), C.cast(bases, C.c_void_p), _ptr(sizes), len(stamps),
                         _ptr(ps) if ps.size else None, ps.size, list_cap, seed, _ptr(results) if ps.size else None, _ptr(counts))
    return rc, results, counts[0]


def host_check(ps, sizes):
    ps = pastes(ps)
    s = np.zeros((max(len(sizes), 1), 3), np.uint32)
    for k, v in enumerate(sizes):
        if v is not None:
            s[k] = v
    return load().sh_check(_ptr(ps) if ps.size else None, ps.size, _ptr(s), len(sizes))


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

_grids = {}


def terrain_grid(n):
    """a fields.terrain_field grid with fields.materials_for materials and the codec's flags (a fresh copy)"""
    if n not in _grids:
        import island_oracle
        import smooth_oracle
        d, m, b = smooth_oracle.terrain(n)
        _grids[n] = Grid(d, m, b, island_oracle.codec_flags(d))
    return _grids[n].copy()


def noise_stamp(size, seed):
    """uniform random bytes in every field, -128 included"""
    rng = np.random.default_rng(seed)
    shape = tuple(size)[::-1]
    return St(rng.integers(-128, 128, shape, dtype=np.int8), rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8))


def solid_stamp(size, value, mat=7, blend=200):
    shape = tuple(size)[::-1]
    return St(np.full(shape, value, np.int8), np.full(shape, mat, np.uint8), np.full(shape, blend, np.uint8))


class Case:
    """name, grid edge, stamp entries (an St, None, or ("capture", lo, hi): taken from the grid before the batch), PASTE_DTYPE array"""

    def __init__(self, name, n, stamps, rows):
        self.name, self.n, self.entries, self.pastes = name, n, stamps, pastes(rows)

    def grid(self):
        return terrain_grid(self.n)

    def stamps(self, g):
        return [capture(g, (e[1], e[2])) if isinstance(e, tuple) else e for e in self.entries]


def cases():
    R, U, S, P = MODES
    out = []
    one = noise_stamp((1, 1, 1), 1)
    cube = noise_stamp((16, 16, 16), 2)
    bar = noise_stamp((17, 5, 3), 3)
    huge = noise_stamp((70, 60, 52), 4)
    low = St(np.full((4, 6, 9), -128, np.int8), np.full((4, 6, 9), 3, np.uint8), np.full((4, 6, 9), 9, np.uint8))
    out.append(Case("1x1x1", 48, [one], [((20, 21, 22), 0, 0, R), ((47, 0, 16), 0, 5, R)]))
    out.append(Case("16^3 aligned", 48, [cube], [((16, 32, 0), 0, 0, R)]))
    out.append(Case("16^3 at (1, 15, 17)", 48, [cube], [((1, 15, 17), 0, 3, R)]))
    for o in range(8):
        out.append(Case("17x5x3 orient %d" % o, 48, [bar], [((9, 12, 14), 0, o, R), ((30, 29, 31), 0, o, U)]))
    out.append(Case("larger than the grid", 48, [huge], [((-11, -6, -2), 0, 1, R)]))
    out.append(Case("negative origins", 64, [bar, cube], [((-5, 3, 60), 0, 2, R), ((10, -15, -15), 1, 6, U), ((-16, -16, -16), 1, 0, R), ((-15, -15, -15), 1, 7, S)]))
    out.append(Case("a miss", 48, [bar], [((48, 0, 0), 0, 0, R), ((0, -5, 0), 0, 0, R), ((2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31), 0, 3, R)]))
    out.append(Case("-128 under SUBTRACT", 48, [low], [((12, 13, 5), 0, 1, S)]))
    for mode, name in zip(MODES, ("REPLACE", "UNION", "SUBTRACT", "PAINT")):
        out.append(Case("mode " + name, 48, [noise_stamp((20, 21, 22), 5)], [((11, 9, 3), 0, 4, mode)]))
    out.append(Case("order matters", 48, [noise_stamp((12, 12, 12), 6), noise_stamp((12, 12, 12), 7)], [((10, 10, 10), 0, 0, R), ((14, 13, 12), 1, 1, R), ((12, 12, 11), 0, 2, U)]))
    out.append(Case("PAINT only", 48, [noise_stamp((30, 9, 20), 8)], [((5, 20, 2), 0, 0, P), ((20, 5, 8), 0, 3, P)]))
    rng = np.random.default_rng(9)
    small = [noise_stamp((5, 4, 3), 10), noise_stamp((2, 7, 6), 11)]
    out.append(Case("300 on one block", 48, small, [(tuple(int(v) for v in rng.integers(16, 26, 3)), int(rng.integers(2)), int(rng.integers(8)), int(rng.integers(4))) for _ in range(300)]))
    out.append(Case("the whole grid", 48, [noise_stamp((48, 24, 48), 12), solid_stamp((24, 48, 48), -100)], [((0, 0, 0), 0, 0, R), ((0, 24, 0), 0, 2, U), ((0, 0, 0), 1, 1, S)]))
    out.append(Case("captured, over its source", 64, [("capture", (10, 20, 5), (40, 41, 30))], [((18, 25, 9), 0, 0, R), ((2, 30, 9), 0, 5, U), ((30, 12, 20), 0, 3, P)]))
    return out


def random_batch(n, seed):
    """-> (stamps, PASTE_DTYPE array): a few small noise stamps and up to 40 pastes that mostly reach the grid"""
    rng = np.random.default_rng(seed)
    stamps = [noise_stamp(tuple(int(v) for v in rng.integers(1, 24, 3)), seed * 16 + k) for k in range(int(rng.integers(1, 4)))]
    rows = [(tuple(int(v) for v in rng.integers(-20, n + 4, 3)), int(rng.integers(len(stamps))), int(rng.integers(8)), int(rng.integers(4)))
            for _ in range(int(rng.integers(1, 41)))]
    return stamps, pastes(rows)
