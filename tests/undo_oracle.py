"""The specification of the undo records (include/voxels_hip.h, "undo records") stated again in numpy, from the header's text and
not from voxels_amd/csrc/tv_undo.h; test-only access to the host build of that header (tests/undo/undo_host.cpp); and the case
list the CPU tests run.  Dense fields are indexed [z, y, x] (internal axes, Z up); a grid is a Grid of dist / mat / blend and one
flag byte per block; a record is a Rec of ascending ids, [blocks, 16, 16, 16] fields and flags."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import BOX_DTYPE, BRUSH_DTYPE, RECORD_MAX_BLOCKS, RECORD_MAX_BOXES, SWAP_RESULT_DTYPE, boxes  # noqa: E402,F401

SO = os.path.join(ROOT, "tests", "undo", "libvoxels_undo_host.so")
F = np.float32

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32 = C.c_void_p, C.c_uint32
        lib.uh_check.argtypes = [u32, vp, u32]
        lib.uh_capture.argtypes = [u32, vp, vp, vp, vp, vp, u32, u32, vp, vp, vp, vp, vp]
        lib.uh_trim.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp]
        lib.uh_swap.argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp, vp, vp, vp]
        lib.uh_brush_box.argtypes = [vp, u32, vp]
        lib.uh_layout.argtypes = [u32, vp]
        lib.uh_layout.restype = u32
        lib.uh_limit.argtypes = [u32]
        lib.uh_limit.restype = u32
        for name in ("uh_check", "uh_capture", "uh_trim", "uh_swap", "uh_brush_box"):
            getattr(lib, name).restype = C.c_int
        _lib = lib
    return _lib


class Grid:
    def __init__(self, dist, mat, blend, flags):
        self.dist, self.mat, self.blend = (np.ascontiguousarray(a).copy() for a in (dist, mat, blend))
        self.flags = np.ascontiguousarray(flags, np.uint8).copy()
        self.n = self.dist.shape[0]
        assert self.flags.size == (self.n // 16) ** 3

    def copy(self):
        return Grid(self.dist, self.mat, self.blend, self.flags)

    def same_as(self, o):
        return all(np.array_equal(a, b) for a, b in ((self.dist, o.dist), (self.mat, o.mat), (self.blend, o.blend), (self.flags, o.flags)))

    def block(self, bid):
        """views of the three fields of block `bid`"""
        nb = self.n // 16
        bx, by, bz = bid % nb, (bid // nb) % nb, bid // (nb * nb)
        s = (slice(bz * 16, bz * 16 + 16), slice(by * 16, by * 16 + 16), slice(bx * 16, bx * 16 + 16))
        return self.dist[s], self.mat[s], self.blend[s]


class Rec:
    def __init__(self, ids, dist, mat, blend, flags):
        self.ids, self.dist, self.mat, self.blend, self.flags = ids, dist, mat, blend, flags

    @property
    def blocks(self):
        return int(self.ids.size)

    def copy(self):
        return Rec(*(a.copy() for a in (self.ids, self.dist, self.mat, self.blend, self.flags)))

    def same_as(self, o):
        return all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
                   for a, b in ((self.ids, o.ids), (self.dist, o.dist), (self.mat, o.mat), (self.blend, o.blend), (self.flags, o.flags)))


def empty_rec(blocks=0):
    return Rec(np.zeros(blocks, np.uint32), np.zeros((blocks, 16, 16, 16), np.int8), np.zeros((blocks, 16, 16, 16), np.uint8),
               np.zeros((blocks, 16, 16, 16), np.uint8), np.zeros(blocks, np.uint8))


# ---- the header's text ------------------------------------------------------------------------------------------------------

def check(n, bx):
    """what vx_grid_capture returns for the box array alone: 0, or -1 (VX_ERR_INVALID)"""
    bx = boxes(bx)
    if bx.size > RECORD_MAX_BOXES:
        return -1
    for b in bx:
        if not all(int(b["lo"][k]) < int(b["hi"][k]) <= n for k in range(3)):
            return -1
    return 0


def block_set(n, bx):
    """the ascending ids of the blocks that at least one box intersects"""
    nb = n // 16
    held = np.zeros((nb, nb, nb), bool)   # [bz, by, bx]
    for b in boxes(bx):
        lo, hi = [int(v) // 16 for v in b["lo"]], [(int(v) - 1) // 16 for v in b["hi"]]
        held[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = True
    return np.flatnonzero(held.reshape(-1)).astype(np.uint32)


def capture(g, bx):
    ids = block_set(g.n, bx)
    r = empty_rec(ids.size)
    r.ids = ids
    for i, bid in enumerate(ids):
        r.dist[i], r.mat[i], r.blend[i] = g.block(int(bid))
        r.flags[i] = g.flags[bid]
    return r


def differs(g, r, i):
    d, m, b = g.block(int(r.ids[i]))
    return not (np.array_equal(d, r.dist[i]) and np.array_equal(m, r.mat[i]) and np.array_equal(b, r.blend[i]) and g.flags[r.ids[i]] == r.flags[i])


def trim(g, r):
    """-> (the trimmed record, blocks dropped)"""
    keep = np.array([differs(g, r, i) for i in range(r.blocks)], bool)
    return Rec(r.ids[keep], r.dist[keep], r.mat[keep], r.blend[keep], r.flags[keep]), int((~keep).sum())


def swap(g, r):
    """exchanges in place -> the SWAP_RESULT_DTYPE record"""
    res = np.zeros(1, SWAP_RESULT_DTYPE)[0]
    n, nb = g.n, g.n // 16
    lo, hi, voxels, blocks, flag_changes = [n] * 3, [-1] * 3, 0, 0, 0
    for i in range(r.blocks):
        bid = int(r.ids[i])
        d, m, b = g.block(bid)
        diff = (d != r.dist[i]) | (m != r.mat[i]) | (b != r.blend[i])
        flag = g.flags[bid] != r.flags[i]
        if diff.any():
            org = (bid % nb * 16, (bid // nb) % nb * 16, bid // (nb * nb) * 16)
            z, y, x = np.nonzero(diff)
            for k, c in enumerate((x, y, z)):
                lo[k], hi[k] = min(lo[k], org[k] + int(c.min())), max(hi[k], org[k] + int(c.max()))
            voxels += int(diff.sum())
        blocks += int(diff.any() or flag)
        flag_changes += int(flag)
        for mine, theirs in ((d, r.dist[i]), (m, r.mat[i]), (b, r.blend[i])):
            keep = mine.copy()
            mine[...] = theirs
            theirs[...] = keep
        g.flags[bid], r.flags[i] = r.flags[i], g.flags[bid]
    if voxels:
        res["out_min"] = [min(lo[k], n) for k in (0, 2, 1)]          # output order: x, then the internal z, then the internal y
        res["out_max"] = [min(hi[k] + 1, n) for k in (0, 2, 1)]
    res["changed_voxels"], res["changed_blocks"], res["flag_changes"] = voxels, blocks, flag_changes
    return res


def touched_blocks_1d(n, pos, ext):
    """the blocks of one axis that the position -+ extents test of the edits finds, in float32: a bool per block"""
    b = np.arange(n // 16, dtype=np.uint32)
    bmin = (b * np.uint32(16)).astype(F)
    bmax = (bmin + F(8)) + F(8)
    return ~((F(pos) - F(ext) > bmax) | (bmin > F(pos) + F(ext)))


def brush_box(brush, n):
    """-> (1 or 0, the BOX_DTYPE record)"""
    out = np.zeros(1, BOX_DTYPE)[0]
    per_axis = [np.flatnonzero(touched_blocks_1d(n, brush["position"][k], brush["extents"][k])) for k in range(3)]
    if any(a.size == 0 for a in per_axis):
        return 0, out
    out["lo"] = [16 * int(a[0]) for a in per_axis]
    out["hi"] = [16 * (int(a[0]) + a.size) for a in per_axis]
    return 1, out


# ---- the host build of tv_undo.h ----------------------------------------------------------------------------------------------

def host_capture(g, bx, capacity=None):
    """-> (rc, Rec): rc = the block count, or -1"""
    bx = boxes(bx)
    cap = (g.n // 16) ** 3 if capacity is None else capacity
    r = empty_rec(cap)
    rc = load().uh_capture(g.n, _ptr(g.dist), _ptr(g.mat), _ptr(g.blend), _ptr(g.flags), _ptr(bx) if bx.size else None, bx.size, cap,
                           _ptr(r.ids), _ptr(r.dist), _ptr(r.mat), _ptr(r.blend), _ptr(r.flags))
    k = max(rc, 0)
    return rc, Rec(r.ids[:k].copy(), r.dist[:k].copy(), r.mat[:k].copy(), r.blend[:k].copy(), r.flags[:k].copy())


def host_trim(g, r):
    r = r.copy()
    kept = load().uh_trim(g.n, _ptr(g.dist), _ptr(g.mat), _ptr(g.blend), _ptr(g.flags), r.blocks, _ptr(r.ids), _ptr(r.dist), _ptr(r.mat), _ptr(r.blend), _ptr(r.flags))
    assert 0 <= kept <= r.blocks
    return Rec(r.ids[:kept].copy(), r.dist[:kept].copy(), r.mat[:kept].copy(), r.blend[:kept].copy(), r.flags[:kept].copy()), r.blocks - kept


def host_swap(g, r):
    """exchanges in place -> the SWAP_RESULT_DTYPE record"""
    res = np.zeros(1, SWAP_RESULT_DTYPE)
    rc = load().uh_swap(g.n, _ptr(g.dist), _ptr(g.mat), _ptr(g.blend), _ptr(g.flags), r.blocks, _ptr(r.ids), _ptr(r.dist), _ptr(r.mat), _ptr(r.blend), _ptr(r.flags), _ptr(res))
    assert rc == 0
    return res[0]


def host_brush_box(brush, n):
    out = np.zeros(1, BOX_DTYPE)
    b = np.ascontiguousarray(np.asarray(brush, BRUSH_DTYPE).reshape(1))
    return load().uh_brush_box(_ptr(b), n, _ptr(out)), out[0]


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

def noise_grid(n, seed):
    """uniform random bytes in every field and random flag bytes: any indexing slip changes bytes"""
    rng = np.random.default_rng(seed)
    return Grid(rng.integers(-128, 128, (n, n, n), dtype=np.int8), rng.integers(0, 256, (n, n, n), dtype=np.uint8),
                rng.integers(0, 256, (n, n, n), dtype=np.uint8), rng.integers(0, 2, (n // 16) ** 3, dtype=np.uint8))


def cases():
    """[(name, grid before, boxes, grid after the "edit")] - an edit here is any rewrite of bytes: the records do not care"""
    out = []
    whole = lambda n: [((0, 0, 0), (n, n, n))]

    def edited(g, fn):
        e = g.copy()
        fn(e)
        return e

    g32, g48, g80 = noise_grid(32, 1), noise_grid(48, 2), noise_grid(80, 3)

    def one_voxel(e):
        e.dist[17, 3, 40] ^= 1

    def three_fields(e):
        e.dist[10:20, 30:34, 0:5] = 7
        e.mat[47, 47, 47] ^= 0x80
        e.blend[16, 15, 31] ^= 1

    def flags_only(e):
        e.flags[[0, 5, 26]] ^= 1

    def everything(e):
        e.dist[...] = ~e.dist
        e.flags[...] ^= 1

    def a_corner(e):
        e.dist[0:8, 0:8, 12:20] = 5

    def rows_at_block_corners(e):   # first and last byte of first and last row of a block
        for z in (32, 47):
            for y in (16, 31):
                e.mat[z, y, 64] ^= 1
                e.blend[z, y, 79] ^= 1

    out.append(("32 two overlapping boxes", g32, [((1, 2, 3), (17, 5, 9)), ((10, 0, 0), (20, 16, 16))], edited(g32, a_corner)))
    out.append(("48 whole, one voxel", g48, whole(48), edited(g48, one_voxel)))
    out.append(("48 whole, three fields", g48, whole(48), edited(g48, three_fields)))
    out.append(("48 whole, flags only", g48, whole(48), edited(g48, flags_only)))
    out.append(("48 whole, everything", g48, whole(48), edited(g48, everything)))
    out.append(("48 whole, nothing", g48, whole(48), g48.copy()))
    out.append(("48 scattered boxes, three fields", g48, [((40, 40, 40), (48, 48, 48)), ((0, 30, 10), (6, 34, 20)), ((16, 15, 16), (32, 16, 17)), ((40, 40, 40), (41, 41, 41))], edited(g48, three_fields)))
    out.append(("80 nine groups, block corners", g80, whole(80), edited(g80, rows_at_block_corners)))
    out.append(("80 a row of blocks and a column", g80, [((0, 37, 37), (80, 38, 38)), ((70, 0, 5), (71, 80, 6))], edited(g80, everything)))
    out.append(("48 no boxes", g48, [], edited(g48, one_voxel)))
    return out
