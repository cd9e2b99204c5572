"""The specification of the overlap queries (include/voxels_hip.h, "overlap queries") stated again in numpy, from the header's
text and not from voxels_amd/csrc/tv_overlap.h: brute force over every triangle of every table entry, no index and no pruning;
the case list the tests share; and test-only access to the host build of that header (tests/overlap/overlap_host.cpp).
Mesh space throughout (Y up)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import (LISTED_BLOCK_DTYPE, OVERLAP_BOX_DTYPE, OVERLAP_COUNTS_DTYPE, OVERLAP_MAX_QUERIES,  # noqa: E402,F401
                                OVERLAP_RANGE_DTYPE, OVERLAP_TRI_DTYPE, VERTEX_DTYPE, overlap_boxes)

SO = os.path.join(ROOT, "tests", "overlap", "libvoxels_overlap_host.so")
F, U = np.float32, np.uint32
INVALID, OVERFLOW = -1, -3

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32 = C.c_void_p, C.c_uint32
        lib.ov_layout.argtypes = [u32]
        lib.ov_layout.restype = u32
        lib.ov_overlap.argtypes = [u32, vp, u32, vp, vp, u32, vp, u32, u32, vp, vp, vp, vp, u32, vp]
        lib.ov_overlap.restype = C.c_int
        _lib = lib
    return _lib


def counts_dict(rec):
    return {k: int(rec[k]) for k in OVERLAP_COUNTS_DTYPE.names}


def host_overlap(level, cnt, table, verts, idx, boxes, capacity=None, corners=True, seed=0):
    """tv_overlap.h on the host, over an index built there (its buckets shuffled by `seed`):
    (rc, tris, corners, ranges, counts dict, straddling); capacity None = two calls, counts first"""
    lib = load()
    table, verts, idx = np.ascontiguousarray(table, LISTED_BLOCK_DTYPE), np.ascontiguousarray(verts, VERTEX_DTYPE), np.ascontiguousarray(idx, U)
    boxes = np.ascontiguousarray(boxes, OVERLAP_BOX_DTYPE).reshape(-1)
    counts, straddling = np.zeros(1, OVERLAP_COUNTS_DTYPE), np.zeros(1, np.uint64)
    args = (level, _ptr(table), len(table), _ptr(verts), _ptr(idx), cnt, _ptr(boxes), len(boxes))
    if capacity is None:
        lib.ov_overlap(*args, 0, None, None, None, _ptr(counts), seed, None)
        capacity = int(counts["triangles"][0])
    tris, ranges = np.zeros(capacity, OVERLAP_TRI_DTYPE), np.zeros(len(boxes), OVERLAP_RANGE_DTYPE)
    crn = np.zeros((capacity, 3, 4), F) if corners else None
    rc = lib.ov_overlap(*args, capacity, _ptr(tris), _ptr(crn), _ptr(ranges), _ptr(counts), seed, _ptr(straddling))
    c = counts_dict(counts[0])
    k = min(capacity, c["triangles"])
    return rc, tris[:k], None if crn is None else crn[:k], ranges, c, int(straddling[0])


# ---- the header's text ------------------------------------------------------------------------------------------------------

class LevelTriangles:
    """every regular triangle of a level's table, in (coord_id, tri) order: what a query is compared with"""

    def __init__(self, table, verts, idx):
        self.entries = len(table)
        order = np.argsort(np.asarray(table["coord_id"], np.int64), kind="stable") if len(table) else np.zeros(0, np.int64)
        pos, ent, tri = [], [], []
        for e in order:
            t = table[e]
            k = int(t["i_count"]) // 3
            ix = idx[int(t["i_off"]):int(t["i_off"]) + 3 * k].reshape(-1, 3).astype(np.int64) + int(t["v_off"])
            pos.append(verts["pos"][ix])
            ent.append(np.full(k, e, U))
            tri.append(np.arange(k, dtype=U))
        self.pos = np.concatenate(pos) if pos else np.zeros((0, 3, 3), F)      # [T, vertex, axis]
        self.entry = np.concatenate(ent) if ent else np.zeros(0, U)
        self.tri = np.concatenate(tri) if tri else np.zeros(0, U)
        self.block_id = np.asarray(table["id"], U)[self.entry] if len(table) else np.zeros(0, U)
        self.lo, self.hi = self.pos.min(axis=1), self.pos.max(axis=1)           # the triangles' bounding boxes
        assert self.pos.dtype == F

    def matches(self, lo, hi):
        """indices (ascending: coord_id, then tri) of the triangles that match the closed box [lo, hi]"""
        lo, hi = np.asarray(lo, F), np.asarray(hi, F)
        if not np.all(lo <= hi):  # a NaN, or an inverted axis: an empty query
            return np.zeros(0, np.int64)
        k = np.nonzero((self.lo[:, 0] <= hi[0]) & (self.hi[:, 0] >= lo[0]))[0]
        for a in (1, 2):
            k = k[(self.lo[k, a] <= hi[a]) & (self.hi[k, a] >= lo[a])]
        return k


def overlap(level_tris, boxes, capacity=None, corners=True):
    """vx_overlap_boxes as the header states it: (rc, tris, corners [k, 3, 4] or None, ranges, counts dict)"""
    boxes = np.ascontiguousarray(boxes, OVERLAP_BOX_DTYPE).reshape(-1)
    n = len(boxes)
    ranges = np.zeros(n, OVERLAP_RANGE_DTYPE)
    c = dict.fromkeys(OVERLAP_COUNTS_DTYPE.names, 0)
    if level_tris.entries == 0:  # an empty table: zero counts, zero ranges
        return 0, np.zeros(0, OVERLAP_TRI_DTYPE), np.zeros((0, 3, 4), F), ranges, c
    c["queries"] = n
    found = [level_tris.matches(b["lo"], b["hi"]) for b in boxes]
    sizes = np.array([len(k) for k in found], np.int64)
    c["triangles"] = int(sizes.sum())
    c["hit_queries"] = int(np.count_nonzero(sizes))
    c["max_per_query"] = int(sizes.max()) if n else 0
    c["pairs"] = int(sum(len(np.unique(level_tris.entry[k])) for k in found))
    if c["triangles"] > 0xFFFFFFFF:
        return OVERFLOW, np.zeros(0, OVERLAP_TRI_DTYPE), np.zeros((0, 3, 4), F), ranges, c
    ranges["first"], ranges["count"] = np.cumsum(sizes) - sizes, sizes
    k = np.concatenate(found) if n else np.zeros(0, np.int64)
    tris = np.zeros(len(k), OVERLAP_TRI_DTYPE)
    tris["query"] = np.repeat(np.arange(n, dtype=U), sizes)
    tris["entry"], tris["block_id"], tris["tri"] = level_tris.entry[k], level_tris.block_id[k], level_tris.tri[k]
    cap = c["triangles"] if capacity is None else capacity
    crn = None
    if corners:
        crn = np.zeros((min(len(k), cap), 3, 4), F)
        crn[:, :, :3] = level_tris.pos[k[:cap]]
    return (OVERFLOW if c["triangles"] > cap else 0), tris[:cap], crn, ranges, c


# ---- the case list ----------------------------------------------------------------------------------------------------------

def cases(level, n, level_tris, seed=2024, random_boxes=1000):
    """the shared case list for one level of a grid of edge n: (boxes OVERLAP_BOX_DTYPE, labels).  Sizes are relative to the
    level's block edge S and sub-brick edge S / 4.  Needs a level with triangles."""
    S = float(16 << level)
    sub = S / 4
    ext = float(n)
    inf, nan = float("inf"), float("nan")
    rng = np.random.RandomState(seed + level)
    verts = level_tris.pos.reshape(-1, 3)
    picks = verts[rng.randint(0, len(verts), 20)]
    lo, hi, labels = [], [], []

    def add(label, a, b):
        lo.append(np.asarray(a, np.float64).reshape(3))
        hi.append(np.asarray(b, np.float64).reshape(3))
        labels.append(label)

    add("whole level", [0, 0, 0], [ext] * 3)
    add("infinite", [-inf] * 3, [inf] * 3)
    v = picks[0].astype(np.float64)
    cell = np.floor(v / sub) * sub  # the sub-brick of a mesh vertex
    add("inside one sub-brick", cell + 0.25 * sub, cell + 0.75 * sub)
    blk = np.floor(v / S) * S
    for name, plane, step in (("block", blk, S), ("sub-brick", cell, sub)):
        for a in range(3):
            for k in (0, 1):  # the lower and the upper plane of that block / sub-brick on axis a
                at = plane[a] + k * step
                below_lo, below_hi, above_lo, above_hi = np.zeros(3), np.full(3, ext), np.zeros(3), np.full(3, ext)
                below_lo[a], below_hi[a] = at - 0.75 * sub, at     # ends exactly on the plane
                above_lo[a], above_hi[a] = at, at + 0.75 * sub     # starts exactly on it
                add("%s plane %g on axis %d from below" % (name, at, a), below_lo, below_hi)
                add("%s plane %g on axis %d from above" % (name, at, a), above_lo, above_hi)
                flat_lo, flat_hi = np.zeros(3), np.full(3, ext)
                flat_lo[a] = flat_hi[a] = at
                add("%s plane %g on axis %d itself" % (name, at, a), flat_lo, flat_hi)
    corner = np.where(blk > 0, blk, S)  # a block corner inside the level where there is one
    add("8 blocks at a block corner", corner - 1.0, corner + 1.0)
    add("8 blocks at a block corner, one sub-brick each", corner - sub, corner + sub)
    for i, pt in enumerate(picks):
        pt = pt.astype(np.float64)
        add("point on vertex %d" % i, pt, pt)
        a = i % 3
        line_lo, line_hi = pt.copy(), pt.copy()
        line_lo[a], line_hi[a] = -inf if i & 1 else 0.0, inf if i & 1 else ext
        add("line through vertex %d along axis %d" % (i, a), line_lo, line_hi)
        plane_lo, plane_hi = np.zeros(3), np.full(3, ext)
        plane_lo[a] = plane_hi[a] = pt[a]
        add("plane through vertex %d across axis %d" % (i, a), plane_lo, plane_hi)
    add("outside below", [-40, -40, -40], [-1, -1, -1])
    add("outside above", [ext + 1] * 3, [ext + 30] * 3)
    add("outside on one axis", [0, ext + 0.5, 0], [ext, ext + 9, ext])
    add("outside, huge", [1e30, 1e30, 1e30], [3e38, 3e38, 3e38])
    add("partly outside below", [-25.5, -3, -1e9], [0.4 * ext, 0.6 * ext, 0.5 * ext])
    add("partly outside above", [0.5 * ext, 0.3 * ext, 0.45 * ext], [ext + 12, 2 * ext, 1e20])
    add("partly outside, half infinite", [-inf, 0.25 * ext, -inf], [0.5 * ext, inf, 0.75 * ext])
    # small boxes between surface and air that no triangle meets: cell centres near mesh vertices, kept when nothing matches
    empty = 0
    for pt in verts[rng.randint(0, len(verts), 400)].astype(np.float64):
        c = np.floor(pt / (S / 16)) * (S / 16) + (S / 32) + np.array([0.0, 1.5 * S / 16, 0.0])
        if empty < 8 and len(level_tris.matches(F(c - 0.05), F(c + 0.05))) == 0:
            add("between surface and air %d" % empty, c - 0.05, c + 0.05)
            empty += 1
    for k in range(6):
        a, b = np.full(3, 0.25 * ext), np.full(3, 0.75 * ext)
        (a if k < 3 else b)[k % 3] = nan
        add("NaN in float %d" % k, a, b)
    for a in range(3):
        p, q = np.full(3, 0.25 * ext), np.full(3, 0.75 * ext)
        p[a], q[a] = q[a], p[a]
        add("inverted on axis %d" % a, p, q)
    centres = verts[rng.randint(0, len(verts), random_boxes)].astype(np.float64) + rng.uniform(-2.0, 2.0, (random_boxes, 3))
    edges = np.exp(rng.uniform(np.log(0.25), np.log(40.0), (random_boxes, 3)))
    for i in range(random_boxes):
        add("random %d" % i, centres[i] - 0.5 * edges[i], centres[i] + 0.5 * edges[i])
    with np.errstate(over="ignore"):
        return overlap_boxes(np.array(lo), np.array(hi)), labels
