"""Test-only access to the host side of vx_grid_walk_field (tests/walk/walk_host.cpp) and the scenes the walk tests share.
`oracle` is the header's definition written out plainly with a Dijkstra over the reversed moves; `emulate` is the tile pipeline
of voxels_amd/csrc/tv_walk.h run sequentially, sweep loop included.  The two share no code."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import (WALK_COUNTS_DTYPE, WALK_GOAL_DTYPE, WALK_MAX_GOALS, WALK_QUERY_DTYPE, WALK_UNREACHED,  # noqa: E402,F401
                                walk_goals, walk_query)

SO = os.path.join(ROOT, "tests", "walk", "libvoxels_walk_host.so")
SOLID, EMPTY = np.int8(-4), np.int8(4)
DETERMINISTIC = [k for k in WALK_COUNTS_DTYPE.names if k != "sweeps"]
# horizontal offsets of the move codes 0..7
DX = (1, -1, 0, 0, 1, -1, 1, -1)
DY = (0, 0, 1, -1, 1, 1, -1, -1)

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32 = C.c_void_p, C.c_uint32
        for name in ("wh_oracle", "wh_emulate"):
            getattr(lib, name).argtypes = [u32, vp, vp, vp, u32, vp, vp, vp]
            getattr(lib, name).restype = C.c_int
        lib.wh_sizes.argtypes = [u32]
        lib.wh_sizes.restype = u32
        lib.wh_offset.argtypes = [u32, u32]
        lib.wh_offset.restype = u32
        _lib = lib
    return _lib


def extent(n, box):
    return [n] * 3 if box is None else [int(h) - int(l) for l, h in zip(box[0], box[1])]


def deterministic(counts):
    """the bytes of a counts record without `sweeps`, the one field scheduling may change"""
    return b"".join(np.asarray(counts[k]).tobytes() for k in DETERMINISTIC)


class Result:
    def same_as(self, other):
        """byte for byte: return code, field, direction bytes, the deterministic counts"""
        if self.rc != other.rc:
            return False, "rc"
        for name in ("field", "dirs"):
            if getattr(self, name).tobytes() != getattr(other, name).tobytes():
                return False, name
        if deterministic(self.counts) != deterministic(other.counts):
            return False, "counts"
        return True, ""


def run(kind, dist, box=None, goals=(), **kw):
    """kind = "oracle" | "emulate" -> Result with .rc, .field (uint32 [ez, ey, ex]), .dirs (uint8, same shape), .counts"""
    fn = getattr(load(), "wh_" + kind)
    n = dist.shape[0]
    q = walk_query(box, **kw)
    g = walk_goals(goals)
    ext = extent(n, box)
    ok = all(0 < e <= n for e in ext)
    shape = (ext[2], ext[1], ext[0]) if ok else (1, 1, 1)
    r = Result()
    r.field = np.full(shape, 0xDEADBEEF, np.uint32)
    r.dirs = np.full(shape, 0xDD, np.uint8)
    counts = np.zeros(1, WALK_COUNTS_DTYPE)
    r.rc = fn(n, _ptr(np.ascontiguousarray(dist)), _ptr(q), _ptr(g) if g.size else None, g.size, _ptr(r.field), _ptr(r.dirs), _ptr(counts))
    r.counts = counts[0].copy()
    return r


def air(n):
    return np.full((n, n, n), EMPTY, np.int8)


def floor(n, h):
    """solid below z = h: the standable cells are the layer z = h"""
    d = air(n)
    d[:h] = SOLID
    return d


def heights(n, h):
    """solid below z = h[y, x]"""
    z = np.arange(n).reshape(n, 1, 1)
    return np.where(z < np.asarray(h).reshape(1, n, n), SOLID, EMPTY).astype(np.int8)


def staircase(n, rise):
    """steps along x; rise 1: one per voxel, the step from x = 15 to 16 goes from z = 15 to 16; rise 4: one per four voxels, the
    step from x = 15 to 16 goes from z = 14 to 18"""
    x = np.arange(n)
    h = np.maximum(x, 1) if rise == 1 else 2 + 4 * (x // 4)
    return heights(n, np.broadcast_to(h, (n, n)))


def cliff(n=32):
    """a plateau of height 12 for x < 16, ground of height 9 beyond: a drop of three"""
    return heights(n, np.broadcast_to(np.where(np.arange(n) < 16, 12, 9), (n, n)))


def wall_corner(n=32):
    """a floor and a wall one voxel wide along x = 16 that ends at y = 15: its corner is the corner of four tiles"""
    d = floor(n, 8)
    d[8:, :16, 16] = SOLID
    return d


def bridge(n=32):
    """a floor, a bridge over it with its deck at z = 14, and stairs up to the bridge"""
    d = floor(n, 6)
    d[12:14, 14:18, 8:24] = SOLID
    for x in range(9):
        d[:6 + x, 14:18, x] = SOLID
    return d


def serpentine(n=48):
    """walls across the whole floor, open at alternating ends: one corridor two voxels wide, with doors one voxel wide"""
    d = floor(n, 4)
    for i, y in enumerate(range(2, n - 1, 3)):
        if i % 2 == 0:
            d[4:, y, :n - 1] = SOLID
        else:
            d[4:, y, 1:] = SOLID
    return d


def corridor(n=32):
    """a passage one voxel wide along x at y = 5 between walls up to the top"""
    d = floor(n, 8)
    d[8:] = SOLID
    d[8:, 5, :] = EMPTY
    return d


def narrow_staircase(n=32):
    """the staircase of rise 1, one voxel wide at y = 10 between walls up to the top: it crosses z = 15/16 at x = 15/16"""
    d = staircase(n, 1)
    d[:, :10, :] = SOLID
    d[:, 11:, :] = SOLID
    return d


def narrow_fours(n=32):
    """the staircase of rise 4, one voxel wide at y = 10: the step from x = 15 to 16 goes from z = 14 to 18"""
    d = staircase(n, 4)
    d[:, :10, :] = SOLID
    d[:, 11:, :] = SOLID
    return d


def empty_blocks(n=32):
    """all-air blocks lying on all-solid blocks (both BF_Empty): the standable cells are the bottom layer of "empty" blocks"""
    return floor(n, 16)


def terrain64():
    from golden_io import Golden
    return np.ascontiguousarray(Golden("terrain64_carve_modify").dist)


def standable_numpy(dist, clearance):
    """the definition on the whole grid in numpy: [z, y, x] bool"""
    n = dist.shape[0]
    solid = dist < 0
    s = np.zeros_like(solid)
    s[1:] = solid[:-1]
    for k in range(clearance):
        clear = np.ones_like(solid)
        clear[:n - k] = ~solid[k:] if k else ~solid
        s &= clear
    return s


def surface_band(dist, clearance=2):
    """(z0, z1): the layers that hold standable cells"""
    zs = np.nonzero(standable_numpy(dist, clearance).any(axis=(1, 2)))[0]
    return int(zs.min()), int(zs.max()) + 1


def many_goals(n=48, count=WALK_MAX_GOALS, seed=5):
    rng = np.random.RandomState(seed)
    g = np.zeros(count, WALK_GOAL_DTYPE)
    g["x"], g["y"] = rng.randint(0, n, count), rng.randint(0, n, count)
    g["z"] = rng.randint(3, 6, count)          # the floor is at 4: two thirds stand in the air or in the ground
    g["cost"] = rng.randint(0, 400, count)
    return g


def cases():
    """[(name, dist, keywords of run())] - the list the CPU and the GPU tests both run"""
    out = []
    flat = floor(32, 8)
    out.append(("flat floor 4-neighbour", flat, dict(goals=[(5, 7, 8)], cost_diagonal=0)))
    out.append(("flat floor 8-neighbour", flat, dict(goals=[(5, 7, 8)])))
    out.append(("flat floor unaligned box", floor(48, 10), dict(box=((3, 5, 2), (45, 41, 30)), goals=[(20, 20, 10)])))
    out.append(("floor below lo.z", flat, dict(box=((0, 0, 8), (32, 32, 12)), goals=[(5, 7, 8)])))
    roof = flat.copy()
    roof[12:14] = SOLID
    out.append(("clearance reaches above hi.z, free", roof, dict(box=((0, 0, 4), (32, 32, 10)), goals=[(5, 7, 8)], clearance=4)))
    out.append(("clearance reaches above hi.z, blocked", roof, dict(box=((0, 0, 4), (32, 32, 10)), goals=[(5, 7, 8)], clearance=5)))
    out.append(("clearance reaches above z = n", floor(32, 30), dict(goals=[(5, 7, 30)], clearance=8)))
    out.append(("one-voxel region", flat, dict(box=((5, 7, 8), (6, 8, 9)), goals=[(5, 7, 8, 9)])))
    out.append(("region one voxel thick in z", flat, dict(box=((0, 0, 8), (32, 32, 9)), goals=[(5, 7, 8)])))
    out.append(("region one voxel thick in x", flat, dict(box=((17, 0, 0), (18, 32, 32)), goals=[(17, 3, 8)])))
    # a goal on a tile border that is the only way into the tile next door: seeding has to start both tiles
    for y in (15, 16):
        out.append(("thin region, goal at y = %d" % y, flat, dict(box=((17, 0, 0), (18, 32, 32)), goals=[(17, y, 8)])))
    for x in (15, 16):
        out.append(("corridor, goal at x = %d" % x, corridor(), dict(goals=[(x, 5, 8)])))
        out.append(("narrow staircase, goal at x = z = %d" % x, narrow_staircase(), dict(goals=[(x, 10, x)], cost_climb=3)))
    out.append(("narrow staircase of fours, goal below the z border", narrow_fours(), dict(goals=[(14, 10, 14)], step_up=4, step_down=4)))
    out.append(("narrow staircase of fours, goal above the z border", narrow_fours(), dict(goals=[(16, 10, 18)], step_up=4, step_down=4)))
    out.append(("staircase across z = 15/16 and x = 15/16", staircase(32, 1), dict(goals=[(2, 10, 2)], cost_climb=3)))
    out.append(("staircase of fours, steps of 4", staircase(32, 4), dict(goals=[(2, 10, 2)], step_up=4, step_down=4, cost_climb=3)))
    out.append(("staircase of fours, steps of 1", staircase(32, 4), dict(goals=[(2, 10, 2)])))
    out.append(("cliff, goal below", cliff(), dict(goals=[(30, 16, 9)], step_down=3, step_up=1, cost_climb=2)))
    out.append(("cliff, goal on top", cliff(), dict(goals=[(2, 16, 12)], step_down=3, step_up=1, cost_climb=2)))
    out.append(("wall corner at a tile corner", wall_corner(), dict(goals=[(20, 10, 8)])))
    out.append(("wall corner at a tile corner, no diagonals", wall_corner(), dict(goals=[(20, 10, 8)], cost_diagonal=0)))
    out.append(("bridge over a floor", bridge(), dict(goals=[(16, 16, 6)])))
    out.append(("serpentine 48", serpentine(), dict(goals=[(0, 0, 4)])))
    out.append(("serpentine 48 unaligned box", serpentine(), dict(box=((0, 0, 3), (47, 47, 9)), goals=[(0, 0, 4)], cost_diagonal=0)))
    out.append(("max_cost on a cell's distance", flat, dict(goals=[(5, 7, 8)], cost_diagonal=0, max_cost=50)))
    out.append(("max_cost one below a cell's distance", flat, dict(goals=[(5, 7, 8)], cost_diagonal=0, max_cost=49)))
    out.append(("max_cost 0", flat, dict(goals=[(5, 7, 8)], max_cost=0)))
    mixed = [(5, 7, 8, 0), (20, 20, 8, 35), (5, 7, 8, 3), (20, 20, 8, 20), (5, 7, 9, 0), (1, 1, 8, 0), (10, 10, 8, 201), (40, 3, 8, 0)]
    out.append(("goals: costs, duplicates, ignored ones", flat, dict(box=((2, 2, 4), (30, 30, 12)), goals=mixed, max_cost=200)))
    out.append(("goals: none used", flat, dict(goals=[(5, 7, 9, 0), (5, 7, 8, 11)], max_cost=10)))
    out.append(("goals: none given", flat, dict()))
    out.append(("goals: 65536", floor(48, 4), dict(goals=many_goals(), max_cost=300)))
    out.append(("empty blocks: air on solid", empty_blocks(), dict(goals=[(16, 16, 16)])))
    t = terrain64()
    z0, z1 = surface_band(t)
    s = standable_numpy(t, 2)
    gz = int(np.nonzero(s[:, 32, 32])[0][0])
    out.append(("terrain 64 surface band", t, dict(box=((0, 0, z0), (64, 64, z1)), goals=[(32, 32, gz)], step_up=2, step_down=2, cost_climb=3)))
    out.append(("terrain 64 unaligned band, range limit", t, dict(box=((3, 5, z0), (61, 59, z1)), goals=[(32, 32, gz), (10, 50, 0)], max_cost=240)))
    return out
