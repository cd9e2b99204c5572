"""Test-only access to the host side of vx_grid_islands (tests/island/island_host.cpp) and the scenes the island tests share.
`oracle` is a breadth-first flood fill over the dense region; `emulate` is the tile pipeline of voxels_amd/csrc/tv_island.h run
sequentially.  The two share no code."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import (ISLAND_COUNTS_DTYPE, ISLAND_DTYPE, ISLAND_QUERY_DTYPE, island_query)  # noqa: E402,F401

SO = os.path.join(ROOT, "tests", "island", "libvoxels_island_host.so")
AIR = 0xFFFFFFFF
SOLID, EMPTY = np.int8(-4), np.int8(4)

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32 = C.c_void_p, C.c_uint32
        for name in ("ih_oracle", "ih_emulate"):
            getattr(lib, name).argtypes = [u32, vp, vp, vp, vp, u32, vp, vp, vp, vp]
            getattr(lib, name).restype = C.c_int
        lib.ih_sizes.argtypes = [u32]
        lib.ih_sizes.restype = u32
        _lib = lib
    return _lib


class Result:
    def same_as(self, other):
        """byte for byte: return code, labels volume, records, counts, distances and flags afterwards, the dirty box"""
        for name in ("rc", "labels", "records", "counts", "dist", "flags", "out_min", "out_max"):
            a, b = getattr(self, name), getattr(other, name)
            if not (a == b if name == "rc" else a.tobytes() == b.tobytes()):
                return False, name
        return True, ""


def codec_flags(dist):
    """BF_Empty of every block as the port's grid class keeps it"""
    import vxo
    return vxo.load_port().grid_from_dense(np.ascontiguousarray(dist)).block_flags()


def run(kind, dist, flags=None, box=None, capacity=None, **kw):
    """kind = "oracle" | "emulate" on copies of dist (and flags, default: the codec's) -> Result.  capacity=None: room for
    everything listed."""
    fn = getattr(load(), "ih_" + kind)
    n = dist.shape[0]
    q = island_query(box, **kw)
    ext = [n] * 3 if box is None else [int(h) - int(l) for l, h in zip(box[0], box[1])]
    volume = max(1, ext[0] * ext[1] * ext[2]) if all(0 < e <= n for e in ext) else 1
    flags = codec_flags(dist) if flags is None else flags
    r = Result()

    def call(query, room):
        r.dist, r.flags = dist.copy(), np.ascontiguousarray(flags, np.uint8).copy()
        r.labels = np.zeros(volume, np.uint32)
        r.counts = np.zeros(1, ISLAND_COUNTS_DTYPE)
        r.out_min, r.out_max = np.zeros(3, np.float32), np.zeros(3, np.float32)
        recs = np.zeros(room, ISLAND_DTYPE)
        r.rc = fn(n, _ptr(r.dist), _ptr(r.flags), _ptr(query), _ptr(recs) if room else None, room, _ptr(r.counts), _ptr(r.labels), _ptr(r.out_min), _ptr(r.out_max))
        r.records = recs[:min(room, int(r.counts["listed"][0]))].copy()

    if capacity is None:
        probe = q.copy()
        probe["flags"] &= ~np.uint32(2)
        call(probe, 0)
        capacity = int(r.counts["listed"][0])
    call(q, int(capacity))
    r.counts = r.counts[0].copy()
    r.labels3 = r.labels.reshape(ext[2], ext[1], ext[0]) if volume > 1 or ext == [1, 1, 1] else None
    return r


def air(n):
    return np.full((n, n, n), EMPTY, np.int8)


def serpentine(n):
    """one voxel thick: full x-rows at even (y, z), joined at alternating ends; crosses every block face many times"""
    d = air(n)
    for z in range(0, n, 2):
        for y in range(0, n, 2):
            d[z, y, :] = SOLID
        for y in range(1, n - 1, 2):
            d[z, y, n - 1 if (y // 2) % 2 == 0 else 0] = SOLID
    for z in range(1, n - 1, 2):
        d[z, 0 if (z // 2) % 2 else n - 2, 0] = SOLID
    return d


def floating(n=48):
    """a ground slab, a floating 6^3 cube (216 voxels), a floating 2^3 cube (8 voxels) and a pillar that stands on the ground"""
    d = air(n)
    d[:10] = SOLID
    d[20:26, 20:26, 20:26] = SOLID
    d[36:38, 36:38, 10:12] = SOLID
    d[10:30, 40:42, 40:42] = SOLID
    return d


def caves(n, seed):
    """(dist, mat, blend) of a fields.terrain_field grid with caves: many components come from the data"""
    import fields
    import vxo
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    return vxo.load_port().grid_from_float(f, m, b).read_dense()


def cases():
    """[(name, dist, query keywords)] - the list the CPU and the GPU tests both run"""
    out = []
    out.append(("all air", air(16), {}))
    out.append(("all solid", np.full((32, 32, 32), SOLID, np.int8), {}))
    out.append(("exact zeros", np.zeros((16, 16, 16), np.int8), {}))
    for name, second in (("edge contact", (slice(4, 8), slice(8, 12), slice(8, 12))), ("corner contact", (slice(8, 12), slice(8, 12), slice(8, 12)))):
        d = air(32)
        d[4:8, 4:8, 4:8] = SOLID
        d[second] = SOLID
        out.append((name, d, {}))
    out.append(("serpentine", serpentine(48), {}))
    u = air(32)
    u[4:21, 16, 8] = SOLID; u[4:21, 16, 20] = SOLID; u[4, 16, 8:21] = SOLID
    out.append(("U whole", u, {}))
    out.append(("U cut", u, {"box": ((0, 0, 8), (32, 32, 32))}))
    z, y, x = np.indices((32, 32, 32))
    out.append(("checkerboard", np.where((x + y + z) % 2 == 0, SOLID, EMPTY).astype(np.int8), {}))
    bar = air(80)
    bar[40, 40, :] = SOLID
    out.append(("bar over five blocks", bar, {}))
    bar = air(80)
    bar[40, 3:77, 41] = SOLID; bar[7:70, 9, 17] = SOLID
    out.append(("bars along y and z", bar, {"remove": True}))
    cd = caves(48, 6)[0]
    out.append(("caves 48", cd, {}))
    out.append(("caves 48 unaligned", cd, {"box": ((3, 17, 5), (45, 40, 33))}))
    out.append(("caves 48 unaligned remove", cd, {"box": ((3, 17, 5), (45, 40, 33)), "remove": True, "anchor_faces": 0x10, "air_value": 1}))
    out.append(("caves 48 one voxel solid", cd, {"box": ((5, 5, 1), (6, 6, 2))}))
    out.append(("caves 48 one voxel air", cd, {"box": ((5, 5, 46), (6, 6, 47)), "remove": True}))
    out.append(("caves 80 remove", caves(80, 6)[0], {"remove": True, "anchor_faces": 0x1F}))
    f = floating()
    for anchor in (0x3F, 0x1F, 0x10, 0x20, 0):
        out.append(("floating anchor %#x" % anchor, f, {"anchor_faces": anchor, "detached_only": True}))
    for limit in (0, 7, 8, 215, 216):
        out.append(("floating remove up to %d" % limit, f, {"remove": True, "max_voxels": limit, "air_value": 1 if limit % 2 else 127}))
    out.append(("floating remove in a box", f, {"remove": True, "box": ((16, 16, 12), (32, 32, 32)), "detached_only": True}))
    out.append(("all solid remove, nothing anchors", np.full((32, 32, 32), SOLID, np.int8), {"remove": True, "anchor_faces": 0, "box": ((0, 0, 0), (32, 32, 24))}))
    return out
