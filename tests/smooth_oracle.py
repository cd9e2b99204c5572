"""The specification of vx_grid_smooth (include/voxels_hip.h, "smoothing") stated again in numpy, from the header's text and not
from voxels_amd/csrc/tv_smooth.h; test-only access to the host build of that header (tests/smooth/smooth_host.cpp); and the case
list the CPU and the GPU tests share.  Dense fields are indexed [z, y, x] (internal axes, Z up)."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from voxels_amd.binding import SMOOTH_DTYPE, SMOOTH_RESULT_DTYPE, smooth_op  # noqa: E402,F401

SO = os.path.join(ROOT, "tests", "smooth", "libvoxels_smooth_host.so")
F = np.float32

_lib = None


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def load():
    global _lib
    if _lib is None:
        lib = C.CDLL(SO)  # built by __graft_entry__.build(); a missing library is an error
        vp, u32 = C.c_void_p, C.c_uint32
        for name in ("sh_plain", "sh_tiles"):
            getattr(lib, name).argtypes = [u32, vp, vp, u32, vp, vp, vp, vp]
            getattr(lib, name).restype = C.c_int
        lib.sh_weight.argtypes = [u32, vp, vp, vp, vp, vp]
        lib.sh_weight.restype = None
        lib.sh_value.argtypes = [C.c_int, C.c_int, C.c_float]
        lib.sh_value.restype = C.c_int8
        lib.sh_sizes.argtypes = [u32]
        lib.sh_sizes.restype = u32
        _lib = lib
    return _lib


class Result:
    def same_as(self, other):
        """byte for byte: distances afterwards, per-op results, the union box, the count"""
        for name in ("dist", "results", "union_min", "union_max", "changed"):
            a, b = getattr(self, name), getattr(other, name)
            if not (a == b if name == "changed" else a.tobytes() == b.tobytes()):
                return False, name
        return True, ""


def stack(ops):
    return np.concatenate([np.asarray(o, SMOOTH_DTYPE).reshape(-1) for o in ops]) if len(ops) else np.zeros(0, SMOOTH_DTYPE)


# ---- the header's text ------------------------------------------------------------------------------------------------------

def weight(lo, hi, center, radius, strength):
    """w of every voxel of the box, float32, one rounding per written operation -> array [z, y, x]"""
    shape = tuple(int(hi[k]) - int(lo[k]) for k in (2, 1, 0))
    strength = F(strength)
    if F(radius) == F(0):
        return np.full(shape, strength, F)
    px = (np.arange(lo[0], hi[0]).astype(F) - F(center[0]))[None, None, :]
    py = (np.arange(lo[1], hi[1]).astype(F) - F(center[1]))[None, :, None]
    pz = (np.arange(lo[2], hi[2]).astype(F) - F(center[2]))[:, None, None]
    xx, yy, zz = px * px, py * py, pz * pz
    r = np.sqrt((xx + yy) + zz)
    q = F(1.0) - r / F(radius)
    assert r.dtype == F and q.dtype == F
    return strength * np.where(q > 0, q, F(0)).astype(F)


def iteration(d, lo, hi, w):
    """one Jacobi iteration of one op: d (int8 [z, y, x]) -> the new values of the box"""
    n = d.shape[0]
    ix, iy, iz = (np.clip(np.arange(int(lo[k]) - 1, int(hi[k]) + 1), 0, n - 1) for k in range(3))
    padded = d[np.ix_(iz, iy, ix)].astype(np.int32)       # the box with one layer around it, edge-clamped at the grid's faces
    ez, ey, ex = padded.shape[0] - 2, padded.shape[1] - 2, padded.shape[2] - 2
    k = (1, 2, 1)
    S = np.zeros((ez, ey, ex), np.int32)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                S += k[dz] * k[dy] * k[dx] * padded[dz:dz + ez, dy:dy + ey, dx:dx + ex]
    old = padded[1:-1, 1:-1, 1:-1].astype(F)
    t = S.astype(F) * F(0.015625)
    diff = t - old
    prod = w * diff
    f = old + prod
    assert f.dtype == F
    return np.clip(np.rint(f), F(-128), F(127)).astype(np.int8)


def apply(dist, ops):
    """the ops in array order on a copy of dist -> Result"""
    ops = np.asarray(ops, SMOOTH_DTYPE).reshape(-1)
    d = np.ascontiguousarray(dist, np.int8).copy()
    n = d.shape[0]
    r = Result()
    r.results = np.zeros(ops.size, SMOOTH_RESULT_DTYPE)
    r.union_min, r.union_max, r.changed = np.zeros(3, F), np.zeros(3, F), 0
    any_changed = False
    for i, o in enumerate(ops):
        if int(o["iterations"]) == 0 or F(o["strength"]) == F(0):
            continue
        lo, hi = [int(v) for v in o["lo"]], [int(v) for v in o["hi"]]
        box = (slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0]))
        first = d[box].copy()
        w = weight(lo, hi, o["center"], o["radius"], o["strength"])
        for _ in range(int(o["iterations"])):
            d[box] = iteration(d, lo, hi, w)
        where = np.nonzero(d[box] != first)
        count = len(where[0])
        if not count:
            continue
        a = [lo[0] + int(where[2].min()), lo[1] + int(where[1].min()), lo[2] + int(where[0].min())]
        b = [lo[0] + int(where[2].max()), lo[1] + int(where[1].max()), lo[2] + int(where[0].max())]
        mn = np.array([min(a[k], n) for k in (0, 2, 1)], F)          # output order: x, then the internal z, then the internal y
        mx = np.array([min(b[k] + 1, n) for k in (0, 2, 1)], F)
        r.results[i]["out_min"], r.results[i]["out_max"], r.results[i]["changed_voxels"] = mn, mx, count
        r.union_min = np.minimum(r.union_min, mn) if any_changed else mn
        r.union_max = np.maximum(r.union_max, mx) if any_changed else mx
        any_changed = True
        r.changed += count
    r.dist = d
    r.rc = 0
    return r


# ---- the host build of tv_smooth.h --------------------------------------------------------------------------------------------

def run(kind, dist, ops):
    """kind = "plain" | "tiles" on a copy of dist -> Result (rc = what vx_grid_smooth would return)"""
    fn = getattr(load(), "sh_" + kind)
    ops = np.ascontiguousarray(np.asarray(ops, SMOOTH_DTYPE).reshape(-1))
    r = Result()
    r.dist = np.ascontiguousarray(dist, np.int8).copy()
    r.results = np.zeros(ops.size, SMOOTH_RESULT_DTYPE)
    r.union_min, r.union_max = np.zeros(3, F), np.zeros(3, F)
    changed = C.c_uint64()
    r.rc = fn(dist.shape[0], _ptr(r.dist), _ptr(ops) if ops.size else None, ops.size, _ptr(r.results) if ops.size else None,
              _ptr(r.union_min), _ptr(r.union_max), C.byref(changed))
    r.changed = int(changed.value)
    return r


# ---- fields and cases ---------------------------------------------------------------------------------------------------------

def noise(n, seed):
    """uniform random int8 over -128..127: any indexing or halo slip changes bytes"""
    return np.random.default_rng(seed).integers(-128, 128, (n, n, n), dtype=np.int8)


def sphere(n, radius=None):
    z, y, x = np.indices((n, n, n)).astype(np.float32)
    c = (n - 1) / 2.0
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2) - (n * 0.3 if radius is None else radius)
    return np.clip(np.rint(r * 8), -127, 127).astype(np.int8)


def blobs(n=48):
    """a ground slab and floating cubes with hard +-127 steps: large constant stretches, so most voxels do not change"""
    d = np.full((n, n, n), 127, np.int8)
    d[:10] = -127
    d[20:26, 20:26, 20:26] = -127
    d[36:38, 36:38, 10:12] = -127
    d[10:30, 40:42, 40:42] = -127
    return d


_terrain = {}


def terrain(n, seed=4):
    """(dist, mat, blend) of a fields.terrain_field grid as the port's grid class stores it"""
    if (n, seed) not in _terrain:
        import fields
        import vxo
        f = fields.terrain_field(n, seed)
        m, b = fields.materials_for(n, seed)
        _terrain[(n, seed)] = vxo.load_port().grid_from_float(f, m, b).read_dense()
    return _terrain[(n, seed)]


UNALIGNED = ((5, 17, 30), (43, 33, 47))   # n = 48: spans 3 x 2 x 2 blocks, touches no grid face
FLUSH = ((29, 20, 37), (48, 48, 48))      # n = 48: flush with the +x, +y and +z grid faces


def stroke(count=40, n=48):
    """overlapping ball ops along a line: each reads what the ones before it wrote"""
    ops = []
    for i in range(count):
        c = np.array([8.25 + 0.8 * i, 12.5 + 0.55 * i, 20.75 + 0.3 * i], np.float32)
        lo = np.clip(np.floor(c - 6).astype(np.int64), 0, n)
        hi = np.clip(np.ceil(c + 6).astype(np.int64) + 1, 0, n)
        ops.append(smooth_op((lo, hi), c, 6.0, 1.0 if i % 3 else 0.37, 1 + (i % 5 == 0)))
    return stack(ops)


def cases():
    """[(name, dist, ops)] - the list the CPU and the GPU tests both run"""
    whole = lambda n: ((0, 0, 0), (n, n, n))
    n16, n48 = noise(16, 1), noise(48, 2)
    out = []
    out.append(("16 whole noise", n16, smooth_op(whole(16))))
    out.append(("16 whole noise 3 x 0.37", n16, smooth_op(whole(16), strength=0.37, iterations=3)))
    out.append(("16 whole noise ball", n16, smooth_op(whole(16), (7.3, 8.6, 5.1), 9.5, 1.0, 3)))
    out.append(("48 unaligned noise 0.37", n48, smooth_op(UNALIGNED, strength=0.37)))
    out.append(("48 unaligned noise 3", n48, smooth_op(UNALIGNED, iterations=3)))
    out.append(("48 unaligned noise ball inside 3", n48, smooth_op(UNALIGNED, (24.25, 25.5, 38.75), 9.5, 1.0, 3)))
    out.append(("48 unaligned noise ball outside", n48, smooth_op(UNALIGNED, (2.5, 12.25, 28.0), 9.5, 0.37, 1)))
    out.append(("48 flush noise 3 x 0.37", n48, smooth_op(FLUSH, strength=0.37, iterations=3)))
    out.append(("48 flush noise ball", n48, smooth_op(FLUSH, (47.5, 40.25, 49.0), 9.5, 1.0, 1)))
    out.append(("48 one voxel", n48, smooth_op(((17, 31, 16), (18, 32, 17)))))
    out.append(("48 one voxel 3", n48, smooth_op(((17, 31, 16), (18, 32, 17)), iterations=3)))
    out.append(("80 whole noise", noise(80, 3), smooth_op(whole(80))))
    out.append(("80 whole terrain 3 x 0.37", terrain(80)[0], smooth_op(whole(80), strength=0.37, iterations=3)))
    out.append(("48 sphere unaligned ball 3", sphere(48), smooth_op(UNALIGNED, (24.25, 25.5, 38.75), 9.5, 1.0, 3)))
    out.append(("48 terrain unaligned ball outside 3", terrain(48)[0], smooth_op(UNALIGNED, (35.5, 15.5, 30.5), 9.5, 1.0, 3)))
    out.append(("48 terrain flush", terrain(48)[0], smooth_op(FLUSH)))
    out.append(("48 blobs whole", blobs(), smooth_op(whole(48))))
    out.append(("48 blobs whole 3 x 0.37", blobs(), smooth_op(whole(48), strength=0.37, iterations=3)))
    out.append(("48 terrain stroke of 40", terrain(48)[0], stroke()))
    out.append(("48 noise stroke of 40", n48, stroke()))
    out.append(("48 noise idle ops between", n48, stack([smooth_op(UNALIGNED, strength=0.0, iterations=2), smooth_op(FLUSH, iterations=2),
                                                           smooth_op(UNALIGNED, iterations=0), smooth_op(UNALIGNED, strength=0.37)])))
    return out
