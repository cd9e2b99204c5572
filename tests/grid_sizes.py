"""Grid edges that are not powers of two: what the reference makes of them, and the inputs the oracle, emulation and GPU tests
run at those sizes.

The reference builds floor(log2(n / 16)) + 1 levels; level L has cnt_L = (n / 16) >> L blocks per axis, so when n / 16 is not a
power of two a coarse level covers only [0, 16 * 2^L * cnt_L) of each axis and the band beyond it is meshed by finer levels
alone (n = 80: levels 1 and 2 cover 64; n = 208: levels 1, 2 and 3 cover 192, 192 and 128).  Child lookups, LOD chains,
transition faces toward a level that stops, the floored dirty boxes of incremental runs and slab bounds all meet these edges;
with power-of-two edges every one of those floors is exact."""
import numpy as np

import fields

ODD_SIZES = (16, 48, 80, 112, 208)


def ref_levels(n):
    nb, levels = n // 16, 0
    while nb >> levels:
        levels += 1
    return levels


def covered_extents(n):
    """The distinct ends (in voxels) of what the coarse levels (L >= 1) cover along each axis, below n."""
    out = set()
    for L in range(1, ref_levels(n)):
        e = 16 * (1 << L) * ((n // 16) >> L)
        if e < n:
            out.add(e)
    return sorted(out)


def plane_field(n, axis, h):
    """Axis-aligned plane at `h` along internal axis 0 (z), 1 (y) or 2 (x): distances clamped to +-4 like Grid::Create's."""
    c = np.arange(n, dtype=np.float64)
    shape = [1, 1, 1]
    shape[axis] = n
    c = np.broadcast_to(c.reshape(shape), (n, n, n))
    return np.ascontiguousarray(np.clip(np.sign(c - h) * np.ceil(np.abs(c - h)), -4, 4).astype(np.int8))


def plane_heights(n):
    """Planes at the last covered coarse block boundary of each partial level, and half a voxel to either side."""
    return [e + dh for e in covered_extents(n) for dh in (-0.5, 0.0, 0.5)]


def zero_heavy(n, seed):
    return np.clip(np.round(fields.smooth_noise(n, seed, scale=8, amp=2.0) * 1.5), -4, 4).astype(np.int8)


def edit_chain(n):
    """Ball and material brushes (kind, type or material, position, extent, radius or add) centred in the band the coarsest
    levels leave uncovered: the far faces, edges and corner of the grid, the boundaries of the covered prefixes, and one
    brush partly outside the grid.  Positions are (x, y, z) of the dense arrays' [z][y][x]; the terrains of
    fields.terrain_field put the ground near z = n / 2.  Types: 0 adds the ball, 1 keeps only it, 2 carves it."""
    c, f = n / 2.0, n - 6.0
    chain = [("ball", 2, (f, c - 1.5, c + 0.25), (16, 16, 16), 7.0),          # far x face, through the ground
             ("ball", 0, (c + 0.5, f, c - 2.0), (14, 14, 14), 6.0),           # far y face
             ("ball", 2, (c - 3.0, c + 1.0, f + 0.5), (16, 16, 16), 7.5),     # far z face
             ("ball", 1, (f, c - 4.0, f), (12, 12, 12), 5.5),                 # far x-z edge
             ("ball", 0, (n - 4.0, n - 4.0, n - 4.0), (10, 10, 10), 7.0),     # far corner
             ("mat", 3, (f, c, f), (14, 14, 14), 1),                          # material at the far edge
             ("ball", 2, (n + 3.0, c - 2.0, n - 10.0), (14, 14, 14), 9.0)]    # partly outside the grid
    for e in covered_extents(n):                                              # straddling each covered prefix's end
        chain += [("ball", 2, (e - 0.5, c, e + 0.25), (12, 12, 12), 6.0),
                  ("ball", 0, (e + 1.0, e if e > c + 8 else c + 9.0, c), (10, 10, 10), 5.0),
                  ("mat", 5, (e, c - 1.0, e - 2.0), (10, 10, 10), 0)]
    return chain


def apply_edit(g, edit):
    """One brush of edit_chain on an oracle grid or a Polygonizer (same signatures): the modified box."""
    kind, a, pos, ext, r = edit
    if kind == "ball":
        return g.inject_ball(pos, ext, r, a)
    return g.inject_material(pos, ext, a, bool(r))


def heightmap_for(n, seed):
    """A seeded height map whose surface lies inside an n-voxel column (Grid::Create(w, heightmap) puts distance
    (z - 127) - height at z)."""
    rng = np.random.RandomState(seed)
    base = fields.smooth_noise(n, seed, scale=max(4, n // 4), amp=0.2 * n, octaves=3)[0]
    return np.clip(np.round(base + rng.uniform(-1, 1, (n, n))) + (n // 2 - 127), -128, 127).astype(np.int8)


def large_heightmap(n, seed):
    """A seeded height map for grids too big to hold a float field: a bilinear 9 x 9 lattice plus a voxel of jitter, without
    any n^3 intermediate.  Heights are int8, so the surface lies in planes z = 127 + height, [0, 255)."""
    rng = np.random.RandomState(seed)
    lat = rng.uniform(-1, 1, (10, 10))
    c = np.arange(n) * (9.0 / n)
    i0 = c.astype(np.int64)
    t = c - i0
    rows = lat[i0] * (1 - t)[:, None] + lat[i0 + 1] * t[:, None]
    h = rows[:, i0] * (1 - t)[None, :] + rows[:, i0 + 1] * t[None, :]
    return np.clip(np.round(60.0 * h + rng.uniform(-1, 1, (n, n))), -128, 127).astype(np.int8)


def large_edits(n):
    """Ball brushes that put surface where a large grid's offsets are large: the far corner, and across the last coarse block
    boundary of each axis (the end of the shortest covered prefix, or the middle when every level covers the grid) high up in
    the other two.  Each contains a point of the coarsest levels' 128-voxel sample lattice, so the top levels see it."""
    e = (covered_extents(n) or [n // 2])[0]
    hi = 128 * ((n - 64) // 128)
    return [("ball", 0, (n - 4.0, n - 4.0, n - 4.0), (12, 12, 12), 7.0),
            ("ball", 0, (e + 0.5, hi, hi), (20, 20, 20), 9.0),
            ("ball", 0, (hi, e - 0.5, hi), (20, 20, 20), 9.0),
            ("ball", 0, (hi, hi, e + 0.25), (20, 20, 20), 9.0)]
