"""vx_occlusion without a GPU (include/voxels_hip.h, "ambient occlusion"): the written-out answers of the rule, the literal
direction table against its rule, the quantisation against numpy float32, and the host build of voxels_amd/csrc/tv_occlusion.h
run two ways - a plain loop over the dense grid, and the kernel's pipeline of staged row masks followed by probes - byte for
byte against the numpy statement of the header's text (tests/occlusion_oracle.py)."""
import numpy as np
import pytest

import occlusion_oracle as oo


def one(dist, steps, g, n=(0, 0, 127), level=0):
    """the byte of one vertex at grid position g with the quantised normal n (grid axes): the oracle's, and the host build's"""
    pos = np.array([[g[0], g[2], g[1]]], np.float32)
    nrm = np.array([[n[0], n[2], n[1]]], np.float32) / np.float32(127.0)
    P, N, baked = oo.quantise(pos, nrm, level)
    assert baked[0] and N[0].tolist() == list(n)
    want = int(oo.bake(dist, level, steps, pos, nrm)[0][0])
    rc, got, _, _ = oo.host_bake(0, dist, level, steps, oo.vertices(pos, nrm))
    assert rc == 0 and int(got[0]) == want
    return want


def grid40(solid):
    z, y, x = np.meshgrid(*([np.arange(40)] * 3), indexing="ij")
    return np.where(solid(x, y, z), -100, 100).astype(np.int8)


# ---- the written-out answers ----------------------------------------------------------------------------------------------------

def quantised_normal(a):
    """the exact normal of z = a x + b, quantised: N of m = (-a, 0, 1) / |.|"""
    m = np.array([-a, 0.0, 1.0]) / np.sqrt(a * a + 1.0)
    return np.floor(m.astype(np.float32) * np.float32(127.0) + np.float32(0.5)).astype(np.int64)


@pytest.mark.parametrize("steps", [4, 8, 12])
def test_planes_and_slopes_are_fully_open(steps):
    cases = [(0.0, h) for h in (20.0, 20.01, 20.5, 20.99)] + [(1.0, 0.3), (0.5, 8.2), (2.0, -20.4), (0.25, 12.6)]
    for a, b in cases:
        dist = grid40(lambda x, y, z: z < a * x + b)
        N = quantised_normal(a)
        g = []
        for x in range(40):                                   # the edges along z that the surface crosses
            h = a * x + b
            if 0.0 <= h <= 39.0:
                g.append((x, 17.0, h))
        if a:
            for z in range(40):                               # ... and those along x
                x = (z - b) / a
                if 0.0 <= x <= 39.0:
                    g.append((x, 17.0, z))
        g = np.array(g, np.float32)
        assert len(g) >= 20
        pos = g[:, [0, 2, 1]]
        nrm = np.repeat((N[[0, 2, 1]].astype(np.float32) / np.float32(127.0))[None, :], len(g), axis=0)
        assert oo.quantise(pos, nrm, 0)[1][0].tolist() == N.tolist()
        ao, baked = oo.bake(dist, 0, steps, pos, nrm)
        assert baked.all() and (ao == 255).all(), (a, b, steps, g[ao != 255].tolist(), ao[ao != 255].tolist())
        rc, got, counts, _ = oo.host_bake(0, dist, 0, steps, oo.vertices(pos, nrm))
        assert rc == 0 and (got == 255).all() and int(counts["open"]) == int(counts["vertices"]) == len(g) and int(counts["darkest"]) == 255


WALL = {8: (102, 175, 197, 236, 255), 4: (102, 195, 232, 255, 255), 12: (102, 168, 182, 215, 250)}


@pytest.mark.parametrize("steps", sorted(WALL))
def test_a_wall_beside_the_floor(steps):
    dist = grid40(lambda x, y, z: (z < 20) | (x >= 25))
    got = tuple(one(dist, steps, (24.5 - t, 17.0, 19.5)) for t in (0, 1, 2, 4, 8))
    assert got == WALL[steps]


@pytest.mark.parametrize("steps,want", [(4, 138), (8, 74), (12, 53)])
def test_the_bottom_of_a_shaft(steps, want):
    dist = grid40(lambda x, y, z: ~((np.abs(x - 20) <= 1) & (np.abs(y - 20) <= 1) & (z >= 10)))
    assert one(dist, steps, (20.0, 20.0, 9.5)) == want


# ---- the direction table ----------------------------------------------------------------------------------------------------------

def test_the_literal_table_is_its_rule():
    lib = oo.load()
    assert lib.oh_limit(2) == 98 and lib.oh_limit(3) == 45
    rows, k = [], 0
    for dz in range(-2, 3):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                if max(abs(dx), abs(dy), abs(dz)) != 2:
                    continue
                out = np.zeros(3, np.int32)
                lib.oh_dir(k, out.ctypes.data)
                d = np.array([dx, dy, dz], np.float64)
                want = np.floor(256.0 * d / np.linalg.norm(d) + 0.5)
                assert out.tolist() == want.tolist() == oo.DIRS[k].tolist(), (k, dx, dy, dz)
                assert np.abs(256.0 * d / np.linalg.norm(d) - want).max() < 0.49   # (no entry sits on a rounding edge)
                rows.append(tuple(sorted(np.abs(out).tolist(), reverse=True)))
                k += 1
    assert k == 98
    assert sorted(set(rows)) == sorted([(256, 0, 0), (229, 114, 0), (181, 181, 0), (209, 105, 105), (171, 171, 85), (148, 148, 148)])


# ---- quantisation -------------------------------------------------------------------------------------------------------------------

def test_quantisation_is_numpy_float32():
    rng = np.random.RandomState(3)
    nan, inf, tiny = np.nan, np.inf, np.float32(1e-45)
    special = [0.0, -0.0, tiny, -tiny, 1.17549435e-38, 0.5 / 127, -0.5 / 127, 0.00393700786, 1.0, -1.0, 1.0000001, 3.0, -3.0, 1e30, -1e30, 3e38, nan, inf, -inf]
    pos = [rng.uniform(0, 2048, 3) for _ in range(300)] + [rng.uniform(-1, 1, 3) for _ in range(50)]
    pos += [(v, 5.0, 7.0) for v in (0.0, -0.0, tiny, 0.001953125, 0.998046875, 4096.0, -4096.0, 4096.0005, -4096.0005, 1e9, nan, inf, -inf)]
    pos += [(3.0, v, 7.0) for v in (4096.5, nan, -inf, 12.498047)] + [(3.0, 7.0, v) for v in (5000.0, inf, 100.00195)]
    for level in range(8):
        for i, p in enumerate(pos):
            m = [special[(i + a * 7 + level) % len(special)] if i % 2 else rng.uniform(-1, 1) for a in range(3)]
            p32, m32 = np.array([p], np.float32), np.array([m], np.float32)
            P, N, baked = oo.quantise(p32, m32, level)
            ok, hp, hn = oo.host_quantise(p32[0], m32[0], level)
            assert ok == bool(baked[0]), (level, p, m)
            assert np.abs(N).max() <= 127
            if ok:
                assert hp.tolist() == P[0].tolist() and hn.tolist() == N[0].tolist(), (level, p, m)
    # mesh axes to grid axes, and what is not baked
    ok, hp, hn = oo.host_quantise((1.0, 2.0, 3.0), (0.25, 0.5, -1.0), 1)
    assert ok and hp.tolist() == [128, 384, 256] and hn.tolist() == [32, -127, 64]
    for bad in ((nan, 1, 1), (1, inf, 1), (1, 1, -inf), (4096.001, 1, 1), (1, -4097, 1)):
        assert not oo.host_quantise(bad, (0, 1, 0), 0)[0]
    assert oo.host_quantise((4096.0, -4096.0, 0.0), (nan, inf, -inf), 0)[2].tolist() == [0, 0, 0]
    v = oo.vertices([(nan, 1, 1), (1, 1, 1)], [(0, 1, 0), (0, 1, 0)])
    dist = np.full((16, 16, 16), 100, np.int8)
    for path in (0, 1):
        rc, out, counts, _ = oo.host_bake(path, dist, 0, 4, v)
        assert rc == 0 and out.tolist() == [255, 255] and int(counts["vertices"]) == 1 and int(counts["sum"]) == 255   # written, counted nowhere
    assert oo.bake(dist, 0, 4, v["pos"], v["nrm"])[1].tolist() == [False, True]


# ---- the host build, two ways ---------------------------------------------------------------------------------------------------------

_cases = {}


def block_cases(name, level):
    """per grid and level: [(block, vertices)] at every face of the grid - shared, read-only"""
    if (name, level) not in _cases:
        dist = oo.grids()[name]
        _cases[name, level] = [(b, oo.surface_vertices(dist, level, b, 48, 100 + k)) for k, b in enumerate(oo.face_blocks(dist.shape[0], level))]
    return _cases[name, level]


@pytest.mark.parametrize("level", oo.LEVELS)
@pytest.mark.parametrize("name", ["sphere32", "terrain48", "caves64"])
def test_the_host_build_equals_the_oracle(name, level):
    dist = oo.grids()[name]
    blocks = block_cases(name, level)
    if name == "terrain48" and level == 2:
        assert len(blocks) == 1 and 16 << level > 48                # the level covers only a prefix of each axis
    allv = np.concatenate([v for _, v in blocks])
    darkened = fallbacks = 0
    for steps in oo.STEPS:
        want, baked = oo.bake(dist, level, steps, allv["pos"], allv["nrm"])
        assert baked.all()
        darkened += int((want < 255).sum())
        at = 0
        for b, v in blocks:
            w = want[at:at + len(v)]
            at += len(v)
            rc, plain, counts, _ = oo.host_bake(0, dist, level, steps, v)
            assert rc == 0 and plain.tobytes() == w.tobytes(), (name, level, steps, b)
            assert (int(counts["vertices"]), int(counts["sum"]), int(counts["darkest"]), int(counts["open"])) == (len(v), int(w.astype(np.int64).sum()), int(w.min()), int((w == 255).sum()))
            for skip in (0, 1):                                      # the sign summaries withheld and given
                rc, staged, c2, outside = oo.host_bake(1, dist, level, steps, v, b, skip=skip)
                assert rc == 0 and staged.tobytes() == w.tobytes() and c2.tobytes() == counts.tobytes(), (name, level, steps, b, skip)
                assert outside == 0                                  # the reach of steps + 2 holds every sample of a vertex inside its block's span
            for reach in (0, 2):                                     # the region shrunk: reads from the grid itself
                rc, shrunk, c3, outside = oo.host_bake(1, dist, level, steps, v, b, reach=reach, skip=1)
                assert rc == 0 and shrunk.tobytes() == w.tobytes() and c3.tobytes() == counts.tobytes(), (name, level, steps, b, reach)
                fallbacks += outside
    assert darkened > 0
    assert fallbacks > 0 or dist.shape[0] <= 17 << level                 # (a grid the shrunk region still holds has nothing to read)


def test_a_vertex_outside_its_block_reads_the_grid():
    """the pipeline of block (0, 0, 0) given the vertices of the far corner: nothing is staged for them, nothing changes"""
    dist = oo.grids()["caves64"]
    v = block_cases("caves64", 0)[-1][1]
    want = oo.bake(dist, 0, 12, v["pos"], v["nrm"])[0]
    rc, got, _, outside = oo.host_bake(1, dist, 0, 12, v, (0, 0, 0), skip=1)
    assert rc == 0 and got.tobytes() == want.tobytes() and outside > 0
