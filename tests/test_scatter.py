"""vx_scatter without a GPU: the numpy statement of the header (tests/scatter_oracle.py) against hand answers and its own
properties, and the host build of voxels_amd/csrc/tv_scatter.h (tests/scatter/scatter_host.cpp) against it byte for byte, on the
golden fixtures."""
import functools

import numpy as np
import pytest

import scatter_oracle as so
from golden_io import Golden
from scatter_oracle import F, U, scatter_params

GOLDENS = ["sphere64", "terrain32_mat", "noise64_fullrange_mat"]
DENSITIES = [0.25, 1.0, 7.5, 64.0]


@functools.lru_cache(maxsize=None)
def golden(name):
    """(grid edge, per level (table, verts, idx)) - shared by the tests, never changed"""
    g = Golden(name)
    n = int(g.dist.shape[0])
    return n, [(so.golden_table(lvl, L, n), lvl.verts, lvl.idx) for L, lvl in enumerate(g.levels)]


def all_levels():
    return [(name, L) for name in GOLDENS for L in range(len(golden(name)[1]))]


@functools.lru_cache(maxsize=None)
def unfiltered(name, L, density=1.0, seed=1234):
    tab, verts, idx = golden(name)[1][L]
    return so.scatter(L, scatter_params(seed=seed, density=density), tab, verts, idx)


def same(a, b):
    return a[0] == b[0] and a[3] == b[3] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# 1 -------------------------------------------------------------------------------------------------------------------------
def test_hand_answer():
    verts = np.zeros(3, so.VERTEX_DTYPE)
    verts["pos"] = [[0, 0, 0], [4, 0, 0], [0, 0, 4]]
    verts["nrm"] = [0, -1, 0]  # (e1 x e2 of this winding points down; the normals are data of their own anyway)
    idx = np.arange(3, dtype=U)
    tab = np.zeros(1, so.LISTED_BLOCK_DTYPE)
    tab["v_count"], tab["i_count"], tab["max_corner"], tab["id"] = 3, 3, 16, 7
    ht = so.tri_hash(so.block_hash(5, 0, 0), np.arange(1, dtype=U))
    count, m, valid = so.candidate_counts(verts["pos"][None, :, :], 1.0, ht)
    assert valid[0] and m[0] == F(8.0) and count[0] == 8
    rc, pts, ranges, c = so.scatter(0, scatter_params(seed=5, density=1.0), tab, verts, idx)
    assert rc == 0 and c == dict(points=8, candidates=8, triangles=1, entries=1, visited_entries=1, reserved=0)
    assert ranges.tolist() == [(0, 8)] and len(pts) == 8
    assert np.all(pts["pos"][:, 1] == 0) and np.all(pts["pos"][:, 0] >= 0) and np.all(pts["pos"][:, 2] >= 0)
    assert np.all(pts["pos"][:, 0] + pts["pos"][:, 2] <= 4)
    assert np.all(pts["nrm"] == F([0, -1, 0])) and np.all((pts["rand"] >= 0) & (pts["rand"] < 1))
    assert np.all(pts["block_id"] == 7) and np.all(pts["tri"] == 0) and np.all(pts["entry"] == 0)
    # the hash by hand: mix(0) = 0, and U() of all ones is the largest value below 1
    assert so.mix(0)[0] == 0 and so.unit(np.array([0xFFFFFFFF], U))[0] == F(1.0) - F(2.0 ** -24)
    x = 1
    x ^= x >> 16; x = x * 0x7feb352d & 0xFFFFFFFF; x ^= x >> 15; x = x * 0x846ca68b & 0xFFFFFFFF; x ^= x >> 16
    assert so.mix(1)[0] == x


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L,density", [(name, L, d) for name, L in all_levels() for d in DENSITIES
                                            if d != 64.0 or name != "noise64_fullrange_mat"])  # (64 on the two smaller fixtures)
def test_unbiased_count(name, L, density):
    tab, verts, idx = golden(name)[1][L]
    rc, pts, ranges, c = unfiltered(name, L, density) if density == 1.0 else so.scatter(L, scatter_params(seed=1234, density=density), tab, verts, idx)
    area, var = 0.0, 0.0
    for entry in tab:
        P = so.triangles(entry, verts, idx)[0]
        _, m, valid = so.candidate_counts(P, density, np.zeros(len(P), U))
        frac = (m - np.floor(m)).astype(np.float64)[valid]
        var += float(np.sum(frac * (1.0 - frac)))
        P = P.astype(np.float64)
        area += float(np.sum(0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)))
    sigma = np.sqrt(var)
    print("%s L%d density %g: points %d, density*A %.1f, sigma %.2f, off by %.2f sigma" % (name, L, density, c["points"], density * area, sigma, (c["points"] - density * area) / sigma))
    assert c["points"] == c["candidates"] == len(pts)
    assert abs(c["points"] - density * area) <= 4.0 * sigma


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", all_levels())
def test_placement(name, L):
    tab, verts, idx = golden(name)[1][L]
    rc, pts, ranges, c = unfiltered(name, L)
    assert rc == 0 and len(pts) > 0
    size = float(16 << L)
    for e, entry in enumerate(tab):
        mine = pts[int(ranges[e]["first"]):int(ranges[e]["first"]) + int(ranges[e]["count"])]
        assert np.all(mine["entry"] == e) and np.all(mine["block_id"] == entry["id"])
        P = so.triangles(entry, verts, idx)[0].astype(np.float64)[mine["tri"]]
        v0, e1, e2, q = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0], mine["pos"].astype(np.float64) - P[:, 0]
        nrm = np.cross(e1, e2)
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        assert np.all(np.abs(np.sum(q * nrm, axis=1)) <= 1e-4 * size)
        d11, d12, d22 = np.sum(e1 * e1, axis=1), np.sum(e1 * e2, axis=1), np.sum(e2 * e2, axis=1)
        q1, q2 = np.sum(q * e1, axis=1), np.sum(q * e2, axis=1)
        det = d11 * d22 - d12 * d12
        b1, b2 = (d22 * q1 - d12 * q2) / det, (d11 * q2 - d12 * q1) / det
        assert min(b1.min(), b2.min(), (1.0 - b1 - b2).min()) >= -1e-5
    assert np.all(np.abs(np.linalg.norm(pts["nrm"].astype(np.float64), axis=1) - 1.0) <= 1e-6)


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_normals_point_from_solid_to_air():
    tab, verts, idx = golden("terrain32_mat")[1][0]
    assert 0.85 < float(np.mean(verts["nrm"][:, 1] > 0)) < 0.93  # a terrain is mostly floor
    floors = so.scatter(0, scatter_params(seed=1234, min_up=0.5), tab, verts, idx)[3]["points"]
    ceilings = so.scatter(0, scatter_params(seed=1234, max_up=-0.5), tab, verts, idx)[3]["points"]
    assert floors > 0 and ceilings < floors


# 5 -------------------------------------------------------------------------------------------------------------------------
def filter_cases(n):
    h = F(n / 2)
    return {
        "slope": dict(min_up=0.3, max_up=0.95),
        "box": dict(box_min=[3.5, 2.25, h - 9.5], box_max=[h + 6.25, n - 7.0, n + 100.0]),
        "texture {3}": dict(texture_slot=5, texture_values=[3]),
        "texture {9, 15}": dict(texture_slot=5, texture_values=[9, 15]),
        "all": dict(min_up=0.3, max_up=0.95, box_min=[3.5, 2.25, h - 9.5], box_max=[h + 6.25, n - 7.0, n + 100.0], texture_slot=5, texture_values=[3, 9]),
    }


def predicate(prm, pts):
    """the filters of a parameter record on a list of unfiltered points, written out once more"""
    p = prm[0]
    keep = (pts["nrm"][:, 1] >= p["min_up"]) & (pts["nrm"][:, 1] <= p["max_up"])
    for a in range(3):
        keep &= (pts["pos"][:, a] >= p["box_min"][a]) & (pts["pos"][:, a] <= p["box_max"][a])
    value = (pts["tex"].copy().view(np.uint8).reshape(-1, 8)[:, int(p["texture_slot"])]).astype(np.int64)
    return keep & (((p["texture_mask"][value >> 5] >> (value & 31).astype(U)) & U(1)) != 0)


@pytest.mark.parametrize("case", ["slope", "box", "texture {3}", "texture {9, 15}", "all"])
def test_filters_are_predicates(case):
    n, levels = golden("terrain32_mat")
    assert {3, 9, 15} <= set(np.unique(levels[0][1]["tex"][:, 5]).tolist())
    for L, (tab, verts, idx) in enumerate(levels):
        rc, pts, ranges, c = unfiltered("terrain32_mat", L)
        prm = scatter_params(seed=1234, density=1.0, **filter_cases(n)[case])
        rc2, got, granges, gc = so.scatter(L, prm, tab, verts, idx)
        want = pts[predicate(prm, pts)]
        assert 0 < len(want) < len(pts), (case, L)
        assert got.tobytes() == want.tobytes(), (case, L)
        assert gc["points"] == len(want) and gc["candidates"] <= c["candidates"] and gc["entries"] == len(tab)
        assert granges["count"].tolist() == np.bincount(want["entry"], minlength=len(tab)).tolist()
        assert granges["first"].tolist() == (np.cumsum(granges["count"]) - granges["count"]).tolist()
        assert gc["triangles"] <= c["triangles"] and gc["visited_entries"] <= c["visited_entries"]


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_seeds():
    tab, verts, idx = golden("sphere64")[1][1]
    a = so.scatter(1, scatter_params(seed=1, density=1.0), tab, verts, idx)
    b = so.scatter(1, scatter_params(seed=2, density=1.0), tab, verts, idx)
    again = so.scatter(1, scatter_params(seed=1, density=1.0), tab, verts, idx)
    assert same(a, again)
    assert a[1].tobytes() != b[1].tobytes()
    k = min(len(a[1]), len(b[1]))
    assert k > 1000 and np.mean(np.all(a[1]["pos"][:k] == b[1]["pos"][:k], axis=1)) < 0.01
    # the level is part of the key as well: the same table scattered as another level gives other points
    assert so.scatter(0, scatter_params(seed=1, density=1.0), tab, verts, idx)[1].tobytes() != a[1].tobytes()


# 7 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", all_levels())
def test_host_build_equals_the_oracle(name, L):
    n, levels = golden(name)
    tab, verts, idx = levels[L]
    for density in DENSITIES:
        want = unfiltered(name, L) if density == 1.0 else so.scatter(L, scatter_params(seed=1234, density=density), tab, verts, idx)
        assert same(so.host_scatter(L, scatter_params(seed=1234, density=density), tab, verts, idx), want), (name, L, density)
        for case, kw in filter_cases(n).items():
            prm = scatter_params(seed=77, density=density, **kw)
            assert same(so.host_scatter(L, prm, tab, verts, idx), so.scatter(L, prm, tab, verts, idx)), (name, L, density, case)


def test_host_build_capacity_and_counts():
    tab, verts, idx = golden("terrain32_mat")[1][0]
    prm = scatter_params(seed=9, density=2.0, min_up=0.2)
    full = so.scatter(0, prm, tab, verts, idx)
    for cap in (0, 1, full[3]["points"] - 1, full[3]["points"]):
        assert same(so.host_scatter(0, prm, tab, verts, idx, cap), so.scatter(0, prm, tab, verts, idx, cap)), cap
    assert so.host_scatter(0, prm, tab, verts, idx, full[3]["points"] - 1)[0] == so.OVERFLOW
    assert so.host_scatter(0, prm, tab, verts, idx, full[3]["points"])[0] == 0
