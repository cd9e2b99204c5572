"""The overlap queries without a GPU: the numpy statement of the header (tests/overlap_oracle.py) against hand answers, and the
host build of voxels_amd/csrc/tv_overlap.h over a host-built index (tests/overlap/overlap_host.cpp) against it byte for byte, on
the golden fixtures, with the buckets of the index shuffled by three seeds."""
import functools

import numpy as np
import pytest

import overlap_oracle as oo
import scatter_oracle as so
from golden_io import Golden
from overlap_oracle import U, overlap_boxes

GOLDENS = ["sphere64", "terrain32_mat"]
SEEDS = [0, 1, 77]


@functools.lru_cache(maxsize=None)
def golden(name):
    """(grid edge, per level (table, verts, idx, LevelTriangles)) - shared by the tests, never changed"""
    g = Golden(name)
    n = int(g.dist.shape[0])
    out = []
    for L, lvl in enumerate(g.levels):
        tab = so.golden_table(lvl, L, n)
        out.append((tab, lvl.verts, lvl.idx, oo.LevelTriangles(tab, lvl.verts, lvl.idx)))
    return n, out


def all_levels():
    return [(name, L) for name in GOLDENS for L in range(len(golden(name)[1]))]


@functools.lru_cache(maxsize=None)
def expected(name, L):
    """(boxes, labels, the oracle's answer) for the case list on one level"""
    n, levels = golden(name)
    boxes, labels = oo.cases(L, n, levels[L][3])
    return boxes, labels, oo.overlap(levels[L][3], boxes)


def same(got, want, label=""):
    """(rc, tris, corners, ranges, counts dict) twice: equal bytes"""
    assert got[4] == want[4], (label, got[4], want[4])
    assert got[0] == want[0], (label, got[0], want[0])
    assert got[3].tobytes() == want[3].tobytes(), label
    assert got[1].tobytes() == want[1].tobytes(), label
    if got[2] is not None:
        assert got[2].tobytes() == want[2].tobytes(), label


# 1 -------------------------------------------------------------------------------------------------------------------------
def hand_table():
    """two level-0 blocks side by side in x (coord_id 0 and 1 of a 32^3 grid, the second listed FIRST), six triangles"""
    verts = np.zeros(18, so.VERTEX_DTYPE)
    verts["pos"] = [
        # block at x in [0, 16] (coord_id 0): vertices 0..8
        [1, 1, 1], [2, 1, 1], [1, 2, 1],              # tri 0: x 1..2, y 1..2, z 1
        [10, 5, 5], [12, 5, 5], [10, 5, 7],           # tri 1: x 10..12, y 5, z 5..7
        [14, 8, 8], [16, 8, 8], [14, 9, 8],           # tri 2: touches the plane x = 16 from below
        # block at x in [16, 32] (coord_id 1): vertices 9..17
        [17, 8, 8], [18, 8, 8], [17, 9, 8],           # tri 0: x 17..18
        [20, 1, 1], [21, 1, 1], [20, 2, 1],           # tri 1
        [30, 15, 15], [31, 15, 15], [30, 16, 15],     # tri 2: touches the plane y = 16
    ]
    idx = np.tile(np.arange(9, dtype=U), 2)   # block-local indices
    tab = np.zeros(2, so.LISTED_BLOCK_DTYPE)
    tab["coord_id"], tab["id"] = [1, 0], [41, 40]
    tab["v_off"], tab["i_off"] = [9, 0], [9, 0]
    tab["v_count"], tab["i_count"] = 9, 9
    tab["min_corner"], tab["max_corner"] = [[16, 0, 0], [0, 0, 0]], [[32, 16, 16], [16, 16, 16]]
    return tab, verts, idx


def test_hand_answers():
    tab, verts, idx = hand_table()
    lt = oo.LevelTriangles(tab, verts, idx)
    nan, inf = float("nan"), float("inf")
    boxes = overlap_boxes(
        [[0, 0, 0], [13, 0, 0], [16, 0, 0], [16.5, 0, 0], [12, 5, 5], [-inf] * 3, [0, nan, 0], [5, 0, 0], [0, 0, 0], [12.5, 0, 0]],
        [[32, 32, 32], [16, 32, 32], [16.75, 32, 32], [17, 32, 32], [12, 5, 5], [inf] * 3, [32, 32, 32], [4, 32, 32], [32, 0.5, 32], [13.5, 32, 32]])
    rc, tris, corners, ranges, c = oo.overlap(lt, boxes)
    assert rc == 0
    # (query, entry, block_id, tri): entry 1 is the block with coord_id 0, so it comes first
    whole = [(1, 40, 0), (1, 40, 1), (1, 40, 2), (0, 41, 0), (0, 41, 1), (0, 41, 2)]
    want = ([(0,) + t for t in whole]
            + [(1, 1, 40, 2)]                    # a box ending exactly at 16.0 meets the triangle that touches x = 16
            + [(2, 1, 40, 2)]                    # ... and so does one starting there; x 17.. begins beyond 16.75
            + [(3, 0, 41, 0)]                    # 16.5..17 meets only the triangle starting at 17
            + [(4, 1, 40, 1)]                    # a point box on a vertex
            + [(5,) + t for t in whole])         # the infinite box; the NaN box (6), the inverted box (7) and (8), (9) are empty
    assert tris.tolist() == want
    assert ranges.tolist() == [(0, 6), (6, 1), (7, 1), (8, 1), (9, 1), (10, 6), (16, 0), (16, 0), (16, 0), (16, 0)]
    assert c == dict(triangles=16, pairs=8, queries=10, hit_queries=6, max_per_query=6, reserved=0)
    assert corners[6].tolist() == [[14, 8, 8, 0], [16, 8, 8, 0], [14, 9, 8, 0]] and corners[9].tolist() == [[10, 5, 5, 0], [12, 5, 5, 0], [10, 5, 7, 0]]
    # the capacity cuts the arrays, not the ranges or the counts
    rc, t7, c7, r7, k7 = oo.overlap(lt, boxes, 7)
    assert rc == oo.OVERFLOW and t7.tolist() == want[:7] and len(c7) == 7 and r7.tobytes() == ranges.tobytes() and k7 == c
    # the host pipeline on the same table (a 32^3 grid: two blocks per axis)
    for seed in SEEDS:
        same(oo.host_overlap(0, 2, tab, verts, idx, boxes, seed=seed)[:5], (0, tris, corners, ranges, c), seed)
    # an empty table: zero counts and zero ranges
    none = oo.LevelTriangles(tab[:0], verts, idx)
    rc, t0, c0, r0, k0 = oo.overlap(none, boxes)
    assert rc == 0 and len(t0) == 0 and not r0.view(U).any() and not any(k0.values())
    same(oo.host_overlap(0, 2, tab[:0], verts, idx, boxes)[:5], (rc, t0, c0, r0, k0))


# 2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", all_levels())
def test_the_case_list_covers_what_it_names(name, L):
    boxes, labels, (rc, tris, corners, ranges, c) = expected(name, L)
    count = dict(zip(labels, ranges["count"].tolist()))
    total = len(golden(name)[1][L][3].tri)
    assert rc == 0 and count["whole level"] == count["infinite"] == total > 0
    assert all(count["point on vertex %d" % i] >= 1 for i in range(20))
    assert all(count[k] == 0 for k in labels if k.startswith(("outside", "NaN", "inverted", "between surface and air")))
    assert sum(k.startswith("between surface and air") for k in labels) >= 1
    assert any(0 < count[k] < total for k in labels if "from below" in k) and any(0 < count[k] < total for k in labels if "from above" in k)
    assert c["queries"] == len(boxes) and c["max_per_query"] == total and c["triangles"] == int(ranges["count"].astype(np.int64).sum())
    assert 0 < c["hit_queries"] < len(boxes) and c["pairs"] >= c["hit_queries"]
    # ordered by query, then coord_id, then tri
    table = golden(name)[1][L][0]
    key = np.stack([tris["query"].astype(np.int64), table["coord_id"][tris["entry"]].astype(np.int64), tris["tri"].astype(np.int64)], axis=1)
    assert key.tolist() == sorted(key.tolist())
    assert np.array_equal(tris["block_id"], table["id"][tris["entry"]]) and np.all(corners[:, :, 3] == 0)


# 3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", all_levels())
def test_host_pipeline_equals_the_oracle(name, L):
    n, levels = golden(name)
    tab, verts, idx, lt = levels[L]
    boxes, labels, want = expected(name, L)
    cnt = (n // 16) >> L
    first = None
    for seed in SEEDS:
        got = oo.host_overlap(L, cnt, tab, verts, idx, boxes, seed=seed)
        assert got[5] == 0, "straddling triangles in the host-built index"
        same(got[:5], want, (name, L, seed))
        blob = b"".join(a.tobytes() for a in got[1:4])
        first = first or blob
        assert blob == first  # the order of a bucket's slice of the permutation changes nothing
    # every query alone gives its own range of the batch (a walk knows nothing of its neighbours)
    for q in (0, 2, len(boxes) - 1):
        alone = oo.host_overlap(L, cnt, tab, verts, idx, boxes[q:q + 1])
        lo, k = int(want[3][q]["first"]), int(want[3][q]["count"])
        assert alone[4]["triangles"] == k and not alone[1]["query"].any() and alone[2].tobytes() == want[2][lo:lo + k].tobytes()
        assert all(np.array_equal(alone[1][f], want[1][lo:lo + k][f]) for f in ("entry", "block_id", "tri"))


def test_host_pipeline_capacity():
    n, levels = golden("terrain32_mat")
    tab, verts, idx, lt = levels[0]
    boxes, labels, full = expected("terrain32_mat", 0)
    total = full[4]["triangles"]
    for cap in (0, 1, total - 1, total, total + 7):
        want = oo.overlap(lt, boxes, cap)
        assert want[0] == (oo.OVERFLOW if cap < total else 0)
        same(oo.host_overlap(0, n // 16, tab, verts, idx, boxes, cap)[:5], want, cap)
