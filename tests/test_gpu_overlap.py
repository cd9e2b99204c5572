"""vx_overlap_boxes / vx_overlap_boxes_device on the MI355X against the numpy oracle of tests/overlap_oracle.py, byte for byte, on
the block tables and the mesh pools copied from the same context."""
import ctypes as C

import numpy as np
import pytest

import overlap_oracle as oo
from overlap_oracle import overlap_boxes
from test_gpu_scatter import golden_poly, new_poly, snapshot, synth_poly

pytestmark = pytest.mark.gpu

INVALID, OVERFLOW = -1, -3
POISON = 0xCD


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.init()
    return torch


def level_triangles(snap, level):
    tabs, verts, idx = snap
    return oo.LevelTriangles(tabs[level], verts, idx)


def host_form(p, level, boxes, capacity=None, corners=True):
    """vx_overlap_boxes -> (rc, tris, corners, ranges, counts dict); capacity None = counts first, then the fill"""
    if capacity is None:
        rc, _, _, _, counts = p.overlap_boxes_raw(level, boxes, 0)
        assert rc in (0, OVERFLOW)
        capacity = int(counts["triangles"])
    rc, tris, crn, ranges, counts = p.overlap_boxes_raw(level, boxes, capacity, corners)
    c = oo.counts_dict(counts)
    k = min(capacity, c["triangles"])
    return rc, tris[:k], None if crn is None else crn[:k], ranges, c


def device_form(torch, p, level, boxes, capacity, corners=True, guard=64, null_arrays=False):
    """vx_overlap_boxes_device into poisoned torch tensors on a stream of its own -> (tris, corners, ranges, counts dict, guards
    intact); null_arrays: the count-only form (capacity 0, no result arrays)"""
    boxes = np.ascontiguousarray(boxes, oo.OVERLAP_BOX_DTYPE).reshape(-1)
    n = len(boxes)
    d_boxes = torch.from_numpy(boxes.view(np.uint8).copy()).cuda() if n else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_tris = torch.full(((capacity + guard) * 16,), POISON, dtype=torch.uint8, device="cuda")
    d_corners = torch.full(((capacity + guard) * 48,), POISON, dtype=torch.uint8, device="cuda") if corners else None
    d_ranges = torch.full(((n + guard) * 8,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((32 + guard,), POISON, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.overlap_boxes_device(level, d_boxes.data_ptr() if n else None, n, capacity, None if null_arrays else d_tris.data_ptr(),
                           None if null_arrays or d_corners is None else d_corners.data_ptr(), d_ranges.data_ptr(), d_counts.data_ptr())
    s.synchronize()
    p.set_stream(0)
    tris, rng, cnt = d_tris.cpu().numpy(), d_ranges.cpu().numpy(), d_counts.cpu().numpy()
    c = oo.counts_dict(cnt[:32].view(oo.OVERLAP_COUNTS_DTYPE)[0])
    filled = 0 if null_arrays else min(capacity, c["triangles"])
    intact = bool(np.all(tris[filled * 16:] == POISON) and np.all(rng[n * 8:] == POISON) and np.all(cnt[32:] == POISON))
    crn = None
    if corners:
        raw = d_corners.cpu().numpy()
        intact = intact and bool(np.all(raw[filled * 48:] == POISON))
        crn = raw[:filled * 48].view(np.float32).reshape(-1, 3, 4)
    return tris[:filled * 16].view(oo.OVERLAP_TRI_DTYPE), crn, rng[:n * 8].view(oo.OVERLAP_RANGE_DTYPE), c, intact


def same(got, want, label):
    """(rc, tris, corners, ranges, counts dict) twice: equal bytes"""
    assert got[4] == want[4], (label, got[4], want[4])
    assert got[0] == want[0], (label, got[0], want[0])
    assert got[3].tobytes() == want[3].tobytes(), (label, "ranges")
    assert got[1].tobytes() == want[1].tobytes(), (label, "tris")
    if got[2] is not None:
        assert got[2].tobytes() == want[2].tobytes(), (label, "corners")


def check(torch, p, lt, level, boxes, label, corners=True, device=True):
    want = oo.overlap(lt, boxes, corners=corners)
    same(host_form(p, level, boxes, corners=corners), want, (label, "host form"))
    if device:
        tris, crn, ranges, c, intact = device_form(torch, p, level, boxes, want[4]["triangles"], corners=corners)
        assert intact, (label, "bytes beyond what was filled")
        same((0, tris, crn, ranges, c), want, (label, "device form"))
    return want


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat", "noise64_fullrange_mat"])
def test_overlap_matches_the_oracle(torch, name):
    p = golden_poly(name)
    snap = snapshot(p)
    words = 0
    for L in range(p.info.levels):
        assert p.raycast_prepare(L)["straddling"] == 0
        lt = level_triangles(snap, L)
        boxes, labels = oo.cases(L, p.n, lt)
        rc, tris, corners, ranges, c = check(torch, p, lt, L, boxes, "%s L%d" % (name, L))
        assert c["max_per_query"] == len(lt.tri) > 0 and 0 < c["hit_queries"] < len(boxes)
        words = max(words, (int(snap[0][L]["i_count"].max()) // 3 + 31) // 32)
    assert name != "noise64_fullrange_mat" or words > 64  # a block whose bitmap takes the wave more than one pass
    p.close()


# 2 -------------------------------------------------------------------------------------------------------------------------
def test_heavy_single_block(torch):
    p = golden_poly("sphere64")
    snap = snapshot(p)
    assert len(snap[0][2]) == 1
    lt = level_triangles(snap, 2)
    copies = 4096
    lo, hi = np.zeros((copies + 1, 3)), np.full((copies + 1, 3), float(p.n))
    lo[copies] = hi[copies] = lt.pos[len(lt.pos) // 2, 1]  # one point box, on a vertex
    boxes = overlap_boxes(lo, hi)
    want = check(torch, p, lt, 2, boxes, "sphere64 L2 heavy", corners=False)
    c = want[4]
    assert c["max_per_query"] == len(lt.tri) > 1024 and c["pairs"] == copies + 1 and c["hit_queries"] == copies + 1
    assert c["triangles"] == copies * len(lt.tri) + int(want[3][copies]["count"]) and int(want[3][copies]["count"]) > 0
    p.close()


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_capacity(torch):
    p = golden_poly("terrain32_mat")
    snap = snapshot(p)
    lt = level_triangles(snap, 0)
    boxes, labels = oo.cases(0, p.n, lt, random_boxes=100)
    full = oo.overlap(lt, boxes)
    total = full[4]["triangles"]
    assert total > 1000
    # the count-only form: capacity 0 and null arrays
    rc, _, _, ranges, counts = p.overlap_boxes_raw(0, boxes, 0)
    assert rc == OVERFLOW and oo.counts_dict(counts) == full[4] and ranges.tobytes() == full[3].tobytes()
    tris, crn, ranges, c, intact = device_form(torch, p, 0, boxes, 0, null_arrays=True)
    assert intact and c == full[4] and ranges.tobytes() == full[3].tobytes()
    for cap in (total - 1, total + 7, 1):
        want = oo.overlap(lt, boxes, cap)
        assert want[0] == (OVERFLOW if cap < total else 0) and len(want[1]) == min(cap, total)
        same(host_form(p, 0, boxes, cap), want, ("host form", cap))
        tris, crn, ranges, c, intact = device_form(torch, p, 0, boxes, cap)
        assert intact, cap
        same((want[0], tris, crn, ranges, c), want, ("device form", cap))
    p.close()


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_corners_are_the_pool_bytes(torch):
    p = golden_poly("terrain32_mat")
    tabs, verts, idx = snapshot(p)
    for L in range(p.info.levels):
        boxes = overlap_boxes([[3.5, 0, 2.25], [0, 0, 0]], [[20.75, 32, 17.5], [32, 32, 32]])
        tris, crn, ranges, c = p.overlap_boxes(L, boxes, corners=True)
        assert len(tris) == c["triangles"] > 0 and crn.shape == (len(tris), 3, 4)
        t = tabs[L][tris["entry"]]
        at = t["i_off"].astype(np.int64)[:, None] + 3 * tris["tri"].astype(np.int64)[:, None] + np.arange(3)
        pos = verts["pos"][idx[at].astype(np.int64) + t["v_off"].astype(np.int64)[:, None]]
        assert crn[:, :, :3].tobytes() == np.ascontiguousarray(pos).tobytes()
        assert not crn[:, :, 3].view(np.uint32).any()  # +0.0f
        assert np.array_equal(tris["block_id"], t["id"])
    p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def keyed(table, answer, q, with_tri=True):
    """the list of query q as (coord_id, tri, corner bytes): what must not depend on the table's order"""
    rc, tris, corners, ranges, c = answer
    lo, k = int(ranges[q]["first"]), int(ranges[q]["count"])
    mine = tris[lo:lo + k]
    coord = table["coord_id"][mine["entry"]]
    return [(int(a), int(b) if with_tri else 0, corners[lo + i].tobytes()) for i, (a, b) in enumerate(zip(coord, mine["tri"]))]


def test_edits(torch):
    """The same surface gives the same lists, up to entry and block_id, whether it came from a full run or from a chain of
    incremental ones.  Far from a carve nothing changes at all at the levels whose blocks are smaller than the distance (levels
    0 and 1 of this grid); the one block of level 2 holds the carve itself, so an incremental run meshes it anew and numbers its
    triangles anew: there the corners of a far box's list, in order, are what stays.  Measured on this very case (the carve
    dirties [7.5, 12.5] x [28.5, 33.5] x [7.5, 12.5] and rebuilds 25 blocks): of the far boxes with matches, 71 of 71 at level 0 and
    73 of 73 at level 1 keep their list with the ordinals; at level 2 none of 69 keeps the ordinals and 69 of 69 keep the corners
    in order."""
    n = 64
    p = synth_poly(n, seed=21)
    levels = p.info.levels
    before_snap = snapshot(p)
    queries = [oo.cases(L, n, level_triangles(before_snap, L), random_boxes=300)[0] for L in range(levels)]
    before = [check(torch, p, level_triangles(before_snap, L), L, queries[L], "before L%d" % L, device=False) for L in range(levels)]
    mn, mx = p.inject_ball((10.0, 10.0, 31.0), (5, 5, 5), 4.0, 2)   # grid coordinates (Z-up); the box comes back in mesh space
    assert len(p.execute_dirty(mn, mx))

    def far(b):
        """at least 40 voxels from the carve on some axis (finite boxes only)"""
        return bool(np.all(np.isfinite(b["lo"])) and np.all(np.isfinite(b["hi"])) and np.all(b["lo"] <= b["hi"])
                    and np.any((b["lo"] >= mx + 40) | (b["hi"] <= mn - 40)))

    def compare(label, poly, device):
        snap = snapshot(poly)
        kept = 0
        for L in range(levels):
            answer = check(torch, poly, level_triangles(snap, L), L, queries[L], "%s L%d" % (label, L), device=device and L == 0)
            for q, b in enumerate(queries[L]):
                if far(b) and int(before[L][3][q]["count"]):
                    assert keyed(snap[0][L], answer, q, L < 2) == keyed(before_snap[0][L], before[L], q, L < 2), (label, L, q)
                    kept += 1
        assert kept > 10, label
        return snap

    after_snap = compare("after the incremental run", p, True)
    near = overlap_boxes(mn - 1, mx + 1)   # ... and at the carve the surface is another
    assert oo.overlap(level_triangles(after_snap, 0), near)[2].tobytes() != oo.overlap(level_triangles(before_snap, 0), near)[2].tobytes()
    p.compact_pools()
    compare("after compaction", p, False)
    p.execute()
    full_snap = compare("after a full run", p, False)
    # level 0: the chain of runs and the full run left the same surface, so every list is the same up to entry and block_id
    chain, full = oo.overlap(level_triangles(after_snap, 0), queries[0]), oo.overlap(level_triangles(full_snap, 0), queries[0])
    assert chain[3].tobytes() == full[3].tobytes() and chain[2].tobytes() == full[2].tobytes() and np.array_equal(chain[1]["tri"], full[1]["tri"])
    assert np.array_equal(after_snap[0][0]["coord_id"][chain[1]["entry"]], full_snap[0][0]["coord_id"][full[1]["entry"]])
    p.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_empty_level(torch):
    n = 32
    p = new_poly()
    p.upload(np.full((n, n, n), 127, np.int8), np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint8), np.ones((n // 16) ** 3, np.uint8))
    p.execute()
    assert p.info.levels >= 1 and p.device_block_table(0)[1] == 0
    boxes = overlap_boxes([[0, 0, 0], [-np.inf] * 3], [[n, n, n], [np.inf] * 3])
    counts, ranges = np.full(32, POISON, np.uint8), np.full(16, POISON, np.uint8)
    rc = p._L.lib.vx_overlap_boxes(p._h, 0, boxes.ctypes.data_as(C.c_void_p), 2, 0, None, None, ranges.ctypes.data_as(C.c_void_p),
                                   counts.ctypes.data_as(C.c_void_p))
    assert rc == 0 and not counts.any() and not ranges.any()
    tris, crn, dranges, dc, intact = device_form(torch, p, 0, boxes, 16)
    assert intact and not any(dc.values()) and len(tris) == 0 and not dranges.view(np.uint32).any()
    p.close()


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_n_zero(torch):
    p = golden_poly("terrain32_mat")
    counts = np.full(32, POISON, np.uint8)
    rc = p._L.lib.vx_overlap_boxes(p._h, 0, None, 0, 0, None, None, None, counts.ctypes.data_as(C.c_void_p))
    assert rc == 0 and not counts.any()
    tris, crn, ranges, dc, intact = device_form(torch, p, 0, np.zeros(0, oo.OVERLAP_BOX_DTYPE), 8)
    assert intact and not any(dc.values()) and len(tris) == 0
    p.close()


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_validation(torch):
    p = golden_poly("terrain32_mat")
    lib, vp = p._L.lib, C.c_void_p
    n, cap = 4, 64
    boxes = overlap_boxes(np.zeros((n, 3)), np.full((n, 3), 32.0))
    d_boxes = torch.from_numpy(boxes.view(np.uint8).copy()).cuda()
    d_tris = torch.full((cap * 16 + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_corners = torch.full((cap * 48 + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_ranges = torch.full((n * 8 + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((48,), POISON, dtype=torch.uint8, device="cuda")
    tris, corners = np.full(cap * 16, POISON, np.uint8), np.full(cap * 48, POISON, np.uint8)
    ranges, counts = np.full(n * 8, POISON, np.uint8), np.full(32, POISON, np.uint8)

    def ptr(a):
        return a.ctypes.data_as(vp)

    def dev(t, off=0):
        return vp(t.data_ptr() + off)

    def both(label, level=0, count=n, capacity=cap, no_boxes=False, no_tris=False, no_corners=False, no_counts=False, ctx=p):
        rc = ctx._L.lib.vx_overlap_boxes(ctx._h, level, None if no_boxes else ptr(boxes), count, capacity, None if no_tris else ptr(tris),
                                         None if no_corners else ptr(corners), ptr(ranges), None if no_counts else ptr(counts))
        assert rc == INVALID, ("host", label, rc)
        rc = ctx._L.lib.vx_overlap_boxes_device(ctx._h, level, None if no_boxes else dev(d_boxes), count, capacity, None if no_tris else dev(d_tris),
                                                None if no_corners else dev(d_corners), dev(d_ranges), None if no_counts else dev(d_counts))
        assert rc == INVALID, ("device", label, rc)

    both("level beyond the run", level=p.info.levels)
    both("null counts", no_counts=True)
    both("null boxes with n > 0", no_boxes=True)
    both("too many queries", count=oo.OVERLAP_MAX_QUERIES + 1)
    both("null tris with a capacity", no_tris=True, no_corners=True)
    both("corners without tris", capacity=0, no_tris=True)
    for label, off in (("boxes", (4, 0, 0, 0, 0)), ("tris", (0, 8, 0, 0, 0)), ("corners", (0, 0, 4, 0, 0)), ("ranges", (0, 0, 0, 4, 0)), ("counts", (0, 0, 0, 0, 8))):
        rc = lib.vx_overlap_boxes_device(p._h, 0, dev(d_boxes, off[0]), n - 1, cap, dev(d_tris, off[1]), dev(d_corners, off[2]), dev(d_ranges, off[3]),
                                         dev(d_counts, off[4]))
        assert rc == INVALID, ("misaligned " + label, rc)
    empty = new_poly()  # no surface yet
    both("no surface", ctx=empty)
    empty.close()
    torch.cuda.synchronize()
    for a in (tris, corners, ranges, counts, d_tris.cpu().numpy(), d_corners.cpu().numpy(), d_ranges.cpu().numpy(), d_counts.cpu().numpy()):
        assert np.all(a == POISON)
    # and the same buffers are written by a valid call
    assert lib.vx_overlap_boxes(p._h, 0, ptr(boxes), n, cap, ptr(tris), ptr(corners), ptr(ranges), ptr(counts)) == OVERFLOW
    assert not np.all(tris == POISON) and not np.all(corners == POISON) and not np.all(ranges == POISON) and not np.all(counts == POISON)
    p.close()


# 9 -------------------------------------------------------------------------------------------------------------------------
def test_index_is_built_on_demand(torch):
    p = synth_poly(64, seed=21)   # a fresh context: no vx_raycast_prepare, no ray cast
    snap = snapshot(p)
    lt = level_triangles(snap, 0)
    boxes, labels = oo.cases(0, 64, lt, random_boxes=100)
    check(torch, p, lt, 0, boxes, "first call")
    mn, mx = p.inject_ball((40.0, 24.0, 30.0), (5, 5, 5), 4.0, 2)
    assert len(p.execute_dirty(mn, mx))
    snap = snapshot(p)
    again = check(torch, p, level_triangles(snap, 0), 0, boxes, "after an incremental run")
    near = overlap_boxes(mn - 1, mx + 1)
    assert oo.overlap(lt, near)[2].tobytes() != check(torch, p, level_triangles(snap, 0), 0, near, "at the carve")[2].tobytes()
    assert again[4]["triangles"] > 0
    p.close()
