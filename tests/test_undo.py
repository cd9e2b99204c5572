"""The undo records without a GPU: the numpy statement of the header's text (tests/undo_oracle.py) against answers written by
hand, and the host build of the kernels' pipeline (tests/undo/undo_host.cpp: mark, scan, list, capture, diff, pack, swap with the
lanes as loops) against that oracle, byte for byte, over the shared case list.  tests/test_gpu_undo.py runs the device."""
import numpy as np
import pytest

import brush_oracle as bo
import undo_oracle as uo

CASES = uo.cases()


# ---- the oracle against answers written by hand -------------------------------------------------------------------------------

def test_block_set_by_hand():
    # 32^3: blocks 0..7, id = (bz * 2 + by) * 2 + bx.  The first box stays in block 0 but for x, where 16 is one voxel over the
    # border: blocks 0 and 1.  The second overlaps it and spans x 10..19: blocks 0 and 1 again.
    assert uo.block_set(32, [((1, 2, 3), (17, 5, 9)), ((10, 0, 0), (20, 16, 16))]).tolist() == [0, 1]
    assert uo.block_set(32, [((1, 2, 3), (16, 5, 9))]).tolist() == [0]                       # hi = 16 is exclusive
    assert uo.block_set(32, [((15, 15, 15), (17, 17, 17))]).tolist() == list(range(8))       # one voxel over every border
    assert uo.block_set(32, [((31, 31, 31), (32, 32, 32)), ((0, 0, 0), (1, 1, 1))]).tolist() == [0, 7]   # ascending, whatever the order
    assert uo.block_set(48, [((0, 0, 0), (48, 48, 48))]).tolist() == list(range(27))
    assert uo.block_set(48, [((0, 20, 40), (48, 21, 41))]).tolist() == [21, 22, 23]          # bz = 2, by = 1
    assert uo.block_set(32, []).size == 0


def test_capture_trim_swap_by_hand():
    g = uo.noise_grid(32, 7)
    before = g.copy()
    r = uo.capture(g, [((1, 2, 3), (17, 5, 9)), ((10, 0, 0), (20, 16, 16))])
    assert r.ids.tolist() == [0, 1] and g.same_as(before)
    assert np.array_equal(r.dist[1], before.dist[0:16, 0:16, 16:32]) and r.flags.tolist() == before.flags[:2].tolist()
    # the edit: voxels (x, y, z) = (14, 3, 2) .. (18, 3, 2) of the distance field, and a material at (20, 9, 15)
    g.dist[2, 3, 14:19] = before.dist[2, 3, 14:19] ^ 1
    g.mat[15, 9, 20] ^= 4
    edited = g.copy()
    t, dropped = uo.trim(g, r)
    assert dropped == 0 and t.same_as(r)
    res = uo.swap(g, r)
    assert g.same_as(before)
    # x 14..20, y 3..9, z 2..15 -> [a, b + 1], output order (x, z, y)
    assert res["out_min"].tolist() == [14.0, 2.0, 3.0] and res["out_max"].tolist() == [21.0, 16.0, 10.0]
    assert (int(res["changed_voxels"]), int(res["changed_blocks"]), int(res["flag_changes"]), int(res["reserved"])) == (6, 2, 0, 0)
    again = uo.swap(g, r)
    assert g.same_as(edited) and again.tobytes() == res.tobytes()
    # the box is clamped to n
    g.blend[31, 31, 31] ^= 1
    r = uo.capture(g, [((0, 0, 0), (32, 32, 32))])
    g.blend[31, 31, 31] ^= 1
    res = uo.swap(g, r)
    assert res["out_min"].tolist() == [31.0, 31.0, 31.0] and res["out_max"].tolist() == [32.0, 32.0, 32.0] and int(res["changed_blocks"]) == 1


def test_a_flag_only_block_counts_as_changed_and_moves_no_box():
    g = uo.noise_grid(32, 8)
    r = uo.capture(g, [((0, 0, 0), (32, 32, 32))])
    g.flags[5] ^= 1
    g.dist[0, 0, 0] ^= 1
    t, dropped = uo.trim(g, r)
    assert t.ids.tolist() == [0, 5] and dropped == 6
    res = uo.swap(g, t)
    assert res["out_min"].tolist() == [0.0, 0.0, 0.0] and res["out_max"].tolist() == [1.0, 1.0, 1.0]
    assert (int(res["changed_voxels"]), int(res["changed_blocks"]), int(res["flag_changes"])) == (1, 2, 1)
    # the flag alone: a zero box
    g.flags[3] ^= 1
    only = uo.trim(g, uo.capture(uo.Grid(g.dist, g.mat, g.blend, g.flags ^ np.uint8(0)), [((0, 0, 0), (32, 32, 32))]))[0]
    assert only.blocks == 0
    r = uo.capture(g, [((16, 16, 0), (32, 32, 16))])
    assert r.ids.tolist() == [3]
    g.flags[3] ^= 1
    res = uo.swap(g, r)
    assert not res["out_min"].any() and not res["out_max"].any()
    assert (int(res["changed_voxels"]), int(res["changed_blocks"]), int(res["flag_changes"])) == (0, 1, 1)


# ---- the host pipeline against the oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_host_pipeline_equals_the_oracle(case):
    _, g0, boxes, g1 = case
    want = uo.capture(g0, boxes)
    grid = g0.copy()
    rc, got = uo.host_capture(grid, boxes)
    assert rc == want.blocks and got.same_as(want) and grid.same_as(g0)
    # trim against the edited grid
    want_t, want_dropped = uo.trim(g1, want)
    grid = g1.copy()
    got_t, dropped = uo.host_trim(grid, got)
    assert dropped == want_dropped and got_t.same_as(want_t) and grid.same_as(g1)
    assert want_t.ids.tolist() == [int(i) for k, i in enumerate(want.ids) if uo.differs(g1, want, k)]
    # swap: the untrimmed and the trimmed record both take the edit back inside the captured blocks, with the same result
    for rec_o, rec_h in ((want, got), (want_t, got_t)):
        go, gh, ro, rh = g1.copy(), g1.copy(), rec_o.copy(), rec_h.copy()
        res_o, res_h = uo.swap(go, ro), uo.host_swap(gh, rh)
        assert res_h.tobytes() == res_o.tobytes(), (res_h, res_o)
        assert gh.same_as(go) and rh.same_as(ro)
        for bid in rec_o.ids:
            assert all(np.array_equal(a, b) for a, b in zip(gh.block(int(bid)), g0.block(int(bid)))) and gh.flags[bid] == g0.flags[bid]
        # swap o swap = identity
        again = uo.host_swap(gh, rh)
        assert gh.same_as(g1) and rh.same_as(rec_h) and again.tobytes() == res_h.tobytes()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_trim_after_no_edit_leaves_nothing(case):
    _, g0, boxes, _ = case
    grid = g0.copy()
    rc, rec = uo.host_capture(grid, boxes)
    t, dropped = uo.host_trim(grid, rec)
    assert t.blocks == 0 and dropped == rc and grid.same_as(g0)
    res = uo.host_swap(grid, rec)   # a record equal to the grid
    assert res.tobytes() == np.zeros(1, uo.SWAP_RESULT_DTYPE).tobytes() and grid.same_as(g0)


def test_a_capacity_below_the_block_count_is_refused():
    g = uo.noise_grid(48, 2)
    assert uo.host_capture(g, [((0, 0, 0), (48, 48, 48))], capacity=26)[0] == -1
    assert uo.host_capture(g, [((0, 0, 0), (48, 48, 48))], capacity=27)[0] == 27


# ---- vx_brush_box ---------------------------------------------------------------------------------------------------------------

def brush_cases(n):
    fn = float(n)
    out = [bo.ball((24.0, 24.0, 24.0), (8.0, 8.0, 8.0), 5.0, 2),            # 16..32 exactly: bmax = 16 and bmin = 32 both still touch
           bo.ball((24.0, 24.0, 24.0), (7.999, 8.0, 8.001), 5.0, 0),
           bo.ball((32.0, 16.0, 0.0), (16.0, 16.0, 16.0), 5.0, 2),           # position +- extents on multiples of 16
           bo.ball((np.nextafter(np.float32(16.0), np.float32(17.0)), 16.0, np.nextafter(np.float32(16.0), np.float32(0.0))), (0.0, 0.0, 0.0), 1.0, 2),
           bo.material((8.0, 40.0, 24.0), (8.0, 8.0, 8.0), 7, True),
           bo.brush(1, (20.5, 20.5, 20.5), (12.25, 3.0, 30.0), 2, 2.0, (-5, 0, 0), (5, 0, 0)),
           bo.box((fn / 2, fn / 2, fn / 2), (2 * fn, 2 * fn, 2 * fn), (9, 9, 9), 1.0, 2),   # larger than the grid
           bo.ball((-30.0, 20.0, 20.0), (10.0, 10.0, 10.0), 4.0, 2),        # misses the grid
           bo.ball((20.0, fn + 16.001, 20.0), (16.0, 16.0, 16.0), 4.0, 2),  # misses it by a hair
           bo.ball((20.0, fn + 16.0, 20.0), (16.0, 16.0, 16.0), 4.0, 2),    # touches the last block: bmax = n
           bo.ball((fn, fn, fn), (0.0, 0.0, 0.0), 1.0, 2)]
    return out + list(bo.anywhere_balls(n, 40, seed=5))


@pytest.mark.parametrize("n", [16, 48, 64])
def test_brush_box_equals_the_block_test_in_float32(n):
    from voxels_amd import binding
    lib = binding.HipLibrary()
    hits = 0
    for k, br in enumerate(brush_cases(n)):
        want_rc, want = uo.brush_box(br, n)
        rc, got = uo.host_brush_box(br, n)
        assert rc == want_rc and got.tobytes() == want.tobytes(), (k, br, got, want)
        # the library's export and brush_boxes say the same
        mine = binding.brush_boxes(bo.stack([br]), n, lib)
        assert mine.size == want_rc and (not want_rc or mine[0].tobytes() == want.tobytes()), k
        if want_rc:
            # the box holds exactly the blocks the per-axis test finds
            per_axis = [np.flatnonzero(uo.touched_blocks_1d(n, br["position"][a], br["extents"][a])) for a in range(3)]
            nb = n // 16
            ids = sorted((bz * nb + by) * nb + bx for bz in per_axis[2] for by in per_axis[1] for bx in per_axis[0])
            assert uo.block_set(n, [want]).tolist() == ids
            hits += 1
    assert 5 < hits < len(brush_cases(n))


def test_brush_box_by_hand():
    rc, box = uo.brush_box(bo.ball((24.0, 24.0, 24.0), (8.0, 8.0, 8.0), 5.0, 2), 64)
    assert rc == 1 and box["lo"].tolist() == [0, 0, 0] and box["hi"].tolist() == [48, 48, 48]   # 16 and 32 are touched borders
    rc, box = uo.brush_box(bo.ball((24.0, 24.0, 24.0), (7.0, 7.0, 7.0), 5.0, 2), 64)
    assert rc == 1 and box["lo"].tolist() == [16, 16, 16] and box["hi"].tolist() == [32, 32, 32]
    rc, box = uo.brush_box(bo.ball((-30.0, 20.0, 20.0), (10.0, 10.0, 10.0), 4.0, 2), 64)
    assert rc == 0 and not box["lo"].any() and not box["hi"].any()
    rc, box = uo.brush_box(bo.ball((32.0, 32.0, 32.0), (500.0, 500.0, 500.0), 5.0, 2), 64)
    assert rc == 1 and box["lo"].tolist() == [0, 0, 0] and box["hi"].tolist() == [64, 64, 64]
    lib = __import__("voxels_amd.binding", fromlist=["x"]).HipLibrary().lib
    assert lib.vx_brush_box(None, 64, None) == -1
    b, o = bo.stack([bo.ball((1.0, 1.0, 1.0), (1.0, 1.0, 1.0), 1.0, 2)]), np.zeros(1, uo.BOX_DTYPE)
    assert lib.vx_brush_box(b.ctypes.data, 60, o.ctypes.data) == -1 and lib.vx_brush_box(b.ctypes.data, 0, o.ctypes.data) == -1
