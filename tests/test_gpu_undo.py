"""The undo records on the MI355X against the numpy statement of the header's text (tests/undo_oracle.py), exactly.  The state
of the device grid is read back - the packed file (vx_grid_pack) expanded by the port, and the flag bytes, which a pack
recomputes, by vx_grid_read_block - before and after real edits: a brush batch, a smoothing op, an island removal.  Records
are read with vx_record_block_ids / vx_record_read_block; after a swap the packed file must be the one from before the edit,
byte for byte.  tests/test_undo.py anchors the oracle to answers written by hand."""
import ctypes as C

import numpy as np
import pytest

import brush_oracle as bo
import fields
import island_oracle as io
import smooth_oracle as so
import undo_oracle as uo
import vxo

pytestmark = pytest.mark.gpu

ZERO_RESULT = np.zeros(1, uo.SWAP_RESULT_DTYPE).tobytes()


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    assert p._L.has_undo
    p.set_materials(vxo.default_lut())
    return p


def resident(dist, mat=None, blend=None):
    n = dist.shape[0]
    if mat is None:
        mat, blend = fields.materials_for(n, 3)
    g = vxo.load_port().grid_from_dense(np.ascontiguousarray(dist), mat, blend)
    p = new_poly()
    p.upload_packed(g.pack())
    return p


def packed(g):
    return vxo.load_port().grid_from_dense(g.dist, g.mat, g.blend).pack()


def device_flags(p):
    f = np.zeros((p.n // 16) ** 3, np.uint8)
    for bid in range(f.size):
        p._check(p._lib.vx_grid_read_block(p._h, bid, None, None, None, f[bid:bid + 1].ctypes.data), "vx_grid_read_block")
    return f


def device_grid(p, pack=None):
    """the resident grid as a uo.Grid: the fields out of the packed file, the flag bytes block by block"""
    d, m, b = vxo.load_port().grid_load(p.pack() if pack is None else pack).read_dense()
    return uo.Grid(d, m, b, device_flags(p))


def changed_blocks(a, b):
    return [bid for bid in range(a.flags.size)
            if a.flags[bid] != b.flags[bid] or any(not np.array_equal(x, y) for x, y in zip(a.block(bid), b.block(bid)))]


def same_result(got, want):
    assert got.tobytes() == want.tobytes(), (got, want)


def carve_batch(n):
    """ball, capsule, box and material brushes; one misses the grid"""
    c = n / 2.0
    return bo.stack([bo.ball((c + 1.5, c - 2.25, c), (14.0, 14.0, 14.0), 5.0, 2),
                     bo.brush(1, (c - 6.0, c + 4.0, c + 2.0), (20.0, 9.0, 9.0), 2, 2.5, (-7.0, 0.0, 0.0), (7.0, 1.0, -1.0)),
                     bo.box((c + 8.0, c, c - 5.0), (12.0, 12.0, 12.0), (3.0, 4.0, 2.0), 1.0, 0),
                     bo.material((c, c, c - 3.0), (18.0, 10.0, 12.0), 9, True),
                     bo.ball((-40.0, c, c), (10.0, 10.0, 10.0), 4.0, 2)])


def paint_batch(n):
    """material brushes only"""
    c = n / 2.0
    return bo.stack([bo.material((c, c, c - 3.0), (18.0, 10.0, 12.0), 9, True), bo.material((c + 5.0, c - 4.0, c), (7.0, 20.0, 30.0), 11, False)])


def edit_brushes(p):
    from voxels_amd import brush_boxes
    brushes = carve_batch(p.n)
    boxes = brush_boxes(brushes, p.n)
    assert boxes.size == brushes.size - 1

    def edit():
        return p.inject_brushes(brushes)[3]
    return boxes, edit


def edit_smooth(p):
    box = ((5, 17, 4), (43, 33, 40))      # 18 blocks; the ball around the surface at z = 11 changes voxels in two of them
    op = so.smooth_op(box, (24.25, 25.5, 16.0), 6.0, 1.0, 2)

    def edit():
        assert p.smooth(op)[3] > 0
        return None
    return uo.boxes([box]), edit


def edit_islands(p):
    def edit():
        counts = p.islands(remove=True)[1]
        assert int(counts["removed"]) == 2
        return None
    return uo.boxes([((0, 0, 0), (p.n, p.n, p.n))]), edit


EDITS = [("brushes", lambda: so.terrain(48)[0], edit_brushes), ("smooth", lambda: so.terrain(48)[0], edit_smooth), ("islands", io.floating, edit_islands)]


@pytest.mark.parametrize("kind", EDITS, ids=[k[0] for k in EDITS])
def test_capture_edit_trim_swap_swap(kind):
    _, field, make = kind
    p = resident(field())
    boxes, edit = make(p)
    pack0 = p.pack()
    before = device_grid(p, pack0)
    blocks0 = {bid: p.read_block(bid) for bid in range(before.flags.size)}
    rec = p.capture(boxes)
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), before.flags)   # a capture changes nothing
    held = rec.block_ids()
    assert held.tolist() == uo.block_set(p.n, boxes).tolist()
    touched = edit()
    if touched is not None:
        assert held.size == touched          # exactly the blocks the batch reports
    pack1 = p.pack()
    after = device_grid(p, pack1)
    changed = changed_blocks(before, after)
    assert 0 < len(changed) < held.size and set(changed) <= set(held.tolist())
    # trim
    dropped = rec.trim()
    assert rec.block_ids().tolist() == changed and dropped == held.size - len(changed)
    info = rec.info()
    assert (int(info["n"]), int(info["blocks"]), int(info["bytes"]), int(info["swaps"])) == (p.n, len(changed), 12293 * len(changed), 0)
    nb = p.n // 16
    coords = np.array([(b % nb, (b // nb) % nb, b // (nb * nb)) for b in changed])
    assert info["min"].tolist() == coords.min(0).tolist() and info["max"].tolist() == coords.max(0).tolist()
    for i, bid in enumerate(changed):
        got, want = rec.read_block(i), blocks0[bid]
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], bid
    assert np.array_equal(p.pack(), pack1)                                                       # a trim changes nothing
    # swap: the grid from before the edit
    orec = uo.trim(after, uo.capture(before, boxes))[0]
    state = after.copy()
    want = uo.swap(state, orec)
    assert int(want["changed_voxels"]) > 0 and state.same_as(before)
    same_result(rec.swap(), want)
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), before.flags)
    for i, bid in enumerate(changed):
        got, now = rec.read_block(i), after.block(bid)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], now)) and got[3] == after.flags[bid], bid
    # swap again: the edit
    same_result(rec.swap(), uo.swap(state, orec))
    assert state.same_as(after)
    assert np.array_equal(p.pack(), pack1) and np.array_equal(device_flags(p), after.flags)
    assert int(rec.info()["swaps"]) == 2
    rec.free()


def level0_equals_fresh(p, fresh):
    part, full = p.all_levels()[0], fresh.all_levels()[0]
    assert len(part.infos) == len(full.infos)
    at = {tuple(c): i for c, i in zip(full.infos["min_corner"].tolist(), full.infos["id"])}
    part.infos = part.infos.copy()
    part.infos["id"] = [at[tuple(c)] for c in part.infos["min_corner"].tolist()]
    ok, msg = fields.listed_blocks_equal_by_id(part, full)
    assert ok, msg


@pytest.mark.parametrize("batch", [carve_batch, paint_batch], ids=["carve", "materials only"])
def test_a_swap_feeds_the_incremental_path(batch):
    """full run, capture, edit, incremental run, swap, incremental run over the swap's box: level 0 equals a fresh full run of the
    original grid block by block, paired by corner as tests/test_gpu_smooth.py pairs them; then a full run equals the port's on
    the original grid, statistics included, so the mirrors followed the swap.  The batch of material brushes alone asks whether
    [a, b + 1] is enough where no distance differs."""
    from voxels_amd import brush_boxes
    n = 64
    port = vxo.load_port()
    d, m, b = so.terrain(n, 12)
    g = port.grid_from_dense(d, m, b)
    fresh = port.execute(g)
    p = new_poly()
    p.upload_packed(g.pack())
    pack0 = p.pack()
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    brushes = batch(n)
    rec = p.capture(brush_boxes(brushes, n))
    _, umin, umax, touched = p.inject_brushes(brushes)
    assert touched == int(rec.info()["blocks"]) > 0
    assert not np.array_equal(p.pack(), pack0)
    p.execute_dirty(umin, umax)
    assert rec.trim() > 0
    res = rec.swap()
    assert int(res["changed_voxels"]) > 50 and np.array_equal(p.pack(), pack0)
    p.execute_dirty(res["out_min"], res["out_max"])
    level0_equals_fresh(p, fresh)
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())
    assert np.array_equal(p.pack(), pack0)


def test_a_stack_of_three_edits_undone_and_redone():
    from voxels_amd import brush_boxes
    n = 48
    p = resident(so.terrain(n)[0])
    c = n / 2.0
    carve = bo.stack([bo.ball((c, c, c), (16.0, 16.0, 16.0), 6.0, 2)])
    paint = bo.stack([bo.material((c + 4.0, c, c), (12.0, 12.0, 12.0), 9, True)])
    box = ((16, 14, 12), (38, 36, 34))
    steps = [(brush_boxes(carve, n), lambda: p.inject_brushes(carve)), (uo.boxes([box]), lambda: p.smooth(so.smooth_op(box, iterations=2))),
             (brush_boxes(paint, n), lambda: p.inject_brushes(paint))]
    states, recs, orecs = [device_grid(p)], [], []
    for boxes, edit in steps:
        rec = p.capture(boxes)
        edit()
        states.append(device_grid(p))
        rec.trim()
        assert int(rec.info()["blocks"]) > 0
        recs.append(rec)
        orecs.append(uo.trim(states[-1], uo.capture(states[-2], boxes))[0])
        assert rec.block_ids().tolist() == orecs[-1].ids.tolist()
    # the three edits overlap: they share blocks
    assert set(orecs[0].ids.tolist()) & set(orecs[1].ids.tolist()) & set(orecs[2].ids.tolist())
    cur = states[3].copy()
    for k, to in ((2, 2), (1, 1), (0, 0), (0, 1), (1, 2), (2, 3)):   # undo 3, 2, 1, then redo 1, 2, 3
        same_result(recs[k].swap(), uo.swap(cur, orecs[k]))
        assert cur.same_as(states[to]), (k, to)
        assert np.array_equal(p.pack(), packed(cur)) and np.array_equal(device_flags(p), cur.flags), (k, to)
    assert [int(r.info()["swaps"]) for r in recs] == [2, 2, 2]


def test_no_edit_nothing_changes_and_full_runs_still_replay():
    from voxels_amd import synth
    n = 64
    d, m, b = synth.terrain(n, seed=21)      # (a field whose full runs are single-stream ones: tests/test_gpu_matstore.py)
    p = resident(d, m, b)
    pack0 = p.pack()
    flags0 = device_flags(p)
    for _ in range(4):          # the first runs of a context vote, then capture; the ones behind them replay
        p.execute()
        if p.material_path_counts()[1]:
            break
    counts = p.material_path_counts()
    assert counts[0] == 0 and counts[1] > 0, counts
    whole = [((0, 0, 0), (n, n, n))]
    rec = p.capture(whole)
    assert int(rec.info()["blocks"]) == 64
    p.execute()
    assert p.material_path_counts() == counts            # a capture leaves the store alone
    same_result(rec.swap(), np.zeros(1, uo.SWAP_RESULT_DTYPE)[0])   # a record equal to the grid
    p.execute()
    assert p.material_path_counts() == counts
    assert rec.trim() == 64 and int(rec.info()["blocks"]) == 0 and int(rec.info()["bytes"]) == 0
    assert rec.block_ids().size == 0 and not rec.info()["min"].any() and not rec.info()["max"].any()
    assert rec.swap().tobytes() == ZERO_RESULT and rec.trim() == 0
    empty = p.capture([])
    assert int(empty.info()["blocks"]) == 0 and empty.swap().tobytes() == ZERO_RESULT and empty.trim() == 0
    p.execute()
    assert p.material_path_counts() == counts
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), flags0)
    assert int(rec.info()["swaps"]) == 2 and int(empty.info()["swaps"]) == 1
    # a swap that changes something drops the store: the next run votes
    one = p.capture(whole)
    p.inject_ball((32.0, 32.0, 32.0), (12.0, 12.0, 12.0), 5.0, 2)
    for _ in range(4):
        p.execute()
        if p.material_path_counts()[1]:
            break
    assert p.material_path_counts()[0] == 0
    assert int(one.swap()["changed_blocks"]) > 0
    p.execute()
    assert p.material_path_counts()[0] > 0
    assert np.array_equal(p.pack(), pack0)


def test_a_whole_grid_capture_at_48_holds_27_blocks():
    p = resident(so.terrain(48)[0])
    rec = p.capture([((0, 0, 0), (48, 48, 48))])
    info = rec.info()
    assert (int(info["blocks"]), int(info["bytes"])) == (27, 27 * 12293)
    assert info["min"].tolist() == [0, 0, 0] and info["max"].tolist() == [2, 2, 2]
    assert rec.block_ids().tolist() == list(range(27))
    for i in (0, 13, 26):
        got, want = rec.read_block(i), p.read_block(i)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3]
    # overlapping and repeated boxes in any order: each block once, ascending
    again = p.capture([((40, 40, 40), (48, 48, 48)), ((0, 0, 0), (17, 1, 1)), ((40, 40, 40), (48, 48, 48)), ((15, 0, 0), (16, 1, 1))])
    assert again.block_ids().tolist() == [0, 1, 26]


def test_invalid_calls_leave_everything_untouched():
    import torch
    from voxels_amd import RECORD_INFO_DTYPE
    n = 48
    d = so.noise(n, 2)
    p = resident(d)
    before = p.pack()
    lib, h = p._lib, p._h
    good = uo.boxes([((0, 0, 0), (n, n, n))])
    out = C.c_void_p()

    def capture(boxes, count=None, ctx=h, dest=out):
        boxes = None if boxes is None else np.ascontiguousarray(boxes)
        return lib.vx_grid_capture(ctx, None if boxes is None else boxes.ctypes.data, boxes.size if count is None else count, None if dest is None else C.byref(dest))

    for lo, hi in (((4, 4, 4), (4, 8, 8)), ((4, 9, 4), (8, 8, 8)), ((4, 4, 4), (8, 8, 49)), ((4, 4, 4), (49, 8, 8)), ((0, 48, 0), (1, 49, 1))):
        for boxes in (uo.boxes([(lo, hi)]), uo.boxes([((0, 0, 0), (n, n, n)), (lo, hi)])):     # the bad box alone, and behind a good one
            out.value = 1
            assert capture(boxes) == -1 and out.value is None, (lo, hi)
    assert capture(None, 1) == -1
    assert capture(np.repeat(good, (1 << 16) + 1)) == -1
    assert capture(good, dest=None) == -1 and capture(good, ctx=None) == -1
    assert capture(np.repeat(good, 1 << 16)) == 0                        # the limit itself is fine: 27 blocks
    full = out.value
    ids = np.zeros(27, np.uint32)
    info = np.zeros(1, RECORD_INFO_DTYPE)
    assert lib.vx_record_block_ids(h, full, ids.ctypes.data, 26) == -1 and lib.vx_record_block_ids(h, full, None, 27) == -1
    assert lib.vx_record_block_ids(h, full, ids.ctypes.data, 27) == 0 and ids.tolist() == list(range(27))
    blk = np.zeros(4096, np.uint8)
    assert lib.vx_record_read_block(h, full, 27, blk.ctypes.data, None, None, None) == -1
    assert lib.vx_record_read_block(h, full, 26, blk.ctypes.data, None, None, None) == 0
    assert lib.vx_record_read_block(h, None, 0, blk.ctypes.data, None, None, None) == -1
    assert lib.vx_record_info_get(h, full, None) == -1 and lib.vx_record_info_get(h, None, info.ctypes.data) == -1 and lib.vx_record_info_get(None, full, info.ctypes.data) == -1
    for fn in (lib.vx_record_trim, lib.vx_record_swap):
        assert fn(h, None, None) == -1 and fn(None, full, None) == -1
    lib.vx_record_free(h, None)
    assert np.array_equal(p.pack(), before)
    # a record used with another context
    other = resident(so.noise(n, 5))
    other_before = other.pack()
    for fn in (lib.vx_record_trim, lib.vx_record_swap):
        assert fn(other._h, full, None) == -1
    assert lib.vx_record_info_get(other._h, full, info.ctypes.data) == -1 and lib.vx_record_block_ids(other._h, full, ids.ctypes.data, 27) == -1
    assert lib.vx_record_read_block(other._h, full, 0, blk.ctypes.data, None, None, None) == -1
    lib.vx_record_free(other._h, full)                                   # not its record: nothing happens
    assert np.array_equal(other.pack(), other_before) and np.array_equal(p.pack(), before)
    assert lib.vx_record_block_ids(h, full, ids.ctypes.data, 27) == 0
    # the outputs may be NULL
    p.inject_ball((24.0, 24.0, 24.0), (10.0, 10.0, 10.0), 5.0, 2)
    edited = p.pack()
    assert not np.array_equal(edited, before)
    assert lib.vx_record_trim(h, full, None) == 0 and lib.vx_record_swap(h, full, None) == 0
    assert np.array_equal(p.pack(), before)
    # a record used after the context uploaded a grid of another size; and again after one of its own size
    rec = p.capture(good)
    p.upload_packed(vxo.load_port().grid_from_dense(so.noise(32, 4), *fields.materials_for(32, 3)).pack())
    small = p.pack()
    for fn in (lib.vx_record_trim, lib.vx_record_swap):
        assert fn(h, rec._r, None) == -1
    assert capture(good) == -1                                           # hi > n now
    assert np.array_equal(p.pack(), small)
    assert int(rec.info()["blocks"]) == 27                               # reading it stays legal
    p.upload_packed(edited)
    same = rec.swap()
    assert int(same["changed_blocks"]) > 0 and np.array_equal(p.pack(), before)
    # an attached grid is not the context's own; neither is no grid at all
    dev = torch.device("cuda:0")
    mat, blend = fields.materials_for(n, 3)
    g = vxo.load_port().grid_from_dense(d, mat, blend)
    td, tm, tb = (torch.from_numpy(x.copy()).to(dev) for x in (d, mat, blend))
    tf = torch.from_numpy(g.block_flags().copy()).to(dev)
    a = new_poly()
    a.attach(n, 0, n, td.data_ptr(), 0, tm.data_ptr(), tb.data_ptr(), 0, tf.data_ptr())
    assert capture(good, ctx=a._h) == -1 and capture(np.zeros(0, uo.BOX_DTYPE), 0, ctx=a._h) == -1
    bare = new_poly()
    assert capture(good, ctx=bare._h) == -1
    torch.cuda.synchronize()
    assert np.array_equal(td.cpu().numpy(), d)


def test_records_survive_runs_and_pool_compaction():
    from voxels_amd import brush_boxes
    n = 64
    port = vxo.load_port()
    d, m, b = so.terrain(n, 12)
    g = port.grid_from_dense(d, m, b)
    p = new_poly()
    p.upload_packed(g.pack())
    pack0 = p.pack()
    p.execute()
    brushes = carve_batch(n)
    rec = p.capture(brush_boxes(brushes, n))
    _, umin, umax, _ = p.inject_brushes(brushes)
    p.execute_dirty(umin, umax)
    p.compact_pools()
    p.execute()
    p.compact_pools()
    edited = p.pack()
    assert rec.trim() > 0
    res = rec.swap()
    assert int(res["changed_voxels"]) > 0 and np.array_equal(p.pack(), pack0)
    p.execute()
    fresh = port.execute(g)
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())
    p.compact_pools()
    again = rec.swap()
    assert again.tobytes() == res.tobytes() and np.array_equal(p.pack(), edited)
