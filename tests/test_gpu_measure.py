"""The measurements on the MI355X against the numpy statement of the header's text (tests/measure_oracle.py), exactly: results,
deltas and tallies are compared as bytes.  Where the grid has been edited on the device, the oracle measures the device grid read
back as tests/test_gpu_undo.py reads it - the packed file expanded by the port, the flag bytes by vx_grid_read_block.
tests/test_measure.py anchors the oracle to answers written by hand."""
import numpy as np
import pytest

import brush_oracle as bo
import island_oracle as io
import measure_oracle as mo
import stamp_oracle as sto
import undo_oracle as uo
import vxo

pytestmark = pytest.mark.gpu

GRIDS = mo.grids() + [("80 terrain", mo.terrain_grid(80))]
INVALID = -1


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    assert p._L.has_measure
    p.set_materials(vxo.default_lut())
    return p


def resident(g):
    """a context that holds grid g, flag bytes included (a dense upload takes them from the caller)"""
    p = new_poly()
    p.upload(g.dist, g.mat, g.blend, g.flags)
    return p


def device_flags(p):
    f = np.zeros((p.n // 16) ** 3, np.uint8)
    for bid in range(f.size):
        p._check(p._lib.vx_grid_read_block(p._h, bid, None, None, None, f[bid:bid + 1].ctypes.data), "vx_grid_read_block")
    return f


def device_grid(p):
    d, m, b = vxo.load_port().grid_load(p.pack()).read_dense()
    return uo.Grid(d, m, b, device_flags(p))


def chunk(p, pairs):
    assert p._lib.vx_debug_measure_chunk(p._h, pairs) == 0


def shortcuts(p, on):
    assert p._lib.vx_debug_measure_shortcuts(p._h, int(on)) == 0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


def check_boxes(p, g, bx, tallies=True):
    want, want_t = mo.measure(g, bx)
    res, t = p.measure(bx, tallies=tallies)
    same(res, want)
    if tallies:
        same(t, want_t)
    else:
        assert t is None


def all_solid_blocks(g):
    nb = g.n // 16
    return (g.dist.reshape(nb, 16, nb, 16, nb, 16) < 0).all(axis=(1, 3, 5))


# ---- the case list --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,g", GRIDS, ids=[k for k, _ in GRIDS])
def test_case_lists_on_the_device(name, g):
    p = resident(g)
    lists = mo.box_lists(g.n)
    wanted = [mo.measure(g, bx) for _, bx in lists]
    # a fresh upload: the mirrors are stale, no summary is read.  After a full run they are current: with the shortcuts, then without.
    for state in ("fresh", "summaries", "summaries off"):
        if state == "summaries":
            p.execute()
        shortcuts(p, state != "summaries off")
        for pairs in (1, 7, 0):
            chunk(p, pairs)
            for (list_name, bx), (want, want_t) in zip(lists, wanted):
                res, t = p.measure(bx)
                same(res, want); same(t, want_t)
    chunk(p, 7)
    shortcuts(p, True)
    for (list_name, bx), (want, _) in zip(lists, wanted):
        res, t = p.measure(bx, tallies=False)
        assert t is None
        same(res, want)
    res, t = p.measure([])                 # count = 0
    assert res.size == 0 and t.shape == (0, 256)


def test_the_largest_grid():
    n = 208
    g = mo.layered_grid(n)
    assert all_solid_blocks(g).any()
    bx = np.concatenate([mo.boxes([((0, 0, 0), (n, n, n))]), mo.random_boxes(n, 1000, 12, largest=48)])
    want, want_t = mo.measure(g, bx)
    p = resident(g)
    p.execute()
    for on in (True, False):
        shortcuts(p, on)
        res, t = p.measure(bx)
        same(res, want); same(t, want_t)
    chunk(p, 1000)
    res, t = p.measure(bx)
    same(res, want); same(t, want_t)


# ---- after edits: no stale summary is used ----------------------------------------------------------------------------------------

def test_a_measure_after_a_carve():
    g = mo.layered_grid(48)                # its lowest block layer is all solid, its highest all air
    p = resident(g)
    p.execute()                            # the summaries are current
    lists = mo.box_lists(48, randoms=100)
    for _, bx in lists[3:5]:
        check_boxes(p, g, bx)
    solid0 = all_solid_blocks(g)
    p.inject_ball((20.0, 27.0, 6.0), (20.0, 20.0, 20.0), 7.0, 2)   # into blocks that were all solid
    after = device_grid(p)
    assert (solid0 & ~all_solid_blocks(after)).any()
    for _, bx in lists:
        check_boxes(p, after, bx)
    p.inject_ball((30.0, 20.0, 30.0), (20.0, 20.0, 20.0), 7.0, 0)   # into blocks that were all air
    after = device_grid(p)
    for _, bx in lists:
        check_boxes(p, after, bx)


def test_a_measure_after_an_island_removal_and_after_a_paste():
    d = io.floating()
    m = np.full(d.shape, 3, np.uint8)
    m[20:26] = 8
    g = uo.Grid(d, m, np.zeros(d.shape, np.uint8), io.codec_flags(d))
    p = resident(g)
    p.execute()
    lists = mo.box_lists(48, randoms=100)
    check_boxes(p, g, lists[3][1])
    counts = p.islands(remove=True)[1]
    assert int(counts["removed"]) == 2
    after = device_grid(p)
    assert int((after.dist < 0).sum()) == int((g.dist < 0).sum()) - 216 - 8
    for _, bx in lists:
        check_boxes(p, after, bx)
    stamp = sto.solid_stamp((20, 18, 17), -90, 5, 77)
    p.paste([p.upload_stamp(stamp.dist, stamp.mat, stamp.blend)], sto.pastes([((14, 15, 16), 0, 1, sto.PASTE_REPLACE), ((0, 0, 0), 0, 0, sto.PASTE_SUBTRACT)]))
    after = device_grid(p)
    for _, bx in lists:
        check_boxes(p, after, bx)


# ---- vx_record_measure ------------------------------------------------------------------------------------------------------------

def edit_brushes(p):
    from voxels_amd import brush_boxes
    c = p.n / 2.0
    brushes = bo.stack([bo.ball((c + 1.5, c - 2.25, 9.0), (14.0, 14.0, 14.0), 5.0, 2),
                        bo.brush(1, (c - 6.0, c + 4.0, 14.0), (20.0, 9.0, 9.0), 0, 2.5, (-7.0, 0.0, 0.0), (7.0, 1.0, -1.0)),
                        bo.material((c, c, 8.0), (18.0, 10.0, 12.0), 9, True)])
    return brush_boxes(brushes, p.n), lambda: p.inject_brushes(brushes)


def edit_smooth(p):
    from voxels_amd.binding import smooth_op
    box = ((5, 17, 4), (43, 33, 40))
    return uo.boxes([box]), lambda: p.smooth(smooth_op(box, (24.25, 25.5, 16.0), 6.0, 1.0, 2))


def edit_paste(p):
    from voxels_amd import paste_boxes
    stamps = [sto.noise_stamp((17, 5, 3), 5), sto.solid_stamp((9, 9, 9), -90, 5, 77)]
    ps = sto.pastes([((9, 12, 8), 0, 3, sto.PASTE_REPLACE), ((25, 25, 4), 1, 0, sto.PASTE_SUBTRACT), ((3, 30, 20), 1, 6, sto.PASTE_UNION), ((20, 5, 6), 1, 0, sto.PASTE_PAINT)])
    dev = [p.upload_stamp(s.dist, s.mat, s.blend) for s in stamps]
    return paste_boxes(ps, [s.size for s in stamps], p.n), lambda: p.paste(dev, ps)


EDITS = [("brushes", edit_brushes), ("smooth", edit_smooth), ("pastes", edit_paste)]


def check_delta(rec, grid, held):
    want = mo.record_delta(grid, held)
    got = rec.measure()
    same(got[0], want[0]); same(got[1], want[1]); same(got[2], want[2])
    only, none_r, none_a = rec.measure(tallies=False)
    assert none_r is None and none_a is None
    same(only, want[0])
    return want


@pytest.mark.parametrize("kind", EDITS, ids=[k[0] for k in EDITS])
def test_record_measure_around_an_edit(kind):
    g = mo.terrain_grid(48)
    p = resident(g)
    p.execute()
    boxes, edit = kind[1](p)
    rec = p.capture(boxes)
    held = uo.capture(g, boxes)
    zero = check_delta(rec, g, held)       # untouched: zeros
    assert zero[0].tobytes() == bytes(64)
    edit()
    after = device_grid(p)
    want = check_delta(rec, after, held)
    d = want[0]
    if kind[0] != "smooth":                # (a smoothing pass need not move a sign)
        assert int(d["removed_voxels"]) > 0 and int(d["added_voxels"]) > 0
    # after the swap the record holds the edited state: the redo's effect, removed and added exchanged
    rec.swap()
    g2, r2 = after.copy(), held.copy()
    uo.swap(g2, r2)
    redo = check_delta(rec, g2, r2)
    assert (int(redo[0]["removed_voxels"]), int(redo[0]["added_voxels"])) == (int(d["added_voxels"]), int(d["removed_voxels"]))
    rec.swap()
    # after the trim: fewer blocks held, the same answer
    blocks0 = int(rec.info()["blocks"])
    dropped = rec.trim()
    assert int(rec.info()["blocks"]) == blocks0 - dropped >= int(d["blocks"])
    again = rec.measure()
    same(again[0], want[0]); same(again[1], want[1]); same(again[2], want[2])
    empty = p.capture([])
    e = empty.measure()
    assert e[0].tobytes() == bytes(64) and not e[1].any() and not e[2].any()


def test_the_yield_of_a_carve():
    from voxels_amd import brush_boxes
    g = mo.terrain_grid(48)
    p = resident(g)
    carve = bo.stack([bo.ball((22.0, 26.0, 8.0), (18.0, 18.0, 18.0), 7.0, 2)])
    box = brush_boxes(carve, 48)
    assert box.size == 1
    before = p.measure(box)
    rec = p.capture(box)
    p.inject_brushes(carve)
    after = p.measure(box)
    delta, removed, added = rec.measure()
    assert int(delta["removed_voxels"]) > 100 and int(delta["added_voxels"]) == 0 and not added.any()
    assert np.array_equal(removed, before[1][0] - after[1][0])
    assert int(delta["removed_voxels"]) == int(before[0][0]["solid_voxels"]) - int(after[0][0]["solid_voxels"])


# ---- nothing changes ----------------------------------------------------------------------------------------------------------------

def test_nothing_changes_and_full_runs_still_replay():
    from voxels_amd import synth
    n = 64
    d, m, b = synth.terrain(n, seed=21)      # (a field whose full runs are single-stream ones: tests/test_gpu_matstore.py)
    p = new_poly()
    p.upload_packed(vxo.load_port().grid_from_dense(np.ascontiguousarray(d), m, b).pack())
    pack0, flags0 = p.pack(), device_flags(p)
    for _ in range(4):          # the first runs of a context vote, then capture; the ones behind them replay
        p.execute()
        if p.material_path_counts()[1]:
            break
    rec = p.capture([((0, 0, 0), (n, n, n))])
    held = [rec.read_block(k) for k in (0, 21, 63)]
    p.execute()
    plan_a = p.slot_plan_counts()
    p.execute()
    plan_b, mats = p.slot_plan_counts(), p.material_path_counts()
    step = (plan_b[0] - plan_a[0], plan_b[1] - plan_a[1])
    bx = np.concatenate([mo.boxes([((0, 0, 0), (n, n, n))]), mo.random_boxes(n, 50, 3)])
    first = p.measure(bx)
    delta = rec.measure()
    assert delta[0].tobytes() == bytes(64)
    p.execute()
    plan_c = p.slot_plan_counts()
    assert (plan_c[0] - plan_b[0], plan_c[1] - plan_b[1]) == step and p.material_path_counts() == mats, (plan_a, plan_b, plan_c)
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), flags0)
    for k, blk in zip((0, 21, 63), held):
        for x, y in zip(rec.read_block(k), blk):
            assert np.array_equal(x, y)
    second = p.measure(bx)
    same(second[0], first[0]); same(second[1], first[1])
    want = mo.measure(device_grid(p), bx)
    same(first[0], want[0]); same(first[1], want[1])


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_every_listed_error_is_invalid():
    from voxels_amd import Polygonizer, binding
    g48, g64 = mo.terrain_grid(48), sto.terrain_grid(64)
    p, other = resident(g48), resident(g48)
    lib, h = p._lib, p._h
    good = binding.boxes([((0, 0, 0), (8, 8, 8))])
    res = np.zeros(4, binding.MEASURE_DTYPE)
    t = np.zeros((4, 256), np.uint64)
    assert lib.vx_grid_measure(h, good.ctypes.data, 1, res.ctypes.data, t.ctypes.data) == 0
    assert lib.vx_grid_measure(None, good.ctypes.data, 1, res.ctypes.data, None) == INVALID
    assert lib.vx_grid_measure(h, good.ctypes.data, 1, None, None) == INVALID
    assert lib.vx_grid_measure(h, None, 1, res.ctypes.data, None) == INVALID
    many = np.repeat(good, binding.MEASURE_MAX_BOXES + 1)
    big = np.zeros(many.size, binding.MEASURE_DTYPE)
    assert lib.vx_grid_measure(h, many.ctypes.data, many.size, big.ctypes.data, None) == INVALID
    assert lib.vx_grid_measure(h, many.ctypes.data, many.size - 1, big.ctypes.data, None) == 0
    same(big[:-1], np.repeat(res[:1], binding.MEASURE_MAX_BOXES))
    for lo, hi in (((4, 4, 4), (4, 8, 8)), ((0, 0, 0), (49, 8, 8)), ((0, 9, 0), (8, 8, 8)), ((0, 0, 48), (1, 1, 49))):
        bad = binding.boxes([((0, 0, 0), (8, 8, 8)), (lo, hi)])
        assert lib.vx_grid_measure(h, bad.ctypes.data, 2, res.ctypes.data, None) == INVALID, (lo, hi)
    bare = Polygonizer(device=0)           # owns no grid
    assert bare._lib.vx_grid_measure(bare._h, good.ctypes.data, 1, res.ctypes.data, None) == INVALID
    assert lib.vx_grid_measure(h, None, 0, None, None) == 0                  # count = 0 writes nothing
    assert lib.vx_debug_measure_chunk(None, 1) == INVALID
    # the record call
    mine, theirs = p.capture(good), other.capture(good)
    delta = np.zeros(1, binding.RECORD_DELTA_DTYPE)
    assert lib.vx_record_measure(h, mine._r, delta.ctypes.data, None, None) == 0
    assert lib.vx_record_measure(None, mine._r, delta.ctypes.data, None, None) == INVALID
    assert lib.vx_record_measure(h, None, delta.ctypes.data, None, None) == INVALID
    assert lib.vx_record_measure(h, mine._r, None, None, None) == INVALID
    assert lib.vx_record_measure(h, theirs._r, delta.ctypes.data, None, None) == INVALID      # a record of another context
    p.upload(g64.dist, g64.mat, g64.blend, g64.flags)
    assert lib.vx_record_measure(h, mine._r, delta.ctypes.data, None, None) == INVALID        # a record from a grid of another edge
    assert lib.vx_grid_measure(h, binding.boxes([((0, 0, 0), (64, 64, 64))]).ctypes.data, 1, res.ctypes.data, None) == 0
    assert int(res[0]["voxels"]) == 64 ** 3 and int(res[0]["solid_voxels"]) == int((g64.dist < 0).sum())
