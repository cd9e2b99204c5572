"""The height maps on the MI355X against the numpy statement of the header's text (tests/height_oracle.py), exactly: heights,
materials, surface counts and the counts record are compared as bytes.  Where the grid has been edited on the device, the oracle
reads the device grid back as tests/test_gpu_measure.py reads it.  tests/test_height.py anchors the oracle to answers written by
hand."""
import numpy as np
import pytest

import height_oracle as ho
import island_oracle as io
import measure_oracle as mo
import stamp_oracle as sto
import undo_oracle as uo
import vxo

pytestmark = pytest.mark.gpu

GRIDS = ho.grids()
INVALID = -1
TOP, BOTTOM = ho.HEIGHT_FROM_TOP, ho.HEIGHT_FROM_BOTTOM


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    assert p._L.has_height
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


def shortcuts(p, on):
    assert p._lib.vx_debug_height_shortcuts(p._h, int(on)) == 0


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (a, b)


def check_case(p, want, box, direction, layers, flag):
    h, m, s, c = p.heightmap(box, direction, layers, True, flag)
    same(h, want[0]); same(m, want[1]); same(c, want[3])
    if flag:
        same(s, want[2])
    else:
        assert s is None
    return h


def check_grid(p, g, boxes, layer_list=ho.LAYERS, memo=None):
    """every box, both directions, both walks, against the oracle of grid g (not a shared one: computed here, once per box and
    direction where the caller keeps `memo` between calls on the same grid)"""
    memo = {} if memo is None else memo
    for _, box in boxes:
        for direction in ho.DIRECTIONS:
            if (box, direction) not in memo:
                memo[box, direction] = ho.heightmap(g, box, direction, ho.HEIGHT_MAX_LAYERS, True)
            full = memo[box, direction]
            for layers in layer_list:
                for flag in (False, True):
                    c = full[3].copy()
                    if not flag:
                        c["surfaces"] = 0
                        c["max_surfaces"] = 0
                    check_case(p, (full[0][:layers], full[1][:layers], full[2], c), box, direction, layers, flag)


# ---- the case list --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,g", GRIDS, ids=[k for k, _ in GRIDS])
def test_case_lists_on_the_device(name, g):
    p = resident(g)
    cases = ho.cases(g.n)
    wanted = [ho.expected(name, g, box, direction, layers, flag) for _, box, direction, layers, flag in cases]
    # a fresh upload: the mirrors are stale, no summary is read.  After a full run they are current: with the shortcuts, then without.
    for state in ("fresh", "summaries", "summaries off"):
        if state == "summaries":
            p.execute()
        shortcuts(p, state != "summaries off")
        got = {}
        for (what, box, direction, layers, flag), want in zip(cases, wanted):
            got[what, direction, layers, flag] = check_case(p, want, box, direction, layers, flag)
        for (what, direction, layers, flag), h in got.items():     # the heights are the same bytes between the two walks
            if flag:
                same(h, got[what, direction, layers, False])
    # without the materials
    for (what, box, direction, layers, flag), want in list(zip(cases, wanted))[::7]:
        h, m, s, c = p.heightmap(box, direction, layers, False, flag)
        assert m is None
        same(h, want[0]); same(c, want[3])


def test_the_largest_grid():
    n = 208
    g = mo.terrain_grid(n)
    boxes = [("the whole grid", ((0, 0, 0), (n, n, n))), ("unaligned", ((5, 7, 3), (n - 3, n - 6, n - 2)))]
    p = resident(g)
    p.execute()
    memo = {}
    for on in (True, False):
        shortcuts(p, on)
        check_grid(p, g, boxes, (1, 8), memo)


def test_every_pair_of_samples_on_the_device():
    g = ho.pairs_grid()                    # the device's integer division on all 16 384 pairs (d0, d1)
    n = g.n
    box = ((0, 0, 0), (n, n, n))
    p = resident(g)
    for direction in ho.DIRECTIONS:
        want = ho.heightmap(g, box, direction, 2, True)
        check_case(p, want, box, direction, 2, True)
    y, x = np.mgrid[0:n, 0:n]
    same(p.heightmap(box, TOP, 1, False, False)[0][0], (5 * 256 + (256 * (x + 1)) // (y + x + 1)).astype(np.uint32))


# ---- after edits: no stale summary is used ----------------------------------------------------------------------------------------

def test_after_a_carve():
    g = mo.layered_grid(48)                # its lowest block layer is all solid, its highest all air
    p = resident(g)
    p.execute()                            # the summaries are current
    boxes = ho.boxes(48)
    check_grid(p, g, boxes[:1], (2,))
    p.inject_ball((20.0, 27.0, 6.0), (20.0, 20.0, 20.0), 7.0, 2)   # into blocks that were all solid
    p.inject_ball((30.0, 20.0, 40.0), (20.0, 20.0, 20.0), 7.0, 0)   # into blocks that were all air
    after = device_grid(p)
    assert not np.array_equal(after.dist, g.dist)
    for on in (True, False):
        shortcuts(p, on)
        check_grid(p, after, [boxes[0], boxes[6]], (1, 8))


def test_after_an_island_removal_and_after_a_paste():
    d = io.floating()
    m = np.full(d.shape, 3, np.uint8)
    m[20:26] = 8
    g = uo.Grid(d, m, np.zeros(d.shape, np.uint8), io.codec_flags(d))
    p = resident(g)
    p.execute()
    boxes = ho.boxes(48)
    check_grid(p, g, boxes[:1], (8,))
    counts = p.islands(remove=True)[1]
    assert int(counts["removed"]) == 2
    after = device_grid(p)
    for on in (True, False):
        shortcuts(p, on)
        check_grid(p, after, [boxes[0], boxes[6]], (1, 8))
    stamp = sto.solid_stamp((20, 18, 17), -90, 5, 77)
    p.paste([p.upload_stamp(stamp.dist, stamp.mat, stamp.blend)], sto.pastes([((14, 15, 16), 0, 1, sto.PASTE_REPLACE), ((0, 0, 0), 0, 0, sto.PASTE_SUBTRACT)]))
    after = device_grid(p)
    for on in (True, False):
        shortcuts(p, on)
        check_grid(p, after, [boxes[0], boxes[6]], (1, 8))


# ---- the device form ----------------------------------------------------------------------------------------------------------------

def test_the_device_form_writes_the_same_bytes():
    import torch
    name, g = GRIDS[2]                     # 48^3 white noise
    p = resident(g)
    p.execute()
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    box = ((5, 7, 3), (45, 42, 46))
    w, h = 40, 35
    for direction in ho.DIRECTIONS:
        for layers, flag in ((1, False), (8, True), (2, False)):
            want = ho.expected(name, g, box, direction, layers, flag)
            host = p.heightmap(box, direction, layers, True, flag)
            dh = torch.full((layers * h * w,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
            dm = torch.full((layers * h * w,), 0x5A, dtype=torch.uint8, device="cuda:0")
            ds = torch.full((h * w,), 0x5A5A, dtype=torch.int16, device="cuda:0") if flag else None
            torch.cuda.synchronize()
            counts = p.heightmap_device(box, dh, direction, layers, dm, ds)
            same(counts, want[3]); same(counts, host[3])
            same(dh.cpu().numpy().view(np.uint32).reshape(layers, h, w), host[0])
            same(dm.cpu().numpy().reshape(layers, h, w), host[1])
            if flag:
                same(ds.cpu().numpy().view(np.uint16).reshape(h, w), host[2])
            same(host[0], want[0])
            # without counts: queued on the context's stream, not waited for
            dh.fill_(0x5A5A5A5A)
            torch.cuda.synchronize()
            assert p.heightmap_device(box, dh.data_ptr(), direction, layers, None, None if ds is None else ds.data_ptr(), counts=False) is None
            stream.synchronize()
            same(dh.cpu().numpy().view(np.uint32).reshape(layers, h, w), host[0])
    p.set_stream(0)


# ---- nothing changes ----------------------------------------------------------------------------------------------------------------

def test_nothing_changes_and_full_runs_still_replay():
    from voxels_amd import synth
    from voxels_amd.digest import digests_equal, surface_digest
    n = 64
    d, m, b = synth.terrain(n, seed=21)      # (a field whose full runs are single-stream ones: tests/test_gpu_matstore.py)
    p = new_poly()
    p.upload_packed(vxo.load_port().grid_from_dense(np.ascontiguousarray(d), m, b).pack())
    pack0, flags0 = p.pack(), device_flags(p)
    for _ in range(4):          # the first runs of a context vote, then capture; the ones behind them replay
        p.execute()
        if p.material_path_counts()[1]:
            break
    p.execute()
    digest0 = surface_digest(p.all_levels())
    plan_a = p.slot_plan_counts()
    p.execute()
    plan_b, mats = p.slot_plan_counts(), p.material_path_counts()
    step = (plan_b[0] - plan_a[0], plan_b[1] - plan_a[1])
    box = ((0, 0, 0), (n, n, n))
    first = [p.heightmap(box, direction, layers, True, flag) for direction in ho.DIRECTIONS for layers, flag in ((1, False), (8, True))]
    first.append(p.heightmap(((3, 9, 7), (50, 41, 33)), TOP, 2, True, True))
    p.execute()
    plan_c = p.slot_plan_counts()
    assert (plan_c[0] - plan_b[0], plan_c[1] - plan_b[1]) == step and p.material_path_counts() == mats, (plan_a, plan_b, plan_c)
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), flags0)
    assert digests_equal(surface_digest(p.all_levels()), digest0)
    second = [p.heightmap(box, direction, layers, True, flag) for direction in ho.DIRECTIONS for layers, flag in ((1, False), (8, True))]
    for a, b2 in zip(first, second):
        for x, y in zip(a, b2):
            same(x, y)
    g = device_grid(p)
    want = ho.heightmap(g, box, TOP, 1, False)
    same(first[0][0], want[0]); same(first[0][1], want[1]); same(first[0][3], want[3])


# ---- errors -------------------------------------------------------------------------------------------------------------------------

def test_every_listed_error_leaves_the_outputs_untouched():
    import torch
    from voxels_amd import Polygonizer
    g = GRIDS[1][1]
    p = resident(g)
    lib, h = p._lib, p._h
    good = ho.height_query(((0, 0, 0), (8, 8, 8)), "top", 2, True)
    heights = np.full(2 * 64, 0xA5A5A5A5, np.uint32)
    mats = np.full(2 * 64, 0xA5, np.uint8)
    surfaces = np.full(64, 0xA5A5, np.uint16)
    counts = np.full(48, 0xA5, np.uint8)
    dh = torch.full((2 * 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    ds = torch.full((64,), 0x5A5A, dtype=torch.int16, device="cuda:0")

    def refused(ctx, q, hp=heights.ctypes.data, sp=surfaces.ctypes.data):
        qp = None if q is None else q.ctypes.data
        assert lib.vx_grid_heightmap(ctx, qp, hp, mats.ctypes.data, sp, counts.ctypes.data) == INVALID
        dhp = None if hp is None else dh.data_ptr()
        dsp = None if sp is None else ds.data_ptr()
        assert lib.vx_grid_heightmap_device(ctx, qp, dhp, None, dsp, counts.ctypes.data) == INVALID
        assert lib.vx_grid_heightmap_device(ctx, qp, dhp, None, dsp, None) == INVALID

    def changed(**fields):
        q = good.copy()
        for k, v in fields.items():
            q[k] = v
        return q

    refused(None, good)
    refused(h, None)
    refused(h, good, hp=None)
    for lo, hi in (((4, 4, 4), (4, 8, 8)), ((0, 0, 0), (49, 8, 8)), ((0, 9, 0), (8, 8, 8)), ((0, 0, 48), (1, 1, 49))):
        q = good.copy()
        q["box"]["lo"], q["box"]["hi"] = lo, hi
        refused(h, q)
    refused(h, changed(direction=2))
    refused(h, changed(layers=0))
    refused(h, changed(layers=ho.HEIGHT_MAX_LAYERS + 1))
    refused(h, changed(flags=3))
    refused(h, changed(reserved=[0, 0, 1]))
    refused(h, changed(flags=0))                                   # a surfaces array without the flag
    bare = Polygonizer(device=0)                                   # owns no grid
    refused(bare._h, good)
    assert lib.vx_grid_heightmap_device(h, good.ctypes.data, dh.data_ptr() + 2, None, None, None) == INVALID       # misaligned
    torch.cuda.synchronize()
    assert (heights == 0xA5A5A5A5).all() and (mats == 0xA5).all() and (surfaces == 0xA5A5).all() and (counts == 0xA5).all()
    assert (dh.cpu().numpy() == 0x5A5A5A5A).all() and (ds.cpu().numpy() == 0x5A5A).all()
    assert lib.vx_grid_heightmap(h, good.ctypes.data, heights.ctypes.data, mats.ctypes.data, surfaces.ctypes.data, counts.ctypes.data) == 0
    want = ho.heightmap(g, ((0, 0, 0), (8, 8, 8)), TOP, 2, True)
    same(heights.reshape(2, 8, 8), want[0]); same(counts.view(ho.HEIGHT_COUNTS_DTYPE)[0], want[3])


# ---- the life of the working memory -------------------------------------------------------------------------------------------------

def test_working_memory_small_regrown_small_and_a_second_context():
    name, g = GRIDS[2]                     # 48^3 white noise
    p, fresh = resident(g), resident(g)
    small, large = ((7, 9, 5), (8, 10, 6)), ((0, 0, 0), (48, 48, 48))

    def call(q, box, layers):
        return q.heightmap(box, TOP, layers, True, True)

    first, big, third = call(p, small, 1), call(p, large, 8), call(p, small, 1)
    for a, b in zip(first, third):
        same(a, b)
    for a, b in zip(big, call(fresh, large, 8)):
        same(a, b)
    want = ho.expected(name, g, large, TOP, 8, True)
    same(big[0], want[0]); same(big[3], want[3])
    assert int(big[3]["max_surfaces"]) > 8
    p.close()                              # with live state
    again = call(fresh, small, 1)
    for a, b in zip(first, again):
        same(a, b)
    fresh.close()
    q = new_poly()                         # a context no module touched but the debug switch
    shortcuts(q, False)
    q.close()
