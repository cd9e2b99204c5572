"""The index pool kept across full runs (vx_index_keep_counts): a full run that keeps the mesh layout
(tests/test_gpu_layout.py) finds every index it would store in the pool already - an index is a vertex base of the kept layout
plus an ordinal that follows from the signs and material ids of the unchanged grid - so its table-driven bodies write no
triangle descriptor, run no triangle lane and store no index (MainPlan::layout 2; VX_KEEP_INDICES=1, the default).
VX_KEEP_INDICES=0 rewrites them as before (layout 1).  Vertices are computed and stored either way.

  1. chain run, assigning run, three kept runs on the zero-free fields, planes and surface-less grids of steady_fields.py: every
     run equals the oracle, the kept runs are one launch and keep the indices;
  2. the control arm, a context created under VX_KEEP_INDICES=0: the same runs rewrite the indices, and per block the pool
     contents found through vx_level_ranges are the same in both contexts;
  3. fields whose kept runs stay two launches move neither counter; a material table change between kept runs leaves one launch
     and the indices kept, and the vertices equal the oracle's under the new table;
  4. the store really is gone: index ranges zeroed behind the library's back stay zero through a kept run, and whatever drops the
     layout - vx_compact_pools, another level count, an incremental run - makes the next full run write them again;
  5. a block whose mesh needs more than one descriptor chunk (tests/index_keep_fields.py).

Every run states through vx_slot_plan_counts, vx_layout_keep_counts and vx_index_keep_counts which form it took."""
import ctypes as C

import numpy as np
import pytest

import fields
import vxo
import index_keep_fields as ikf
import steady_fields as sf
import test_gpu_cellmap as cellmap
from test_gpu_layout import HANDS_OUT, KEPT_ONE, KEPT_TWO, run, run_equals, same_tables, tables, warm
from test_gpu_matstore import make_poly
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_slotplan import reported
from voxels_amd.binding import VERTEX_DTYPE

pytestmark = pytest.mark.gpu

REWROTE, KEPT_IDX, NEITHER = (1, 0), (0, 1), (0, 0)
ONE_LAUNCH_FIELDS = sf.NOZERO + sf.PLANES + sf.NO_SURFACE + ("gentle64_one_zero_unstaged",)
TWO_LAUNCH_FIELDS = ("gentle64_one_zero_staged", "plane64_16.0")


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


@pytest.fixture(scope="module")
def control():
    p = make_poly(VX_KEEP_INDICES=0)
    yield p
    p.close()


ORACLE = {}  # (one oracle run per field, shared by the cases and left unchanged)


def field(name):
    return ikf.chunks64() if name == "chunks64" else sf.make(name)[:3]


def oracle(port, name):
    if name not in ORACLE:
        ORACLE[name] = port.execute(port.grid_from_dense(*field(name)))
    return ORACLE[name]


def upload(p, name):
    d, m, b = field(name)
    p.upload(d, m, b, cellmap.flags_of(d))


def counted(p, want, fn, *args, **kw):
    """fn(p, ...) - one call of vx_polygonize - and what its attempts did with the index pool: (rewrote, kept) by vx_index_keep_counts"""
    before = p.index_keep_counts()
    info = fn(p, *args, **kw)
    after = p.index_keep_counts()
    got = (after[0] - before[0], after[1] - before[1])
    assert got == want, "%s: layout-kept attempts that (rewrote, kept) the indices = %s, expected %s" % (kw.get("label", ""), got, want)
    return info


def sequence(p, port, name, kept, idx, compare=True):
    """chain run, assigning run, three kept runs of the form `kept` that do `idx` with the index pool"""
    s = oracle(port, name)
    upload(p, name)
    p.forget_hints()
    step = (lambda q, expect, label: run_equals(q, s, expect, label=label)) if compare else (lambda q, expect, label: run(q, expect, label=label))
    layout0, index0 = p.layout_keep_counts(), p.index_keep_counts()
    counted(p, NEITHER, step, HANDS_OUT, label=name + ", chain of launches")
    first = counted(p, NEITHER, step, HANDS_OUT, label=name + ", assigning")
    before = tables(p, first)
    for k in range(3):
        info = counted(p, idx, step, kept, label="%s, kept run %d" % (name, k))
        assert reported(info) == reported(first), "%s, kept run %d" % (name, k)
        now = tables(p, info)
        if kept == KEPT_ONE:
            assert same_tables(now, before), "%s, kept run %d: tables or pool ranges differ from the run before" % (name, k)
        before = now
    layout1, index1 = p.layout_keep_counts(), p.index_keep_counts()
    # (as tests/test_gpu_steady.py expects: three kept attempts, all of one form)
    assert (layout1[0] - layout0[0], layout1[1] - layout0[1]) == ((0, 3) if kept == KEPT_ONE else (3, 0)), name
    assert (index1[0] - index0[0], index1[1] - index0[1]) == tuple(3 * x for x in idx), name
    return first


# ---- the pools as a renderer sees them: through the HIP runtime the library itself is linked against -------------------------------
def runtime(p):
    """the HIP runtime entry points, bound with ctypes as tests/ipc_reader.py binds them - looked up through the library's own handle,
    so that they are the runtime whose pointers vx_device_meshes hands out"""
    rt = p._lib
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return rt


def pools(p):
    """host copies of both pools (vertices, indices) up to the run's cursors"""
    rt = runtime(p)
    dv, di, nv, ni = p.device_meshes()
    verts, idx = np.zeros(nv, VERTEX_DTYPE), np.zeros(ni, np.uint32)
    assert rt.hipDeviceSynchronize() == 0
    if nv:
        assert rt.hipMemcpy(verts.ctypes.data_as(C.c_void_p), C.c_void_p(dv), nv * VERTEX_DTYPE.itemsize, 2) == 0
    if ni:
        assert rt.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(di), ni * 4, 2) == 0
    return verts, idx


def block_contents(p, info):
    """per level and block (download order): the bytes of its regular vertices and indices and of its six transition meshes, cut out
    of the pools at the offsets of vx_level_ranges"""
    verts, idx = pools(p)
    out = []
    for l in range(int(info.levels)):
        infos, ranges = p.level(l, with_data=False).infos, p.level_ranges(l)
        blocks = []
        for i, r in zip(infos, ranges):
            parts = [verts[r["v_off"]:r["v_off"] + i["n_verts"]].tobytes(), idx[r["i_off"]:r["i_off"] + i["n_idx"]].tobytes()]
            assert len(parts[0]) == int(i["n_verts"]) * VERTEX_DTYPE.itemsize and len(parts[1]) == int(i["n_idx"]) * 4
            for f in range(6):
                parts.append(verts[r["tv_off"][f]:r["tv_off"][f] + i["n_tverts"][f]].tobytes())
                parts.append(idx[r["ti_off"][f]:r["ti_off"][f] + i["n_tidx"][f]].tobytes())
                assert len(parts[-2]) == int(i["n_tverts"][f]) * VERTEX_DTYPE.itemsize and len(parts[-1]) == int(i["n_tidx"][f]) * 4
            blocks.append((int(i["id"]), tuple(parts)))
        out.append(blocks)
    return out


# ---- 1. kept runs against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_LAUNCH_FIELDS)
def test_kept_runs_keep_the_indices_and_equal_the_oracle(poly, port, name):
    assert sf.FIELDS[name][1] == KEPT_ONE
    first = sequence(poly, port, name, KEPT_ONE, KEPT_IDX)
    if name == "gentle128_nozero":
        assert int(first.levels) == 4 and all(int(first.active_blocks[l]) > 0 for l in range(4))  # (planes from a lattice copy: mult 4)


# ---- 2. the control arm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_LAUNCH_FIELDS)
def test_control_arm_rewrites_the_indices_and_leaves_the_same_pools(poly, control, port, name):
    a = sequence(control, port, name, KEPT_ONE, REWROTE)
    c = sequence(poly, port, name, KEPT_ONE, KEPT_IDX, compare=False)
    assert reported(a) == reported(c) and np.array_equal(poly.stats(), control.stats())
    mine, theirs = block_contents(poly, c), block_contents(control, a)
    assert len(mine) == len(theirs) == int(a.levels)
    for l, (x, y) in enumerate(zip(mine, theirs)):
        assert [b[0] for b in x] == [b[0] for b in y], "%s L%d: block lists differ" % (name, l)
        for (bid, px), (_, py) in zip(x, y):
            assert px == py, "%s L%d block %d: pool contents differ between VX_KEEP_INDICES=1 and 0" % (name, l, bid)
    # (something was compared: regular indices wherever there is a surface, transition indices where a level below the last has
    # active blocks on every face - gentle48's two levels have none: its one level-1 block is the last level's)
    assert any(len(parts[1]) for blocks in mine for _, parts in blocks) == (name not in sf.NO_SURFACE)
    if name in ("gentle64_nozero", "gentle128_nozero"):
        assert any(len(parts[3 + 2 * f]) for blocks in mine for _, parts in blocks for f in range(6))


# ---- 3. the kept form of two launches, and a material table change ------------------------------------------------------------------
@pytest.mark.parametrize("name", TWO_LAUNCH_FIELDS)
def test_runs_of_two_launches_move_neither_counter(poly, port, name):
    assert sf.FIELDS[name][1] == KEPT_TWO
    sequence(poly, port, name, KEPT_TWO, NEITHER)


def test_material_table_change_keeps_one_launch_and_the_indices(poly, port):
    name = "gentle64_nozero"
    d, m, b = field(name)
    lut = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
    assert not np.array_equal(lut, vxo.default_lut())
    try:
        upload(poly, name)
        warm(poly)
        info = counted(poly, KEPT_IDX, run_equals, oracle(port, name), KEPT_ONE, label="default table")
        before = tables(poly, info)
        old_idx = pools(poly)[1]
        old_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        poly.set_materials(lut)
        s = port.execute(port.grid_from_dense(d, m, b), lut=lut)
        # (surface_equal compares every vertex, texture bytes included, and every index)
        info = counted(poly, KEPT_IDX, run_equals, s, KEPT_ONE, label="behind vx_material_lut")
        assert same_tables(tables(poly, info), before)
        assert np.array_equal(pools(poly)[1], old_idx)
        new_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        for li, (x, y) in enumerate(zip(old_tex, new_tex)):  # (same vertices, other ids: the run did compute and store them)
            assert x.shape == y.shape and x.size and not np.array_equal(x, y), "L%d: the run returned the old texture ids" % li
        counted(poly, KEPT_IDX, run_equals, s, KEPT_ONE, label="second run behind vx_material_lut")
    finally:
        poly.set_materials(vxo.default_lut())


# ---- 4. the store really is gone ----------------------------------------------------------------------------------------------------
def index_ranges(p, info):
    """(first index, count) of the regular mesh of one block of every level and of one non-empty transition face, inside the pool"""
    ni = p.device_meshes()[3]
    out, face = [], None
    for l in range(int(info.levels)):
        infos, ranges = p.level(l, with_data=False).infos, p.level_ranges(l)
        k = int(np.argmax(infos["n_idx"]))
        assert infos["n_idx"][k] > 0, "L%d has no regular mesh" % l
        out.append((int(ranges["i_off"][k]), int(infos["n_idx"][k])))
        if face is None and infos["n_tidx"].any():
            k, f = [int(x) for x in np.argwhere(infos["n_tidx"] > 0)[0]]
            face = (int(ranges["ti_off"][k][f]), int(infos["n_tidx"][k][f]))
    assert face is not None, "no transition face with a mesh"
    out.append(face)
    assert all(0 <= off and cnt > 0 and off + cnt <= ni for off, cnt in out), (out, ni)
    return out


def zero_ranges(p, ranges):
    rt = runtime(p)
    di = p.device_meshes()[1]
    assert rt.hipDeviceSynchronize() == 0
    for off, cnt in ranges:
        assert rt.hipMemset(C.c_void_p(di + 4 * off), 0, 4 * cnt) == 0
    assert rt.hipDeviceSynchronize() == 0


def ranges_are_zero(p, ranges):
    idx = pools(p)[1]
    return [not idx[off:off + cnt].any() for off, cnt in ranges]


def test_zeroed_index_ranges_stay_zero_until_the_layout_is_dropped(poly, port):
    name = "gentle64_nozero"
    s = oracle(port, name)
    upload(poly, name)
    warm(poly)

    def kept_run_leaves_zeros(label):
        """a kept run, zeros into the pool, another kept run: the zeros are still there (and nothing else has changed)"""
        info = counted(poly, KEPT_IDX, run_equals, s, KEPT_ONE, label="kept run, " + label)
        ranges = index_ranges(poly, info)
        assert len(ranges) == int(info.levels) + 1 == 4
        assert not any(ranges_are_zero(poly, ranges)), "a mesh of zeros only"
        zero_ranges(poly, ranges)
        again = counted(poly, KEPT_IDX, run, KEPT_ONE, label="kept run over the zeroed ranges, " + label)
        assert reported(again) == reported(info) and same_tables(tables(poly, again), tables(poly, info))
        assert all(ranges_are_zero(poly, ranges)), "%s: a run that keeps the indices stored into the pool" % label
        # (the vertices are the run's own, as ever)
        got, want = poly.all_levels(), s.all_levels()
        for lv, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g.infos, w.infos) and len(g.idx) == len(w.idx) and not np.array_equal(g.idx, w.idx), "L%d" % lv

    kept_run_leaves_zeros("first")
    poly.compact_pools()
    counted(poly, NEITHER, run_equals, s, KEPT_TWO, label="first run behind vx_compact_pools")
    kept_run_leaves_zeros("behind vx_compact_pools")
    counted(poly, NEITHER, run_equals, s, HANDS_OUT, 2, label="two levels")
    counted(poly, NEITHER, run_equals, s, HANDS_OUT, label="all levels again")
    kept_run_leaves_zeros("behind a changed level count")
    box = poly.inject_ball(*cellmap.BALL)
    poly.execute_dirty(*box)
    g = port.grid_load(poly.pack())
    assert not np.array_equal(g.read_dense()[0], field(name)[0])
    counted(poly, NEITHER, run_equals, port.execute(g), HANDS_OUT, label="full run behind an incremental one")


# ---- 5. more than one descriptor chunk ----------------------------------------------------------------------------------------------
def test_block_with_more_than_one_descriptor_chunk(poly, control, port):
    name = "chunks64"
    s = oracle(port, name)
    info0 = s.all_levels()[0].infos
    assert len(info0) == 1 and int(info0[0]["n_verts"]) > ikf.F0_VDESC and int(info0[0]["n_idx"]) // 3 > ikf.F0_TDESC
    c = sequence(poly, port, name, KEPT_ONE, KEPT_IDX)
    a = sequence(control, port, name, KEPT_ONE, REWROTE)
    assert reported(a) == reported(c)
    mine, theirs = block_contents(poly, c), block_contents(control, a)
    assert mine == theirs
    # ... and the second chunk's triangles are not there because a run just wrote them: zeroed, they stay zero
    ranges = index_ranges_regular(poly, c)
    zero_ranges(poly, ranges)
    counted(poly, KEPT_IDX, run, KEPT_ONE, label="kept run over the zeroed ranges")
    assert all(ranges_are_zero(poly, ranges))
    poly.compact_pools()
    counted(poly, NEITHER, run_equals, s, KEPT_TWO, label="first run behind vx_compact_pools")


def index_ranges_regular(p, info):
    ni = p.device_meshes()[3]
    out = []
    for l in range(int(info.levels)):
        infos, ranges = p.level(l, with_data=False).infos, p.level_ranges(l)
        out += [(int(r["i_off"]), int(i["n_idx"])) for i, r in zip(infos, ranges) if i["n_idx"]]
    assert out and all(off + cnt <= ni for off, cnt in out)
    return out
