"""The geometry of the regular vertices kept across full runs (vx_geometry_keep_counts): a full run that keeps the
mesh layout (tests/test_gpu_layout.py) finds bytes 0..39 of every regular vertex - position, secondary position, secW, normal:
functions of the unchanged grid - in the pool already, so f0_walk and f1_block compute and store the texture bytes alone, bytes
40..47, the one part of a vertex the material table enters (MainPlan::geometry 1; VX_KEEP_GEOMETRY=1, the default).
VX_KEEP_GEOMETRY=0 computes and stores whole vertices as before.  Transition vertices are written whole either way.

  1. chain run, assigning run, three kept runs on the one-launch fields of steady_fields.py: every run equals the oracle in all 48
     bytes, the kept runs report "texture bytes only"; the two-launch fields move neither counter;
  2. the control arm, a context created under VX_KEEP_GEOMETRY=0: the same runs report "whole vertices", and per block the pool
     contents found through vx_level_ranges are the same in both contexts;
  3. table changes between kept runs, default -> permuted -> a table with invalid rows -> default: one launch each, every vertex
     equals the oracle's under that table, the blend byte is back where a row is valid again, and pos, sec, secW and nrm are the
     bytes of the run before;
  4. the store really is gone: bytes 0..39 of regular vertices overwritten behind the library's back keep the pattern through a
     kept run while bytes 40..47 are the oracle's again, a transition range is whole again, and whatever drops the layout -
     vx_compact_pools, another level count, an incremental run - makes the next full run equal the oracle in every byte;
  5. chunks64, the block whose vertices need more than one descriptor chunk, through 1 and 4.

Every run states through vx_slot_plan_counts, vx_layout_keep_counts and vx_geometry_keep_counts which form it took."""
import ctypes as C

import numpy as np
import pytest

import fields
import vxo
import index_keep_fields as ikf
import steady_fields as sf
import test_gpu_cellmap as cellmap
from test_gpu_index_keep import ONE_LAUNCH_FIELDS, TWO_LAUNCH_FIELDS, block_contents, field, oracle, pools, runtime, upload
from test_gpu_layout import HANDS_OUT, KEPT_ONE, KEPT_TWO, run, run_equals, same_tables, tables, warm
from test_gpu_matstore import make_poly
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_slotplan import reported
from voxels_amd.binding import VERTEX_DTYPE

pytestmark = pytest.mark.gpu

WHOLE, TEX_ONLY, NEITHER = (1, 0), (0, 1), (0, 0)
GEOMETRY = ("pos", "sec", "nrm")  # (VERTEX_DTYPE: sec has four components, the fourth is secW)
INVALID_IDS = (1, 5)  # two of the ids of matstore.mixed_materials {0, 1, 2, 5, 9}
PATTERN_GEOMETRY, PATTERN_TEX = 0xA5, 0x5A  # (0xA5A5A5A5 as a float is about -2.9e-16, as secW it has bits no flag has; no id is 0x5A under these tables)


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


@pytest.fixture(scope="module")
def control():
    p = make_poly(VX_KEEP_GEOMETRY=0)
    yield p
    p.close()


def counted(p, want, fn, *args, **kw):
    """fn(p, ...) - one call of vx_polygonize - and what its attempts did with the regular vertices: (whole, texture bytes only) by
    vx_geometry_keep_counts"""
    before = p.geometry_keep_counts()
    info = fn(p, *args, **kw)
    after = p.geometry_keep_counts()
    got = (after[0] - before[0], after[1] - before[1])
    assert got == want, "%s: layout-kept attempts that stored (whole vertices, texture bytes only) = %s, expected %s" % (kw.get("label", ""), got, want)
    return info


def sequence(p, port, name, kept, geo, compare=True):
    """chain run, assigning run, three kept runs of the form `kept` that do `geo` with the regular vertices"""
    s = oracle(port, name)
    upload(p, name)
    p.forget_hints()
    step = (lambda q, expect, label: run_equals(q, s, expect, label=label)) if compare else (lambda q, expect, label: run(q, expect, label=label))
    layout0, geo0 = p.layout_keep_counts(), p.geometry_keep_counts()
    counted(p, NEITHER, step, HANDS_OUT, label=name + ", chain of launches")
    first = counted(p, NEITHER, step, HANDS_OUT, label=name + ", assigning")
    before = tables(p, first)
    for k in range(3):
        info = counted(p, geo, step, kept, label="%s, kept run %d" % (name, k))
        assert reported(info) == reported(first), "%s, kept run %d" % (name, k)
        now = tables(p, info)
        if kept == KEPT_ONE:
            assert same_tables(now, before), "%s, kept run %d: tables or pool ranges differ from the run before" % (name, k)
        before = now
    layout1, geo1 = p.layout_keep_counts(), p.geometry_keep_counts()
    assert (layout1[0] - layout0[0], layout1[1] - layout0[1]) == ((0, 3) if kept == KEPT_ONE else (3, 0)), name
    assert (geo1[0] - geo0[0], geo1[1] - geo0[1]) == tuple(3 * x for x in geo), name
    return first


def exact(p, s, label):
    """every vertex of every level equals the oracle's in all 48 bytes (run_equals compares the normals within parity.NRM_TOL:
    here the bytes themselves, the normals' too - the device forms are the oracle's arithmetic, vx_selftest)"""
    got, want = p.all_levels(), s.all_levels()
    assert len(got) == len(want), label
    for l, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g.infos, w.infos), "%s L%d: block tables" % (label, l)
        for part in ("verts", "tverts"):
            a, b = getattr(g, part), getattr(w, part)
            assert a.dtype == b.dtype and a.dtype.itemsize == 48
            assert a.tobytes() == b.tobytes(), "%s L%d %s: differs from the oracle in %s" % (label, l, part, [f for f in a.dtype.names if a[f].tobytes() != b[f].tobytes()])
        assert np.array_equal(g.idx, w.idx) and np.array_equal(g.tidx, w.tidx), "%s L%d: indices" % (label, l)


# ---- 1. kept runs against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_LAUNCH_FIELDS)
def test_kept_runs_store_texture_bytes_only_and_equal_the_oracle(poly, port, name):
    assert sf.FIELDS[name][1] == KEPT_ONE
    first = sequence(poly, port, name, KEPT_ONE, TEX_ONLY)
    exact(poly, oracle(port, name), name + ", third kept run")
    if name == "gentle128_nozero":
        assert int(first.levels) == 4 and all(int(first.active_blocks[l]) > 0 for l in range(4))  # (chains of three steps)


@pytest.mark.parametrize("name", TWO_LAUNCH_FIELDS)
def test_runs_of_two_launches_move_neither_counter(poly, port, name):
    assert sf.FIELDS[name][1] == KEPT_TWO
    sequence(poly, port, name, KEPT_TWO, NEITHER)


# ---- 2. the control arm -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ONE_LAUNCH_FIELDS)
def test_control_arm_stores_whole_vertices_and_leaves_the_same_pools(poly, control, port, name):
    a = sequence(control, port, name, KEPT_ONE, WHOLE)
    c = sequence(poly, port, name, KEPT_ONE, TEX_ONLY, compare=False)
    assert reported(a) == reported(c) and np.array_equal(poly.stats(), control.stats())
    mine, theirs = block_contents(poly, c), block_contents(control, a)
    assert len(mine) == len(theirs) == int(a.levels)
    for l, (x, y) in enumerate(zip(mine, theirs)):
        assert [b[0] for b in x] == [b[0] for b in y], "%s L%d: block lists differ" % (name, l)
        for (bid, px), (_, py) in zip(x, y):
            assert px == py, "%s L%d block %d: pool contents differ between VX_KEEP_GEOMETRY=1 and 0" % (name, l, bid)
    assert any(len(parts[0]) for blocks in mine for _, parts in blocks) == (name not in sf.NO_SURFACE)


# ---- 3. table changes between kept runs ---------------------------------------------------------------------------------------------
def test_table_changes_between_kept_runs_rewrite_the_texture_bytes_alone(poly, port):
    name = "gentle64_nozero"
    d, m, b = field(name)
    default = vxo.default_lut()
    permuted = ((default.astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
    assert not np.array_equal(permuted, default)
    valid = np.ones(256, np.uint8)
    valid[list(INVALID_IDS)] = 0
    steps = [("permuted", permuted, None), ("invalid rows", default, valid), ("default again", default, None)]
    try:
        upload(poly, name)
        warm(poly)
        info = counted(poly, TEX_ONLY, run_equals, oracle(port, name), KEPT_ONE, label="default table")
        exact(poly, oracle(port, name), "default table")
        before = tables(poly, info)
        first = last = [np.array(lv.verts) for lv in poly.all_levels()]
        first_t = last_t = [np.array(lv.tverts) for lv in poly.all_levels()]
        for label, lut, ok in steps:
            poly.set_materials(lut, ok)
            s = port.execute(port.grid_from_dense(d, m, b), lut=lut, valid=ok)
            info = counted(poly, TEX_ONLY, run_equals, s, KEPT_ONE, label=label)
            exact(poly, s, label)
            assert same_tables(tables(poly, info), before), label
            now, now_t = [np.array(lv.verts) for lv in poly.all_levels()], [np.array(lv.tverts) for lv in poly.all_levels()]
            for li, (x, y) in enumerate(zip(last, now)):
                assert x.shape == y.shape and x.size
                for f in GEOMETRY:
                    assert x[f].tobytes() == y[f].tobytes(), "%s L%d: %s changed with the table" % (label, li, f)
                if label != "default again":
                    assert not np.array_equal(x["tex"], y["tex"]), "%s L%d: the run returned the old texture bytes" % (label, li)
            for li, (x, y) in enumerate(zip(last_t, now_t)):
                for f in GEOMETRY:
                    assert x[f].tobytes() == y[f].tobytes(), "%s L%d: %s of the transition vertices changed with the table" % (label, li, f)
            if label == "invalid rows":  # (an invalid row forces all eight bytes to 0, the blend byte too)
                zeroed = [(v["tex"] == 0).all(axis=1) for v in now]
                assert all(z.any() and not z.all() for z in zeroed)
                assert all(f["tex"][z][:, 1].any() for f, z in zip(first, zeroed)), "no vertex of an invalid row had a blend"
            last, last_t = now, now_t
        # the blend byte is back where a row is valid again - with every other byte
        for li, (x, y) in enumerate(zip(first, last)):
            assert x.tobytes() == y.tobytes(), "L%d: the vertices under the default table differ from those four runs earlier" % li
        for li, (x, y) in enumerate(zip(first_t, last_t)):
            assert x.tobytes() == y.tobytes(), "L%d: transition vertices" % li
    finally:
        poly.set_materials(vxo.default_lut())


# ---- 4. the store really is gone ----------------------------------------------------------------------------------------------------
def vertex_ranges(p, info, every_block=False):
    """(first vertex, count) of the regular vertices of one block of every level (or of every block), and of one non-empty
    transition face (None where there is none), inside the pool"""
    nv = p.device_meshes()[2]
    regular, face = [], None
    for l in range(int(info.levels)):
        infos, ranges = p.level(l, with_data=False).infos, p.level_ranges(l)
        if every_block:
            regular += [(int(r["v_off"]), int(i["n_verts"])) for i, r in zip(infos, ranges) if i["n_verts"]]
        else:
            k = int(np.argmax(infos["n_verts"]))
            assert infos["n_verts"][k] > 0, "L%d has no regular mesh" % l
            regular.append((int(ranges["v_off"][k]), int(infos["n_verts"][k])))
        if face is None and infos["n_tverts"].any():
            k, f = [int(x) for x in np.argwhere(infos["n_tverts"] > 0)[0]]
            face = (int(ranges["tv_off"][k][f]), int(infos["n_tverts"][k][f]))
    assert regular and all(0 <= off and cnt > 0 and off + cnt <= nv for off, cnt in regular + ([face] if face else [])), (regular, face, nv)
    return regular, face


def overwrite(p, ranges):
    """bytes 0..39 of every vertex of the ranges <- PATTERN_GEOMETRY, bytes 40..47 <- PATTERN_TEX, through the HIP runtime"""
    rt = runtime(p)
    dv = p.device_meshes()[0]
    size = VERTEX_DTYPE.itemsize
    assert size == 48 and rt.hipDeviceSynchronize() == 0
    for off, cnt in ranges:
        img = np.full((cnt, size), PATTERN_GEOMETRY, np.uint8)
        img[:, 40:] = PATTERN_TEX
        assert rt.hipMemcpy(C.c_void_p(dv + size * off), img.ctypes.data_as(C.c_void_p), size * cnt, 1) == 0
    assert rt.hipDeviceSynchronize() == 0


def raw(p, rng):
    off, cnt = rng
    return pools(p)[0][off:off + cnt].view(np.uint8).reshape(cnt, VERTEX_DTYPE.itemsize)


def kept_run_leaves_the_pattern(p, s, label, every_block=False):
    """a kept run, the patterns into the pool, another kept run: bytes 0..39 of the regular ranges still hold the pattern, their
    bytes 40..47 are the run's, and the transition range is whole again"""
    info = counted(p, TEX_ONLY, run_equals, s, KEPT_ONE, label="kept run, " + label)
    exact(p, s, "kept run, " + label)
    regular, face = vertex_ranges(p, info, every_block)
    clean = [raw(p, r).copy() for r in regular + ([face] if face else [])]
    assert not any((c[:, :40] == PATTERN_GEOMETRY).all() or (c[:, 40:] == PATTERN_TEX).all(axis=1).any() for c in clean), "a vertex of the pattern"
    overwrite(p, regular + ([face] if face else []))
    again = counted(p, TEX_ONLY, run, KEPT_ONE, label="kept run over the overwritten ranges, " + label)
    assert reported(again) == reported(info) and same_tables(tables(p, again), tables(p, info))
    for r, c in zip(regular, clean):
        now = raw(p, r)
        assert (now[:, :40] == PATTERN_GEOMETRY).all(), "%s: a run that keeps the geometry stored into bytes 0..39 of a regular vertex" % label
        assert np.array_equal(now[:, 40:], c[:, 40:]), "%s: the texture bytes of a regular range are not the run's" % label
    if face:
        assert np.array_equal(raw(p, face), clean[-1]), "%s: the transition range is not whole again" % label
    return face


def test_overwritten_geometry_stays_until_the_layout_is_dropped(poly, port):
    name = "gentle64_nozero"
    s = oracle(port, name)
    upload(poly, name)
    warm(poly)
    assert kept_run_leaves_the_pattern(poly, s, "first") is not None
    poly.compact_pools()
    counted(poly, NEITHER, run_equals, s, KEPT_TWO, label="first run behind vx_compact_pools")
    exact(poly, s, "first run behind vx_compact_pools")
    kept_run_leaves_the_pattern(poly, s, "behind vx_compact_pools")
    counted(poly, NEITHER, run_equals, s, HANDS_OUT, 2, label="two levels")
    counted(poly, NEITHER, run_equals, s, HANDS_OUT, label="all levels again")
    exact(poly, s, "all levels again")
    kept_run_leaves_the_pattern(poly, s, "behind a changed level count")
    box = poly.inject_ball(*cellmap.BALL)
    poly.execute_dirty(*box)
    g = port.grid_load(poly.pack())
    assert not np.array_equal(g.read_dense()[0], field(name)[0])
    after = port.execute(g)
    counted(poly, NEITHER, run_equals, after, HANDS_OUT, label="full run behind an incremental one")
    exact(poly, after, "full run behind an incremental one")


# ---- 5. more than one descriptor chunk ----------------------------------------------------------------------------------------------
def test_block_with_more_than_one_descriptor_chunk(poly, control, port):
    name = "chunks64"
    s = oracle(port, name)
    info0 = s.all_levels()[0].infos
    assert len(info0) == 1 and int(info0[0]["n_verts"]) > ikf.F0_VDESC
    c = sequence(poly, port, name, KEPT_ONE, TEX_ONLY)
    exact(poly, s, name)
    a = sequence(control, port, name, KEPT_ONE, WHOLE)
    assert reported(a) == reported(c)
    assert block_contents(poly, c) == block_contents(control, a)
    # ... and the second chunk's geometry is not there because a run just wrote it
    kept_run_leaves_the_pattern(poly, s, name, every_block=True)
    poly.compact_pools()
    counted(poly, NEITHER, run_equals, s, KEPT_TWO, label="first run behind vx_compact_pools")
    exact(poly, s, "first run behind vx_compact_pools")
