"""The steady-state full run against the oracle, on the fields of tests/steady_fields.py: a context that polygonizes the same
grid again and again keeps the slot plan, leaves the material caches in their slots and keeps the mesh layout - one launch of
k_main, whose blocks take their pool ranges from the records an earlier run left and whose last workgroup writes the header's
cursors and list totals from host copies (tests/test_gpu_layout.py has the mechanics on height fields).  Here
the form runs on what stresses the table-driven bodies: full-range noise without an exact zero under random materials (every
transition face, non-trivial votes, odd block counts per edge, four levels), axis-aligned planes, one zero that is staged and
one that is not, grids without a surface and the single-block grid.

  1. per field: chain of launches, assigning run, then three kept runs of the form steady_fields.py expects - every run equals
     the oracle, reports what the assigning run reported, and a one-launch run returns the tables and pool ranges of the run
     before;
  2. level limits on four levels: 1, 2, 3 and all, in turn;
  3. VX_LAYOUT=1 against VX_LAYOUT=0 and the conservative-sync library, run by run;
  4. edits that leave no zero: the run behind them hands out its slots, the runs behind that are one launch;
  5. vx_material_lut between two one-launch runs on four levels.

Every run states through vx_slot_plan_counts and vx_layout_keep_counts (test_gpu_layout.run) which form it took, so nothing
passes because a run fell back.  The premises of the fields are checked in numpy by tests/test_steady_fields.py."""
import os

import numpy as np
import pytest

import fields
import vxo
import steady_fields as sf
import test_gpu_cellmap as cellmap
from test_gpu_layout import HANDS_OUT, KEPT_ONE, KEPT_TWO, hands_on, run, run_equals, same_tables, tables, warm
from test_gpu_matstore import make_poly
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_slotplan import reported

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


ORACLE = {}  # (one oracle run per field, shared by the cases and left unchanged)


def oracle(port, name):
    if name not in ORACLE:
        d, m, b, _ = sf.make(name)
        ORACLE[name] = port.execute(port.grid_from_dense(d, m, b))
    return ORACLE[name]


def upload(p, name):
    d, m, b, kept = sf.make(name)
    p.upload(d, m, b, cellmap.flags_of(d))
    return kept


def kept_runs(p, s, first, before, kept, levels, label, count=3):
    """`count` kept runs of the form `kept` behind the run `first`, whose tables were `before`"""
    for k in range(count):
        info = run_equals(p, s, kept, levels, "%s, kept run %d" % (label, k))
        assert reported(info) == reported(first), "%s, kept run %d: %s vs %s" % (label, k, reported(info), reported(first))
        now = tables(p, info)
        if kept == KEPT_ONE:
            assert same_tables(now, before), "%s, kept run %d: tables or pool ranges differ from the run before" % (label, k)
        else:  # (whoever reserves hands out new ranges; the tables without them stay)
            assert len(now) == len(before) and all(np.array_equal(x[0], y[0]) for x, y in zip(now, before)), "%s, kept run %d" % (label, k)
        before = now
    return before


# ---- 1. the sequence, per field ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sf.FIELDS))
def test_chain_assign_then_three_kept_runs(poly, port, name):
    s = oracle(port, name)
    kept = upload(poly, name)
    d = sf.make(name)[0]
    levels = sf.level_count(d.shape[0])
    if levels > 1:
        assert kept == (KEPT_TWO if hands_on(d) else KEPT_ONE)
    else:
        assert kept == HANDS_OUT  # (one level: no single-stream run, steady_fields.py)
    poly.forget_hints()
    run_equals(poly, s, HANDS_OUT, label=name + ", chain of launches")
    first = run_equals(poly, s, HANDS_OUT, label=name + ", assigning")
    assert int(first.levels) == levels
    assert (sum(first.active_blocks) == 0) == (name in sf.NO_SURFACE)
    kept_runs(poly, s, first, tables(poly, first), kept, 0, name)


# ---- 2. level limits in steady state ------------------------------------------------------------------------------------------------
def test_level_limits_on_four_levels(poly, port):
    """levels = 1: no upper queue, and no single-stream run either (Backend::main_applies asks for more than one level): every
    run is the chain of launches and hands out its slots.  levels = 2: level 1 closes the run and still has transition cells
    (LevelDesc::hasTransitions goes by the grid's level count, not the run's).  levels = 3 and all four: the levels whose
    transition planes come from the lattice copies.  A change of the level count drops plan and layout: the run behind it
    hands out its slots, the ones behind that are one launch (test_gpu_layout.py states the same for a terrain)."""
    name = "gentle128_nozero"
    s = oracle(port, name)
    assert upload(poly, name) == KEPT_ONE
    warm(poly)
    for levels in (1, 2, 3, 0):
        label = "%s, %d levels" % (name, levels)
        first = run_equals(poly, s, HANDS_OUT, levels, label + ", first run")
        assert int(first.levels) == (levels or 4)
        kept_runs(poly, s, first, tables(poly, first), HANDS_OUT if levels == 1 else KEPT_ONE, levels, label)


# ---- 3. builds and knobs ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["VX_LAYOUT=0", "conservative"])
def test_same_bytes_with_and_without_the_layout(other):
    from voxels_amd import digest
    from voxels_amd.binding import HipLibrary
    on = make_poly(VX_LAYOUT=1)
    if other == "conservative":
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxels_amd", "csrc", "libvoxels_hip_conservative.so")
        assert os.path.exists(path), "libvoxels_hip_conservative.so missing (run __graft_entry__.build())"
        off, kept = make_poly(library=HipLibrary(path), VX_LAYOUT=1), KEPT_ONE
    else:
        off, kept = make_poly(VX_LAYOUT=0), KEPT_TWO
    try:
        for name in ("gentle64_nozero", "gentle80_nozero"):
            for p in (on, off):
                upload(p, name)
                p.forget_hints()
            last = [None, None]
            for k, (e_on, e_off) in enumerate(((HANDS_OUT, HANDS_OUT), (HANDS_OUT, HANDS_OUT), (KEPT_ONE, kept), (KEPT_ONE, kept), (KEPT_ONE, kept))):
                a = run(on, e_on, label="%s run %d, VX_LAYOUT=1" % (name, k))
                c = run(off, e_off, label="%s run %d, %s" % (name, k, other))
                assert digest.digests_equal(digest.surface_digest(on.all_levels()), digest.surface_digest(off.all_levels())), "%s run %d" % (name, k)
                assert np.array_equal(on.stats(), off.stats()) and reported(a) == reported(c), "%s run %d" % (name, k)
                for i, (p, info, e) in enumerate(((on, a, e_on), (off, c, e_off))):
                    now = tables(p, info)
                    if e == KEPT_ONE:
                        assert same_tables(now, last[i]), "%s run %d, context %d: offsets differ from the run before" % (name, k, i)
                    last[i] = now
                # (without their pool ranges the tables are the same in both contexts)
                assert all(np.array_equal(x[0], y[0]) for x, y in zip(last[0], last[1])), "%s run %d" % (name, k)
    finally:
        on.close(); off.close()


# ---- 4. edits that leave no zero ----------------------------------------------------------------------------------------------------
CUBE = (slice(28, 36),) * 3  # (across the corner shared by eight level-0 blocks)


def negated_cube(d):
    """d with the samples of CUBE negated (and clamped: -(-128) has no int8): zero-free where d is"""
    d2 = d.copy()
    d2[CUBE] = np.clip(-d[CUBE].astype(np.int16), -127, 127).astype(np.int8)
    return d2


def _edit_update_blocks(p):
    d, m, b, _ = sf.make("gentle64_nozero")
    d2 = negated_cube(d)
    ids, (dd, mm, bb) = fields.edited_blocks((d, m, b), (d2, m, b))
    assert len(ids) == 8
    p.update_blocks(ids, dd, mm, bb, cellmap.flags_of(d2))


def _edit_inject_material(p):
    p.inject_material((30.0, 33.5, 31.25), (28.0, 28.0, 28.0), 7, 1)


@pytest.mark.parametrize("what", ["update_blocks", "inject_material"])
def test_edits_that_leave_no_zero(poly, port, what):
    name = "gentle64_nozero"
    assert upload(poly, name) == KEPT_ONE
    first = warm(poly)
    before = tables(poly, run(poly, KEPT_ONE, label="before " + what))
    {"update_blocks": _edit_update_blocks, "inject_material": _edit_inject_material}[what](poly)
    g = port.grid_load(poly.pack())
    d_now, m_now, _ = g.read_dense()
    d, m, _, _ = sf.make(name)
    if what == "update_blocks":
        assert np.array_equal(d_now, negated_cube(d)) and not np.array_equal(d_now, d)
    else:
        assert np.array_equal(d_now, d) and not np.array_equal(m_now, m)
    # the premises of the one-launch form, on the grid that is resident now
    assert not (d_now == 0).any() and not hands_on(d_now)
    assert all(c.max() <= sf.LARGE_THRESHOLD for c in sf.per_level(d_now))
    s = port.execute(g)
    info = run_equals(poly, s, HANDS_OUT, label="first run behind " + what)
    if what == "update_blocks":
        assert reported(info) != reported(first), "the edit changed no mesh"
    now = tables(poly, info)
    assert what != "update_blocks" or not same_tables(now, before)
    kept_runs(poly, s, info, now, KEPT_ONE, 0, "behind " + what, count=2)


# ---- 5. the material map changes between two one-launch runs, four levels ----------------------------------------------------------------
def test_material_lut_between_one_launch_runs_on_four_levels(poly, port):
    from voxels_amd import digest
    name = "gentle128_nozero"
    d, m, b, _ = sf.make(name)
    g = port.grid_from_dense(d, m, b)
    lut = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
    assert not np.array_equal(lut, vxo.default_lut())
    fresh = make_poly()
    try:
        upload(poly, name)
        first = warm(poly)
        info = run_equals(poly, oracle(port, name), KEPT_ONE, label="default map")
        assert int(info.levels) == 4
        before = tables(poly, info)
        old_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        old_ttex = [np.array(lv.tverts["tex"]) for lv in poly.all_levels()]
        poly.set_materials(lut)
        s = port.execute(g, lut=lut)
        info = run_equals(poly, s, KEPT_ONE, label="behind vx_material_lut")  # (surface_equal compares the texture bytes of every vertex)
        assert reported(info) == reported(first) and same_tables(tables(poly, info), before)
        new_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        new_ttex = [np.array(lv.tverts["tex"]) for lv in poly.all_levels()]
        assert len(new_tex) == 4
        for li, (a, c) in enumerate(zip(old_tex, new_tex)):  # (same vertices, other ids: the run re-meshed into the same ranges)
            assert a.shape == c.shape and a.size and not np.array_equal(a, c), "L%d: the run returned the old texture ids" % li
        for li in (1, 2):  # (the levels with transition cells)
            a, c = old_ttex[li], new_ttex[li]
            assert a.shape == c.shape and a.size and not np.array_equal(a, c), "L%d: transition vertices with the old texture ids" % li
        run_equals(poly, s, KEPT_ONE, label="second run behind vx_material_lut")
        fresh.set_materials(lut)
        upload(fresh, name)
        fresh.forget_hints()
        run(fresh, HANDS_OUT, label="fresh context with the table from the start")
        assert digest.digests_equal(digest.surface_digest(poly.all_levels()), digest.surface_digest(fresh.all_levels()))
        assert np.array_equal(poly.stats(), fresh.stats())
    finally:
        poly.set_materials(vxo.default_lut())
        fresh.close()
