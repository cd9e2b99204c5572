"""The mesh layout kept across full runs (vx_layout_keep_counts): a full run in place (tests/test_gpu_inplace.py) on
slots whose last accepted run left its layout behind - every slot's record, the block lists and their totals, the pool cursors -
takes every block's pool ranges from its record, stores no record, list entry or level-0 bitmap, and is ONE launch: k_main, whose
last workgroup seeds the next run's counters and publishes the header (VX_LAYOUT=1, the default; VX_LAYOUT=0 keeps k_main | k_tail).

  1. chain run, assigning run, then kept runs: on a field without an exact zero the first kept run and every one behind it is one
     launch, equals the oracle and returns the tables, offsets and figures of the run before; a field whose blocks hold exact
     zeros hands them to the general passes, so it never leaves a layout and its kept runs stay two launches;
  2. VX_LAYOUT=1, VX_LAYOUT=0 and the conservative-sync library give the same bytes run by run.  Pool offsets are handed out in
     arrival order by whichever run reserves, so they are compared where they are defined: inside a context, against the run
     before (equal wherever the layout is kept);
  3. vx_material_lut between two one-launch runs: the run behind it is one launch and equals a context that had the table from
     the start;
  4. everything that drops the layout - each kind of grid change, an incremental run, a partial run, another level count,
     vx_compact_pools, a pool overflow inside one call: the next run is not one launch and equals the oracle, the one behind it is -
     unless the edit left an exact zero among the samples a meshed block stages (hands_on, in numpy from the resident grid): then
     the kept runs behind it are stated to be two launches;
  5. exact zeros: blocks are handed to the general passes, kept runs stay two launches and equal the oracle;
  6. 140 one-launch runs in a row (SETTLE_EVERY twice, every set of counters many times), then a LUT change, then an edit;
  7. two contexts alternating on one GPU; slabs of one grid on one GPU.

Every case states through vx_slot_plan_counts and vx_layout_keep_counts which path each run took, so that nothing passes because a
run fell back to two launches.  No case corrupts state: the miss path (a block whose totals are not its record's) is the safety
net of an unchanged grid and cannot be reached from outside."""
import os

import numpy as np
import pytest

import fields
import vxo
import test_gpu_cellmap as cellmap
import test_gpu_matstore as matstore
import test_gpu_slotplan as slotplan
from test_gpu_matstore import make_poly
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_slotplan import ASSIGN, KEPT, plan_field, oracle, reported

pytestmark = pytest.mark.gpu

NRM_TOL = slotplan.NRM_TOL
TWO, ONE = "two launches", "one launch"
HANDS_OUT = (ASSIGN, None)   # the run hands out its slots (its repeats inside the call, if any, are kept ones of two launches)
KEPT_TWO = (KEPT, TWO)       # keeps the plan; k_main | k_tail
KEPT_ONE = (KEPT, ONE)       # keeps plan and layout; k_main alone


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


def run(p, expect, levels=0, label=""):
    """one call of vx_polygonize; where its slots came from (slotplan.run) and the launches of its kept attempts"""
    plan, launches = expect
    before = p.layout_keep_counts()
    info = slotplan.run(p, plan, levels, label)
    after = p.layout_keep_counts()
    got = (after[0] - before[0], after[1] - before[1])
    attempts = 1 + int(info.retries)
    if plan == ASSIGN:
        ok = got[1] == 0 and got[0] <= int(info.retries)
    elif launches == TWO:
        ok = got == (attempts, 0)
    else:
        ok = got == (0, 1) and int(info.retries) == 0
    assert ok, "%s: kept attempts by (two launches, one) = %s with %d retries, expected %s" % (label, got, int(info.retries), expect)
    return info


def run_equals(p, s, expect, levels=0, label=""):
    """... and its surface and statistics against the oracle's surface s"""
    info = run(p, expect, levels, label)
    want = s.all_levels()
    ok, msg = fields.surface_equal(p.all_levels(), want[:levels] if levels else want, nrm_tol=NRM_TOL)
    assert ok, "%s %s vs the oracle: %s" % (label, expect, msg)
    if not levels:
        assert np.array_equal(p.stats(), s.stats()), "%s %s: stats %s vs %s" % (label, expect, p.stats(), s.stats())
    return info


def tables(p, info):
    """what a renderer addresses the pools with: per level the block table and the blocks' pool ranges"""
    return [(p.level(l, with_data=False).infos, p.level_ranges(l)) for l in range(int(info.levels))]


def same_tables(a, b):
    return len(a) == len(b) and all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def warm(p, levels=0):
    """behind an upload: the runs up to and including the one that leaves plan, store and layout"""
    p.forget_hints()
    run(p, HANDS_OUT, levels, "first run (chain of launches)")
    return run(p, HANDS_OUT, levels, "second run (single-stream: assigns, captures, leaves the layout)")


def has_exact_zero(d):
    return bool((np.asarray(d) == 0).any())


def hands_on(d):
    """Does a full single-stream run on the distance field d ([z][y][x], int8) hand a block to the general passes - so that it
    leaves no layout and its kept runs stay two launches?  In numpy, what the table-driven regular bodies decide per block: a
    block with a non-trivial cell (eight corners not of one sign; 0 counts as positive) is meshed, and it is handed on when a
    sample it stages is exactly 0.  Staged are, on level 0 (f0_deposit), the block's samples x = 0..16, y and z = -1..17, and on a
    level L >= 1 (f1_block) its 17^3 lattice samples at stride 2^L - coordinates beyond the grid clamped to its last sample.
    A zero that no meshed block stages - alone among samples of its own sign - changes nothing.  (Transition blocks with a zero on a
    plane take their general phases in place and hand nothing on.)"""
    d = np.asarray(d)
    n = d.shape[0]
    neg, zero = d < 0, d == 0
    if not zero.any():
        return False
    levels, v = 1, n >> 5
    while v:
        levels, v = levels + 1, v >> 1
    for lvl in range(levels):
        mult, cnt = 1 << lvl, (n >> 4) >> lvl
        if not cnt:
            break
        at = np.minimum(np.arange(16 * cnt + 1) * mult, n - 1)  # the level's lattice
        s = neg[np.ix_(at, at, at)].astype(np.int8)
        corners = sum(s[a:a + 16 * cnt, b:b + 16 * cnt, c:c + 16 * cnt] for a in (0, 1) for b in (0, 1) for c in (0, 1))
        meshed = ((corners > 0) & (corners < 8)).reshape(cnt, 16, cnt, 16, cnt, 16).any(axis=(1, 3, 5))
        lo, hi = (-1, 18) if lvl == 0 else (0, 17)
        for bz, by, bx in zip(*np.nonzero(meshed)):
            z = np.minimum(np.clip(np.arange(16 * bz + lo, 16 * bz + hi), 0, None) * mult, n - 1)
            y = np.minimum(np.clip(np.arange(16 * by + lo, 16 * by + hi), 0, None) * mult, n - 1)
            x = np.minimum(np.arange(16 * bx, 16 * bx + 17) * mult, n - 1)
            if zero[np.ix_(z, y, x)].any():
                return True
    return False


# ---- 1. the basic sequence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["terrain64", "terrain80", "terrain128", "gentle64_mixed"])
def test_chain_assign_then_kept_runs(poly, port, name):
    d, m, b = plan_field(name)
    s = oracle(port, name)
    # (the terrains hold no exact zero; the smooth full-range noise does, in blocks that are meshed: they go to the general passes)
    assert has_exact_zero(d) == (name == "gentle64_mixed") and hands_on(d) == (name == "gentle64_mixed")
    kept = KEPT_TWO if hands_on(d) else KEPT_ONE
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run_equals(poly, s, HANDS_OUT, label=name + ", chain of launches")
    first = run_equals(poly, s, HANDS_OUT, label=name + ", assigning")
    assert sum(first.active_blocks) > 0 and int(first.blocks_read) > 0
    last = tables(poly, first)
    for k in range(3):
        info = run_equals(poly, s, kept, label=name + ", kept run %d" % k)
        assert reported(info) == reported(first), "%s, kept run %d: %s vs %s" % (name, k, reported(info), reported(first))
        now = tables(poly, info)
        if kept == KEPT_ONE:
            assert same_tables(now, last), "%s, kept run %d: tables or pool ranges differ from the run before" % (name, k)
        else:  # (whoever reserves hands out new ranges; the tables without them stay)
            assert all(np.array_equal(x[0], y[0]) for x, y in zip(now, last)), "%s, kept run %d" % (name, k)
        last = now


# ---- 2. same bytes across builds and knobs ------------------------------------------------------------------------------------------
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
        for name in ("terrain64", "terrain80", "terrain128"):
            d, m, b = plan_field(name)
            fl = cellmap.flags_of(d)
            for p in (on, off):
                p.upload(d, m, b, fl)
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


# ---- 3. the material map changes between two one-launch runs ---------------------------------------------------------------------------
def test_material_lut_between_one_launch_runs(poly, port):
    from voxels_amd import digest
    d, _, _ = plan_field("terrain64")
    m, b = matstore.mixed_materials(64, 5)
    g = port.grid_from_dense(d, m, b)
    lut = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
    assert not np.array_equal(lut, vxo.default_lut())
    fresh = make_poly()
    try:
        poly.upload(d, m, b, cellmap.flags_of(d))
        first = warm(poly)
        info = run_equals(poly, port.execute(g), KEPT_ONE, label="default map")
        before = tables(poly, info)
        old_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        poly.set_materials(lut)
        s = port.execute(g, lut=lut)
        info = run_equals(poly, s, KEPT_ONE, label="behind vx_material_lut")  # (surface_equal compares the texture bytes of every vertex)
        assert reported(info) == reported(first) and same_tables(tables(poly, info), before)
        new_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        for li, (a, c) in enumerate(zip(old_tex, new_tex)):  # (same vertices, other ids: the run re-meshed into the same ranges)
            assert a.shape == c.shape and a.size and not np.array_equal(a, c), "L%d: the run returned the old texture ids" % li
        fresh.set_materials(lut)
        fresh.upload(d, m, b, cellmap.flags_of(d))
        fresh.forget_hints()
        run(fresh, HANDS_OUT, label="fresh context with the table from the start")
        assert digest.digests_equal(digest.surface_digest(poly.all_levels()), digest.surface_digest(fresh.all_levels()))
        assert np.array_equal(poly.stats(), fresh.stats())
    finally:
        poly.set_materials(vxo.default_lut())
        fresh.close()


# ---- 4. whatever drops the layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(matstore.MUTATIONS))
def test_layout_is_dropped_by_a_changed_grid(poly, port, what):
    d, m, b = plan_field("terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    if what == "islands_remove":
        poly.inject_ball(*matstore.FLOATING_BALL)  # (something for the removal to take away, resident before the layout is left)
    # A brush can leave samples that are exactly 0 (the ball does wherever x^2 + y^2 + z^2 = r^2 has lattice solutions; so does
    # flipping the bits of a -1).  Where a meshed block stages such a sample it goes to the general passes and the run leaves no
    # layout (case 5); a zero alone among samples of its own sign is staged by nobody and changes nothing.  Which of the two holds
    # is a function of the resident grid (hands_on), so every kept run's path is stated: one launch, or two.
    def kept_path(label):
        d_now = port.grid_load(poly.pack()).read_dense()[0]
        return d_now, (KEPT_TWO if hands_on(d_now) else KEPT_ONE)

    _, before = kept_path("before " + what)
    assert before == (KEPT_TWO if what == "islands_remove" else KEPT_ONE)  # (the floating ball's shell holds zeros beside its solid voxels)
    warm(poly)
    run(poly, before, label="before " + what)
    matstore.MUTATIONS[what](poly, port)
    d_now, kept = kept_path("behind " + what)
    if what in ("upload", "upload_packed", "create_terrain", "update_blocks_material_only", "inject_material"):
        assert not has_exact_zero(d_now) and kept == KEPT_ONE
    if what in ("inject_ball", "inject_brushes", "update_blocks"):
        assert kept == KEPT_TWO  # (zeros on the new surface)
    if what == "islands_remove":
        assert has_exact_zero(d_now) and kept == KEPT_ONE  # (the removed ball's zeros are left in the air: no block stages them)
    s = port.execute(port.grid_load(poly.pack()))
    run_equals(poly, s, HANDS_OUT, label="first run behind " + what)
    for k in range(2):
        run_equals(poly, s, kept, label="kept run %d behind %s" % (k, what))


def test_layout_is_dropped_by_flags_alone(poly, port):
    d, m, b = plan_field("terrain64")
    fl = cellmap.flags_of(d)
    assert fl.any()
    poly.upload(d, m, b, np.zeros_like(fl))
    warm(poly)
    run(poly, KEPT_ONE, label="before the flags")
    poly.update_blocks(np.zeros(0, np.uint32), None, None, None, fl)
    s = oracle(port, "terrain64")
    run_equals(poly, s, HANDS_OUT, label="first run behind the flags")
    run_equals(poly, s, KEPT_ONE, label="second run behind the flags")


def test_layout_is_dropped_by_an_incremental_run(poly, port):
    g = cellmap._terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    warm(poly)
    run(poly, KEPT_ONE, label="before the incremental run")
    # an incremental run over a box in which nothing has changed still hands out slots and appends the box's meshes to the pools
    poly.execute_dirty(np.array([16.0, 16.0, 16.0], np.float32), np.array([40.0, 40.0, 40.0], np.float32))
    s = port.execute(g)
    run_equals(poly, s, HANDS_OUT, label="full run behind the incremental one")
    run_equals(poly, s, KEPT_ONE, label="the run behind it")


def test_layout_is_dropped_by_a_partial_run(poly, port):
    d, m, b = plan_field("terrain128")
    s = oracle(port, "terrain128")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    run_equals(poly, s, KEPT_ONE, label="before the partial run")
    info = poly.execute_from(0, 1)
    assert int(info.first_meshed_level) == 1, "the run was not a partial one"
    run_equals(poly, s, HANDS_OUT, label="behind the partial run")
    run_equals(poly, s, KEPT_ONE, label="the run behind it")


def test_layout_is_dropped_by_another_level_count(poly, port):
    d, m, b = plan_field("terrain128")
    s = oracle(port, "terrain128")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    for levels, expect in ((0, KEPT_ONE), (2, HANDS_OUT), (2, KEPT_ONE), (2, KEPT_ONE), (0, HANDS_OUT), (0, KEPT_ONE)):
        run_equals(poly, s, expect, levels, "%d levels" % levels)


def test_layout_is_dropped_by_compact_pools(poly, port):
    d, m, b = plan_field("terrain64")
    s = oracle(port, "terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    run_equals(poly, s, KEPT_ONE, label="before vx_compact_pools")
    poly.compact_pools()
    run_equals(poly, s, KEPT_TWO, label="first run behind vx_compact_pools")
    run_equals(poly, s, KEPT_ONE, label="second run behind vx_compact_pools")


def test_attempt_that_overflows_leaves_no_layout_and_its_repeat_does(port):
    """VX_POOL_SLACK=64, provoked like case 9 of tests/test_gpu_slotplan.py: the first attempt of the call behind a change to a larger
    grid hands out the slots and overflows - no layout; the pools grow, the repeat keeps the plan, is two launches and is accepted - it
    leaves the layout; the call behind it is one launch."""
    from voxels_amd import synth
    p = make_poly(VX_POOL_SLACK=64)
    try:
        d, m, b = synth.terrain(32, seed=21)
        p.upload(d, m, b, cellmap.flags_of(d))
        assert p.execute().retries >= 1
        p.execute()
        d, m, b = plan_field("terrain64")
        p.upload(d, m, b, cellmap.flags_of(d))
        plan0, lay0 = p.slot_plan_counts(), p.layout_keep_counts()
        info = p.execute()
        plan1, lay1 = p.slot_plan_counts(), p.layout_keep_counts()
        assert info.retries >= 1
        assert (plan1[0] - plan0[0], plan1[1] - plan0[1]) == (1, int(info.retries)), "slots of the call's attempts"
        assert (lay1[0] - lay0[0], lay1[1] - lay0[1]) == (int(info.retries), 0), "launches of the call's kept attempts: %s -> %s" % (lay0, lay1)
        s = oracle(port, "terrain64")
        ok, msg = fields.surface_equal(p.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
        assert ok, msg
        assert np.array_equal(p.stats(), s.stats())
        before = tables(p, info)
        after = run_equals(p, s, KEPT_ONE, label="the call behind the repeated one")
        assert same_tables(tables(p, after), before)
    finally:
        p.close()


# ---- 5. exact zeros ---------------------------------------------------------------------------------------------------------------------
def test_blocks_with_exact_zeros_keep_two_launches(poly, port):
    """smooth full-range noise (fields.py): every level-0 block within the first capacity class, thousands of samples that are exactly
    0 - their blocks leave the table-driven bodies for the general passes of k_tail, which reserve in an order of their own"""
    d = fields.quantize_full_range(fields.smooth_noise(64, 16, scale=40, amp=3.0, octaves=1))
    counts = cellmap.numpy_cell_map(d)[1]
    assert counts.max() <= cellmap.LARGE_THRESHOLD
    zero_blocks = (d == 0).reshape(4, 16, 4, 16, 4, 16).any(axis=(1, 3, 5))
    assert (zero_blocks & (counts.reshape(zero_blocks.shape) > 0)).sum() > 8, "no surface block with an exact zero: nothing is handed on"
    m, b = matstore.mixed_materials(64, 5)
    s = port.execute(port.grid_from_dense(d, m, b))
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run_equals(poly, s, HANDS_OUT, label="chain of launches")
    first = run_equals(poly, s, HANDS_OUT, label="assigning")
    for k in range(3):
        info = run_equals(poly, s, KEPT_TWO, label="kept run %d" % k)
        assert reported(info) == reported(first)


# ---- 6. many runs -----------------------------------------------------------------------------------------------------------------------
def test_many_one_launch_runs_then_a_lut_change_then_an_edit(poly, port):
    from voxels_amd import digest
    g = cellmap._terrain64(port)
    s = port.execute(g)
    poly.upload(*g.read_dense(), g.block_flags())
    first = warm(poly)
    want = digest.surface_digest(poly.all_levels())
    stats = poly.stats()
    ranges = tables(poly, first)
    try:
        for k in range(140):
            if k == 0 or k == 139:
                info = run_equals(poly, s, KEPT_ONE, label="one launch %d" % k)
            else:
                info = run(poly, KEPT_ONE, label="one launch %d" % k)
            assert reported(info) == reported(first), "one launch %d" % k
            if k % 10 == 9:
                assert digest.digests_equal(digest.surface_digest(poly.all_levels()), want), "one launch %d" % k
                assert np.array_equal(poly.stats(), stats)
        assert same_tables(tables(poly, info), ranges)
        lut = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
        poly.set_materials(lut)
        run_equals(poly, port.execute(g, lut=lut), KEPT_ONE, label="behind vx_material_lut")
        poly.set_materials(vxo.default_lut())
        run_equals(poly, s, KEPT_ONE, label="the default map again")
        g.inject_ball(*cellmap.BALL)
        poly.inject_ball(*cellmap.BALL)
        s = port.execute(g)
        run_equals(poly, s, HANDS_OUT, label="first run behind the edit")
        assert hands_on(g.read_dense()[0])  # (the ball leaves zeros on the carved surface)
        run_equals(poly, s, KEPT_TWO, label="second run behind the edit")
    finally:
        poly.set_materials(vxo.default_lut())


# ---- 7. contexts and slabs --------------------------------------------------------------------------------------------------------------
def test_two_contexts_alternate(port):
    from voxels_amd import synth
    ps = [make_poly(), make_poly()]
    try:
        want = []
        for p, seed in zip(ps, (21, 22)):
            d, m, b = synth.terrain(64, seed=seed)
            assert cellmap.numpy_cell_map(d)[1].max() <= cellmap.LARGE_THRESHOLD and not has_exact_zero(d)
            want.append(port.execute(port.grid_from_dense(d, m, b)))
            p.upload(d, m, b, cellmap.flags_of(d))
            p.forget_hints()
        last = [None, None]
        for k, expect in enumerate((HANDS_OUT, HANDS_OUT, KEPT_ONE, KEPT_ONE, KEPT_ONE)):
            for i, p in enumerate(ps):
                info = run_equals(p, want[i], expect, label="context %d, run %d" % (i, k))
                now = tables(p, info)
                if expect == KEPT_ONE:
                    assert same_tables(now, last[i]), "context %d, run %d" % (i, k)
                last[i] = now
    finally:
        for p in ps:
            p.close()


@pytest.mark.parametrize("axis", ["y", "z"])
def test_two_slabs_equal_the_whole_grid(poly, axis):
    import torch
    from voxels_amd import Polygonizer, digest
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world = 128, 2
    levels = sharded_levels(n, world)
    assert levels >= 3
    d, m, b = plan_field("terrain128")
    fl = cellmap.flags_of(d)
    poly.upload(d, m, b, fl)
    warm(poly, levels)
    run(poly, KEPT_ONE, levels, "whole grid")
    whole = digest.surface_digest(poly.all_levels())
    parts = []
    try:
        for r in range(world):
            p = make_poly()
            parts.append(p)
            slab = SlabBuffers(torch, n, r, world, torch.device("cuda", 0), axis=axis)
            slab.fill_from_full(d, m, b, fl)
            p._slab = slab  # (keeps the tensors alive)
            torch.cuda.synchronize()
            slab.attach(p)
            warm(p, levels)
            run(p, KEPT_ONE, levels, "slab %d" % r)
        assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
        Polygonizer.halo_exchange_group(parts)  # (the halos hold the neighbours' layers already: the same bytes arrive)
        for expect in (HANDS_OUT, KEPT_ONE, KEPT_ONE):
            for r, p in enumerate(parts):
                run(p, expect, levels, "slab %d behind the halo exchange" % r)
            assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
    finally:
        for p in parts:
            p.close()
