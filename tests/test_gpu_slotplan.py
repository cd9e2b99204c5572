"""The slot plan (vx_slot_plan_counts): a full single-stream run that reads the cell map hands out its slots with
k_run_head, and the full runs behind it on an unchanged grid, with the same level count, launch no k_run_head: the head's whole
output - the block -> slot maps and slot coordinates of every level, skip and cell count of the level-0 slots, the slot counts
and the head's two statistics - is still in memory (VX_PLAN=1, the default).

  1. an assigning run, then kept runs: every run equals the oracle, and a kept run reports what an assigning one reports;
  2. VX_PLAN=1 and VX_PLAN=0 give the same bytes, so do VX_MATSTORE=0 with the plan kept and the conservative-sync library;
  3. every way the grid can change drops the plan: the next full run assigns (and equals the oracle on the new grid), the one
     behind it is kept;
  4. incremental runs, partial runs and runs on the chain of launches hand out slots themselves: the full run behind them assigns;
  5. level limits: a run whose level count differs from the plan's assigns;
  6. 140 kept runs in a row (SETTLE_EVERY twice, every set of counters many times), then an edit;
  7. two contexts on one GPU, alternating: each keeps its own plan;
  8. slabs of one grid on one GPU; a halo exchange drops the plan;
  9. an attempt that overflows its pools inside one call: the repeat inside the call and the call behind it are kept.

Every case states through vx_slot_plan_counts which path each run took, so that nothing passes because the runs fell back to
handing out their slots.  A context's first run launches every capacity class (the chain of launches, which hands out its
slots in a classification pass); where it met no block beyond the first class the run behind it is a single-stream one, which
assigns and leaves the plan, and the third one is kept.  vx_ctx_forget_hints puts a context back in front of that sequence."""
import os
import time

import numpy as np
import pytest

import fields
import vxo
import test_gpu_cellmap as cellmap
import test_gpu_matstore as matstore
import test_gpu_parity as parity
from test_gpu_matstore import make_poly, mixed_materials, field  # noqa: F401
from test_gpu_parity import port  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NRM_TOL = parity.NRM_TOL
ASSIGN, KEPT = "assigns", "keeps"


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


def terrain80():
    """5 blocks per edge: n / 16 is no power of two, so the last level-0 layer of every axis has no ancestors (k_run_head)"""
    from voxels_amd import synth
    return synth.terrain(80, seed=6)  # (fullest level-0 block: 606 non-trivial cells)


TERRAIN80 = []


def plan_field(name):
    if name != "terrain80":
        return field(name)
    if not TERRAIN80:
        TERRAIN80.append(terrain80())
    return TERRAIN80[0]


ORACLE = {}  # (one oracle run per field, shared by the cases)


def oracle(port, name):
    if name not in ORACLE:
        d, m, b = plan_field(name)
        # (fields beyond the first capacity class take the chain of launches and never keep a plan)
        assert cellmap.numpy_cell_map(d)[1].max() <= cellmap.LARGE_THRESHOLD, name
        ORACLE[name] = port.execute(port.grid_from_dense(d, m, b))
    return ORACLE[name]


def run(p, expect, levels=0, label=""):
    """one call of vx_polygonize; where the slots of its attempts came from.  A run that assigns: its first attempt hands them out,
    and so does every repeat (a chain of launches whose pools had to grow) - unless the repeat is single-stream, which then runs on
    the slots the first attempt handed out (case 9).  A run that keeps: no attempt hands out a slot."""
    before = p.slot_plan_counts()
    t0 = time.perf_counter()
    info = p.execute(levels)
    wall_ms = (time.perf_counter() - t0) * 1e3
    after = p.slot_plan_counts()
    got = (after[0] - before[0], after[1] - before[1])
    ok = (got[0] >= 1 and got[1] <= int(info.retries)) if expect == ASSIGN else (got[0] == 0 and got[1] == 1 + int(info.retries))
    assert ok, "%s: (handed out, kept) = %s with %d retries, expected a run that %s" % (label, got, int(info.retries), expect)
    if expect == KEPT:
        assert 0.0 < float(info.device_ms) < wall_ms, "%s: device_ms %.4f, the call took %.4f ms" % (label, info.device_ms, wall_ms)
    return info


def reported(info):
    return (int(info.levels), int(info.total_verts), int(info.total_indices), tuple(int(x) for x in info.active_blocks), int(info.blocks_read),
            int(info.algorithmic_bytes))


def run_equals(p, s, expect, levels=0, label=""):
    """... and its surface and statistics against the oracle's surface s"""
    info = run(p, expect, levels, label)
    want = s.all_levels()
    ok, msg = fields.surface_equal(p.all_levels(), want[:levels] if levels else want, nrm_tol=NRM_TOL)
    assert ok, "%s (%s) vs the oracle: %s" % (label, expect, msg)
    if not levels:
        assert np.array_equal(p.stats(), s.stats()), "%s (%s): stats %s vs %s" % (label, expect, p.stats(), s.stats())
    return info


def warm(p, levels=0):
    """behind an upload: the runs up to and including the one that leaves the plan (a new context starts on the chain of launches)"""
    p.forget_hints()
    run(p, ASSIGN, levels, "first run (chain of launches)")
    return run(p, ASSIGN, levels, "second run (single-stream, hands out the plan's slots)")


# ---- 1. an assigning run, then kept runs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["terrain64", "terrain128", "gentle64_mixed", "terrain80"])
def test_assign_then_kept_runs_equal_the_oracle(poly, port, name):
    d, m, b = plan_field(name)
    s = oracle(port, name)
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run_equals(poly, s, ASSIGN, label=name + ", chain of launches")
    first = run_equals(poly, s, ASSIGN, label=name + ", assigning")
    assert sum(first.active_blocks) > 0 and int(first.blocks_read) > 0
    for k in range(2):
        info = run_equals(poly, s, KEPT, label=name + ", kept run %d" % k)
        assert reported(info) == reported(first), "%s, kept run %d: %s vs %s" % (name, k, reported(info), reported(first))
    poly.set_materials(vxo.default_lut())  # (the LUT is no input of the head)
    info = run_equals(poly, s, KEPT, label=name + ", kept behind vx_material_lut")
    assert reported(info) == reported(first)


# ---- 2. same bytes either way --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["VX_PLAN=0", "VX_MATSTORE=0", "conservative"])
def test_same_bytes_with_and_without_the_plan(other):
    from voxels_amd import digest
    from voxels_amd.binding import HipLibrary
    on = make_poly(VX_PLAN=1)
    if other == "conservative":
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxels_amd", "csrc", "libvoxels_hip_conservative.so")
        assert os.path.exists(path), "libvoxels_hip_conservative.so missing (run __graft_entry__.build())"
        off = make_poly(library=HipLibrary(path), VX_PLAN=1)
    elif other == "VX_MATSTORE=0":
        off = make_poly(VX_MATSTORE=0)
    else:
        off = make_poly(VX_PLAN=0)
    try:
        for name in ("terrain64", "gentle64_mixed", "terrain80"):
            d, m, b = plan_field(name)
            fl = cellmap.flags_of(d)
            for p in (on, off):
                p.upload(d, m, b, fl)
                p.forget_hints()
            for k, expect in enumerate((ASSIGN, ASSIGN, KEPT, KEPT)):
                a = run(on, expect, label="%s run %d, VX_PLAN=1" % (name, k))
                c = run(off, ASSIGN if other == "VX_PLAN=0" else expect, label="%s run %d, %s" % (name, k, other))
                assert digest.digests_equal(digest.surface_digest(on.all_levels()), digest.surface_digest(off.all_levels())), "%s run %d" % (name, k)
                assert np.array_equal(on.stats(), off.stats()) and reported(a) == reported(c)
            if other == "VX_MATSTORE=0":
                assert off.material_path_counts()[1] == 0, "VX_MATSTORE=0 replayed"
    finally:
        on.close(); off.close()


# ---- 3. whatever changes the grid drops the plan ----------------------------------------------------------------------------------
@pytest.mark.parametrize("what", sorted(matstore.MUTATIONS))
def test_plan_is_dropped_by(poly, port, what):
    d, m, b = field("terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    if what == "islands_remove":
        poly.inject_ball(*matstore.FLOATING_BALL)  # (something for the removal to take away, resident before the plan is made)
    warm(poly)
    run(poly, KEPT, label="before " + what)
    matstore.MUTATIONS[what](poly, port)
    s = port.execute(port.grid_load(poly.pack()))
    run_equals(poly, s, ASSIGN, label="first run behind " + what)
    run_equals(poly, s, KEPT, label="second run behind " + what)


def test_plan_is_dropped_by_flags_alone(poly, port):
    """vx_grid_update_blocks with no block and a new flag array: nothing but the BF_Empty flags changes - which the head reads."""
    d, m, b = field("terrain64")
    fl = cellmap.flags_of(d)
    assert fl.any()
    poly.upload(d, m, b, np.zeros_like(fl))
    warm(poly)
    run(poly, KEPT, label="before the flags")
    poly.update_blocks(np.zeros(0, np.uint32), None, None, None, fl)
    s = oracle(port, "terrain64")
    run_equals(poly, s, ASSIGN, label="first run behind the flags")
    run_equals(poly, s, KEPT, label="second run behind the flags")


@pytest.mark.parametrize("how", ["invalidate", "attach"])
def test_plan_is_dropped_by_attached_memory_rewritten(port, how):
    import torch
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers
    n = 64
    p = make_poly()
    try:
        slab = SlabBuffers(torch, n, 0, 1, torch.device("cuda", 0), axis="z")
        for k, seed in enumerate((3, 19)):
            d, m, b = synth.terrain(n, 0, n, seed)
            slab.fill_from_full(d, m, b, cellmap.flags_of(d))
            torch.cuda.synchronize()
            if k == 0 or how == "attach":
                slab.attach(p)
            else:
                p.invalidate()
            s = port.execute(port.grid_from_dense(d, m, b))
            if k == 0:
                warm(p)
            else:
                run_equals(p, s, ASSIGN, label="first run behind " + how)
            run_equals(p, s, KEPT, label="kept, seed %d" % seed)
    finally:
        p.close()


# ---- 4. runs that drop the plan by themselves ---------------------------------------------------------------------------------
def test_full_run_behind_an_incremental_run_assigns(poly, port):
    from voxels_amd import digest
    g = cellmap._terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    warm(poly)
    run(poly, KEPT, label="before the edit")
    mn, mx = g.inject_ball(*cellmap.BALL)
    poly.inject_ball(*cellmap.BALL)
    poly.execute_dirty(mn, mx)
    s = port.execute(g)
    run_equals(poly, s, ASSIGN, label="full run behind the incremental one")
    assigned = digest.surface_digest(poly.all_levels())
    run_equals(poly, s, KEPT, label="the run behind it")
    assert digest.digests_equal(digest.surface_digest(poly.all_levels()), assigned)
    # an incremental run over a box that changes nothing still hands out and rewrites slots
    poly.execute_dirty(mn, mx)
    run_equals(poly, s, ASSIGN, label="full run behind an incremental run without an edit")


def test_full_run_behind_a_partial_run_assigns_and_chain_contexts_always_do(poly, port):
    from voxels_amd import digest
    d, m, b = field("terrain128")
    s = oracle(port, "terrain128")
    fl = cellmap.flags_of(d)
    poly.upload(d, m, b, fl)
    warm(poly)
    run_equals(poly, s, KEPT, label="before")
    before = digest.surface_digest(poly.all_levels())
    counts = poly.slot_plan_counts()
    info = poly.execute_from(0, 1)
    assert int(info.first_meshed_level) == 1, "the run was not a partial one"
    after = poly.slot_plan_counts()
    assert (after[0] - counts[0], after[1] - counts[1]) == (1, 0), "a partial run hands out its slots"
    run_equals(poly, s, ASSIGN, label="behind the partial run")
    run_equals(poly, s, KEPT, label="the run behind it")
    assert digest.digests_equal(digest.surface_digest(poly.all_levels()), before)
    chain = make_poly(VX_UPPER=0)
    try:
        chain.upload(d, m, b, fl)
        for k in range(3):
            run(chain, ASSIGN, label="VX_UPPER=0, run %d" % k)
        assert digest.digests_equal(digest.surface_digest(chain.all_levels()), before)
    finally:
        chain.close()


# ---- 5. level limits ---------------------------------------------------------------------------------------------------------
def test_level_limits(poly, port):
    d, m, b = field("terrain128")
    s = oracle(port, "terrain128")
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run(poly, ASSIGN, 3, "first run (chain of launches)")
    for levels, expect in ((3, ASSIGN), (3, KEPT), (2, ASSIGN), (2, KEPT), (3, ASSIGN), (3, KEPT), (0, ASSIGN), (0, KEPT), (4, KEPT)):
        run_equals(poly, s, expect, levels, "%d levels" % levels)


# ---- 6. many runs ------------------------------------------------------------------------------------------------------------
def test_many_kept_runs_then_an_edit(poly, port):
    from voxels_amd import digest
    g = cellmap._terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    first = warm(poly)
    want = digest.surface_digest(poly.all_levels())
    stats = poly.stats()
    for k in range(140):
        info = run(poly, KEPT, label="kept run %d" % k)
        assert reported(info) == reported(first), "kept run %d" % k
        if k % 10 == 9 or k == 139:
            assert digest.digests_equal(digest.surface_digest(poly.all_levels()), want), "kept run %d" % k
            assert np.array_equal(poly.stats(), stats)
    g.inject_ball(*cellmap.BALL)
    poly.inject_ball(*cellmap.BALL)
    s = port.execute(g)
    run_equals(poly, s, ASSIGN, label="first run behind the edit")
    run_equals(poly, s, KEPT, label="second run behind the edit")


# ---- 7. two contexts alternating ---------------------------------------------------------------------------------------------
def test_two_contexts_alternate(port):
    from voxels_amd import synth
    ps = [make_poly(), make_poly()]
    try:
        want = []
        for p, seed in zip(ps, (21, 22)):
            d, m, b = synth.terrain(64, seed=seed)
            assert cellmap.numpy_cell_map(d)[1].max() <= cellmap.LARGE_THRESHOLD
            want.append(port.execute(port.grid_from_dense(d, m, b)))
            p.upload(d, m, b, cellmap.flags_of(d))
            p.forget_hints()
        for k, expect in enumerate((ASSIGN, ASSIGN, KEPT, KEPT, KEPT)):
            for i, p in enumerate(ps):
                run_equals(p, want[i], expect, label="context %d, run %d" % (i, k))
    finally:
        for p in ps:
            p.close()


# ---- 8. slabs on one GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["y", "z"])
def test_two_slabs_equal_the_whole_grid(poly, axis):
    import torch
    from voxels_amd import Polygonizer, digest
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world = 128, 2
    levels = sharded_levels(n, world)
    assert levels >= 3
    d, m, b = field("terrain128")
    fl = cellmap.flags_of(d)
    poly.upload(d, m, b, fl)
    warm(poly, levels)
    run(poly, KEPT, levels, "whole grid")
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
            run(p, KEPT, levels, "slab %d" % r)
        assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
        Polygonizer.halo_exchange_group(parts)  # (the halos hold the neighbours' layers already: the same bytes arrive)
        for expect in (ASSIGN, KEPT):
            for r, p in enumerate(parts):
                run(p, expect, levels, "slab %d behind the halo exchange" % r)
            assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
    finally:
        for p in parts:
            p.close()


# ---- 9. a repeat inside one call ---------------------------------------------------------------------------------------------
def test_attempt_that_overflows_is_repeated_on_the_plan(port):
    """VX_POOL_SLACK=64 (the tight pools of tests/test_gpu_percall.py::test_a_repeated_run): the single-stream run that does not fit
    is the one behind a change to a larger grid.  Its first attempt hands out the slots and overflows; the pools grow, and the
    repeat - on the slots the first attempt handed out - fits."""
    from voxels_amd import synth
    p = make_poly(VX_POOL_SLACK=64)
    try:
        d, m, b = synth.terrain(32, seed=21)
        p.upload(d, m, b, cellmap.flags_of(d))
        assert p.execute().retries >= 1
        p.execute()
        d, m, b = field("terrain64")
        p.upload(d, m, b, cellmap.flags_of(d))
        before = p.slot_plan_counts()
        info = p.execute()
        after = p.slot_plan_counts()
        assert info.retries >= 1
        assert (after[0] - before[0], after[1] - before[1]) == (1, int(info.retries)), "the attempts of the call: %s" % ((after[0] - before[0], after[1] - before[1]),)
        s = oracle(port, "terrain64")
        ok, msg = fields.surface_equal(p.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
        assert ok, msg
        assert np.array_equal(p.stats(), s.stats())
        run_equals(p, s, KEPT, label="the call behind the repeated one")
    finally:
        p.close()
