"""Material caches left in place (vx_material_inplace_counts): a full single-stream run that keeps the slot plan AND
would replay the material store finds every cache block, bitmap, cell count and flat item of the levels >= 1 already in its slot -
the run that left the plan wrote them there - so its upper queue has no material items, and its regular and transition blocks wait
for nobody (VX_MAT_INPLACE=1, the default; VX_MAT_INPLACE=0 keeps the store's copy items in such runs).

  1. chain run, assigning + capturing run, then kept runs in place: every run equals the oracle;
  2. the same bytes and statistics, run by run, as VX_MAT_INPLACE=0, VX_MATSTORE=0 and the conservative-sync library;
  3. the slots really hold the caches: an incremental run behind two runs in place equals the oracle's Modification run;
  4. every way the grid changes between runs in place: the next run assigns and votes, the one behind it is in place again;
  5. level limits: a run with another level count assigns and copies;
  6. vx_material_lut between two runs in place: the texture ids follow the new map;
  7. an attempt that overflows its pools inside one call: the repeat and the call behind it are in place;
  8. 140 runs in place in a row (SETTLE_EVERY twice, every set of counters many times), then an edit;
  9. two contexts on one GPU, alternating: each runs in place on its own slots.

Every case states through vx_slot_plan_counts, vx_material_path_counts and vx_material_inplace_counts which path each run took, so
that nothing passes because the runs fell back to copying or voting.  The fields are those of tests/test_gpu_matstore.py and
tests/test_gpu_slotplan.py, all inside the first capacity class (asserted on the CPU by slotplan.oracle)."""
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
VOTE, REPLAY = matstore.VOTE, matstore.REPLAY
NONE, COPIED, LEFT = "neither", "copied", "left in place"
# a run = (where its slots came from, the body of its material blocks, how replayed blocks came into their slots)
CHAIN = (ASSIGN, VOTE, NONE)        # the chain of launches: a context's first run
CAPTURE = (ASSIGN, VOTE, NONE)      # single-stream: hands out the plan's slots, votes and fills the store
COPY = (ASSIGN, REPLAY, COPIED)     # hands out its slots, copies from the store
INPLACE = (KEPT, REPLAY, LEFT)      # keeps the plan: the caches are in their slots
KEPT_COPY = (KEPT, REPLAY, COPIED)  # VX_MAT_INPLACE=0
KEPT_VOTE = (KEPT, VOTE, NONE)      # VX_MATSTORE=0


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


def run(p, expect, levels=0, label=""):
    """one call of vx_polygonize and the path of its attempts by all three counters.  Attempts of one call that are repeated (info.retries)
    count as slotplan.run counts them; of the replaying attempts of a call every one took the expected way into the slots."""
    plan, mat, how = expect
    before = p.material_inplace_counts()
    info = slotplan.run(p, plan, levels, label)
    after = p.material_inplace_counts()
    got = (after[0] - before[0], after[1] - before[1])
    blocks = sum(int(info.active_blocks[l]) for l in range(1, int(info.levels)))
    assert blocks > 0, "%s: no active block on a level >= 1" % label
    paths = p.material_path_counts()
    assert paths == ((blocks, 0) if mat == VOTE else (0, blocks)), "%s: (voted, replayed) = %s of %d blocks, expected a run that %s" % (label, paths, blocks, mat)
    attempts = 1 + int(info.retries)
    if how == NONE:
        ok = got == (0, 0)
    elif how == COPIED:
        ok = got[1] == 0 and 1 <= got[0] <= attempts
    else:
        ok = got == (0, attempts)
    assert ok, "%s: (copied, left in place) = %s with %d retries, expected %s" % (label, got, int(info.retries), how)
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


def warm(p, levels=0):
    """behind an upload: the runs up to and including the one that leaves plan and store"""
    p.forget_hints()
    run(p, CHAIN, levels, "first run (chain of launches)")
    return run(p, CAPTURE, levels, "second run (single-stream: assigns, captures)")


# ---- 1. the basic sequence --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["terrain64", "terrain80", "terrain128", "gentle64_mixed"])
def test_chain_capture_then_runs_in_place_equal_the_oracle(poly, port, name):
    d, m, b = plan_field(name)
    s = oracle(port, name)
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run_equals(poly, s, CHAIN, label=name + ", chain of launches")
    first = run_equals(poly, s, CAPTURE, label=name + ", assigning and capturing")
    assert sum(first.active_blocks) > 0 and int(first.blocks_read) > 0
    for k in range(3):
        info = run_equals(poly, s, INPLACE, label=name + ", in place %d" % k)
        assert reported(info) == reported(first), "%s, in place %d: %s vs %s" % (name, k, reported(info), reported(first))


# ---- 2. same bytes either way -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["VX_MAT_INPLACE=0", "VX_MATSTORE=0", "conservative"])
def test_same_bytes_in_place_and_not(other):
    from voxels_amd import digest
    from voxels_amd.binding import HipLibrary
    on = make_poly(VX_MAT_INPLACE=1)
    if other == "conservative":
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxels_amd", "csrc", "libvoxels_hip_conservative.so")
        assert os.path.exists(path), "libvoxels_hip_conservative.so missing (run __graft_entry__.build())"
        off, kept = make_poly(library=HipLibrary(path), VX_MAT_INPLACE=1), INPLACE
    elif other == "VX_MATSTORE=0":
        off, kept = make_poly(VX_MATSTORE=0), KEPT_VOTE
    else:
        off, kept = make_poly(VX_MAT_INPLACE=0), KEPT_COPY
    try:
        for name in ("terrain64", "gentle64_mixed", "terrain80", "terrain128"):
            d, m, b = plan_field(name)
            fl = cellmap.flags_of(d)
            for p in (on, off):
                p.upload(d, m, b, fl)
                p.forget_hints()
            for k, (e_on, e_off) in enumerate(((CHAIN, CHAIN), (CAPTURE, CAPTURE), (INPLACE, kept), (INPLACE, kept), (INPLACE, kept))):
                a = run(on, e_on, label="%s run %d, VX_MAT_INPLACE=1" % (name, k))
                c = run(off, e_off, label="%s run %d, %s" % (name, k, other))
                assert digest.digests_equal(digest.surface_digest(on.all_levels()), digest.surface_digest(off.all_levels())), "%s run %d" % (name, k)
                assert np.array_equal(on.stats(), off.stats()) and reported(a) == reported(c), "%s run %d" % (name, k)
    finally:
        on.close(); off.close()


# ---- 3. the slots hold the caches: an incremental run continues from them -----------------------------------------------------------
def test_incremental_run_behind_runs_in_place_equals_the_oracles_modification(poly, port):
    g = cellmap._terrain64(port)
    s = port.execute(g)
    poly.upload(*g.read_dense(), g.block_flags())
    warm(poly)
    for k in range(2):
        run_equals(poly, s, INPLACE, label="in place %d" % k)
    mn, mx = g.inject_ball(*cellmap.BALL)
    ref_ids = port.execute_modify(g, s, mn, mx)  # (s becomes the Modification's surface: old cache contents kept where the reference keeps them)
    a, bq = poly.inject_ball(*cellmap.BALL)
    assert np.array_equal(a, mn) and np.array_equal(bq, mx)
    got = poly.execute_dirty(mn, mx)
    assert np.array_equal(got, ref_ids)
    ok, msg = fields.surface_equal(poly.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
    assert ok, msg
    assert np.array_equal(poly.stats(), s.stats())


# ---- 4. whatever changes the grid --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["inject_ball", "inject_material", "upload"])
def test_a_changed_grid_is_voted_again_by(poly, port, what):
    d, m, b = plan_field("terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    run(poly, INPLACE, label="before " + what)
    matstore.MUTATIONS[what](poly, port)
    s = port.execute(port.grid_load(poly.pack()))
    run_equals(poly, s, CAPTURE, label="first run behind " + what)
    run_equals(poly, s, INPLACE, label="second run behind " + what)
    run_equals(poly, s, INPLACE, label="third run behind " + what)


def test_a_changed_grid_is_voted_again_by_flags_alone(poly, port):
    """vx_grid_update_blocks with no block and a new flag array: the BF_Empty flags mask level-0 cells out of the votes."""
    d, m, b = plan_field("terrain64")
    fl = cellmap.flags_of(d)
    assert fl.any()
    poly.upload(d, m, b, np.zeros_like(fl))
    warm(poly)
    run(poly, INPLACE, label="before the flags")
    poly.update_blocks(np.zeros(0, np.uint32), None, None, None, fl)
    s = oracle(port, "terrain64")
    run_equals(poly, s, CAPTURE, label="first run behind the flags")
    run_equals(poly, s, INPLACE, label="second run behind the flags")


def test_a_changed_grid_is_voted_again_by_invalidate(port):
    """attached tensors rewritten in place by their owner, who says so (vx_grid_invalidate)"""
    import torch
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers
    n = 64
    p = make_poly()
    try:
        slab = SlabBuffers(torch, n, 0, 1, torch.device("cuda", 0), axis="z")
        for k, seed in enumerate((3, 19)):
            d, m, b = synth.terrain(n, 0, n, seed)
            assert cellmap.numpy_cell_map(d)[1].max() <= cellmap.LARGE_THRESHOLD
            slab.fill_from_full(d, m, b, cellmap.flags_of(d))
            torch.cuda.synchronize()
            if k == 0:
                slab.attach(p)
            else:
                p.invalidate()
            s = port.execute(port.grid_from_dense(d, m, b))
            if k == 0:
                warm(p)
            else:
                run_equals(p, s, CAPTURE, label="first run behind vx_grid_invalidate")
            run_equals(p, s, INPLACE, label="in place, seed %d" % seed)
    finally:
        p.close()


# ---- 5. level limits ---------------------------------------------------------------------------------------------------------------
def test_level_limits(poly, port):
    d, m, b = plan_field("terrain128")
    s = oracle(port, "terrain128")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    for levels, expect in ((0, INPLACE), (2, COPY), (2, INPLACE), (0, COPY), (0, INPLACE)):
        run_equals(poly, s, expect, levels, "%d levels" % levels)


# ---- 6. the material map changes between two runs in place --------------------------------------------------------------------------
def test_material_lut_between_runs_in_place(poly, port):
    d, m, b = plan_field("gentle64_mixed")
    g = port.grid_from_dense(d, m, b)
    poly.upload(d, m, b, cellmap.flags_of(d))
    try:
        warm(poly)
        run_equals(poly, oracle(port, "gentle64_mixed"), INPLACE, label="default map")
        old_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        lut = ((vxo.default_lut().astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
        assert not np.array_equal(lut, vxo.default_lut())
        poly.set_materials(lut)
        s = port.execute(g, lut=lut)
        run_equals(poly, s, INPLACE, label="behind vx_material_lut")  # (surface_equal compares the texture bytes of every vertex)
        new_tex = [np.array(lv.verts["tex"]) for lv in poly.all_levels()]
        for li, (a, c) in enumerate(zip(old_tex, new_tex)):  # (same vertices, other ids: the run re-meshed, it did not return the old pools)
            assert a.shape == c.shape and a.size and not np.array_equal(a, c), "L%d: the run returned the old texture ids" % li
    finally:
        poly.set_materials(vxo.default_lut())


# ---- 7. a repeat inside one call ----------------------------------------------------------------------------------------------------
def test_attempt_that_overflows_is_repeated_in_place(port):
    """VX_POOL_SLACK=64, provoked like case 9 of tests/test_gpu_slotplan.py: the single-stream run that does not fit is the one
    behind a change to a larger grid.  Its first attempt hands out the slots, votes, fills the store and overflows; the pools grow,
    and the repeat - on the slots, and with the caches, the first attempt left - is in place."""
    from voxels_amd import synth
    p = make_poly(VX_POOL_SLACK=64)
    try:
        d, m, b = synth.terrain(32, seed=21)
        p.upload(d, m, b, cellmap.flags_of(d))
        assert p.execute().retries >= 1
        p.execute()
        d, m, b = plan_field("terrain64")
        p.upload(d, m, b, cellmap.flags_of(d))
        plan0, how0 = p.slot_plan_counts(), p.material_inplace_counts()
        info = p.execute()
        plan1, how1 = p.slot_plan_counts(), p.material_inplace_counts()
        assert info.retries >= 1
        assert (plan1[0] - plan0[0], plan1[1] - plan0[1]) == (1, int(info.retries)), "slots of the call's attempts"
        assert (how1[0] - how0[0], how1[1] - how0[1]) == (0, int(info.retries)), "the repeats were not in place: %s -> %s" % (how0, how1)
        blocks = sum(int(info.active_blocks[l]) for l in range(1, int(info.levels)))
        assert p.material_path_counts() == (0, blocks)
        s = oracle(port, "terrain64")
        ok, msg = fields.surface_equal(p.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
        assert ok, msg
        assert np.array_equal(p.stats(), s.stats())
        run_equals(p, s, INPLACE, label="the call behind the repeated one")
    finally:
        p.close()


# ---- 8. many runs ------------------------------------------------------------------------------------------------------------------
def test_many_runs_in_place_then_an_edit(poly, port):
    from voxels_amd import digest
    g = cellmap._terrain64(port)
    s = port.execute(g)
    poly.upload(*g.read_dense(), g.block_flags())
    first = warm(poly)
    want = digest.surface_digest(poly.all_levels())
    stats = poly.stats()
    for k in range(140):
        if k == 0 or k == 139:
            info = run_equals(poly, s, INPLACE, label="in place %d" % k)
        else:
            info = run(poly, INPLACE, label="in place %d" % k)
        assert reported(info) == reported(first), "in place %d" % k
        if k % 10 == 9:
            assert digest.digests_equal(digest.surface_digest(poly.all_levels()), want), "in place %d" % k
            assert np.array_equal(poly.stats(), stats)
    g.inject_ball(*cellmap.BALL)
    poly.inject_ball(*cellmap.BALL)
    s = port.execute(g)
    run_equals(poly, s, CAPTURE, label="first run behind the edit")
    run_equals(poly, s, INPLACE, label="second run behind the edit")


# ---- 9. two contexts alternating ---------------------------------------------------------------------------------------------------
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
        for k, expect in enumerate((CHAIN, CAPTURE, INPLACE, INPLACE, INPLACE)):
            for i, p in enumerate(ps):
                run_equals(p, want[i], expect, label="context %d, run %d" % (i, k))
    finally:
        for p in ps:
            p.close()
