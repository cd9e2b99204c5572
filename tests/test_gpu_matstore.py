"""The material store (vx_material_path_counts): a full single-stream run leaves what its material blocks voted
- cache, bitmap, cell count of every active block of a level >= 1 - in a store of its own, and the full runs behind it on an
unchanged grid copy those entries where they would vote again (VX_MATSTORE=1, the default).

  1. capture, then replays: every run equals the oracle;
  2. VX_MATSTORE=1 and VX_MATSTORE=0 give the same bytes, so does the conservative-sync library;
  3. every way the grid can change drops the store: the next full run votes (and equals the oracle on the new grid), the one
     behind it replays;
  4. a full run behind an incremental one votes;
  5. level limits: a store covers the runs with at most as many levels as the run that filled it;
  6. runs that neither capture nor replay (a partial run, a context on the chain of launches) leave the store alone;
  7. slabs of one grid on one GPU; a halo exchange drops the store.

Every case states which body the material blocks of a run took (vx_material_path_counts), so that nothing passes because the
runs fell back to voting.  A context's first run launches every capacity class (the chain of launches: votes, no capture);
where it met no block beyond the first class the run behind it is a single-stream one, which captures, and the third one
replays.  vx_ctx_forget_hints puts a context back in front of that sequence."""
import os

import numpy as np
import pytest

import fields
import vxo
import test_gpu_cellmap as cellmap
import test_gpu_parity as parity
from test_gpu_parity import port  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NRM_TOL = parity.NRM_TOL
VOTE, REPLAY = "votes", "replays"


def make_poly(library=None, **env):
    import torch
    torch.cuda.init()
    from voxels_amd import Polygonizer
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        p = Polygonizer(device=0, library=library)  # (the knobs are read when the context is created)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


@pytest.fixture(scope="module")
def poly():
    p = make_poly()
    yield p
    p.close()


def run(p, expect, levels=0, label=""):
    """one full run; the body its material blocks took: all voted, or all replayed"""
    info = p.execute(levels)
    blocks = sum(int(info.active_blocks[l]) for l in range(1, int(info.levels)))
    assert blocks > 0, "%s: no active block on a level >= 1" % label
    got = p.material_path_counts()
    want = (blocks, 0) if expect == VOTE else (0, blocks)
    assert got == want, "%s: (voted, replayed) = %s, expected %s (a run that %s)" % (label, got, want, expect)
    return info


def run_equals(p, s, expect, levels=0, label=""):
    """... and its surface and statistics against the oracle's surface s"""
    run(p, expect, levels, label)
    want = s.all_levels()
    ok, msg = fields.surface_equal(p.all_levels(), want[:levels] if levels else want, nrm_tol=NRM_TOL)
    assert ok, "%s (%s) vs the oracle: %s" % (label, expect, msg)
    if not levels:
        assert np.array_equal(p.stats(), s.stats()), "%s (%s): stats %s vs %s" % (label, expect, p.stats(), s.stats())


def warm(p, levels=0):
    """behind an upload: the runs up to and including the capturing one (a new context starts on the chain of launches)"""
    p.forget_hints()
    run(p, VOTE, levels, "first run (chain of launches)")
    run(p, VOTE, levels, "second run (captures)")


def mixed_materials(n, seed):
    """per-voxel random ids from a small set and random blends: no vote is trivial"""
    rng = np.random.RandomState(seed)
    return rng.choice(np.array([0, 1, 2, 5, 9], np.uint8), (n, n, n)), rng.randint(0, 256, (n, n, n)).astype(np.uint8)


def _fields():
    from voxels_amd import synth
    from golden_io import Golden
    yield ("terrain64",) + tuple(synth.terrain(64, seed=21))
    yield ("terrain128",) + tuple(synth.terrain(128, seed=43))
    d = cellmap.gentle_field(64, 16, scale=40)
    assert cellmap.numpy_cell_map(d)[1].max() <= cellmap.LARGE_THRESHOLD
    yield ("gentle64_mixed", d) + mixed_materials(64, 5)
    g = Golden("noise64_fullrange_mat")
    yield "noise64_fullrange_mat", np.ascontiguousarray(g.dist), np.ascontiguousarray(g.mat), np.ascontiguousarray(g.blend)


FIELDS = None  # (built by the first test that asks: collecting the module generates nothing)


def field(name):
    global FIELDS
    if FIELDS is None:
        FIELDS = {f[0]: f[1:] for f in _fields()}
    return FIELDS[name]


# ---- 1. capture, then replays --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["terrain64", "terrain128", "gentle64_mixed"])
def test_capture_then_replays_equal_the_oracle(poly, port, name):
    d, m, b = field(name)
    s = port.execute(port.grid_from_dense(d, m, b))
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run_equals(poly, s, VOTE, label=name + ", chain of launches")
    run_equals(poly, s, VOTE, label=name + ", capture")
    run_equals(poly, s, REPLAY, label=name + ", first replay")
    run_equals(poly, s, REPLAY, label=name + ", second replay")
    poly.set_materials(vxo.default_lut())  # (the LUT is no input of the caches)
    run_equals(poly, s, REPLAY, label=name + ", replay behind vx_material_lut")


def test_fixture_beyond_the_first_capacity_class_keeps_voting(poly, port):
    """The committed noise64_fullrange_mat fixture does NOT stay inside the first capacity class: its fullest block has 770
    non-trivial cells on level 0, 1 240 on level 1 and 1 893 on level 2 (numpy restatement, cellmap.numpy_cell_map), against
    LARGE_THRESHOLD = 640.  Its full runs therefore take the chain of launches with every capacity class, which neither
    captures nor replays: the premise that holds for it is that every run votes - after a store was filled for another grid
    on the same context, too - and equals the oracle."""
    d, m, b = field("terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    warm(poly)
    run(poly, REPLAY, label="terrain64 before the fixture")
    d, m, b = field("noise64_fullrange_mat")
    assert cellmap.numpy_cell_map(d)[1].max() > cellmap.LARGE_THRESHOLD
    s = port.execute(port.grid_from_dense(d, m, b))
    poly.upload(d, m, b, cellmap.flags_of(d))
    for k in range(4):
        run_equals(poly, s, VOTE, label="noise64_fullrange_mat, run %d" % k)


# ---- 2. same bytes either way --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("other", ["VX_MATSTORE=0", "conservative"])
def test_same_bytes_with_and_without_the_store(other):
    from voxels_amd import digest
    from voxels_amd.binding import HipLibrary
    on = make_poly(VX_MATSTORE=1)
    if other == "conservative":
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "voxels_amd", "csrc", "libvoxels_hip_conservative.so")
        assert os.path.exists(path), "libvoxels_hip_conservative.so missing (run __graft_entry__.build())"
        off = make_poly(library=HipLibrary(path), VX_MATSTORE=1)
    else:
        off = make_poly(VX_MATSTORE=0)
    try:
        for name in ("terrain64", "gentle64_mixed", "terrain128"):
            d, m, b = field(name)
            fl = cellmap.flags_of(d)
            for p in (on, off):
                p.upload(d, m, b, fl)
                p.forget_hints()
            for k, expect in enumerate((VOTE, VOTE, REPLAY, REPLAY)):
                run(on, expect, label="%s run %d, VX_MATSTORE=1" % (name, k))
                run(off, VOTE if other == "VX_MATSTORE=0" else expect, label="%s run %d, %s" % (name, k, other))
                assert digest.digests_equal(digest.surface_digest(on.all_levels()), digest.surface_digest(off.all_levels())), "%s run %d" % (name, k)
                assert np.array_equal(on.stats(), off.stats())
    finally:
        on.close(); off.close()


# ---- 3. whatever changes the grid drops the store ---------------------------------------------------------------------------------
def _resident_oracle(port, p):
    """the oracle's surface of the grid that is resident now (through the grid file: every voxel of the three fields)"""
    return port.execute(port.grid_load(p.pack()))


def _other_grid():
    from voxels_amd import synth
    return synth.terrain(64, seed=22)


def _mut_upload(p, port):
    d, m, b = _other_grid()
    p.upload(d, m, b, cellmap.flags_of(d))


def _mut_upload_packed(p, port):
    p.upload_packed(port.grid_from_dense(*_other_grid()).pack())


def _mut_create_terrain(p, port):
    p.create_terrain(64, 22)


def _block_update(p, change):
    d, m, b = field("terrain64")
    d2, m2, b2 = change(d.copy(), m.copy(), b.copy())
    ids, (dd, mm, bb) = fields.edited_blocks((d, m, b), (d2, m2, b2))
    assert len(ids) > 0
    p.update_blocks(ids, dd, mm, bb, cellmap.flags_of(d2))


def _mut_update_blocks(p, port):
    def change(d, m, b):
        d[28:36, 28:36, 28:36] = ~d[28:36, 28:36, 28:36]  # (a small cube of flipped signs: its blocks stay within the first capacity class)
        return d, m, b
    _block_update(p, change)


def _mut_update_blocks_material_only(p, port):
    """materials and blends of the voxels around the surface: distances, cell map and flags stay as they are"""
    def change(d, m, b):
        near = np.abs(d.astype(np.int32)) < 100
        assert near.any()
        m[near] = (m[near] + 1) % 3
        b[near] = 255 - b[near]
        return d, m, b
    _block_update(p, change)


def _mut_inject_ball(p, port):
    p.inject_ball(*cellmap.BALL)


def _mut_inject_material(p, port):
    p.inject_material((30.0, 33.5, 31.25), (28.0, 28.0, 28.0), 7, 1)


def _mut_inject_brushes(p, port):
    import brush_oracle as bo
    p.inject_brushes(bo.stack([bo.ball((30.0, 33.5, 31.25), (20.0, 20.0, 20.0), 7.0, 2), bo.material((20.0, 20.0, 30.0), (12.0, 12.0, 12.0), 4, 1)]))


def _mut_smooth(p, port):
    from voxels_amd.binding import smooth_op
    _, _, _, changed = p.smooth(smooth_op(((8, 8, 8), (56, 56, 56)), strength=1.0, iterations=2))
    assert changed > 0


FLOATING_BALL = ((32.0, 32.0, 56.0), (8.0, 8.0, 8.0), 3.0, 0)  # (IT_Add, in the air above the terrain: a detached piece)


def _mut_islands_remove(p, port):
    _, counts, _, _ = p.islands(remove=True)
    assert int(counts["removed"]) > 0 and int(counts["touched_blocks"]) > 0, "nothing was removed: the case does not reach the removal's writes"


MUTATIONS = {"upload": _mut_upload, "upload_packed": _mut_upload_packed, "create_terrain": _mut_create_terrain,
             "update_blocks": _mut_update_blocks,
             "update_blocks_material_only": _mut_update_blocks_material_only, "inject_ball": _mut_inject_ball,
             "inject_material": _mut_inject_material, "inject_brushes": _mut_inject_brushes, "smooth": _mut_smooth,
             "islands_remove": _mut_islands_remove}


@pytest.mark.parametrize("what", sorted(MUTATIONS))
def test_store_is_dropped_by(poly, port, what):
    d, m, b = field("terrain64")
    poly.upload(d, m, b, cellmap.flags_of(d))
    if what == "islands_remove":
        poly.inject_ball(*FLOATING_BALL)  # (something for the removal to take away, resident before the store is filled)
    warm(poly)
    run(poly, REPLAY, label="before " + what)
    MUTATIONS[what](poly, port)
    s = _resident_oracle(port, poly)
    run_equals(poly, s, VOTE, label="first run behind " + what)
    run_equals(poly, s, REPLAY, label="second run behind " + what)


def test_store_is_dropped_by_flags_alone(poly, port):
    """vx_grid_update_blocks with no block and a new flag array: the grid was uploaded with no block marked BF_Empty, the call
    hands in the flags the codec derives.  Nothing but the flags changes - no mirror, no cell map entry."""
    d, m, b = field("terrain64")
    fl = cellmap.flags_of(d)
    assert fl.any()
    poly.upload(d, m, b, np.zeros_like(fl))
    warm(poly)
    run(poly, REPLAY, label="before the flags")
    poly.update_blocks(np.zeros(0, np.uint32), None, None, None, fl)
    s = port.execute(port.grid_from_dense(d, m, b))
    run_equals(poly, s, VOTE, label="first run behind the flags")
    run_equals(poly, s, REPLAY, label="second run behind the flags")


@pytest.mark.parametrize("how", ["invalidate", "attach"])
def test_store_is_dropped_by_attached_memory_rewritten(port, how):
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
                run_equals(p, s, VOTE, label="first run behind " + how)
            run_equals(p, s, REPLAY, label="replay, seed %d" % seed)
    finally:
        p.close()


# ---- 4. a full run behind an incremental one ----------------------------------------------------------------------------------
def test_full_run_behind_an_incremental_run_votes(poly, port):
    from voxels_amd import digest
    g = cellmap._terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    warm(poly)
    run(poly, REPLAY, label="before the edit")
    mn, mx = g.inject_ball(*cellmap.BALL)
    poly.inject_ball(*cellmap.BALL)
    poly.execute_dirty(mn, mx)
    s = port.execute(g)
    run_equals(poly, s, VOTE, label="full run behind the incremental one")
    voted = digest.surface_digest(poly.all_levels())
    run_equals(poly, s, REPLAY, label="the run behind it")
    assert digest.digests_equal(digest.surface_digest(poly.all_levels()), voted)


# ---- 5. level limits ---------------------------------------------------------------------------------------------------------
def test_level_limits(poly, port):
    d, m, b = field("terrain128")
    s = port.execute(port.grid_from_dense(d, m, b))
    poly.upload(d, m, b, cellmap.flags_of(d))
    poly.forget_hints()
    run(poly, VOTE, 3, "first run (chain of launches)")
    for levels, expect in ((3, VOTE), (2, REPLAY), (4, VOTE), (4, REPLAY)):
        run_equals(poly, s, expect, levels, "%d levels" % levels)


# ---- 6. runs that neither capture nor replay ---------------------------------------------------------------------------------
def test_partial_run_and_chain_context_leave_the_store_alone(poly, port):
    from voxels_amd import digest
    d, m, b = field("terrain128")
    s = port.execute(port.grid_from_dense(d, m, b))
    fl = cellmap.flags_of(d)
    poly.upload(d, m, b, fl)
    warm(poly)
    run_equals(poly, s, REPLAY, label="before")
    before = digest.surface_digest(poly.all_levels())
    info = poly.execute_from(0, 1)
    assert int(info.first_meshed_level) == 1, "the run was not a partial one"
    voted, replayed = poly.material_path_counts()
    assert replayed == 0 and voted > 0, "a partial run votes: (%d, %d)" % (voted, replayed)
    chain = make_poly(VX_UPPER=0)
    try:
        chain.upload(d, m, b, fl)
        for k in range(3):
            run(chain, VOTE, label="VX_UPPER=0, run %d" % k)
        assert digest.digests_equal(digest.surface_digest(chain.all_levels()), before)
    finally:
        chain.close()
    run_equals(poly, s, REPLAY, label="behind the partial run")
    assert digest.digests_equal(digest.surface_digest(poly.all_levels()), before)


# ---- 7. slabs on one GPU -----------------------------------------------------------------------------------------------------
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
    run(poly, REPLAY, levels, "whole grid")
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
            run(p, REPLAY, levels, "slab %d" % r)
        assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
        Polygonizer.halo_exchange_group(parts)  # (the halos hold the neighbours' layers already: the same bytes arrive)
        for expect in (VOTE, REPLAY):
            for r, p in enumerate(parts):
                run(p, expect, levels, "slab %d behind the halo exchange" % r)
            assert digest.digests_equal(digest.combine([digest.surface_digest(p.all_levels()) for p in parts]), whole)
    finally:
        for p in parts:
            p.close()
