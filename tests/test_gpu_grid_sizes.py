"""GPU parity at grid edges that are not powers of two (tests/grid_sizes.py) and past 1024^3, through the C ABI, against the
oracle port (which tests/test_oracle.py pins to the reference at the same edges).  Bar: indices, block infos, positions,
secondary positions, texture bytes and statistics bit-exact; normals within NRM_TOL."""
import gc
import os
import resource
import time

import numpy as np
import pytest

import fields
import grid_sizes
import vxo
from test_emu import _packed_case, check_all_level_limits, check_edit_chain, check_heightmap, check_pack
from test_gpu_parity import NRM_TOL, check_packed_hip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def poly():
    import torch
    torch.cuda.init()
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950", "the native HIP library must be the one running"
    p.set_materials(vxo.default_lut())
    yield p
    p.close()


@pytest.fixture(scope="module")
def port():
    o = vxo.load_port()
    assert o is not None, "oracle/libvoxels_port.so missing (run __graft_entry__.build())"
    return o


def context(**env):
    """A context created with the given environment knobs (the library reads them when a context is made)."""
    from voxels_amd import Polygonizer
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        p = Polygonizer(device=0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    p.set_materials(vxo.default_lut())
    return p


@pytest.mark.parametrize("n", [16, 48, 80, 112, 208, 336])
def test_hip_odd_size_fields_every_level_limit(poly, port, n):
    """A terrain with materials, full-range noise, a zero-heavy field and planes at (and half a voxel around) the end of every
    coarse level's covered prefix on each axis: all levels, then each level limit."""
    f = fields.terrain_field(n, 60 + n)
    m, b = fields.materials_for(n, 60 + n)
    check_all_level_limits(poly, port, port.grid_from_float(f, m, b), "n=%d terrain" % n, NRM_TOL)
    q = fields.quantize_full_range(fields.smooth_noise(n, 70 + n, scale=8, amp=3.0))
    check_all_level_limits(poly, port, port.grid_from_dense(q, m, b), "n=%d noise" % n, NRM_TOL)
    zero = np.zeros((n, n, n), np.uint8)
    check_all_level_limits(poly, port, port.grid_from_dense(grid_sizes.zero_heavy(n, 80 + n), m, b), "n=%d zero-heavy" % n, NRM_TOL)
    for axis in range(3):
        for h in grid_sizes.plane_heights(n):
            check_all_level_limits(poly, port, port.grid_from_dense(grid_sizes.plane_field(n, axis, h), zero, zero),
                                   "n=%d plane axis %d at %g" % (n, axis, h), NRM_TOL)


def test_hip_odd_size_1008_device_terrain(poly, port):
    """1008^3: six levels, every coarse one partial (levels 1..5 cover 992, 992, 896, 768, 512).  The grid is generated on the
    device, the oracle gets the host generator's."""
    from voxels_amd import synth
    n = 1008
    d, m, b = synth.terrain(n)
    g = port.grid_from_dense(d, m, b)
    del d, m, b
    s = port.execute(g)
    want, stats = s.all_levels(), s.stats()
    assert len(want) == 6
    poly.create_terrain(n)
    poly.execute()
    ok, msg = fields.surface_equal(poly.all_levels(), want, nrm_tol=NRM_TOL)
    assert ok, msg
    assert np.array_equal(poly.stats(), stats)
    for limit in range(1, len(want)):
        poly.execute(limit)
        ok, msg = fields.surface_equal(poly.all_levels(), want[:limit], nrm_tol=NRM_TOL)
        assert ok, "%d levels: %s" % (limit, msg)


@pytest.mark.parametrize("n", [80, 208])
def test_hip_odd_size_grid_sources(poly, port, n):
    """Every way a grid gets onto the device at an edge that is not a power of two: the packed file (blocks, flags, surface;
    pack() gives the port's bytes back, before and after device edits), the height-map constructor and the terrain generator."""
    for noisy in (False, True):
        d, m, b = _packed_case(n, 21 + n, noisy)
        check_packed_hip(poly, port, d, m, b, "packed n=%d noisy=%s" % (n, noisy))
        check_pack(poly, port, n, 43, noisy)
    check_heightmap(poly, port, n, 9, nrm_tol=NRM_TOL)
    from voxels_amd import synth
    d, m, b = synth.terrain(n, 0, n, 5)
    g = port.grid_from_dense(d, m, b)
    poly.create_terrain(n, 5)
    assert np.array_equal(poly.pack(), g.pack()), "create_terrain(%d) vs the host generator" % n
    poly.execute()
    s = port.execute(g)
    ok, msg = fields.surface_equal(poly.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
    assert ok, msg
    assert np.array_equal(poly.stats(), s.stats())


@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("n", [80, 208])
def test_hip_odd_size_edit_chain(port, n, fused):
    """Brushes in the band the coarsest levels leave uncovered, on both incremental paths: the box, the rebuilt ids, the surface
    and the statistics after each, the grid file and a full run at the end."""
    q = context(VX_DIRTY_FUSED=fused)
    try:
        check_edit_chain(q, port, n, NRM_TOL, upload="packed" if fused == "1" else "dense")
    finally:
        q.close()


@pytest.mark.parametrize("knob,value", [("VX_FAST", "0"), ("VX_FAST", "1"), ("VX_FAST", "2"), ("VX_UPPER", "0")])
def test_hip_odd_size_runtime_knobs(port, knob, value):
    q = context(**{knob: value})
    try:
        check_edit_chain(q, port, 208, NRM_TOL)
    finally:
        q.close()


def test_hip_odd_size_partial_runs(port):
    """vx_polygonize_from at 208^3 for every first meshed level: the levels from it up as in the full run, nothing below; then a
    brush in the uncovered band, after which exactly the rebuilt blocks are listed below, with the oracle's bytes.  (The bench
    generator's terrain: a surface with blocks beyond the first capacity class would make the run mesh every level.)"""
    from voxels_amd import synth
    n = 208
    d, m, b = synth.terrain(n, 0, n, 11)
    levels = grid_sizes.ref_levels(n)
    for first in range(1, levels):
        g = port.grid_from_dense(d, m, b)
        s = port.execute(g)
        q = context()
        try:
            q.upload(*g.read_dense(), g.block_flags())
            info = q.execute_from(0, first)
            assert info.first_meshed_level == first and info.levels == levels
            got, ref = q.all_levels(), s.all_levels()
            ok, msg = fields.surface_equal(got[first:], ref[first:], nrm_tol=0.0)
            assert ok, "first %d: %s" % (first, msg)
            assert not any(len(got[l].infos) for l in range(first)), first
            edit = grid_sizes.edit_chain(n)[first % 3]
            mn, mx = grid_sizes.apply_edit(g, edit)
            grid_sizes.apply_edit(q, edit)
            ref_ids = port.execute_modify(g, s, mn, mx)
            assert np.array_equal(q.execute_dirty(mn, mx), ref_ids), first
            assert np.array_equal(q.stats(), s.stats()), first
            got, ref = q.all_levels(), s.all_levels()
            ok, msg = fields.surface_equal(got[first:], ref[first:], nrm_tol=0.0)
            assert ok, "first %d after the edit: %s" % (first, msg)
            for l in range(first):
                ok, msg = fields.listed_blocks_equal_by_id(got[l], ref[l])
                assert ok, "first %d, level %d: %s" % (first, l, msg)
        finally:
            q.close()


@pytest.mark.parametrize("n,world", [(384, 3), (320, 5)])
@pytest.mark.parametrize("axis", ["z", "y"])
def test_hip_halo_exchange_odd_world(port, n, world, axis):
    """An odd number of slabs on one GPU (384^3 in 3 of 128, 320^3 in 5 of 64; 3 levels): each context holds only its own
    layers, vx_halo_exchange_group brings in the rest, and the union of their runs is the oracle's whole-grid surface."""
    import torch
    from voxels_amd import synth
    levels, seed = 3, 7
    d, m, b = synth.terrain(n, 0, n, seed)
    ref = port.execute(port.grid_from_dense(d, m, b))
    fields.check_halo_exchange_group(context, torch, torch.device("cuda", 0), n, levels, world, axis, ref.all_levels(),
                                     seed=seed, nrm_tol=NRM_TOL)


# ---- past 1024^3 ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1552, 1632, 2048])
def test_hip_grids_beyond_1024(port, n):
    """1552: the 32-bit kernels with offsets past 2^31; 1632: the first edge on the 64-bit path without forcing it; 2048:
    VX_MAX_GRID, whose eighth level (one block, no lattice copy) gathers its samples from the dense field.  The same grid on
    both sides without a dense transfer: a height map, then brushes at the far corner and across the last coarse block boundary
    of each axis.  A full run against the port, a far-corner edit with its incremental run, and the grid file."""
    t0 = time.time()
    hm = grid_sizes.large_heightmap(n, 3)
    g = port.grid_from_heightmap(n, hm)
    q = context()
    try:
        q.create_heightmap(hm)
        for edit in grid_sizes.large_edits(n):
            box = grid_sizes.apply_edit(g, edit)
            box2 = grid_sizes.apply_edit(q, edit)
            assert np.array_equal(box[0], box2[0]) and np.array_equal(box[1], box2[1]), edit
        s = port.execute(g)
        q.execute()
        want = s.all_levels()
        assert len(want) == grid_sizes.ref_levels(n)
        ok, msg = fields.surface_equal(q.all_levels(), want, nrm_tol=NRM_TOL)
        assert ok, "n=%d full run: %s" % (n, msg)
        assert np.array_equal(q.stats(), s.stats())
        del want
        pos, ext, r = (n - 9.5, n - 6.0, n - 7.0), (16.0, 16.0, 16.0), 6.0
        mn, mx = g.inject_ball(pos, ext, r, 2)
        mn2, mx2 = q.inject_ball(pos, ext, r, 2)
        assert np.array_equal(mn, mn2) and np.array_equal(mx, mx2)
        ref_ids = port.execute_modify(g, s, mn, mx)
        assert np.array_equal(q.execute_dirty(mn2, mx2), ref_ids)
        ok, msg = fields.surface_equal(q.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
        assert ok, "n=%d after the edit: %s" % (n, msg)
        assert np.array_equal(q.stats(), s.stats())
        assert np.array_equal(q.pack(), g.pack()), "n=%d: grid file" % n
    finally:
        q.close()
        s = g = None
        gc.collect()
    print("grid %d^3: %.1f s, peak host memory of the process so far %.1f GiB"
          % (n, time.time() - t0, resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 2 ** 20))
