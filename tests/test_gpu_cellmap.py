"""The cell map (vx_grid_cell_map): the non-trivial-cell bitmaps of the level-0 blocks by block coordinate, kept
with the grid's mirrors and read by full single-stream runs instead of forming bitmaps (VX_CELLMAP=1, the default).

  1. the map against a restatement in numpy from the dense array;
  2. VX_CELLMAP=1 and VX_CELLMAP=0 give the same bytes, and the oracle's - also where the chain of launches runs (VX_UPPER=0);
  3. the map follows every way the grid can change (a full run after each, against the oracle on the new grid);
  4. slabs of one grid on one GPU.

A context's first run launches every capacity class (the chain of launches); where it met no block beyond the first class the
runs behind it are single-stream ones, which read the map.  The cases that are about the single-stream path run twice and
check that premise with one more run under stage timing (vx_stage_layout says which form it took)."""
import os
from itertools import product

import numpy as np
import pytest

import fields
import vxo
import test_gpu_parity as parity
from test_gpu_parity import port  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NRM_TOL = parity.NRM_TOL
LARGE_THRESHOLD = 640  # tv_block.h: blocks with more non-trivial cells leave the single-stream path


def make_poly(**env):
    import torch
    torch.cuda.init()
    from voxels_amd import Polygonizer
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        p = Polygonizer(device=0)  # (the knobs are read when the context is created)
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


def numpy_cell_map(d):
    """d: int8 [z, y, x] -> (words uint32 [nb, nb, nb, 128] indexed [bz, by, bx], counts [nb, nb, nb]): a cell is non-trivial
    unless its eight corner samples agree in sign, a zero counting as >= 0, corner coordinates clamped to n - 1; bit
    x | y << 4 | z << 8 of a block's 4096."""
    n = d.shape[0]
    nb = n // 16
    c = np.minimum(np.arange(n + 1), n - 1)
    neg = (d < 0)[np.ix_(c, c, c)]
    any_neg = np.zeros((n, n, n), bool)
    all_neg = np.ones((n, n, n), bool)
    for dz, dy, dx in product((0, 1), repeat=3):
        s = neg[dz:dz + n, dy:dy + n, dx:dx + n]
        any_neg |= s
        all_neg &= s
    nt = any_neg & ~all_neg
    blocks = nt.reshape(nb, 16, nb, 16, nb, 16).transpose(0, 2, 4, 1, 3, 5).reshape(nb, nb, nb, 4096)
    words = np.packbits(blocks, axis=-1, bitorder="little").view("<u4")
    return np.ascontiguousarray(words), blocks.sum(axis=-1)


def noise_field(n, seed):
    return fields.quantize_full_range(fields.smooth_noise(n, seed, scale=8, amp=3.0))


def zero_heavy_field(n, seed):
    return np.clip(np.round(fields.smooth_noise(n, seed, scale=8, amp=2.0) * 1.5), -4, 4).astype(np.int8)


def gentle_field(n, seed, scale=24):
    """A smooth full-range noise field whose blocks stay within the first capacity class (level 0: checked by the callers; all
    levels: by the single-stream premise of run_full)."""
    return fields.quantize_full_range(fields.smooth_noise(n, seed, scale=scale, amp=3.0, octaves=1))


def flags_of(d):
    from voxels_amd import synth
    return synth.block_empty_flags(d)


def run_full(p, runs=2, expect_map=True, levels=0):
    """`runs` full runs (two behind a context's first upload: see above); expect_map: the context's full runs are now
    single-stream ones, i.e. the last of them read the cell map."""
    for _ in range(runs):
        p.execute(levels)
    lv, st = p.all_levels(), p.stats()
    if expect_map:
        p.set_stage_timing(True)
        try:
            p.execute(levels)
            assert p.stage_layout() == 1, "the context's full runs are not single-stream runs: the cell map is not in use"
        finally:
            p.set_stage_timing(False)
    return lv, st


def check_oracle(port, p, d, m, b, label, runs=2, expect_map=True):
    s = port.execute(port.grid_from_dense(d, m, b))
    lv, st = run_full(p, runs, expect_map)
    ok, msg = fields.surface_equal(lv, s.all_levels(), nrm_tol=NRM_TOL)
    assert ok, "%s vs the oracle: %s" % (label, msg)
    assert np.array_equal(st, s.stats()), "%s stats %s vs %s" % (label, st, s.stats())
    return lv


# ---- 1. the map against an independent restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 48, 64])
@pytest.mark.parametrize("kind", ["noise", "zeros"])
def test_cell_map_equals_numpy_restatement(poly, n, kind):
    d = noise_field(n, 60 + n) if kind == "noise" else zero_heavy_field(n, 70 + n)
    if kind == "zeros":
        assert (d == 0).mean() > 0.05
    zero = np.zeros((n, n, n), np.uint8)
    poly.upload(d, zero, zero, flags_of(d))
    want_words, want_counts = numpy_cell_map(d)
    nb = n // 16
    seen_cells = 0
    for bz, by, bx in product(range(nb), repeat=3):
        words, count = poly.cell_map(bx, by, bz)
        assert count == want_counts[bz, by, bx], "count of block (%d, %d, %d): %d vs %d" % (bx, by, bz, count, want_counts[bz, by, bx])
        assert np.array_equal(words, want_words[bz, by, bx]), "bitmap of block (%d, %d, %d)" % (bx, by, bz)
        seen_cells += count != 0
    assert seen_cells > 0


def test_cell_map_of_quiet_blocks_and_bad_arguments(poly):
    """A grid with one bubble: the blocks around it have cells, all others are quiet (zeros, count 0, whatever the map's
    memory held before); a block outside the grid is an error."""
    from voxels_amd.binding import VoxelsHipError
    n = 64
    d = noise_field(n, 5)
    zero = np.zeros((n, n, n), np.uint8)
    poly.upload(d, zero, zero, flags_of(d))
    poly.cell_map(0, 0, 0)  # (the map's memory now holds the noise field's entries)
    d = np.full((n, n, n), 4, np.int8)
    d[32, 16, 48] = -3  # first voxel of block (3, 1, 2): cells of the blocks at -x, -y, -z of it too
    poly.upload(d, zero, zero, flags_of(d))
    want_words, want_counts = numpy_cell_map(d)
    assert want_counts.sum() == 8 and (want_counts > 0).sum() == 8
    for bz, by, bx in product(range(4), repeat=3):
        words, count = poly.cell_map(bx, by, bz)
        assert count == want_counts[bz, by, bx] and np.array_equal(words, want_words[bz, by, bx]), (bx, by, bz)
    with pytest.raises(VoxelsHipError):
        poly.cell_map(4, 0, 0)


# ---- 2. same bytes either way ------------------------------------------------------------------------------------------------
def _inputs_same_bytes():
    from voxels_amd import synth
    n = 64
    m, b = fields.materials_for(n, 52)
    yield "noise64", noise_field(n, 52), m, b, False  # (dense: blocks beyond the first capacity class keep its runs on the chain)
    d = gentle_field(n, 16, scale=40)  # (full-range noise whose blocks stay within the first class: its runs read the map)
    assert numpy_cell_map(d)[1].max() <= LARGE_THRESHOLD
    yield "gentle64", d, m, b, True
    d, m, b = synth.terrain(128, 0, 128, 43)
    yield "terrain128", d, m, b, True


@pytest.mark.parametrize("upper", ["1", "0"])
def test_same_bytes_with_and_without_the_map(port, upper):
    from voxels_amd import digest
    on, off = make_poly(VX_CELLMAP=1, VX_UPPER=upper), make_poly(VX_CELLMAP=0, VX_UPPER=upper)
    try:
        for label, d, m, b, single in _inputs_same_bytes():
            fl = flags_of(d)
            on.upload(d, m, b, fl)
            off.upload(d, m, b, fl)
            lv_on = check_oracle(port, on, d, m, b, "%s VX_CELLMAP=1 VX_UPPER=%s" % (label, upper), expect_map=single and upper == "1")
            lv_off = check_oracle(port, off, d, m, b, "%s VX_CELLMAP=0 VX_UPPER=%s" % (label, upper), expect_map=False)
            assert digest.digests_equal(digest.surface_digest(lv_on), digest.surface_digest(lv_off)), label
            assert np.array_equal(on.stats(), off.stats())
    finally:
        on.close(); off.close()


# ---- 3. staleness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["x0", "y0", "z0", "voxel0"])
def test_map_follows_update_blocks(poly, port, what):
    """Only the plane x = 0 (y = 0, z = 0; the first voxel) of one interior block of a 48^3 grid changes sign: beside the
    block's own cells only those of its -x (-y, -z; -x-y-z and the blocks between) neighbour change, blocks no edit lists."""
    n, nb = 48, 3
    d = gentle_field(n, 13)
    assert numpy_cell_map(d)[1].max() <= LARGE_THRESHOLD
    m, b = fields.materials_for(n, 13)
    poly.upload(d, m, b, flags_of(d))
    check_oracle(port, poly, d, m, b, "before the update")  # (the map is current now)
    d2 = d.copy()
    sel = {"x0": np.s_[16:32, 16:32, 16], "y0": np.s_[16:32, 16, 16:32], "z0": np.s_[16, 16:32, 16:32], "voxel0": np.s_[16, 16, 16]}[what]
    d2[sel] = ~d2[sel]  # (-d - 1: every sample changes its sign class)
    before, after = numpy_cell_map(d)[0], numpy_cell_map(d2)[0]
    changed = {tuple(int(v) for v in c) for c in np.argwhere((before != after).any(axis=-1))}  # (bz, by, bx)
    neighbour = {"x0": (1, 1, 0), "y0": (1, 0, 1), "z0": (0, 1, 1), "voxel0": (0, 0, 0)}[what]
    assert neighbour in changed, "the edit does not reach the neighbour's cells: %s" % sorted(changed)
    ids, (dd, mm, bb) = fields.edited_blocks((d, m, b), (d2, m, b))
    assert list(ids) == [(1 * nb + 1) * nb + 1]
    poly.update_blocks(ids, dd, mm, bb, flags_of(d2))
    s = port.execute(port.grid_from_dense(d2, m, b))
    info = poly.execute()
    assert info.mirror_ms > 0, "the full run behind the update did not rebuild the cell map"  # (the bricks followed the update in place)
    ok, msg = fields.surface_equal(poly.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
    assert ok, "after the update (%s): %s" % (what, msg)
    assert np.array_equal(poly.stats(), s.stats())
    words, count = poly.cell_map(neighbour[2], neighbour[1], neighbour[0])
    assert np.array_equal(words, after[neighbour])


def _terrain64(port):
    from voxels_amd import synth
    d, m, b = synth.terrain(64, seed=21)
    return port.grid_from_dense(d, m, b)


BALL = ((30.0, 33.5, 31.25), (20.0, 20.0, 20.0), 7.0, 2)


def test_map_follows_inject_ball_before_a_full_run(poly, port):
    g = _terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    run_full(poly)
    g.inject_ball(*BALL)
    poly.inject_ball(*BALL)
    s = port.execute(g)
    info = poly.execute()  # a full run, not a dirty one
    assert info.mirror_ms > 0, "the full run behind the edit did not rebuild the cell map"
    ok, msg = fields.surface_equal(poly.all_levels(), s.all_levels(), nrm_tol=NRM_TOL)
    assert ok, msg
    assert np.array_equal(poly.stats(), s.stats())


def test_full_run_behind_an_incremental_run(poly, port):
    """full -> vx_polygonize_dirty -> full on one context: the incremental run neither reads nor updates the map, the full run
    behind it rebuilds it.  The last surface is that of a fresh context with the same final grid, and the oracle's."""
    from voxels_amd import digest
    g = _terrain64(port)
    poly.upload(*g.read_dense(), g.block_flags())
    run_full(poly)
    mn, mx = g.inject_ball(*BALL)
    poly.inject_ball(*BALL)
    poly.execute_dirty(mn, mx)
    poly.execute()
    got = poly.all_levels()
    fresh = make_poly()
    try:
        fresh.upload(*g.read_dense(), g.block_flags())
        want, _ = run_full(fresh)
        assert digest.digests_equal(digest.surface_digest(got), digest.surface_digest(want))
    finally:
        fresh.close()
    ok, msg = fields.surface_equal(got, port.execute(g).all_levels(), nrm_tol=NRM_TOL)
    assert ok, msg


def test_map_follows_create_terrain_with_another_seed(port):
    from voxels_amd import synth
    p = make_poly()
    try:
        for k, seed in enumerate((3, 19)):
            p.create_terrain(64, seed)
            d, m, b = synth.terrain(64, 0, 64, seed)
            check_oracle(port, p, d, m, b, "create_terrain seed %d" % seed, runs=2 if k == 0 else 1)
    finally:
        p.close()


def test_map_follows_invalidate(port):
    """Attached tensors rewritten in place by their owner, who says so (vx_grid_invalidate)."""
    import torch
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers
    n = 64
    p = make_poly()
    try:
        slab = SlabBuffers(torch, n, 0, 1, torch.device("cuda", 0), axis="z")
        for k, seed in enumerate((3, 19)):
            d, m, b = synth.terrain(n, 0, n, seed)
            slab.fill_from_full(d, m, b, flags_of(d))
            torch.cuda.synchronize()
            if k == 0:
                slab.attach(p)
            else:
                p.invalidate()
            check_oracle(port, p, d, m, b, "attached, seed %d" % seed, runs=2 if k == 0 else 1)
    finally:
        p.close()


# ---- 4. slabs on one GPU -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["y", "z"])
def test_two_slabs_equal_the_whole_grid(poly, axis):
    import torch
    from voxels_amd import digest, synth
    from voxels_amd.slab import SlabBuffers, sharded_levels
    n, world, seed = 128, 2, 11
    levels = sharded_levels(n, world)
    d, m, b = synth.terrain(n, 0, n, seed)
    fl = flags_of(d)
    poly.upload(d, m, b, fl)
    whole = digest.surface_digest(run_full(poly, levels=levels)[0])
    parts = []
    for r in range(world):
        p = make_poly()
        try:
            slab = SlabBuffers(torch, n, r, world, torch.device("cuda", 0), axis=axis)
            slab.fill_from_full(d, m, b, fl)
            torch.cuda.synchronize()
            slab.attach(p)
            parts.append(digest.surface_digest(run_full(p, levels=levels)[0]))
            # the slab's own entries of the map are those of the whole grid
            want_words, want_counts = numpy_cell_map(d)
            nb = n // 16
            lo, hi = r * nb // world, (r + 1) * nb // world
            for t in range(lo, hi):
                for u, bx in product((0, nb - 1), (0, nb // 2, nb - 1)):
                    by, bz = (t, u) if axis == "y" else (u, t)
                    words, count = p.cell_map(bx, by, bz)
                    assert count == want_counts[bz, by, bx] and np.array_equal(words, want_words[bz, by, bx]), (bx, by, bz)
        finally:
            p.close()
    assert digest.digests_equal(digest.combine(parts), whole)
