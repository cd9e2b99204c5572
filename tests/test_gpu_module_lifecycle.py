"""The life of the modules' states in a context (vx_host.inl: module_state, dev_grow, the loop of vx_ctx_destroy): one small call
into every query and edit module in one context, the context closed, and the same again in a second one - every array that comes
back has the same bytes both times.  Then the buffers of the ray casts and of the measurements small, regrown and small again.
What each module computes is checked by its own tests; this one only makes ordinary calls and compares a context with another."""
import numpy as np
import pytest

import brush_oracle as bo
import vxo
import walk_oracle as wo
from golden_io import Golden

pytestmark = pytest.mark.gpu

N = 32


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def resident():
    """a context that owns the whole 32^3 fixture grid, polygonized"""
    gold = Golden("terrain32_mat")
    p = new_poly()
    p.upload(gold.dist, gold.mat, gold.blend, gold.flags)
    p.execute()
    return p


def flat(value, out=None):
    """every array in what a call returned, in order, as (dtype, shape, bytes)"""
    out = [] if out is None else out
    if isinstance(value, dict):
        value = sorted(value.items())
    if isinstance(value, (tuple, list)):
        for v in value:
            flat(v, out)
    elif value is not None:
        a = np.asarray(value)
        out.append((str(a.dtype), a.shape, a.tobytes()))
    return out


def every_module(p):
    """one minimal call into every module -> [(what, everything it returned)]"""
    import torch
    from voxels_amd import overlap_boxes, scatter_params
    from voxels_amd.binding import PASTE_REPLACE, smooth_op
    got = []
    # the queries on the level's meshes
    got.append(("ray", p.raycast([[16.5, 40.0, 16.5]], [[0.0, -1.0, 0.0]])))
    got.append(("sphere cast", p.spherecast([[16.5, 40.0, 16.5]], [[0.0, -1.0, 0.0]], 1.5)))
    got.append(("closest point", p.closest_points([[16.5, 20.0, 16.5]])))
    draws, regular, transition, counts = p.lod_select([16.0, 24.0, 16.0])
    for commands in (regular, transition):
        # where a block's meshes lie in the pools is the order in which the run's blocks reserved their room: not a function
        # of the inputs, so not the same in two contexts (tests/test_gpu_lod.py checks them against the context's own tables)
        commands["first_index"] = 0
        commands["vertex_offset"] = 0
    got.append(("lod", (draws, regular, transition, counts)))
    got.append(("scatter", p.scatter(0, scatter_params(seed=7, density=1.0))))
    got.append(("overlap", p.overlap_boxes(0, overlap_boxes([4.0, 0.0, 4.0], [20.0, 32.0, 20.0]), corners=True)))
    # the record first, so that the edits below are what it differs by
    box = ((0, 0, 0), (N, N, 16))
    rec = p.capture([box])
    got.append(("capture", (rec.info(), rec.block_ids())))
    got.append(("brush", p.inject_brushes(bo.stack([bo.ball((16.0, 16.0, 14.0), (12.0, 12.0, 12.0), 4.0, 2)]))))
    got.append(("islands", p.islands()))
    got.append(("smooth", p.smooth(smooth_op(((4, 4, 4), (20, 20, 20))))))
    dirs = torch.full((N * N * N,), 0x5A, dtype=torch.uint8, device="cuda:0")
    counts = p.walk_field(None, [(8, 8, 20)], dirs=dirs)   # (the field in the library's own volume)
    torch.cuda.synchronize()
    got.append(("walk", (wo.deterministic(counts), dirs.cpu().numpy())))
    stamp = p.capture_stamp(((6, 6, 6), (15, 13, 11)))
    got.append(("stamp", (stamp.info(), stamp.read())))
    got.append(("paste", p.paste([stamp], [((12, 9, 3), 0, 0, PASTE_REPLACE)])))
    got.append(("measure", p.measure([box])))
    got.append(("record measure", rec.measure()))
    got.append(("swap", rec.swap()))
    got.append(("grid", p.pack()))
    # (the record and the stamp stay with the context: closing it frees them)
    return got


def test_every_module_in_one_context_twice():
    runs = []
    for _ in range(2):
        p = resident()
        runs.append(every_module(p))
        p.close()
    assert [w for w, _ in runs[0]] == [w for w, _ in runs[1]]
    for (what, a), (_, b) in zip(*runs):
        fa, fb = flat(a), flat(b)
        assert fa and fa == fb, what
    # the calls did something: a hit, points, triangles, an edit, a paste that changed voxels
    byname = dict(runs[0])
    assert np.isfinite(byname["ray"]["t"][0]) and byname["scatter"][2]["points"] > 0 and byname["overlap"][3]["triangles"] > 0
    assert byname["brush"][3] > 0 and int(byname["paste"][1]["changed_voxels"]) > 0 and int(byname["swap"]["changed_voxels"]) > 0


def rays(count):
    """`count` rays straight down onto the terrain, on a lattice over the grid"""
    k = np.arange(count)
    side = int(np.ceil(np.sqrt(count)))
    o = np.stack([(k % side + 0.5) * (N / side), np.full(count, 40.0), (k // side + 0.5) * (N / side)], axis=1)
    return o.astype(np.float32), np.tile(np.float32([0.0, -1.0, 0.0]), (count, 1))


def boxes(count):
    rng = np.random.RandomState(5)
    lo = rng.randint(0, N - 8, (count, 3))
    return [(tuple(l), tuple(l + rng.randint(1, 9, 3))) for l in lo]


def test_buffers_small_regrown_small():
    p, fresh = resident(), resident()
    one, many = rays(1), rays(4096)
    first, large, third = p.raycast(*one), p.raycast(*many), p.raycast(*one)
    assert flat(first) == flat(third)
    assert flat(large) == flat(fresh.raycast(*many))
    assert np.isfinite(large["t"]).sum() > 2048
    one, many = boxes(1), boxes(300)
    first, large, third = p.measure(one), p.measure(many), p.measure(one)
    assert flat(first) == flat(third)
    assert flat(large) == flat(fresh.measure(many))
    assert large[0].size == 300 and int(large[0]["solid_voxels"].sum()) > 0
    p.close()
    fresh.close()


def test_closing_a_context_no_module_touched():
    p = new_poly()
    p.close()
    p = resident()   # a grid and a surface, still no module
    p.close()
