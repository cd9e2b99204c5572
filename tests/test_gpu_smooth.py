"""vx_grid_smooth on the MI355X against the numpy statement of the header's text (tests/smooth_oracle.py), exactly: the packed
file of the device grid (distances, untouched materials and BF_Empty at once) against the pack of the oracle-edited grid, the
per-op results, the union box and the count.  tests/test_smooth.py anchors that oracle to answers written by hand and runs the
same case list through the host build of the kernels' per-lane logic."""
import numpy as np
import pytest

import fields
import smooth_oracle as so
import vxo

pytestmark = pytest.mark.gpu

CASES = so.cases()


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    assert p._L.has_smooth
    p.set_materials(vxo.default_lut())
    return p


def resident(dist, mat=None, blend=None):
    n = dist.shape[0]
    if mat is None:
        mat, blend = fields.materials_for(n, 3)
    g = vxo.load_port().grid_from_dense(np.ascontiguousarray(dist), mat, blend)
    p = new_poly()
    p.upload_packed(g.pack())
    return p, mat, blend, g


def packed(dist, mat, blend):
    return vxo.load_port().grid_from_dense(np.ascontiguousarray(dist), mat, blend).pack()


def same_results(got, want):
    results, umin, umax, changed = got
    assert results.tobytes() == want.results.tobytes(), (results, want.results)
    assert umin.tobytes() == want.union_min.tobytes() and umax.tobytes() == want.union_max.tobytes(), (umin, umax, want.union_min, want.union_max)
    assert changed == want.changed


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_device_equals_the_oracle(case):
    _, dist, ops = case
    want = so.apply(dist, ops)
    assert want.changed > 0
    p, mat, blend, _ = resident(dist)
    same_results(p.smooth(ops), want)
    assert np.array_equal(p.pack(), packed(want.dist, mat, blend))


def test_a_batch_equals_single_calls_and_itself():
    d = so.terrain(48)[0]
    ops = so.stroke(40)
    want = so.apply(d, ops)
    assert (want.results["changed_voxels"] > 0).sum() >= 10
    a, mat, blend, _ = resident(d)
    b, _, _, _ = resident(d)
    c, _, _, _ = resident(d)
    got_a, got_b = a.smooth(ops), b.smooth(ops)
    same_results(got_a, want)
    same_results(got_b, want)
    pa = a.pack()
    assert np.array_equal(pa, b.pack())                  # the same batch twice on equal grids: equal bytes
    changed = 0
    for i in range(ops.size):
        res, mn, mx, cnt = c.smooth(ops[i:i + 1])
        assert res[0].tobytes() == want.results[i].tobytes(), i
        assert mn.tobytes() == want.results[i]["out_min"].tobytes() and mx.tobytes() == want.results[i]["out_max"].tobytes()
        changed += cnt
    assert changed == want.changed
    assert np.array_equal(pa, c.pack())
    assert np.array_equal(pa, packed(want.dist, mat, blend))


def test_a_noise_batch_twice_the_same_bytes():
    d = so.noise(48, 2)
    ops = so.stroke(40)
    want = so.apply(d, ops)
    packs = []
    for _ in range(2):
        p, mat, blend, _ = resident(d)
        same_results(p.smooth(ops), want)
        packs.append(p.pack())
    assert np.array_equal(packs[0], packs[1]) and np.array_equal(packs[0], packed(want.dist, mat, blend))


def test_smoothing_feeds_the_incremental_path():
    """full run, smooth, incremental run over the union box, full run.  The incremental run is compared with the port's
    Modification of the oracle-edited grid over the same box (ids and surface) and, at level 0, block by block with a fresh full
    run of that grid, paired by corner: a surface that went through a Modification numbers its rebuilt blocks anew in the
    reference itself (port.execute_modify against port.execute: 'L0 block info field id differs', whatever the box), and its
    upper levels differ likewise - tests/test_gpu_islands.py pairs the same way.  [a, b + 1] is the box the path needs."""
    n = 64
    port = vxo.load_port()
    d, m, b = so.terrain(n, 12)
    g = port.grid_from_dense(d, m, b)
    ops = so.stack([so.smooth_op(((18, 20, 14), (46, 44, 50)), (32.5, 31.25, 30.0), 14.0, 1.0, 3)])
    want = so.apply(d, ops)
    assert want.changed > 50
    p = new_poly()
    p.upload_packed(g.pack())
    p.execute()
    s = port.execute(g)
    ok, msg = fields.surface_equal(p.all_levels(), s.all_levels())
    assert ok, msg
    got = p.smooth(ops)
    same_results(got, want)
    g2 = port.grid_from_dense(want.dist, m, b)
    assert np.array_equal(p.pack(), g2.pack())
    ref_ids = port.execute_modify(g2, s, got[1], got[2])
    ids = p.execute_dirty(got[1], got[2])
    assert np.array_equal(ids, ref_ids)
    ok, msg = fields.surface_equal(p.all_levels(), s.all_levels())
    assert ok, msg
    fresh = port.execute(g2)
    part, full = p.all_levels()[0], fresh.all_levels()[0]
    assert len(part.infos) == len(full.infos)
    at = {tuple(c): i for c, i in zip(full.infos["min_corner"].tolist(), full.infos["id"])}
    part.infos = part.infos.copy()
    part.infos["id"] = [at[tuple(c)] for c in part.infos["min_corner"].tolist()]
    ok, msg = fields.listed_blocks_equal_by_id(part, full)
    assert ok, msg
    # a full run afterwards: the mirrors followed the smoothing
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())
    assert np.array_equal(p.pack(), g2.pack())


def test_invalid_ops_leave_the_grid_untouched():
    import ctypes as C
    import torch
    from voxels_amd.binding import VoxelsHipError
    n = 48
    d = so.noise(n, 2)
    p, mat, blend, g = resident(d)
    before = p.pack()
    box = ((0, 0, 0), (n, n, n))
    good = so.smooth_op(box)
    bad = [so.smooth_op(((4, 4, 4), (4, 8, 8))), so.smooth_op(((4, 9, 4), (8, 8, 8))), so.smooth_op(((4, 4, 4), (8, 8, 49))), so.smooth_op(((4, 4, 4), (49, 8, 8))),
           so.smooth_op(box, (np.nan, 0.0, 0.0), 4.0), so.smooth_op(box, (0.0, np.inf, 0.0), 4.0), so.smooth_op(box, radius=np.inf), so.smooth_op(box, radius=np.nan),
           so.smooth_op(box, strength=np.nan), so.smooth_op(box, radius=-1.0), so.smooth_op(box, strength=-0.01), so.smooth_op(box, strength=1.01),
           so.smooth_op(box, iterations=65)]

    def call(ops, count=None, with_outputs=True):
        ops = None if ops is None else np.ascontiguousarray(ops)
        count = ops.size if count is None else count
        res = np.zeros(max(count, 1), so.SMOOTH_RESULT_DTYPE)
        mn, mx, ch = np.ones(3, np.float32), np.ones(3, np.float32), C.c_uint64(7)
        rc = p._lib.vx_grid_smooth(p._h, None if ops is None else ops.ctypes.data, count, res.ctypes.data if with_outputs else None,
                                   mn.ctypes.data if with_outputs else None, mx.ctypes.data if with_outputs else None, C.byref(ch) if with_outputs else None)
        return rc, mn, mx, ch.value

    for op in bad:
        for ops in (op, so.stack([good, op])):          # the bad op alone, and behind a good one: nothing may have been launched
            rc, mn, mx, ch = call(ops)
            assert rc == -1, op
            assert not mn.any() and not mx.any() and ch == 0
            assert np.array_equal(p.pack(), before)
    assert call(None, 1)[0] == -1
    assert call(np.repeat(good, (1 << 16) + 1))[0] == -1
    assert np.array_equal(p.pack(), before)
    # nothing to do is not an error
    assert call(None, 0)[0] == 0 and call(good, 0)[0] == 0
    assert np.array_equal(p.pack(), before)
    # the outputs may be NULL
    assert call(so.smooth_op(((4, 4, 4), (9, 9, 9)), strength=0.37), with_outputs=False)[0] == 0
    want = so.apply(d, so.smooth_op(((4, 4, 4), (9, 9, 9)), strength=0.37))
    assert np.array_equal(p.pack(), packed(want.dist, mat, blend))
    # an attached grid is not the context's own; neither is no grid at all
    dev = torch.device("cuda:0")
    td, tm, tb = (torch.from_numpy(x.copy()).to(dev) for x in (d, mat, blend))
    tf = torch.from_numpy(g.block_flags().copy()).to(dev)
    a = new_poly()
    a.attach(n, 0, n, td.data_ptr(), 0, tm.data_ptr(), tb.data_ptr(), 0, tf.data_ptr())
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        a.smooth(good)
    torch.cuda.synchronize()
    assert np.array_equal(td.cpu().numpy(), d)
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        new_poly().smooth(good)
