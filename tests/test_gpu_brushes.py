"""vx_grid_inject_brushes on the MI355X: an ordered batch of brushes in one device pass leaves, byte for byte, what the same
brushes leave one call at a time - against vx_grid_inject_ball / vx_grid_inject_material on a twin context, against the
reference and the port through tests/vxo.py (ball and material lists), and against the host oracle of
tests/brush/brush_host.cpp (capsules and boxes; tests/test_brushes.py anchors that oracle to the reference).  Every
comparison is exact: the packed file of the device grid, the boxes, the counts."""
import ctypes as C

import numpy as np
import pytest

import brush_oracle as bo
import fields
import vxo

pytestmark = pytest.mark.gpu


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def field_grid(oracle, n, seed):
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    return oracle.grid_from_float(f, m, b)


def synth_grid(oracle, n, seed=1337):
    from voxels_amd import synth
    d, m, b = synth.terrain(n, seed=seed)
    return oracle.grid_from_dense(d, m, b)


def checkers(n):
    ref = vxo.load_ref()
    return ([ref] if ref is not None and n <= 80 else []) + [vxo.load_port()]


def check_results(res, umin, umax, touched, boxes, counts, distinct=None):
    assert np.array_equal(np.concatenate([res["out_min"], res["out_max"]], axis=1), boxes)
    assert np.array_equal(res["touched_blocks"], counts)
    wmin, wmax = bo.union_box(boxes, counts)
    assert np.array_equal(umin, wmin) and np.array_equal(umax, wmax)
    if distinct is not None:
        assert touched == distinct


def check_against_host(p, d, m, b, brushes, label):
    """the batch on the device (grid already resident) against the host oracle on the dense fields"""
    want = bo.apply(d, m, b, brushes)
    res, umin, umax, touched = p.inject_brushes(brushes)
    check_results(res, umin, umax, touched, want.boxes, want.touched)
    assert np.array_equal(p.pack(), want.pack), label
    return want, touched


def test_one_brush_batches_equal_the_single_brush_calls():
    """the brush cases of check_brushes_anywhere (tests/test_emu.py), each as a batch of one, against the twin context"""
    port = vxo.load_port()
    n = 48
    g = field_grid(port, n, 3)
    one, twin = new_poly(), new_poly()
    one.upload_packed(g.pack()); twin.upload_packed(g.pack())
    balls = bo.anywhere_balls(n, 48, seed=77)
    for k, br in enumerate(balls):
        mn, mx = twin.inject_ball(br["position"], br["extents"], float(br["radius"]), int(br["type"]))
        res, umin, umax, touched = one.inject_brushes(bo.stack([br]))
        assert np.array_equal(res["out_min"][0], mn) and np.array_equal(res["out_max"][0], mx), k
        assert (touched == 0) == (res["touched_blocks"][0] == 0)
        if touched:
            assert np.array_equal(umin, mn) and np.array_equal(umax, mx), k
        else:
            assert not umin.any() and not umax.any()
        if k % 4 == 3:
            mb = bo.material(br["position"], br["extents"], 7 + k % 5, k % 8 < 4)
            mn, mx = twin.inject_material(mb["position"], mb["extents"], int(mb["material"]), bool(mb["type"]))
            res, _, _, _ = one.inject_brushes(bo.stack([mb]))
            assert np.array_equal(res["out_min"][0], mn) and np.array_equal(res["out_max"][0], mx), k
        assert np.array_equal(one.pack(), twin.pack()), "brush %d" % k
    assert (balls["extents"] == 0).all(axis=1).any()


@pytest.mark.parametrize("n", [64, 80, 256])
@pytest.mark.parametrize("count", [1, 7, 256, 4096])
def test_ball_lists_equal_sequential_calls_on_the_cpu(n, count):
    brushes = bo.anywhere_balls(n, count, seed=count) if count <= 7 else bo.scattered_balls(n, count, seed=count + n)
    for o in checkers(n):
        g = synth_grid(o, n) if n == 256 else field_grid(o, n, 11)
        p = new_poly()
        p.upload_packed(g.pack())
        boxes = bo.sequential(g, brushes)
        res, umin, umax, touched = p.inject_brushes(brushes)
        assert np.array_equal(np.concatenate([res["out_min"], res["out_max"]], axis=1), boxes), (o.kind, n, count)
        wmin, wmax = bo.union_box(boxes, res["touched_blocks"])
        assert np.array_equal(umin, wmin) and np.array_equal(umax, wmax)
        assert np.array_equal(p.pack(), g.pack()), "%d balls on %d^3 (%s)" % (count, n, o.kind)
        assert np.array_equal(np.array([p.read_block(i)[3] for i in range(0, (n // 16) ** 3, 7)], np.uint8), g.block_flags()[::7])
        p.close()


def mixed_list(n, count, seed):
    """ball, capsule, box and material interleaved; all three injection types; some miss the grid"""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        pos = rng.uniform(-4, n + 4, 3).round(2)
        if k % 11 == 5:
            pos = pos + 4.0 * n  # misses the grid, in the middle of the list
        r = float(rng.uniform(2, 6))
        t = (2, 0, 1)[k % 3]
        kind = k % 4
        if kind == 0:
            out.append(bo.ball(pos, (2 * r + 4,) * 3, r, t))
        elif kind == 1:
            q = pos + rng.uniform(-9, 9, 3).round(2)
            out.append(bo.capsule_stroke(pos, q, r, t))
        elif kind == 2:
            half = rng.uniform(1, 7, 3).round(2)
            out.append(bo.box(pos, tuple(2 * half + 2 * 1.5 + 4), half, 1.5, t))
        else:
            out.append(bo.material(pos, tuple(rng.choice([3.0, 8.0, 17.0], 3)), 3 + k % 6, k % 8 < 4))
    return bo.stack(out)


def resident(n, seed):
    port = vxo.load_port()
    g = field_grid(port, n, seed)
    d, m, b = g.read_dense()
    p = new_poly()
    p.upload_packed(g.pack())
    return p, d, m, b, g


@pytest.mark.parametrize("n", [64, 80])
def test_mixed_lists_equal_the_host_oracle(n):
    p, d, m, b, _ = resident(n, 5)
    brushes = mixed_list(n, 600, seed=n)
    assert set(brushes["shape"].tolist()) == {0, 1, 2, 3} and set(brushes[brushes["shape"] != 3]["type"].tolist()) == {0, 1, 2}
    want, _ = check_against_host(p, d, m, b, brushes, "mixed list on %d^3" % n)
    assert (want.touched == 0).any() and (want.touched > 0).any()
    # a second batch goes on from the first one's grid
    more = mixed_list(n, 200, seed=n + 1)
    check_against_host(p, want.dist, want.mat, want.blend, more, "second mixed list on %d^3" % n)


def test_a_stroke_of_500_capsules():
    n = 64
    p, d, m, b, _ = resident(n, 6)
    s = np.linspace(0.0, 1.0, 501)
    path = np.stack([8 + 48 * s, 32 + 18 * np.sin(5 * s), 30 + 10 * np.cos(3 * s)], axis=1).astype(np.float32)
    brushes = bo.stack([bo.capsule_stroke(path[i], path[i + 1], 3.5, 2 if i % 50 else 0) for i in range(500)])
    check_against_host(p, d, m, b, brushes, "capsule stroke")


def test_2000_brushes_on_one_block():
    n = 64
    p, d, m, b, _ = resident(n, 7)
    rng = np.random.RandomState(3)
    out = []
    for k in range(2000):
        pos = rng.uniform(33.0, 47.0, 3).round(2)   # every brush touches block (2, 2, 2)
        r = float(rng.uniform(0.5, 2.5))
        if k % 3 == 0:
            out.append(bo.ball(pos, (2.0, 2.0, 2.0), r, (2, 0, 1)[k % 3]))
        elif k % 3 == 1:
            out.append(bo.capsule_stroke(pos, pos + rng.uniform(-2, 2, 3).round(2), r, (2, 0, 1)[(k // 3) % 3], margin=0.5))
        else:
            out.append(bo.material(pos, (3.0, 3.0, 3.0), k % 5, k % 2 == 0) if k % 2 else bo.box(pos, (4.0, 4.0, 4.0), (1.0, 1.5, 0.5), 0.5, (0, 2, 1)[(k // 3) % 3]))
    brushes = bo.stack(out)
    want, _ = check_against_host(p, d, m, b, brushes, "2000 brushes on one block")
    one = (2 * 4 + 2) * 4 + 2
    assert want.dist_touched[one] and (want.touched > 0).all()


def test_a_list_whose_union_is_the_whole_grid():
    n = 64
    p, d, m, b, _ = resident(n, 8)
    fn = float(n)
    brushes = bo.stack([bo.ball((20.0, 20.0, 20.0), (12.0, 12.0, 12.0), 4.0, 2),
                        bo.box((fn / 2, fn / 2, fn / 2), (fn, fn, fn), (fn / 4, fn / 3, fn / 5), 3.0, 1),
                        bo.material((fn / 2, fn / 2, fn / 2), (fn, fn, fn), 4, True),
                        bo.capsule_stroke((5.0, 5.0, 5.0), (60.0, 58.0, 50.0), 6.0, 2)])
    _, touched = check_against_host(p, d, m, b, brushes, "whole grid")
    res, umin, umax, _ = p.inject_brushes(brushes[1:2])
    assert touched == (n // 16) ** 3 and not umin.any() and (umax == fn).all()


def test_order_matters():
    n = 64
    fwd = bo.stack([bo.ball((32.0, 32.0, 30.0), (20.0, 20.0, 20.0), 8.0, 0), bo.ball((33.0, 32.0, 30.0), (20.0, 20.0, 20.0), 8.0, 2),
                    bo.box((30.0, 34.0, 30.0), (14.0, 14.0, 14.0), (3.0, 3.0, 3.0), 1.0, 0), bo.capsule_stroke((26.0, 30.0, 28.0), (38.0, 34.0, 32.0), 3.0, 2)])
    packs = []
    for brushes in (fwd, fwd[::-1].copy()):
        p, d, m, b, _ = resident(n, 9)
        want, _ = check_against_host(p, d, m, b, brushes, "order")
        packs.append(want.pack)
    assert not np.array_equal(packs[0], packs[1])


def test_flags_follow_the_codec_only_where_a_distance_brush_touched():
    n = 64
    nb = n // 16
    port = vxo.load_port()
    g = field_grid(port, n, 10)
    d, m, b = g.read_dense()
    codec = g.block_flags()
    caller = codec.copy()
    caller[::3] ^= 1   # disagrees with the codec on touched and on untouched blocks
    p = new_poly()
    p.upload(d, m, b, caller)
    brushes = bo.stack([bo.ball((20.0, 20.0, 20.0), (10.0, 10.0, 10.0), 4.0, 2), bo.material((50.0, 50.0, 50.0), (10.0, 10.0, 10.0), 5, True),
                        bo.capsule_stroke((10.0, 40.0, 40.0), (30.0, 44.0, 40.0), 3.0, 0), bo.box((40.0, 10.0, 12.0), (9.0, 9.0, 9.0), (2.0, 2.0, 2.0), 1.0, 2)])
    want = bo.apply(d, m, b, brushes)
    p.inject_brushes(brushes)
    got = np.array([p.read_block(i)[3] for i in range(nb ** 3)], np.uint8)
    expect = np.where(want.dist_touched != 0, want.flags, caller)
    assert np.array_equal(got, expect)
    touched, untouched = want.dist_touched != 0, want.dist_touched == 0
    assert (caller[touched] != want.flags[touched]).any() and (caller[untouched] != codec[untouched]).any()
    # as sequential single-brush calls leave them
    twin = new_poly()
    twin.upload(d, m, b, caller)
    twin.inject_ball(brushes[0]["position"], brushes[0]["extents"], 4.0, 2)
    twin.inject_material(brushes[1]["position"], brushes[1]["extents"], 5, True)
    ball_blocks = bo.apply(d, m, b, brushes[:1]).dist_touched != 0
    tw = np.array([twin.read_block(i)[3] for i in range(nb ** 3)], np.uint8)
    assert np.array_equal(tw[ball_blocks], got[ball_blocks]) and np.array_equal(tw[untouched], got[untouched])
    for blk in np.nonzero(touched)[0][:8]:
        z, y, x = blk // (nb * nb), (blk // nb) % nb, blk % nb
        assert np.array_equal(p.read_block(int(blk))[0], want.dist[z * 16:z * 16 + 16, y * 16:y * 16 + 16, x * 16:x * 16 + 16])


def test_batches_feed_the_incremental_path():
    n = 64
    port = vxo.load_port()
    g = field_grid(port, n, 12)
    s = port.execute(g)
    p = new_poly()
    p.upload_packed(g.pack())
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), s.all_levels())
    assert ok, msg
    for round_, seed in enumerate((1, 2)):
        rng = np.random.RandomState(seed)
        c = rng.uniform(22, 40, 3)
        brushes = bo.stack([bo.ball(tuple((c + rng.uniform(-5, 5, 3)).round(2)), (12.0, 12.0, 12.0), float(rng.uniform(3, 5)), 2 if k % 3 else 0) for k in range(12)])
        boxes = bo.sequential(g, brushes)
        res, umin, umax, touched = p.inject_brushes(brushes)
        assert touched > 0 and np.array_equal(np.concatenate([res["out_min"], res["out_max"]], axis=1), boxes)
        ref_ids = port.execute_modify(g, s, umin, umax)
        got = p.execute_dirty(umin, umax)
        assert np.array_equal(got, ref_ids), round_
        ok, msg = fields.surface_equal(p.all_levels(), s.all_levels())
        assert ok, "batch %d: %s" % (round_, msg)
        assert np.array_equal(p.stats(), s.stats())
    # a full run afterwards: the mirrors and the re-bricking followed the batches
    p.execute()
    fresh = port.execute(g)
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())
    assert np.array_equal(p.pack(), g.pack())


def test_errors_leave_the_grid_untouched():
    from voxels_amd.binding import VoxelsHipError
    import torch
    n = 64
    p, d, m, b, g = resident(n, 13)
    before = p.pack()
    good = bo.scattered_balls(n, 8, seed=1)
    cases = []
    for field, value in (("shape", 4), ("type", 3), ("radius", np.nan), ("position", (1.0, np.inf, 2.0)), ("a", (np.nan, 0.0, 0.0))):
        bad = good.copy()
        bad[field][5] = value
        cases.append(bad)
    bad = good.copy(); bad["shape"][3] = bo.BRUSH_MATERIAL; bad["type"][3] = 2
    cases.append(bad)
    for bad in cases:
        with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
            p.inject_brushes(bad)
        assert np.array_equal(p.pack(), before)
    lib = p._lib
    assert lib.vx_grid_inject_brushes(p._h, None, 3, None, None, None, None) == -1
    assert lib.vx_grid_inject_brushes(p._h, None, 0, None, None, None, None) == 0
    res, umin, umax, touched = p.inject_brushes(np.zeros(0, bo.BRUSH_DTYPE))
    assert len(res) == 0 and touched == 0 and np.array_equal(p.pack(), before)
    # a list that misses the grid: a no-op with zero boxes
    miss = good.copy(); miss["position"] += 1000.0
    res, umin, umax, touched = p.inject_brushes(miss)
    assert touched == 0 and not umin.any() and not umax.any() and np.array_equal(p.pack(), before)
    # an attached grid is not the context's own
    dev = torch.device("cuda:0")
    td, tm, tb = (torch.from_numpy(x.copy()).to(dev) for x in (d, m, b))
    tf = torch.from_numpy(g.block_flags().copy()).to(dev)
    q = new_poly()
    q.attach(n, 0, n, td.data_ptr(), 0, tm.data_ptr(), tb.data_ptr(), 0, tf.data_ptr())
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        q.inject_brushes(good)
    torch.cuda.synchronize()
    assert np.array_equal(td.cpu().numpy(), d) and np.array_equal(tm.cpu().numpy(), m) and np.array_equal(tb.cpu().numpy(), b)
    with pytest.raises(VoxelsHipError, match=r"\(-1\)"):
        new_poly().inject_brushes(good)   # no grid at all


def test_the_same_list_twice_gives_the_same_bytes():
    n = 128
    port = vxo.load_port()
    g = synth_grid(port, n, seed=5)
    blob = g.pack()
    brushes = np.concatenate([bo.scattered_balls(n, 2048, seed=21), mixed_list(n, 2048, seed=22)])
    rng = np.random.RandomState(1)
    brushes = brushes[rng.permutation(len(brushes))]
    packs = []
    for _ in range(2):
        p = new_poly()
        p.upload_packed(blob)
        res, umin, umax, touched = p.inject_brushes(brushes)
        packs.append((p.pack(), res.tobytes(), umin.tobytes(), umax.tobytes(), touched))
        p.close()
    assert np.array_equal(packs[0][0], packs[1][0]) and packs[0][1:] == packs[1][1:]
    assert not np.array_equal(packs[0][0], blob)
