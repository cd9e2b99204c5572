#!/usr/bin/env python3
"""What the height maps (vx_grid_heightmap / vx_grid_heightmap_device) cost on the device terrain, beside three yardsticks taken
in the same run, alternating with the call they stand beside:
  memcpy   a plain device-to-device hipMemcpyAsync of the output bytes plus the distance bytes of the blocks the walk must read.
           Those are counted from the result: per tile the blocks between the highest and the lowest layer-0 surface (with the
           sign summaries on, blocks of one sign need no rows), up to the box's end in the scan direction's back where the
           summaries are off, and the whole stack where the summaries are off and the walk cannot leave early.
  measure  vx_grid_measure of the whole-grid box with the same shortcut setting, the nearest existing walk
  stamp    the route a height map replaces, on a 256 x 256 x n box: vx_stamp_capture + vx_stamp_read + the numpy oracle
Runs: (a) whole-grid top map, one layer; (b) the same with VX_HEIGHT_COUNT_SURFACES; (c) both with the sign summaries off;
(d) 8 layers; (e) from the bottom; (f) a 256 x 256 footprint; (g) the device form without counts, timed by events; (h) 2 000
random columns, 8 layers, both directions, against the numpy oracle of the tests.
One process, warm-up first, medians over the repetitions, wall time of a whole synchronous call (the arrays are allocated and
touched beforehand).
Usage (GPU box): python tools/height_bench.py [n] [repetitions]"""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from undo_bench import DeviceCopy, med, timed  # noqa: E402
from voxels_amd import HEIGHT_COUNTS_DTYPE, HEIGHT_NONE, Polygonizer, height_query, synth  # noqa: E402
from voxels_amd.binding import boxes as make_boxes  # noqa: E402


class Copy:
    """one device-to-device copy of `nbytes`, timed to its completion; the buffers are kept"""

    def __init__(self, copier, nbytes):
        self.hip, self.nbytes = copier.hip, max(int(nbytes), 16)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.a), self.nbytes) == 0 and self.hip.hipMalloc(C.byref(self.b), self.nbytes) == 0

    def __call__(self):
        assert self.hip.hipMemcpyAsync(self.b, self.a, self.nbytes, 3, None) == 0 and self.hip.hipDeviceSynchronize() == 0

    def free(self):
        self.hip.hipFree(self.a); self.hip.hipFree(self.b)


def alternating(reps, *fns):
    """every fn once per round, round after round; 2 warm-up rounds -> the medians in ms"""
    rows = [[] for _ in fns]
    for k in range(reps + 2):
        for i, fn in enumerate(fns):
            t = timed(fn)[0]
            if k >= 2:
                rows[i].append(t)
    return [med(r) for r in rows]


def blocks_read(top_map, n, top, summaries, early):
    """The blocks whose distance rows a walk has to read, per tile, from the layer-0 heights [H, W] of the TOP map of the same
    footprint (aligned to blocks) on a terrain - one surface per column, solid below it, air above: the band of blocks between a
    tile's highest and lowest surface voxel is what holds both signs.
      summaries on, from the top      the band (blocks of one sign need no rows, whether or not the walk leaves early)
      summaries on, from the bottom   nothing where the stack's lowest block is below the band (it is all solid: the clipped
                                      surface at the box's end needs no row), else the band's lowest block
      summaries off, early exit       from the top of the stack down to the band's lowest block (from the top)
      summaries off, no early exit    the whole stack"""
    nb = n // 16
    z = np.clip((top_map.astype(np.int64) - 1) >> 8, 0, n - 1)    # h = z * 256 + f, f = 2..256
    z[top_map == HEIGHT_NONE] = 0
    hh, ww = top_map.shape
    zb = (z >> 4).reshape(hh // 16, 16, ww // 16, 16)
    tiles_hi, tiles_lo = zb.max(axis=(1, 3)), zb.min(axis=(1, 3))
    if summaries:
        return int((tiles_hi - tiles_lo + 1).sum()) if top else int((tiles_lo == 0).sum())
    if not early:
        return tiles_hi.size * nb
    assert top
    return int((nb - tiles_lo).sum())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)                            # the mirrors, and with them the sign summaries, are current
    copier = DeviceCopy()
    lib, h = p._lib, p._h
    whole = ((0, 0, 0), (n, n, n))
    whole_box = make_boxes([whole])
    print("grid %d^3 device terrain, %d repetitions after 2 warm-up rounds, medians, wall time of a whole synchronous call;" % (n, reps))
    print("each call alternates with its yardsticks, round after round")

    def shortcuts(on):
        assert lib.vx_debug_height_shortcuts(h, on) == 0 and lib.vx_debug_measure_shortcuts(h, on) == 0

    def host_call(box, direction, layers, flag):
        q = height_query(box, direction, layers, flag)
        w, hh = int(box[1][0] - box[0][0]), int(box[1][1] - box[0][1])
        heights, mats = np.zeros((layers, hh, w), np.uint32), np.zeros((layers, hh, w), np.uint8)
        surfaces = np.zeros((hh, w), np.uint16) if flag else None
        counts = np.zeros(1, HEIGHT_COUNTS_DTYPE)

        def call():
            rc = lib.vx_grid_heightmap(h, q.ctypes.data, heights.ctypes.data, mats.ctypes.data, None if surfaces is None else surfaces.ctypes.data, counts.ctypes.data)
            assert rc == 0
        return call, heights, mats, surfaces, counts

    tops = {}

    def top_of(box):
        if box not in tops:
            tops[box] = p.heightmap(box, "top", 1, False, False)[0][0]
        return tops[box]

    def row(label, box, direction, layers, flag, summaries, with_measure=True):
        shortcuts(1 if summaries else 0)
        call, heights, mats, surfaces, counts = host_call(box, direction, layers, flag)
        call()
        out_bytes = heights.nbytes + mats.nbytes + (0 if surfaces is None else surfaces.nbytes)
        blocks = blocks_read(top_of(box), n, direction == "top", summaries, not flag and layers == 1)
        copy = Copy(copier, out_bytes + blocks * 4096)
        fns = [call, copy] + ([lambda: p.measure(whole_box, tallies=False)] if with_measure else [])
        t = alternating(reps, *fns)
        copy.free()
        c = counts[0]
        text = "  %s: %.4f ms | memcpy of %.1f MB (%.1f MB out + %d blocks of distances) %.4f ms: call / memcpy %.2f" % (
            label, t[0], copy.nbytes / 1e6, out_bytes / 1e6, blocks, t[1], t[0] / t[1])
        if with_measure:
            text += " | vx_grid_measure of the whole grid %.4f ms: call / measure %.2f" % (t[2], t[0] / t[2])
        print(text)
        print("      covered %d of %d columns, heights %.2f .. %.2f, clipped %d, surfaces %d, most in a column %d" % (
            int(c["covered"]), int(c["columns"]), int(c["min_height"]) / 256.0, int(c["max_height"]) / 256.0, int(c["clipped"]), int(c["surfaces"]), int(c["max_surfaces"])))
        shortcuts(1)
        return t[0], heights, mats

    ta, top1, topm = row("(a) whole grid from the top, 1 layer, early exit, summaries on", whole, "top", 1, False, True)
    row("(b) the same with VX_HEIGHT_COUNT_SURFACES", whole, "top", 1, True, True)
    _, off1, _ = row("(c) as (a), summaries off", whole, "top", 1, False, False)
    row("(c) as (b), summaries off", whole, "top", 1, True, False)
    assert np.array_equal(off1, top1)
    _, top8, _ = row("(d) 8 layers", whole, "top", 8, False, True)
    assert np.array_equal(top8[0], top1[0])
    _, bottom1, _ = row("(e) from the bottom, 1 layer", whole, "bottom", 1, False, True)

    # (f) a 256 x 256 footprint, and the route it replaces
    size = min(256, n)
    lo = n // 2 - size // 2
    foot = ((lo, lo, 0), (lo + size, lo + size, n))
    tf, fh, fm = row("(f) a %d x %d footprint, all z, from the top, 1 layer (%d workgroups)" % (size, size, (size // 16) ** 2), foot, "top", 1, False, True, with_measure=False)
    assert np.array_equal(fh[0], top1[0][lo:lo + size, lo:lo + size])
    import height_oracle as ho

    def stamp_route():
        st = p.capture_stamp(foot)
        d, m, b = st.read()
        st.free()
        return ho.heightmap(SimpleNamespace(dist=d, mat=m), ((0, 0, 0), (size, size, n)), ho.HEIGHT_FROM_TOP, 1, False)
    call = host_call(foot, "top", 1, False)[0]
    t = alternating(min(reps, 5), call, stamp_route)
    want = stamp_route()
    assert np.array_equal(want[0], fh) and np.array_equal(want[1], fm)
    print("      the route it replaces: vx_stamp_capture + vx_stamp_read + the numpy oracle %.1f ms against %.4f ms (%.0f x), the same heights and materials" % (t[1], t[0], t[1] / t[0]))

    # (g) the device form without counts, timed by events on the context's stream
    import torch
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    dh = torch.zeros(n * n, dtype=torch.int32, device="cuda:0")
    dm = torch.zeros(n * n, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    rows = []
    for k in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        p.heightmap_device(whole, dh, "top", 1, dm, None, counts=False)
        e1.record(stream)
        e1.synchronize()
        if k >= 2:
            rows.append(e0.elapsed_time(e1))
    assert np.array_equal(dh.cpu().numpy().view(np.uint32).reshape(n, n), top1[0]) and np.array_equal(dm.cpu().numpy().reshape(n, n), topm[0])
    p.set_stream(0)
    print("  (g) the device form of (a) without counts, between two events on the context's stream: %.4f ms (the host form: %.4f ms)" % (med(rows), ta))

    # (h) 2 000 random columns against the numpy oracle, from a 1 x 1 x n stamp each
    bottom8 = p.heightmap(whole, "bottom", 8, True, False)
    rng = np.random.RandomState(9)
    for x, y in rng.randint(0, n, (2000, 2)):
        st = p.capture_stamp(((x, y, 0), (x + 1, y + 1, n)))
        d, m, b = st.read()
        st.free()
        g = SimpleNamespace(dist=d, mat=m)
        for direction, got in ((ho.HEIGHT_FROM_TOP, (top8, None)), (ho.HEIGHT_FROM_BOTTOM, bottom8)):
            want = ho.heightmap(g, ((0, 0, 0), (1, 1, n)), direction, 8, False)
            assert np.array_equal(want[0][:, 0, 0], got[0][:, y, x]), (x, y, direction)
            if got[1] is not None:
                assert np.array_equal(want[1][:, 0, 0], got[1][:, y, x]), (x, y, direction)
    assert np.array_equal(bottom8[0][0], bottom1[0])
    print("  (h) 2000 random columns, 8 layers, from the top and from the bottom, equal the numpy oracle")


if __name__ == "__main__":
    main()
