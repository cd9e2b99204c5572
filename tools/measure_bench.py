#!/usr/bin/env python3
"""What the measurements (vx_grid_measure / vx_record_measure) cost on the device terrain, beside two yardsticks of the same run:
a plain device-to-device hipMemcpyAsync of the bytes a call must read (distance and material of the covered blocks, 8 192 per
(box, block) pair), and the route the call replaces - vx_stamp_capture + vx_stamp_read + np.bincount on the host - for one 256^3 box.
  (a) one whole-grid box, with and without the sign-summary shortcuts
  (b) 4 096 boxes of 32^3 centred on the craters of tools/undo_bench.py
  (c) 65 536 boxes of 16^3 at random unaligned origins, with and without the copy back of the tallies
  (d) vx_record_measure on the records of the 256-brush stroke and the 4 096 craters of tools/undo_bench.py
  (e) 2 000 boxes of (c) against the numpy oracle of the tests
One process, warm-up first, medians over the repetitions, wall time of a call: both calls wait for the device themselves.
Usage (GPU box): python tools/measure_bench.py [n] [repetitions] [parts, default abcde]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from undo_bench import DeviceCopy, med, timed  # noqa: E402
from voxels_amd import BOX_DTYPE, Polygonizer, brush_boxes, synth  # noqa: E402
from voxels_amd.binding import BRUSH_BALL, BRUSH_DTYPE, boxes as make_boxes  # noqa: E402


def pairs_of(bx):
    return int(np.prod(((bx["hi"].astype(np.int64) + 15) >> 4) - (bx["lo"].astype(np.int64) >> 4), axis=1).sum())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    parts = sys.argv[3] if len(sys.argv) > 3 else "abcde"
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)                            # the mirrors, and with them the sign summaries, are current
    copier = DeviceCopy()
    lib, h = p._lib, p._h
    x0, y0 = n / 2.0 - 154.0, n / 2.0 + 0.37
    col = p.column(n, int(n / 2), int(y0))
    zs = float(np.argmax(col >= 0)) if (col >= 0).any() else n / 2.0
    print("grid %d^3 device terrain (surface near z = %d), %d repetitions after 2 warm-up calls, medians, wall time of a call" % (n, zs, reps))

    def run(bx, tallies, rounds=reps):
        rows = []
        for k in range(rounds + 2):
            t, out = timed(lambda: p.measure(bx, tallies=tallies))
            if k >= 2:
                rows.append(t)
        return med(rows), out

    def report(label, bx, t, rounds=reps):
        pairs = pairs_of(bx)
        copy = copier.ms(pairs * 8192, min(rounds, 5))
        print("  %s: %d boxes, %d (box, block) pairs = %.1f MB of distances and materials; %.4f ms = %.1f GB/s; memcpy of the same bytes %.4f ms: %.2f of its rate"
              % (label, bx.size, pairs, pairs * 8192 / 1e6, t, pairs * 8192 / t / 1e6, copy, copy / t))

    if "a" in parts:
        whole = make_boxes([((0, 0, 0), (n, n, n))])
        for on in (1, 0):
            assert lib.vx_debug_measure_shortcuts(h, on) == 0
            t, (res, tal) = run(whole, True, min(reps, 5))
            report("(a) the whole grid, sign summaries %s" % ("on" if on else "off"), whole, t, 3)
        assert lib.vx_debug_measure_shortcuts(h, 1) == 0
        print("      %d of %d voxels solid, %d materials, bounds %s .. %s" % (int(res[0]["solid_voxels"]), int(res[0]["voxels"]), int(res[0]["materials"]), res[0]["min"].tolist(), res[0]["max"].tolist()))
        size = min(256, n)
        lo = (n // 2 - size // 2, n // 2 - size // 2, int(max(min(zs - size // 2, n - size), 0)))
        box = make_boxes([(lo, tuple(v + size for v in lo))])

        def stamp_route():
            st = p.capture_stamp((tuple(box[0]["lo"]), tuple(box[0]["hi"])))
            d, m, _ = st.read()
            st.free()
            return np.bincount(m[d < 0], minlength=256)
        rows = [timed(stamp_route)[0] for _ in range(5)][2:]
        t, (res, tal) = run(box, True)
        assert np.array_equal(stamp_route().astype(np.uint64), tal[0])
        print("      one %d^3 box: vx_grid_measure %.4f ms | vx_stamp_capture + vx_stamp_read + np.bincount %.1f ms (%.0f x), the same tallies" % (size, t, med(rows), med(rows) / t))

    rng = np.random.RandomState(4)          # the craters of tools/undo_bench.py
    craters = np.zeros(4096, BRUSH_DTYPE)
    craters["position"][:, 0] = rng.uniform(8, n - 8, 4096); craters["position"][:, 1] = rng.uniform(8, n - 8, 4096)
    craters["position"][:, 2] = zs + rng.uniform(-6, 6, 4096)
    craters["shape"] = BRUSH_BALL; craters["radius"] = rng.uniform(3, 6, 4096)
    craters["extents"] = (2 * craters["radius"] + 4)[:, None]; craters["type"] = 2
    if "b" in parts:
        lo = np.clip(np.floor(craters["position"]).astype(np.int64) - 16, 0, n - 32)
        bx = np.zeros(4096, BOX_DTYPE)
        bx["lo"], bx["hi"] = lo, lo + 32
        for tallies in (True, False):
            t, _ = run(bx, tallies)
            report("(b) 32^3 boxes on the craters, tallies %s" % ("copied back" if tallies else "left on the device"), bx, t)

    rng = np.random.RandomState(7)
    lo = rng.randint(0, n - 16, (65536, 3))
    small = np.zeros(65536, BOX_DTYPE)
    small["lo"], small["hi"] = lo, lo + 16
    if "c" in parts:
        for tallies in (True, False):
            t, _ = run(small, tallies, min(reps, 5))
            report("(c) 16^3 boxes at random origins, tallies %s" % ("copied back (134 MB)" if tallies else "left on the device"), small, t, 3)

    if "d" in parts:
        s = np.arange(256, dtype=np.float64)
        stroke = np.zeros(256, BRUSH_DTYPE)
        stroke["position"] = np.stack([x0 + 1.2 * s, y0 + 6.0 * np.sin(s / 20.0), zs + 3.0 * np.cos(s / 33.0)], axis=1).astype(np.float32)
        stroke["shape"] = BRUSH_BALL; stroke["extents"] = 2 * 4.0 + 4; stroke["type"] = 2; stroke["radius"] = 4.0
        for label, brushes in (("256-brush stroke", stroke), ("4096 craters", craters)):
            bx = brush_boxes(brushes, n, p._L)
            rec = p.capture(bx)
            held = int(rec.info()["blocks"])
            p.inject_brushes(brushes)
            rows = [timed(rec.measure)[0] for _ in range(reps + 2)][2:]
            delta, removed, added = rec.measure()
            copy = copier.ms(held * 16384, reps)
            print("  (d) vx_record_measure, %s: %d held blocks = %.1f MB of distances and materials on both sides; %.4f ms = %.1f GB/s; memcpy of the same bytes %.4f ms: %.2f of its rate"
                  % (label, held, held * 16384 / 1e6, med(rows), held * 16384 / med(rows) / 1e6, copy, copy / med(rows)))
            print("      removed %d voxels of %d materials, added %d, repainted %d, in %d blocks" % (int(delta["removed_voxels"]), int((removed > 0).sum()), int(delta["added_voxels"]), int(delta["repainted_voxels"]), int(delta["blocks"])))
            rec.swap()
            rec.free()
        p.execute(0)

    if "e" in parts:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import measure_oracle as mo
        import undo_oracle as uo
        res, tal = p.measure(small)
        nb, blocks = n // 16, {}

        def block(bid):
            if bid not in blocks:
                blocks[bid] = p.read_block(bid)
            return blocks[bid]
        for i in range(2000):
            b = small[i * 32]
            b0 = [min(int(v) // 16, nb - 2) for v in b["lo"]]
            g = uo.Grid(np.zeros((32, 32, 32), np.int8), np.zeros((32, 32, 32), np.uint8), np.zeros((32, 32, 32), np.uint8), np.zeros(8, np.uint8))
            for z in range(2):
                for y in range(2):
                    for x in range(2):
                        s_ = (slice(z * 16, z * 16 + 16), slice(y * 16, y * 16 + 16), slice(x * 16, x * 16 + 16))
                        g.dist[s_], g.mat[s_], g.blend[s_], _ = block(((b0[2] + z) * nb + b0[1] + y) * nb + b0[0] + x)
            org = np.array(b0, np.uint32) * 16
            want, want_t = mo.measure(g, [(b["lo"] - org, b["hi"] - org)])
            if int(want[0]["solid_voxels"]):
                want[0]["min"] += org; want[0]["max"] += org
            assert want[0].tobytes() == res[i * 32].tobytes() and np.array_equal(want_t[0], tal[i * 32]), (i, want[0], res[i * 32])
        print("  (e) 2000 of the 16^3 boxes equal the numpy oracle, tallies included")


if __name__ == "__main__":
    main()
