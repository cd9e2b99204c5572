#!/usr/bin/env python3
"""What the stamps (vx_stamp_capture / vx_grid_paste) cost on the device terrain:
  (a) vx_stamp_capture of a 64^3, a 256^3 and the whole-grid box
  (b) one 64^3 paste per orientation and mode, each followed by its vx_polygonize_dirty; the quarter turns also as a ratio to
      orientation 0 (a ratio far from 1 would mean that the staged stamp reads are not coalesced)
  (c) 4 096 pastes of a 32^3 prefab in one batch against 4 096 single calls
  (d) one 512^3 REPLACE
  (e) per call, for scale: a plain device-to-device hipMemcpyAsync of the bytes the call writes (12 288 per touched block; 3 per
      voxel for a capture), and a brush batch with the same touched blocks
  (f) the blocks of two pastes against the numpy oracle of the tests (125 blocks each)
One process, warm-up first, medians over the repetitions, wall time of a call and of a wait for the device behind it.  Every paste
is taken back with an undo record (not timed), so every repetition sees the same grid.
Usage (GPU box): python tools/stamp_bench.py [n] [repetitions] [parts, default abcdf] - e.g. "b" under a kernel trace."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from undo_bench import DeviceCopy, med, timed  # noqa: E402
from voxels_amd import Polygonizer, paste_boxes, pastes, synth  # noqa: E402
from voxels_amd.binding import BRUSH_BALL, BRUSH_DTYPE  # noqa: E402

MODE_NAMES = ("REPLACE", "UNION", "SUBTRACT", "PAINT")


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    parts = sys.argv[3] if len(sys.argv) > 3 else "abcdf"
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)
    copier = DeviceCopy()

    def settled(fn):
        def call():
            out = fn()
            copier.sync()
            return out
        return call
    col = p.column(n, n // 2, n // 2)
    zs = int(np.argmax(col >= 0)) if (col >= 0).any() else n // 2
    print("grid %d^3 device terrain (surface near z = %d), %d repetitions after 2 warm-up rounds, medians, wall time of call + wait" % (n, zs, reps))

    def paste_round(stamps, ps, rounds):
        """-> (median paste ms, median dirty ms, counts, touched blocks): paste, vx_polygonize_dirty, then the undo (not timed)"""
        boxes = paste_boxes(ps, [s.size for s in stamps], n, p._L)
        rows = []
        for k in range(rounds + 2):
            rec = p.capture(boxes)
            t_paste, (_, counts) = timed(settled(lambda: p.paste(stamps, ps)))
            t_dirty, _ = timed(settled(lambda: p.execute_dirty(counts["out_min"], counts["out_max"])))
            res = rec.swap()
            p.execute_dirty(res["out_min"], res["out_max"])
            rec.free()
            if k >= 2:
                rows.append((t_paste, t_dirty))
        return med([r[0] for r in rows]), med([r[1] for r in rows]), counts, boxes

    def brush_like(boxes, rounds):
        """a brush batch that touches the blocks of `boxes`: one ball per box, its block test cut to the box"""
        b = np.zeros(boxes.size, BRUSH_DTYPE)
        lo, hi = boxes["lo"].astype(np.float32), boxes["hi"].astype(np.float32)
        b["position"] = (lo + hi) / 2
        b["extents"] = (hi - lo) / 2 - 0.5
        b["shape"] = BRUSH_BALL; b["type"] = 2; b["radius"] = 2.0
        rows = []
        for k in range(rounds + 2):
            rec = p.capture(boxes)
            t, out = timed(settled(lambda: p.inject_brushes(b)))
            res = rec.swap()
            p.execute_dirty(res["out_min"], res["out_max"])
            rec.free()
            if k >= 2:
                rows.append(t)
        return med(rows), out[3]

    if "a" in parts:
        for label, lo, size in (("64^3", (n // 2 - 29, n // 2 - 35, max(zs - 30, 0)), 64), ("256^3", (n // 2 - 128, n // 2 - 128, max(min(zs - 128, n - 256), 0)), 256),
                                ("64^3 on 16-byte borders", (n // 2 - 32, n // 2 - 35, max(zs - 30, 0)), 64), ("the whole grid", (0, 0, 0), n)):
            size = min(size, n)
            rows = []
            for k in range(min(reps, 3 if size == n else reps) + 2):
                t, st = timed(settled(lambda: p.capture_stamp((lo, tuple(v + size for v in lo)))))
                st.free()
                if k >= 2:
                    rows.append(t)
            nbytes = 3 * size ** 3
            copy = copier.ms(nbytes, 3)
            print("  (a) capture %s at %s: %.4f ms = %.1f GB/s read + written; memcpy of the same bytes %.4f ms: %.2f of its rate"
                  % (label, lo, med(rows), nbytes / med(rows) / 1e6, copy, copy / med(rows)))

    if "b" in parts or "f" in parts:
        src_lo = (n // 2 - 29, n // 2 - 35, max(zs - 30, 0))
        st64 = p.capture_stamp((src_lo, tuple(v + 64 for v in src_lo)))
        origin = (n // 2 + 41, n // 2 + 7, max(zs - 23, 0))
    if "b" in parts:
        base = {}
        for mode in range(4):
            for orient in range(8):
                ps = pastes([(origin, 0, orient, mode)])
                t_paste, t_dirty, counts, boxes = paste_round([st64], ps, reps)
                touched = int(counts["touched_blocks"])
                if orient == 0:
                    base[mode] = t_paste
                    copy = copier.ms(touched * 12288, reps)
                    t_brush, brush_touched = brush_like(boxes, reps)
                    print("  (b) 64^3 %s: %d touched blocks; memcpy of %.2f MB %.4f ms; a brush batch on %d blocks %.4f ms" % (MODE_NAMES[mode], touched, touched * 12288 / 1e6, copy, brush_touched, t_brush))
                print("      orient %d: paste %.4f ms (%.2f of the memcpy's rate, %.2f x orient 0) | vx_polygonize_dirty %.4f ms | %d voxels differ"
                      % (orient, t_paste, copy / t_paste, t_paste / base[mode], t_dirty, int(counts["changed_voxels"])))

    if "c" in parts:
        rng = np.random.RandomState(5)
        lo = (n // 2 - 16, n // 2 - 16, max(zs - 16, 0))
        prefab = p.capture_stamp((lo, tuple(v + 32 for v in lo)))
        k = 4096
        rows = [((int(rng.randint(-8, n - 24)), int(rng.randint(-8, n - 24)), int(zs - 16 + rng.randint(-6, 7))), 0, int(rng.randint(8)), int(rng.randint(4))) for _ in range(k)]
        ps = pastes(rows)
        t_paste, t_dirty, counts, boxes = paste_round([prefab], ps, min(reps, 5))
        touched = int(counts["touched_blocks"])
        copy = copier.ms(touched * 12288, 3)
        t_brush, brush_touched = brush_like(boxes, 3)
        singles = []
        for r in range(2):
            rec = p.capture(boxes)
            singles.append(timed(settled(lambda: [p.paste([prefab], ps[i:i + 1]) for i in range(k)]))[0])
            rec.swap()
            rec.free()
        p.execute(0)
        print("  (c) %d pastes of a 32^3 prefab: %d distinct touched blocks, %d voxels differ" % (k, touched, int(counts["changed_voxels"])))
        print("      one batch %.3f ms (memcpy of %.1f MB %.3f ms: %.2f of its rate; a brush batch on %d blocks %.3f ms) | vx_polygonize_dirty %.3f ms | %d single calls %.1f ms, %.1f x the batch"
              % (t_paste, touched * 12288 / 1e6, copy, copy / t_paste, brush_touched, t_brush, t_dirty, k, min(singles), min(singles) / t_paste))

    if "d" in parts and n >= 1024:
        lo = (n // 2 - 256, n // 2 - 256, max(min(zs - 256, n - 512), 0))
        big = p.capture_stamp((lo, tuple(v + 512 for v in lo)))
        ps = pastes([((lo[0] + 37, lo[1] - 19, lo[2] + 5), 0, 1, 0)])
        t_paste, t_dirty, counts, boxes = paste_round([big], ps, 3)
        touched = int(counts["touched_blocks"])
        copy = copier.ms(touched * 12288, 3)
        t_brush, brush_touched = brush_like(boxes, 3)
        print("  (d) one 512^3 REPLACE, a quarter turn: %d touched blocks, %d voxels differ: paste %.3f ms (memcpy of %.1f MB %.3f ms: %.2f of its rate; a brush on %d blocks %.3f ms) | vx_polygonize_dirty %.3f ms"
              % (touched, int(counts["changed_voxels"]), t_paste, touched * 12288 / 1e6, copy, copy / t_paste, brush_touched, t_brush, t_dirty))
        big.free()

    if "f" in parts:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import stamp_oracle as sto
        import undo_oracle as uo
        d, m, b = st64.read()
        nb, checked = n // 16, 0
        for orient, mode in ((3, 1), (6, 0)):
            b0 = [v // 16 - 1 for v in origin]                 # a cube of 5^3 blocks around the paste
            g = uo.Grid(np.zeros((80, 80, 80), np.int8), np.zeros((80, 80, 80), np.uint8), np.zeros((80, 80, 80), np.uint8), np.zeros(125, np.uint8))
            cube = [(x, y, z) for z in range(5) for y in range(5) for x in range(5)]
            for x, y, z in cube:
                s = (slice(z * 16, z * 16 + 16), slice(y * 16, y * 16 + 16), slice(x * 16, x * 16 + 16))
                g.dist[s], g.mat[s], g.blend[s], g.flags[(z * 5 + y) * 5 + x] = p.read_block(((b0[2] + z) * nb + b0[1] + y) * nb + b0[0] + x)
            ps = pastes([(origin, 0, orient, mode)])
            rec = p.capture(paste_boxes(ps, [st64.size], n, p._L))
            p.paste([st64], ps)
            local = pastes([(tuple(o - 16 * c for o, c in zip(origin, b0)), 0, orient, mode)])
            sto.paste(g, [sto.St(d, m, b)], local)
            for x, y, z in cube:
                s = (slice(z * 16, z * 16 + 16), slice(y * 16, y * 16 + 16), slice(x * 16, x * 16 + 16))
                got = p.read_block(((b0[2] + z) * nb + b0[1] + y) * nb + b0[0] + x)
                assert np.array_equal(got[0], g.dist[s]) and np.array_equal(got[1], g.mat[s]) and np.array_equal(got[2], g.blend[s]) and got[3] == g.flags[(z * 5 + y) * 5 + x], (orient, mode, x, y, z)
                checked += 1
            rec.swap()
            rec.free()
        print("  (f) %d blocks around two pastes equal the numpy oracle, flags included" % checked)


if __name__ == "__main__":
    main()
