#!/usr/bin/env python3
"""What an ordered brush batch (vx_grid_inject_brushes) buys over one call per brush, on the device terrain:
  (a) a 256-capsule stroke as one batch, and the equivalent 256-ball stroke as one batch
  (b) the same 256 balls as 256 vx_grid_inject_ball calls
  (c) 4096 scattered craters as one batch
  (d) the vx_polygonize_dirty(union box) that follows each of them
One process, warm-up first, medians over the repetitions; the work of an edit does not depend on what the voxels hold, so every
repetition applies the same brushes to the same grid.  Usage (GPU box): python tools/brush_bench.py [n] [repetitions]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxels_amd import Polygonizer, synth  # noqa: E402
from voxels_amd.binding import BRUSH_BALL, BRUSH_DTYPE, capsule_stroke  # noqa: E402


def median_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 25
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)
    # a tool dragged along the surface: 257 positions, 1.2 voxels apart, radius 4
    x0, y0 = n / 2.0 - 154.0, n / 2.0 + 0.37
    col = p.column(n, int(n / 2), int(y0))
    zs = float(np.argmax(col >= 0)) if (col >= 0).any() else n / 2.0
    s = np.arange(257, dtype=np.float64)
    path = np.stack([x0 + 1.2 * s, y0 + 6.0 * np.sin(s / 20.0), zs + 3.0 * np.cos(s / 33.0)], axis=1).astype(np.float32)
    r = 4.0
    capsules = np.array([capsule_stroke(path[i], path[i + 1], r, 2) for i in range(256)], BRUSH_DTYPE)
    balls = np.zeros(256, BRUSH_DTYPE)
    balls["position"] = path[:256]; balls["shape"] = BRUSH_BALL; balls["extents"] = 2 * r + 4; balls["type"] = 2; balls["radius"] = r
    rng = np.random.RandomState(4)
    craters = np.zeros(4096, BRUSH_DTYPE)
    craters["position"][:, 0] = rng.uniform(8, n - 8, 4096); craters["position"][:, 1] = rng.uniform(8, n - 8, 4096)
    craters["position"][:, 2] = zs + rng.uniform(-6, 6, 4096)
    craters["shape"] = BRUSH_BALL; craters["radius"] = rng.uniform(3, 6, 4096)
    craters["extents"] = (2 * craters["radius"] + 4)[:, None]; craters["type"] = 2

    def singles():
        for b in balls:
            p.inject_ball(b["position"], b["extents"], r, 2)

    rows = []
    for label, brushes, fn in (("(a) 256-capsule stroke, one batch", capsules, None), ("(a) 256-ball stroke, one batch", balls, None),
                               ("(b) 256 balls, 256 vx_grid_inject_ball calls", balls, singles), ("(c) 4096 scattered craters, one batch", craters, None)):
        res, umin, umax, touched = p.inject_brushes(brushes)
        edit = median_ms(fn or (lambda: p.inject_brushes(brushes)), reps)
        devs = []

        def dirty():
            p.execute_dirty(umin, umax)
            devs.append(p.info.device_ms)
        poly = median_ms(dirty, reps)
        rows.append((label, len(brushes), touched, int(res["touched_blocks"].sum()), edit, poly, float(np.median(devs[3:]))))
    print("grid %d^3 device terrain, %d repetitions after 3 warm-up calls, medians (best .. worst), wall time of the calls" % (n, reps))
    for label, count, touched, entries, edit, poly, dev in rows:
        print("  %-46s %8.4f ms (%.4f .. %.4f) = %7.3f us per brush; %d distinct blocks, %d block-brush pairs; vx_polygonize_dirty(union) %8.4f ms (device %.4f ms)"
              % (label, edit[0], edit[1], edit[2], edit[0] * 1e3 / count, touched, entries, poly[0], dev))
    a, b = rows[1][4][0], rows[2][4][0]
    print("  256 balls: one batch is %.1f times faster than 256 calls (%.4f ms against %.4f ms)" % (b / a, a, b))
    assert a < b, "the batch must be faster than one call per brush"


if __name__ == "__main__":
    main()
