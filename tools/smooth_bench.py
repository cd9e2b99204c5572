#!/usr/bin/env python3
"""What "soften the crater rim" (vx_grid_smooth) costs on the device terrain:
  (a) one ball op, radius 24, box 48^3 at the surface, 1 iteration
  (b) the same with 4 iterations
  (c) a stroke of 256 ball ops as one batch, against 256 single calls
  (d) the whole grid, 1 iteration, next to the bytes it has to read and write and the rate that makes
  (e) vx_polygonize_dirty of (a)'s box
One process, three warm-up calls, medians over the repetitions, wall time of the calls.  Smoothing is not undone between the
repetitions: every call does the same work whatever the values are.
Usage (GPU box): python tools/smooth_bench.py [n] [repetitions]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxels_amd import Polygonizer, synth  # noqa: E402
from voxels_amd.binding import SMOOTH_DTYPE, smooth_op  # noqa: E402

HBM_MEASURED_TBS = 6.29   # float4 copy on one MI355X; 8.0 TB/s is the specified peak


def timed(fn, reps, warmup=3):
    out = []
    for k in range(warmup + reps):
        t = time.perf_counter()
        fn()
        if k >= warmup:
            out.append((time.perf_counter() - t) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(20, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)
    cx = cy = n // 2
    col = p.column(n, cx, cy)
    zs = int(np.argmax(col >= 0)) if (col >= 0).any() else n // 2
    half = min(24, n // 2)
    lo = [min(max(c - half, 0), n - 2 * half) for c in (cx, cy, zs)]
    box = (tuple(lo), tuple(v + 2 * half for v in lo))
    centre = (cx + 0.5, cy + 0.5, zs + 0.5)
    rows = []

    one = smooth_op(box, centre, 24.0, 1.0, 1)
    res, mn, mx, changed = p.smooth(one)
    rows.append(("(a) one ball op, radius 24, box %d^3 at the surface, 1 iteration (%d voxels changed the first time)" % (2 * half, changed), timed(lambda: p.smooth(one), reps)))
    four = smooth_op(box, centre, 24.0, 1.0, 4)
    rows.append(("(b) the same, 4 iterations", timed(lambda: p.smooth(four), reps)))

    stroke = np.zeros(256, SMOOTH_DTYPE)
    for i in range(256):
        c = np.array([cx - 128 + i + 0.5, cy + 0.25, zs + 0.5], np.float32)
        b0 = np.clip(np.floor(c - 12).astype(np.int64), 0, n - 1)
        b1 = np.clip(b0 + 25, 1, n)
        stroke[i] = smooth_op((b0, b1), c, 12.0, 1.0, 1)[0]
    rows.append(("(c) a stroke of 256 ball ops (radius 12, boxes 25^3), one batch", timed(lambda: p.smooth(stroke), reps)))
    rows.append(("(c) the same stroke, 256 single calls", timed(lambda: [p.smooth(stroke[i:i + 1]) for i in range(256)], reps)))

    whole = smooth_op(((0, 0, 0), (n, n, n)), None, 0.0, 1.0, 1)
    t_whole = timed(lambda: p.smooth(whole), reps)
    rows.append(("(d) the whole grid, 1 iteration", t_whole))

    res, mn, mx, _ = p.smooth(one)
    if not mx.any():          # the repetitions above smoothed it until nothing changes any more: redraw the op's whole box
        mn = np.array([lo[0], lo[2], lo[1]], np.float32)
        mx = mn + 2 * half
    rows.append(("(e) vx_polygonize_dirty of (a)'s box", timed(lambda: p.execute_dirty(mn, mx), reps)))

    print("grid %d^3 device terrain, %d repetitions after 3 warm-up calls, medians (best .. worst), wall time" % (n, reps))
    for label, t in rows:
        print("  %-104s %10.4f ms (%.4f .. %.4f)" % (label, t[0], t[1], t[2]))
    # (d): eval reads the grid and writes the byte volume, commit reads both and writes the grid, the flag pass reads the grid,
    # the mirror pass reads the three fields and writes their mirrors
    v = float(n) ** 3
    smooth_bytes, follow_bytes = 5 * v, (1 + 3 + 3) * v
    print("  (d) in bytes: eval + commit %.2f GB, flags + mirrors %.2f GB; %.2f TB/s over the call (%.0f %% of the %.2f TB/s a float4 copy reaches)"
          % (smooth_bytes / 1e9, follow_bytes / 1e9, (smooth_bytes + follow_bytes) / (t_whole[0] * 1e-3) / 1e12,
             100.0 * (smooth_bytes + follow_bytes) / (t_whole[0] * 1e-3) / 1e12 / HBM_MEASURED_TBS, HBM_MEASURED_TBS))


if __name__ == "__main__":
    main()
