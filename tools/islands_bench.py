#!/usr/bin/env python3
"""What "did that carve cut something loose?" (vx_grid_islands) costs on the device terrain:
  (a) a whole-grid query
  (b) a 128^3 box around a point on the surface
  (c) a stroke of capsule brushes that saws a pillar standing on the terrain loose, then the query with VX_ISLANDS_REMOVE in a
      128^3 box around the cut, then vx_polygonize_dirty of the returned box (the pillar is set up again, untimed, before
      every repetition)
  (d) for scale only: reading the same 128^3 box back with vx_grid_read_block
One process, three warm-up calls, medians over the repetitions, wall time of the calls.
Usage (GPU box): python tools/islands_bench.py [n] [repetitions] [noread]   (noread: without (d), which takes minutes)"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxels_amd import Polygonizer, synth  # noqa: E402
from voxels_amd.binding import BRUSH_BOX, BRUSH_DTYPE, capsule_stroke  # noqa: E402


def timed(fn, reps, warmup=3, before=None):
    out = []
    for k in range(warmup + reps):
        if before:
            before()
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
    half = min(64, n // 2)
    lo = [min(max(c - half, 0), n - 2 * half) for c in (cx, cy, zs)]
    box = (tuple(lo), tuple(v + 2 * half for v in lo))
    rows = []

    recs, counts, _, _ = p.islands()
    rows.append(("(a) whole grid, %d components, %d detached" % (counts["components"], counts["detached"]), timed(lambda: p.islands(capacity=len(recs)), reps)))
    recs, counts, _, _ = p.islands(box=box)
    rows.append(("(b) 128^3 box at the surface, %d components" % counts["components"], timed(lambda: p.islands(box=box, capacity=len(recs)), reps)))

    # (c) a pillar 7 x 7 voxels wide from below the surface to 30 voxels above it, sawn through 12 voxels above the surface
    pillar = np.zeros(1, BRUSH_DTYPE)
    pillar["position"] = (cx, cy, zs + 10.0); pillar["extents"] = (14.0, 14.0, 48.0); pillar["shape"] = BRUSH_BOX
    pillar["a"] = (3.0, 3.0, 20.0); pillar["radius"] = 1.0; pillar["type"] = 0
    saw = np.array([capsule_stroke((cx - 8.0 + 2.0 * i, cy - 8.0 + 16.0 * (j % 2), zs + 12.0), (cx - 6.0 + 2.0 * i, cy + 8.0 - 16.0 * (j % 2), zs + 12.0), 2.0, 2)
                    for j, i in enumerate(range(8))], BRUSH_DTYPE)
    state = {}

    def setup():
        _, mn, mx, _ = p.inject_brushes(pillar)
        p.execute_dirty(mn, mx)

    def stroke():
        _, state["umin"], state["umax"], _ = p.inject_brushes(saw)

    def query():
        state["recs"], state["counts"], state["mn"], state["mx"] = p.islands(box=box, remove=True, detached_only=True, capacity=16)

    def redraw():
        p.execute_dirty(state["mn"], state["mx"])

    def all_three():
        stroke(); p.execute_dirty(state["umin"], state["umax"]); query(); redraw()

    t_all = timed(all_three, reps, before=setup)
    removed = int(state["counts"]["removed"])
    setup(); stroke(); p.execute_dirty(state["umin"], state["umax"])
    t_query = timed(query, reps, before=lambda: (setup(), stroke(), p.execute_dirty(state["umin"], state["umax"])))
    rows.append(("(c) stroke + dirty run + query with removal (%d removed, %d voxels) + dirty run" % (removed, int(state["counts"]["removed_voxels"])), t_all))
    rows.append(("(c) the query with removal alone", t_query))
    setup(); stroke(); p.execute_dirty(state["umin"], state["umax"]); query()
    rows.append(("(c) vx_polygonize_dirty of the returned box alone", timed(redraw, reps)))

    nb = n // 16
    ids = [(bz * nb + by) * nb + bx for bz in range(lo[2] // 16, (lo[2] + 2 * half + 15) // 16) for by in range(lo[1] // 16, (lo[1] + 2 * half + 15) // 16)
           for bx in range(lo[0] // 16, (lo[0] + 2 * half + 15) // 16)]
    if "noread" not in sys.argv[3:]:
        rows.append(("(d) the box read back with vx_grid_read_block, %d blocks" % len(ids), timed(lambda: [p.read_block(i) for i in ids], reps)))


    print("grid %d^3 device terrain, %d repetitions after 3 warm-up calls, medians (best .. worst), wall time" % (n, reps))
    for label, t in rows:
        print("  %-96s %10.4f ms (%.4f .. %.4f)" % (label, t[0], t[1], t[2]))


if __name__ == "__main__":
    main()
