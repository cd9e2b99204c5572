#!/usr/bin/env python3
"""What "where can my agents still walk, and which way?" (vx_grid_walk_field) costs on the device terrain:
  (a) a 256 x 256 box around the surface band with one goal
  (b) the same box with 1 000 goals
  (c) the whole surface: n x n x the z band (cut to keep V <= 2^28)
  (d) the box of (a), range-limited by a small max_cost
  (e) the re-query of the box of (a) after a carve (the carve itself is not timed)
  (f) for scale: the host Dijkstra of the oracle (tests/walk/walk_host.cpp) on the box of (a), and vx_grid_islands on that box
Every device call writes the field and the direction bytes into caller tensors.  2 000 random cells of each device field are
compared with the oracle run on the host copy of the same terrain.  One process, three warm-up calls, medians over the
repetitions, wall time of the calls.
Usage (GPU box): python tools/walk_bench.py [n] [repetitions]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (before the library: see voxels_amd.binding.HipLibrary)
from voxels_amd import Polygonizer, synth  # noqa: E402
from voxels_amd.binding import WALK_GOAL_DTYPE  # noqa: E402
import walk_oracle as wo  # noqa: E402

PARAMS = dict(clearance=2, step_up=1, step_down=1, cost_axial=10, cost_diagonal=14, cost_climb=4)


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
    reps = max(5, int(sys.argv[2])) if len(sys.argv) > 2 else 20
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    dist = synth.terrain(n, materials=False)[0]      # the same field on the host, for the oracle
    solid = dist < 0
    layers = np.nonzero(solid.any(axis=(1, 2)) & (~solid).any(axis=(1, 2)))[0]
    z0, z1 = int(layers.min()), int(layers.max()) + 2
    if (z1 - z0) * n * n > 1 << 28:                    # keep the layers around the median surface height
        mid = int(np.median(solid.sum(axis=0)))
        depth = (1 << 28) // (n * n)
        z0 = min(max(mid - depth // 2, 0), n - depth)
        z1 = z0 + depth
    del solid
    side = min(256, n)
    c0 = (n - side) // 2
    box = ((c0, c0, z0), (c0 + side, c0 + side, z1))
    whole = ((0, 0, z0), (n, n, z1))
    stand = wo.standable_numpy(np.ascontiguousarray(dist[:, c0:c0 + side, c0:c0 + side]), PARAMS["clearance"])[z0:z1]
    cells = np.argwhere(stand)                        # (z, y, x) inside the box
    rng = np.random.RandomState(7)

    def goals_of(count):
        pick = cells[rng.choice(len(cells), count, replace=False)]
        g = np.zeros(count, WALK_GOAL_DTYPE)
        g["z"], g["y"], g["x"] = pick[:, 0] + z0, pick[:, 1] + c0, pick[:, 2] + c0
        return g

    middle = cells[np.argmin(abs(cells[:, 1] - side // 2) + abs(cells[:, 2] - side // 2))]
    one = np.zeros(1, WALK_GOAL_DTYPE)
    one["z"], one["y"], one["x"] = middle[0] + z0, middle[1] + c0, middle[2] + c0
    thousand = goals_of(min(1000, len(cells)))
    rows, state = [], {}

    def device(b, goals, **kw):
        ext = [h - l for l, h in zip(b[0], b[1])]
        V = ext[0] * ext[1] * ext[2]
        key = ("tensors", V)
        if key not in state:
            state[key] = (torch.zeros(V, dtype=torch.int32, device="cuda:0"), torch.zeros(V, dtype=torch.uint8, device="cuda:0"))
        field, dirs = state[key]
        prm = dict(PARAMS, **kw)
        return (lambda: state.__setitem__("counts", p.walk_field(b, goals, field=field, dirs=dirs, **prm))), field, dirs, prm

    def measure(label, b, goals, host=dist, **kw):
        call, field, dirs, prm = device(b, goals, **kw)
        t = timed(call, reps)
        c = state["counts"]
        want = wo.run("oracle", host, box=b, goals=goals, **prm)
        assert wo.deterministic(c) == wo.deterministic(want.counts), (c, want.counts)
        at = torch.from_numpy(rng.randint(0, want.field.size, 2000)).to("cuda:0")
        got_f, got_d = field[at].cpu().numpy().view(np.uint32), dirs[at].cpu().numpy()
        at = at.cpu().numpy()
        assert np.array_equal(got_f, want.field.reshape(-1)[at]) and np.array_equal(got_d, want.dirs.reshape(-1)[at]), label
        rows.append(("%s: %d standable, %d reached, max distance %d, %d sweeps" % (label, c["standable"], c["reached"], c["max_distance"], c["sweeps"]), t))
        return want

    measure("(a) %d x %d x %d box, one goal" % (side, side, z1 - z0), box, one)
    measure("(b) the same box, %d goals" % thousand.size, box, thousand)
    measure("(c) the whole surface %d x %d x %d, %d goals" % (n, n, z1 - z0, thousand.size), whole, thousand)
    measure("(d) the box of (a), max_cost 400", box, one, max_cost=400)
    # (e) a carve next to the goal, then the query again; the host copy follows by reading the touched blocks back
    centre = (float(one["x"][0]) + 12.0, float(one["y"][0]), float(one["z"][0]))
    p.inject_ball(centre, (20.0, 20.0, 20.0), 7.0, 2)
    carved = dist.copy()
    nb = n // 16
    for bz in range(max(int(centre[2] - 12) // 16, 0), min(int(centre[2] + 12) // 16, nb - 1) + 1):
        for by in range(int(centre[1] - 12) // 16, int(centre[1] + 12) // 16 + 1):
            for bx in range(int(centre[0] - 12) // 16, int(centre[0] + 12) // 16 + 1):
                carved[bz * 16:bz * 16 + 16, by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = p.read_block((bz * nb + by) * nb + bx)[0]
    assert not np.array_equal(carved, dist)
    measure("(e) the box of (a) after a carve", box, one, host=carved)
    # (f) for scale
    t = time.perf_counter()
    wo.run("oracle", carved, box=box, goals=one, **PARAMS)
    rows.append(("(f) host Dijkstra of the oracle on the box of (e), one run", ((time.perf_counter() - t) * 1e3,) * 3))
    recs, counts, _, _ = p.islands(box=box)
    rows.append(("(f) vx_grid_islands on the same box, %d components" % counts["components"], timed(lambda: p.islands(box=box, capacity=len(recs)), reps)))

    print("grid %d^3 device terrain, surface band z %d..%d, %d repetitions after 3 warm-up calls, medians (best .. worst), wall time" % (n, z0, z1, reps))
    for label, t in rows:
        print("  %-118s %10.4f ms (%.4f .. %.4f)" % (label, t[0], t[1], t[2]))
    print("2000 random cells of every device field and direction volume, and the counts, agree with the oracle")


if __name__ == "__main__":
    main()
