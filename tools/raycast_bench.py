#!/usr/bin/env python3
"""Ray casts on the bench's 1024^3 device terrain (include/voxels_hip.h, vx_raycast*): throughput of two batches of 1M rays,
index build times, one host-to-host pick, and 2 000 sampled rays of each batch against the float64 oracle of
tests/test_raycast.py.  Prints one JSON line; exits non-zero on any mismatch.

  camera      a 1024 x 1024 frustum from above the terrain, tilted 45 degrees down, lanes in 8 x 8 pixel tiles
  horizontal  long walks at mid height across the whole grid

Batch times are HIP events around one vx_raycast_device on the context's stream after a warm-up (median of --reps).  Kernel
times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/raycast_bench.py` run.
Usage (GPU box): python tools/raycast_bench.py [--n 1024] [--reps 5] [--no-check]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import vxo  # noqa: E402
from test_raycast import OracleLevel, camera_rays, compare_hits, horizontal_rays, make_rays, oracle_cast  # noqa: E402
from voxels_amd import HIT_DTYPE, Polygonizer  # noqa: E402


def time_batch(p, torch, rays, reps):
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).cuda()
    d_hits = torch.zeros(len(rays) * HIT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()   # (not the null stream: set_stream(0) selects the context's own)
    p.set_stream(stream.cuda_stream)
    p.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr())   # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        p.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr())
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    p.set_stream(0)
    hits = d_hits.cpu().numpy().view(HIT_DTYPE)
    return float(np.median(ms)), hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    p = Polygonizer(device=0)
    p.set_materials(vxo.default_lut())
    p.create_terrain(a.n, a.seed)
    info = p.execute()
    out = {"n": a.n, "levels": int(info.levels)}
    idx = [p.raycast_prepare(L) for L in range(info.levels)]
    out["index_build_ms_full_run"] = [round(i["build_ms"], 4) for i in idx]
    out["index_mb"] = [round(i["bytes"] / 2 ** 20, 2) for i in idx]
    out["triangles"] = [i["triangles"] for i in idx]
    out["straddling"] = [i["straddling"] for i in idx]
    batches = {"camera": camera_rays(a.n, 1024), "horizontal": horizontal_rays(a.n, 1 << 20, a.seed)}
    lvl = None if a.no_check else OracleLevel(p.level(0))
    ok = all(s == 0 for s in out["straddling"])
    for name, rays in batches.items():
        ms, hits = time_batch(p, torch, rays, a.reps)
        out[name + "_ms"] = round(ms, 4)
        out[name + "_mrays_per_s"] = round(len(rays) / ms / 1e3, 1)
        out[name + "_hit_share"] = round(float(np.isfinite(hits["t"]).mean()), 4)
        if lvl is not None:
            s = np.random.RandomState(7).choice(len(rays), 2000, replace=False)
            try:
                out[name + "_grazing"] = compare_hits(lvl, rays[s], hits[s], oracle_cast(lvl, rays[s]), 0.01, name)
                out[name + "_oracle"] = "equal"
            except AssertionError as e:
                out[name + "_oracle"] = str(e)[:400]
                ok = False
    # index rebuild after an edit: a ball carved at the surface under the grid's centre, then the incremental run
    pick = p.raycast(make_rays([[a.n / 2 + 0.3, a.n + 5.0, a.n / 2 + 0.7]], [[0, -1, 0]])["origin"], [[0, -1, 0]])
    hx, hy, hz = pick["pos"][0]
    mn, mx = p.inject_ball((hx, hz, hy), (44.0, 44.0, 44.0), 20.0, 2)
    p.execute_dirty(mn, mx)
    out["index_build_ms_after_edit"] = [round(p.raycast_prepare(L)["build_ms"], 4) for L in range(info.levels)]
    # one pick, host to host (index current)
    one = make_rays([[a.n / 2 + 0.3, a.n + 5.0, a.n / 2 + 0.7]], [[0, -1, 0]])
    p.raycast_rays(one)
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        p.raycast_rays(one)
        t.append((time.perf_counter() - t0) * 1e3)
    out["pick_host_ms"] = round(float(np.median(t)), 4)
    out["ok"] = ok
    print(json.dumps(out))
    p.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
