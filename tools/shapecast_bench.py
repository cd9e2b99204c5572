#!/usr/bin/env python3
"""Sphere casts and closest points on the bench's 1024^3 device terrain (include/voxels_hip.h, vx_spherecast*,
vx_closest_point*), level 0 with its index current: device time of 1M-entry batches, and 2 000 sampled entries of each batch
against the float64 oracle of tests/test_shapecast.py.  Prints one JSON line; exits non-zero on any mismatch.

  falling       spheres of radius 2 moving 45 degrees down, at most 32 voxels (tests/test_shapecast.py falling_casts)
  horizontal    long walks at mid height across the whole grid at radius 0.5 and 8
  closest       points within 6 voxels of surface points (the falling batch's contacts), max_dist 8

Batch times are HIP events around one vx_*_device call on the context's stream after a warm-up (median of --reps).  Kernel
times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/shapecast_bench.py` run.
Usage (GPU box): python tools/shapecast_bench.py [--n 1024] [--reps 5] [--no-check]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import vxo  # noqa: E402
from test_raycast import OracleLevel  # noqa: E402
from test_shapecast import (compare_point_hits, compare_sphere_hits, falling_casts, horizontal_casts, oracle_closest,  # noqa: E402
                            oracle_sphere, queries_near)
from voxels_amd import POINT_HIT_DTYPE, SPHERE_HIT_DTYPE, Polygonizer  # noqa: E402


def time_batch(p, records, call, hit_dtype, reps):
    d_in = torch.from_numpy(records.view(np.uint8).copy()).cuda()
    d_out = torch.zeros(len(records) * hit_dtype.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()   # (not the null stream: set_stream(0) selects the context's own)
    p.set_stream(stream.cuda_stream)
    call(d_in.data_ptr(), len(records), d_out.data_ptr())   # warm-up
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call(d_in.data_ptr(), len(records), d_out.data_ptr())
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    p.set_stream(0)
    return float(np.median(ms)), d_out.cpu().numpy().view(hit_dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1337)
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-check", action="store_true")
    a = ap.parse_args()
    torch.cuda.init()
    p = Polygonizer(device=0)
    p.set_materials(vxo.default_lut())
    p.create_terrain(a.n, a.seed)
    info = p.execute()
    idx = p.raycast_prepare(0)
    out = {"n": a.n, "levels": int(info.levels), "triangles": idx["triangles"], "straddling": idx["straddling"], "count": a.count}
    ok = idx["straddling"] == 0
    lvl = None if a.no_check else OracleLevel(p.level(0))
    batches = {"falling_r2": falling_casts(a.n, a.count, a.seed, 2.0, 32.0),
               "horizontal_r0.5": horizontal_casts(a.n, a.count, 0.5, a.seed),
               "horizontal_r8": horizontal_casts(a.n, a.count, 8.0, a.seed + 1)}
    contacts = None
    for name, casts in batches.items():
        ms, hits = time_batch(p, casts, p.spherecast_device, SPHERE_HIT_DTYPE, a.reps)
        out[name + "_ms"] = round(ms, 4)
        out[name + "_mcasts_per_s"] = round(len(casts) / ms / 1e3, 2)
        out[name + "_hit_share"] = round(float(np.isfinite(hits["t"]).mean()), 4)
        if contacts is None:
            contacts = hits["contact"][np.isfinite(hits["t"])]
        if lvl is not None:
            s = np.random.RandomState(7).choice(len(casts), 2000, replace=False)
            try:
                out[name + "_grazing"] = compare_sphere_hits(lvl, casts[s], hits[s], oracle_sphere(lvl, casts[s]), 0.01, name)
                out[name + "_oracle"] = "equal"
            except AssertionError as e:
                out[name + "_oracle"] = str(e)[:400]
                ok = False
    q = queries_near(contacts, a.count, a.seed, 6.0, 8.0)
    ms, qh = time_batch(p, q, p.closest_points_device, POINT_HIT_DTYPE, a.reps)
    out["closest_ms"] = round(ms, 4)
    out["closest_mqueries_per_s"] = round(len(q) / ms / 1e3, 2)
    out["closest_found_share"] = round(float(np.isfinite(qh["dist"]).mean()), 4)
    if lvl is not None:
        s = np.random.RandomState(8).choice(len(q), 2000, replace=False)
        try:
            compare_point_hits(lvl, q[s], qh[s], oracle_closest(lvl, q[s]), "closest")
            out["closest_oracle"] = "equal"
        except AssertionError as e:
            out["closest_oracle"] = str(e)[:400]
            ok = False
    out["ok"] = ok
    print(json.dumps(out))
    p.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
