"""Scattering (vx_scatter_device) on the bench's 1024^3 device terrain, 7 levels: device time between events of the whole call
(three launches) per run, points per second and bytes written, for level 0 over the whole grid at two densities, a 256-voxel box
around a camera on levels 0-3, and the two coarsest levels over the whole grid (few heavy entries: the unbalanced case); and a
sample of table entries checked against the numpy oracle (tests/scatter_oracle.py).  Prints one JSON line; exits non-zero on a
mismatch.  Kernel times come from a separate run under a kernel trace (--trace-only: each run once, no oracle)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=2000, help="table entries compared with the oracle, over all runs")
    ap.add_argument("--trace-only", action="store_true", help="each run once after one warm-up, nothing else (for a kernel trace)")
    args = ap.parse_args()
    import torch
    import scatter_oracle as so
    from voxels_amd import SCATTER_COUNTS_DTYPE, SCATTER_POINT_DTYPE, SCATTER_RANGE_DTYPE, Polygonizer, scatter_params
    from voxels_amd.binding import LISTED_BLOCK_DTYPE, VERTEX_DTYPE
    n = args.n
    p = Polygonizer(device=0)
    p.create_terrain(n, 1337)
    p.execute()
    T = p.info.levels - 1
    cam = np.float32([n / 2, n * 0.35, n / 2])
    box = dict(box_min=cam - 128, box_max=cam + 128)
    runs = [("level 0, whole grid, density 0.25", 0, scatter_params(seed=1, density=0.25)),
            ("level 0, whole grid, density 4", 0, scatter_params(seed=1, density=4.0))]
    runs += [("level %d, 256-voxel box, density 4" % L, L, scatter_params(seed=1, density=4.0, **box)) for L in range(min(4, T + 1))]
    runs += [("level %d, whole grid, density 4" % L, L, scatter_params(seed=1, density=4.0)) for L in sorted({max(T - 1, 0), T})]
    if args.trace_only:
        args.repeats, args.warmup, args.check = 1, 1, 0
    # a stream of our own: events on torch's default stream do not wait for the context's own stream
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    d_counts = torch.zeros(32, dtype=torch.uint8, device="cuda")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    pools = None
    rng = np.random.RandomState(7)
    # the entries to check, shared out over the runs: a coarse level has few, the finer ones take what is left
    quota, left = {}, args.check
    for k, L in sorted(enumerate(r[1] for r in runs), key=lambda kl: p.device_block_table(kl[1])[1]):
        quota[k] = min(p.device_block_table(L)[1], left // (len(runs) - len(quota)))
        left -= quota[k]
    out_runs, bad, checked = [], 0, 0
    for run, (label, L, prm) in enumerate(runs):
        per_run = quota[run]
        tab_ptr, nb = p.device_block_table(L)
        d_ranges = torch.zeros(max(nb, 1) * 8, dtype=torch.uint8, device="cuda")
        p.scatter_device(L, prm, 0, None, d_ranges.data_ptr(), d_counts.data_ptr())
        stream.synchronize()
        counts = d_counts.cpu().numpy().view(SCATTER_COUNTS_DTYPE)[0]
        cap = int(counts["points"])
        d_points = torch.zeros(max(cap, 1) * 48, dtype=torch.uint8, device="cuda")
        times = []
        for k in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            p.scatter_device(L, prm, cap, d_points.data_ptr(), d_ranges.data_ptr(), d_counts.data_ptr())
            b.record(stream)
            stream.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b))
        ms = float(np.median(times))
        written = cap * 48 + nb * 8 + 32
        out_runs.append({"run": label, "entries": int(counts["entries"]), "visited_entries": int(counts["visited_entries"]),
                         "triangles": int(counts["triangles"]), "candidates": int(counts["candidates"]), "points": cap,
                         "device_ms_median": ms, "device_ms_min": float(np.min(times)), "points_per_s": cap / (ms * 1e-3) if ms > 0 else 0.0,
                         "bytes_written": written, "write_GBps": written / (ms * 1e-3) / 1e9 if ms > 0 else 0.0})
        if not per_run or nb == 0:
            continue
        if pools is None:  # the mesh pools on the host, once
            dv, di, nv, ni = p.device_meshes()
            verts, idx = np.zeros(nv, VERTEX_DTYPE), np.zeros(ni, np.uint32)
            assert hip.hipMemcpy(verts.ctypes.data_as(C.c_void_p), C.c_void_p(dv), nv * 48, 2) == 0
            assert hip.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(di), ni * 4, 2) == 0
            pools = (verts, idx)
        table = np.zeros(nb, LISTED_BLOCK_DTYPE)
        assert hip.hipMemcpy(table.ctypes.data_as(C.c_void_p), C.c_void_p(tab_ptr), nb * LISTED_BLOCK_DTYPE.itemsize, 2) == 0
        points = d_points.cpu().numpy()[:cap * 48].view(SCATTER_POINT_DTYPE)
        ranges = d_ranges.cpu().numpy()[:nb * 8].view(SCATTER_RANGE_DTYPE)
        rec = prm[0]
        if int(ranges["count"].astype(np.int64).sum()) != cap or np.any(ranges["first"].astype(np.int64) != np.cumsum(ranges["count"].astype(np.int64)) - ranges["count"]):
            bad += 1
        for e in rng.choice(nb, min(per_run, nb), replace=False):
            entry = table[e]
            want = np.zeros(0, SCATTER_POINT_DTYPE)
            if np.all(entry["min_corner"] <= rec["box_max"]) and np.all(entry["max_corner"] >= rec["box_min"]):
                cand, _ = so.entry_candidates(L, rec, entry, *pools)
                want = cand[so.keeps(rec, cand)]
                want["entry"] = e
            got = points[int(ranges[e]["first"]):int(ranges[e]["first"]) + int(ranges[e]["count"])]
            checked += 1
            if got.tobytes() != want.tobytes():
                bad += 1
    p.set_stream(0)
    out = {"n": n, "levels": int(p.info.levels), "repeats": args.repeats, "runs": out_runs, "checked_entries": checked,
           "check": "not run" if not args.check else ("equal" if bad == 0 else "MISMATCH %d" % bad)}
    print(json.dumps(out))
    p.close()
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
