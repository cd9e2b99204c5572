"""Overlap queries (vx_overlap_boxes_device) on the bench's 1024^3 device terrain, level 0, with the index current: device time
between events of the whole call (three launches) per run - (a) 2^20 body boxes of edge 2 centred on vx_scatter points, (b) the
same with edge 8, (c) 4 096 boxes of edge 64, (d) one whole-level box, (e) (a) count-only, (f) (a) with corners - queries and
triangles per second and the bytes written; (g) a sample of the queries of (a)-(c) against the numpy oracle
(tests/overlap_oracle.py); and for scale vx_closest_point_device on the centres of (a) with max_dist 1 and a device-to-device
hipMemcpyAsync of (d)'s output bytes.  Prints one JSON line; exits non-zero on a mismatch.  Kernel times come from a separate
run under a kernel trace (--trace-only: each run once after its sizing call and one warm-up, nothing else), summarised by
--summarise-trace DB."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summarise_trace(path):
    """the k_overlap_* dispatches of a rocprofv3 --kernel-trace database in order, one line per call (count, scan[, write])"""
    import sqlite3
    db = sqlite3.connect(path)
    tabs = [r[0] for r in db.execute("select name from sqlite_master where type='table'")]
    kd = [t for t in tabs if "kernel_dispatch" in t][0]
    ks = [t for t in tabs if "kernel_symbol" in t][0]
    rows = db.execute(f"select s.kernel_name, d.start, d.end, d.grid_size_x from {kd} d join {ks} s on d.kernel_id = s.id order by d.start").fetchall()
    call = []
    for name, a, b, grid in rows:
        short = next((k for k in ("k_overlap_count", "k_overlap_scan", "k_overlap_write", "k_closest_point") if k in name), None)
        if short is None:
            continue
        if short in ("k_overlap_count", "k_closest_point") and call:
            print("   ".join(call))
            call = []
        call.append("%s %10.1f us (grid %d)" % (short, (b - a) / 1e3, grid))
    if call:
        print("   ".join(call))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=2000, help="queries of (a)-(c) compared with the oracle")
    ap.add_argument("--trace-only", action="store_true", help="each run once after its sizing call and one warm-up, nothing else (for a kernel trace)")
    ap.add_argument("--summarise-trace", metavar="DB", help="print the overlap kernels of a kernel-trace database, call by call, and exit")
    args = ap.parse_args()
    if args.summarise_trace:
        summarise_trace(args.summarise_trace)
        return 0
    import torch
    import overlap_oracle as oo
    from voxels_amd import OVERLAP_COUNTS_DTYPE, OVERLAP_RANGE_DTYPE, OVERLAP_TRI_DTYPE, POINT_QUERY_DTYPE, SCATTER_COUNTS_DTYPE, Polygonizer, scatter_params
    from voxels_amd.binding import LISTED_BLOCK_DTYPE, VERTEX_DTYPE
    n, level = args.n, 0
    if args.trace_only:
        args.repeats, args.warmup, args.check = 1, 1, 0
    p = Polygonizer(device=0)
    p.create_terrain(n, 1337)
    p.execute()
    index = p.raycast_prepare(level)
    # a stream of our own: events on torch's default stream do not wait for the context's own stream
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]

    # centres: vx_scatter points of the level, an evenly spaced choice of them
    d_counts = torch.zeros(32, dtype=torch.uint8, device="cuda")
    prm = scatter_params(seed=1, density=1.0)
    p.scatter_device(level, prm, 0, None, None, d_counts.data_ptr())
    stream.synchronize()
    have = int(d_counts.cpu().numpy().view(SCATTER_COUNTS_DTYPE)[0]["points"])
    prm = scatter_params(seed=1, density=min(64.0, max(1.0, 1.25 * args.queries / max(have, 1))))
    p.scatter_device(level, prm, 0, None, None, d_counts.data_ptr())
    stream.synchronize()
    have = int(d_counts.cpu().numpy().view(SCATTER_COUNTS_DTYPE)[0]["points"])
    d_points = torch.zeros(max(have, 1) * 48, dtype=torch.uint8, device="cuda")
    p.scatter_device(level, prm, have, d_points.data_ptr(), None, d_counts.data_ptr())
    stream.synchronize()
    nq = min(args.queries, have)
    pick = torch.linspace(0, have - 1, nq, dtype=torch.float64, device="cuda").round().long()
    centres = d_points.view(torch.float32).view(-1, 12)[:, :3][pick].contiguous()
    del d_points

    def boxes_of(c, edge):
        b = torch.zeros((len(c), 8), dtype=torch.float32, device="cuda")
        b[:, 0:3], b[:, 4:7] = c - 0.5 * edge, c + 0.5 * edge
        return b

    few = centres[torch.linspace(0, nq - 1, min(4096, nq), dtype=torch.float64, device="cuda").round().long()].contiguous()
    whole = torch.tensor([[0, 0, 0, 0, n, n, n, 0]], dtype=torch.float32, device="cuda")
    runs = [("a: %d boxes of edge 2" % nq, boxes_of(centres, 2.0), True, False),
            ("b: %d boxes of edge 8" % nq, boxes_of(centres, 8.0), True, False),
            ("c: %d boxes of edge 64" % len(few), boxes_of(few, 64.0), True, False),
            ("d: one whole-level box", whole, True, False),
            ("e: (a) count-only", boxes_of(centres, 2.0), False, False),
            ("f: (a) with corners", boxes_of(centres, 2.0), True, True)]

    def timed(call):
        times = []
        for k in range(args.warmup + args.repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            stream.synchronize()
            if k >= args.warmup:
                times.append(a.elapsed_time(b))
        return float(np.median(times)), float(np.min(times)), float(np.max(times))

    out_runs, whole_bytes = [], 0
    for label, d_boxes, fill, corners in runs:
        m = len(d_boxes)
        d_ranges = torch.zeros(m * 8, dtype=torch.uint8, device="cuda")
        p.overlap_boxes_device(level, d_boxes.data_ptr(), m, 0, None, None, d_ranges.data_ptr(), d_counts.data_ptr())
        stream.synchronize()
        counts = oo.counts_dict(d_counts.cpu().numpy().view(OVERLAP_COUNTS_DTYPE)[0])
        total = counts["triangles"]
        assert total <= 0xFFFFFFFF
        cap = total if fill else 0
        d_tris = torch.zeros(max(cap, 1) * 16, dtype=torch.uint8, device="cuda") if fill else None
        d_corners = torch.zeros(max(cap, 1) * 48, dtype=torch.uint8, device="cuda") if corners else None
        ms, lo, hi = timed(lambda: p.overlap_boxes_device(level, d_boxes.data_ptr(), m, cap, d_tris.data_ptr() if fill else None,
                                                          d_corners.data_ptr() if corners else None, d_ranges.data_ptr(), d_counts.data_ptr()))
        # written: results (+ corners), ranges, counts, and the per-query scratch (count pass, then the scan's `first`)
        written = cap * (16 + (48 if corners else 0)) + m * 8 + 32 + m * 16 + m * 8
        # read at least: the boxes and the scratch in both passes, and per match three positions, three indices, one ordinal per pass
        passes = 2 if fill else 1
        read = passes * (m * 32 + total * (48 + 12 + 2)) + m * 16 * passes + (cap * 48 if corners else 0)
        out_runs.append({"run": label, "queries": m, "triangles": total, "pairs": counts["pairs"], "hit_queries": counts["hit_queries"],
                         "max_per_query": counts["max_per_query"], "device_ms_median": ms, "device_ms_min": lo, "device_ms_max": hi,
                         "queries_per_s": m / (ms * 1e-3), "triangles_per_s": total / (ms * 1e-3), "bytes_written": written,
                         "bytes_read_at_least": read, "GBps_written_and_read_at_least": (written + read) / (ms * 1e-3) / 1e9})
        if label.startswith("d:"):
            whole_bytes = cap * 16
            src, dst = d_tris, torch.zeros_like(d_tris)
            ms, lo, hi = timed(lambda: hip.hipMemcpyAsync(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), whole_bytes, 3, C.c_void_p(stream.cuda_stream)))
            out_memcpy = {"bytes": whole_bytes, "device_ms_median": ms, "device_ms_min": lo, "device_ms_max": hi,
                          "GBps_read_plus_written": 2 * whole_bytes / (ms * 1e-3) / 1e9}
        del d_tris, d_corners
    # for scale: the closest point within 1 voxel of the same centres
    d_q = torch.ones((nq, 4), dtype=torch.float32, device="cuda")
    d_q[:, :3] = centres
    d_hits = torch.zeros(nq * 48, dtype=torch.uint8, device="cuda")
    assert POINT_QUERY_DTYPE.itemsize == 16
    ms, lo, hi = timed(lambda: p.closest_points_device(d_q.data_ptr(), nq, d_hits.data_ptr(), level))
    out_closest = {"queries": nq, "max_dist": 1.0, "device_ms_median": ms, "device_ms_min": lo, "device_ms_max": hi, "queries_per_s": nq / (ms * 1e-3)}
    del d_hits

    # (g) a sample of the queries of (a)-(c) against the oracle: brute force over every triangle of the level
    bad, checked, check = 0, 0, "not run"
    if args.check:
        tab_ptr, nb = p.device_block_table(level)
        table = np.zeros(nb, LISTED_BLOCK_DTYPE)
        assert hip.hipMemcpy(table.ctypes.data_as(C.c_void_p), C.c_void_p(tab_ptr), nb * LISTED_BLOCK_DTYPE.itemsize, 2) == 0
        dv, di, nv, ni = p.device_meshes()
        verts, idx = np.zeros(nv, VERTEX_DTYPE), np.zeros(ni, np.uint32)
        assert hip.hipMemcpy(verts.ctypes.data_as(C.c_void_p), C.c_void_p(dv), nv * 48, 2) == 0
        assert hip.hipMemcpy(idx.ctypes.data_as(C.c_void_p), C.c_void_p(di), ni * 4, 2) == 0
        lt = oo.LevelTriangles(table, verts, idx)
        rng = np.random.RandomState(7)
        for label, d_boxes, _, _ in runs[:3]:
            m = len(d_boxes)
            take = np.sort(rng.choice(m, min(args.check // 3, m), replace=False))
            d_sub = d_boxes[torch.from_numpy(take).cuda()].contiguous()
            want = oo.overlap(lt, d_sub.cpu().numpy().view(oo.OVERLAP_BOX_DTYPE).reshape(-1))
            cap = want[4]["triangles"]
            d_tris = torch.zeros(max(cap, 1) * 16, dtype=torch.uint8, device="cuda")
            d_corners = torch.zeros(max(cap, 1) * 48, dtype=torch.uint8, device="cuda")
            d_ranges = torch.zeros(len(take) * 8, dtype=torch.uint8, device="cuda")
            p.overlap_boxes_device(level, d_sub.data_ptr(), len(take), cap, d_tris.data_ptr(), d_corners.data_ptr(), d_ranges.data_ptr(), d_counts.data_ptr())
            stream.synchronize()
            got_counts = oo.counts_dict(d_counts.cpu().numpy().view(OVERLAP_COUNTS_DTYPE)[0])
            got = (d_tris.cpu().numpy()[:cap * 16].view(OVERLAP_TRI_DTYPE), d_corners.cpu().numpy()[:cap * 48].view(np.float32).reshape(-1, 3, 4),
                   d_ranges.cpu().numpy().view(OVERLAP_RANGE_DTYPE))
            checked += len(take)
            if got_counts != want[4] or got[0].tobytes() != want[1].tobytes() or got[1].tobytes() != want[2].tobytes() or got[2].tobytes() != want[3].tobytes():
                bad += 1
        check = "equal" if bad == 0 else "MISMATCH in %d of 3 runs" % bad
    p.set_stream(0)
    out = {"n": n, "level": level, "entries": index["blocks"], "level_triangles": index["triangles"], "index_bytes": index["bytes"],
           "straddling": index["straddling"], "repeats": args.repeats, "runs": out_runs, "closest_point": out_closest, "memcpy_d2d": out_memcpy,
           "checked_queries": checked, "check": check}
    print(json.dumps(out))
    p.close()
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
