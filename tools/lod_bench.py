"""LOD selection (vx_lod_select_device) on the bench's 1024^3 device terrain, 7 levels: device time per frame over a camera
path, the first selection after a full run and after a carve + incremental run, record and command counts, and a sample of
frames checked against the numpy oracle (tests/lod_oracle.py).  Prints one JSON line; exits non-zero on a mismatch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def camera_path(n, frames):
    t = np.linspace(0, 2 * np.pi, frames, endpoint=False)
    cam = np.stack([n / 2 + 0.4 * n * np.cos(t), n * (0.35 + 0.1 * np.sin(3 * t)), n / 2 + 0.4 * n * np.sin(t)], 1)
    look = np.stack([n / 2 + 0.1 * n * np.cos(t + 1.0), np.full(frames, n * 0.3), n / 2 + 0.1 * n * np.sin(t + 1.0)], 1)
    return cam.astype(np.float32), look.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--check", type=int, default=200)
    args = ap.parse_args()
    import torch
    from lod_oracle import Selection, select
    from test_gpu_lod import frustum, tables
    from voxels_amd import LOD_COUNTS_DTYPE, Polygonizer, lod_params, lod_ranges
    n = args.n
    p = Polygonizer(device=0)
    p.create_terrain(n, 1337)
    p.execute()
    cams, looks = camera_path(n, args.frames)
    cap = sum(p.device_block_table(L)[1] for L in range(p.info.levels))
    tcap = 6 * cap
    d_draws = torch.zeros(cap * 32 + 16, dtype=torch.uint8, device="cuda")
    d_reg = torch.zeros(cap * 20 + 16, dtype=torch.uint8, device="cuda")
    d_tr = torch.zeros(tcap * 20 + 16, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(32, dtype=torch.uint8, device="cuda")
    # a stream of our own: set_stream(0) would select the context's own stream, which events on torch's default stream do not wait for
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    ranges = lod_ranges()

    def timed(prm):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        p.lod_select_device(prm, cap, tcap, d_draws.data_ptr(), d_reg.data_ptr(), d_tr.data_ptr(), d_cnt.data_ptr())
        b.record(stream)
        stream.synchronize()
        return a.elapsed_time(b)

    params = [lod_params(c, ranges, frustum(c, l, n)) for c, l in zip(cams, looks)]
    first_full = timed(params[0])
    for prm in params[:20]:
        timed(prm)
    times, recs, trs = [], [], []
    for prm in params:
        times.append(timed(prm))
        cnt = d_cnt.cpu().numpy().view(LOD_COUNTS_DTYPE)[0]
        recs.append(int(cnt["records"]))
        trs.append(int(cnt["transition"]))
    # the frames checked against the oracle (host variant: same launches)
    p.set_stream(0)
    tabs = tables(p)
    bad = 0
    for k in np.linspace(0, args.frames - 1, min(args.check, args.frames)).astype(int):
        pl = frustum(cams[k], looks[k], n)
        got = p.lod_select(cams[k], ranges, pl)
        want = select(Selection(n, p.info.levels, cams[k], ranges), tabs, pl)
        if got[3] != want[3] or any(g.tobytes() != w.tobytes() for g, w in zip(got[:3], want[:3])):
            bad += 1
    # after a carve + incremental run (the tables come back from the host once)
    mn, mx = p.inject_ball((n / 2, n / 2, n / 2), (16, 16, 16), 8.0, 2)
    p.execute_dirty(mn, mx)
    p.set_stream(stream.cuda_stream)
    after_edit = timed(params[0])
    again = timed(params[0])
    p.set_stream(0)
    out = {"n": n, "levels": int(p.info.levels), "frames": args.frames,
           "select_ms_median": float(np.median(times)), "select_ms_p90": float(np.percentile(times, 90)),
           "first_after_full_run_ms": first_full, "first_after_edit_ms": after_edit, "second_after_edit_ms": again,
           "records_median": int(np.median(recs)), "transition_median": int(np.median(trs)), "table_entries": int(cap),
           "checked": int(min(args.check, args.frames)), "check": "equal" if bad == 0 else "MISMATCH %d" % bad}
    print(json.dumps(out))
    p.close()
    return 0 if bad == 0 else 1


if __name__ == "__main__":
    sys.exit(main())
