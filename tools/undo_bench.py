#!/usr/bin/env python3
"""What the undo records (vx_grid_capture / vx_record_trim / vx_record_swap) cost on the device terrain, and what they replace:
  (a) the 256-brush stroke of tools/brush_bench.py: capture its boxes, inject, trim, swap, vx_polygonize_dirty(the swap's box)
  (b) the same for 4096 scattered craters
  (c) a whole-grid capture and swap
  (d) the only alternative without records: vx_grid_pack before the edit, vx_grid_upload_packed and a full run to take it back
  (e) a plain device-to-device hipMemcpyAsync of a record's byte count: the bandwidth yardstick of the same run
  (f) 50 random held blocks of the whole-grid record against vx_grid_read_block
One process, warm-up first, medians over the repetitions, wall time of a call and of a wait for the device behind it: a capture
and a trim return with their copies still queued (they wait once, for a count), so the call alone would not show them.  A swap
puts the grid back, so every repetition sees the same grid.  The rates count a record's bytes (12 293 per block) once per call: a
capture reads and writes them once, a swap reads and writes them twice and rewrites the mirrors of its blocks.
Usage (GPU box): python tools/undo_bench.py [n] [repetitions] [parts, default abcd] - e.g. "b" under a kernel trace."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from voxels_amd import Polygonizer, brush_boxes, synth  # noqa: E402
from voxels_amd.binding import BRUSH_BALL, BRUSH_DTYPE  # noqa: E402


def timed(fn):
    t = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t) * 1e3, out


def med(values):
    return float(np.median(values))


class DeviceCopy:
    """hipMemcpyAsync device to device on the null stream, timed to its completion"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.hip.hipFree.argtypes = [C.c_void_p]

    def sync(self):
        assert self.hip.hipDeviceSynchronize() == 0

    def ms(self, nbytes, reps):
        a, b = C.c_void_p(), C.c_void_p()
        assert self.hip.hipMalloc(C.byref(a), nbytes) == 0 and self.hip.hipMalloc(C.byref(b), nbytes) == 0

        def copy():
            assert self.hip.hipMemcpyAsync(b, a, nbytes, 3, None) == 0 and self.hip.hipDeviceSynchronize() == 0
        for _ in range(2):
            copy()
        out = med([timed(copy)[0] for _ in range(reps)])
        self.hip.hipFree(a); self.hip.hipFree(b)
        return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    parts = sys.argv[3] if len(sys.argv) > 3 else "abcd"
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    p.execute(0)
    copier = DeviceCopy()

    def settled(fn):
        """fn, then a wait for everything it queued"""
        def call():
            out = fn()
            copier.sync()
            return out
        return call
    # the stroke and the craters of tools/brush_bench.py
    x0, y0 = n / 2.0 - 154.0, n / 2.0 + 0.37
    col = p.column(n, int(n / 2), int(y0))
    zs = float(np.argmax(col >= 0)) if (col >= 0).any() else n / 2.0
    s = np.arange(256, dtype=np.float64)
    r = 4.0
    stroke = np.zeros(256, BRUSH_DTYPE)
    stroke["position"] = np.stack([x0 + 1.2 * s, y0 + 6.0 * np.sin(s / 20.0), zs + 3.0 * np.cos(s / 33.0)], axis=1).astype(np.float32)
    stroke["shape"] = BRUSH_BALL; stroke["extents"] = 2 * r + 4; stroke["type"] = 2; stroke["radius"] = r
    rng = np.random.RandomState(4)
    craters = np.zeros(4096, BRUSH_DTYPE)
    craters["position"][:, 0] = rng.uniform(8, n - 8, 4096); craters["position"][:, 1] = rng.uniform(8, n - 8, 4096)
    craters["position"][:, 2] = zs + rng.uniform(-6, 6, 4096)
    craters["shape"] = BRUSH_BALL; craters["radius"] = rng.uniform(3, 6, 4096)
    craters["extents"] = (2 * craters["radius"] + 4)[:, None]; craters["type"] = 2

    print("grid %d^3 device terrain, %d repetitions after 2 warm-up rounds, medians, wall time of call + wait" % (n, reps))
    swap_ms = {}
    for label, brushes in (("(a) 256-brush stroke", stroke), ("(b) 4096 craters", craters)):
        if label[1] not in parts:
            continue
        t_boxes, boxes = timed(lambda: brush_boxes(brushes, n, p._L))
        rows = []
        for k in range(reps + 2):
            t_cap, rec = timed(settled(lambda: p.capture(boxes)))
            held = int(rec.info()["blocks"])
            t_edit, edit = timed(settled(lambda: p.inject_brushes(brushes)))
            assert edit[3] == held, "the record holds the blocks the batch touches"
            t_trim, dropped = timed(settled(rec.trim))
            kept = held - dropped
            t_swap, res = timed(settled(rec.swap))
            t_dirty, _ = timed(settled(lambda: p.execute_dirty(res["out_min"], res["out_max"])))
            rec.free()
            if k >= 2:
                rows.append((t_cap, t_edit, t_trim, t_swap, t_dirty))
        t_cap, t_edit, t_trim, t_swap, t_dirty = (med([row[i] for row in rows]) for i in range(5))
        copy_held, copy_kept = copier.ms(held * 12293, reps), copier.ms(kept * 12293, reps)
        swap_ms[label] = t_swap + t_dirty
        print("  %s: %d boxes (vx_brush_box on the host %.3f ms), %d blocks held (%.2f MB), %d after the trim (%.2f MB), %d voxels differ"
              % (label, boxes.size, t_boxes, held, held * 12293 / 1e6, kept, kept * 12293 / 1e6, int(res["changed_voxels"])))
        print("      capture %.4f ms = %.1f GB/s (memcpy of the same bytes %.4f ms: %.2f of its rate) | inject %.4f ms | trim %.4f ms"
              % (t_cap, held * 12293 / t_cap / 1e6, copy_held, copy_held / t_cap, t_edit, t_trim))
        print("      swap %.4f ms = %.1f GB/s (memcpy of the same bytes %.4f ms: %.2f of its rate) | vx_polygonize_dirty(swap box) %.4f ms"
              % (t_swap, kept * 12293 / t_swap / 1e6, copy_kept, copy_kept / t_swap, t_dirty))

    # (c) the whole grid
    whole = [((0, 0, 0), (n, n, n))]
    nb = n // 16
    caps, swaps = [], []
    for k in range(min(reps, 3) + 1 if "c" in parts else 0):
        t_cap, rec = timed(settled(lambda: p.capture(whole)))
        if k == 0:
            ids = rec.block_ids()
            assert ids.size == nb ** 3
            for i in np.random.RandomState(7).choice(ids.size, 50, replace=False):   # (f)
                got, want = rec.read_block(int(i)), p.read_block(int(ids[i]))
                assert all(np.array_equal(a, b) for a, b in zip(got[:3], want[:3])) and got[3] == want[3], i
        t_swap, res = timed(settled(rec.swap))
        assert int(res["changed_blocks"]) == 0
        rec.free()
        if k >= 1:
            caps.append(t_cap); swaps.append(t_swap)
    nbytes = nb ** 3 * 12293
    copy_all = copier.ms(nbytes, 3) if "c" in parts else 0.0
    if "c" in parts:
        print("  (c) whole grid: %d blocks, %.1f MB: capture %.3f ms = %.1f GB/s, swap %.3f ms = %.1f GB/s; memcpy of the same bytes %.3f ms = %.1f GB/s (capture %.2f, swap %.2f of its rate)"
              % (nb ** 3, nbytes / 1e6, med(caps), nbytes / med(caps) / 1e6, med(swaps), nbytes / med(swaps) / 1e6, copy_all, nbytes / copy_all / 1e6, copy_all / med(caps), copy_all / med(swaps)))
        print("  (f) 50 random held blocks equal vx_grid_read_block")
    if "d" not in parts:
        return

    # (d) without records: pack before the edit; upload the file and run in full to take the edit back
    size = C.c_uint64()
    p._check(p._lib.vx_grid_pack(p._h, None, 0, C.byref(size)), "vx_grid_pack")
    blob = np.zeros(size.value, np.uint8)
    packs, backs = [], []
    for k in range(3):
        t_pack, _ = timed(lambda: p._check(p._lib.vx_grid_pack(p._h, blob.ctypes.data, blob.size, C.byref(size)), "vx_grid_pack"))
        p.inject_brushes(stroke)

        def back():
            p.upload_packed(blob)
            p.execute(0)
        t_back, _ = timed(settled(back))
        if k >= 1:
            packs.append(t_pack); backs.append(t_back)
    print("  (d) without records: vx_grid_pack %.2f ms (%.1f MB) before the edit, vx_grid_upload_packed + full run %.2f ms to take it back"
          % (med(packs), blob.size / 1e6, med(backs)))
    for label, ms in swap_ms.items():
        print("      %s: swap + vx_polygonize_dirty %.4f ms, %.0f times faster than upload + full run" % (label, ms, med(backs) / ms))


if __name__ == "__main__":
    main()
