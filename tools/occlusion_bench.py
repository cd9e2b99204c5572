#!/usr/bin/env python3
"""What the ambient occlusion (vx_occlusion_device / vx_occlusion) costs on the device terrain after a full run, beside two
yardsticks taken in the same run, alternating with the call they stand beside:
  memcpy   a plain device-to-device hipMemcpyAsync of the bytes the call must move: 48 per baked vertex, the samples its
           workgroups stage (per visited entry (16 + 2 (steps + 2) + 1)^3 lattice points, one byte each, whether or not a sign
           summary spares the read) and 1 per vertex out
  rays     the route a bake replaces, on 100 000 sampled vertices of the level: the same probes - one ray per direction with a
           positive weight, from the origin O along S, steps * s voxels long - as one vx_raycast_device call on the level's meshes
Cases: level 0 whole at steps 4, 8 and 12; levels 1-3 at 8 steps; with the transition meshes; sign summaries off; the filtered
re-bake after one crater (vx_grid_inject_ball + vx_polygonize_dirty, the box grown by steps * s + 16 * s); the host form.  Then
2 000 random vertices per level against the numpy oracle of the tests, on a part of the grid read back through a stamp.
One process, medians of the repetitions after 2 warm-up rounds; the device form is timed between two events on the context's stream.
Usage (GPU box): python tools/occlusion_bench.py [n] [repetitions]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from height_bench import Copy  # noqa: E402
from undo_bench import DeviceCopy, med, timed  # noqa: E402
from voxels_amd import Polygonizer, occlusion_params, synth  # noqa: E402
from voxels_amd.binding import LISTED_BLOCK_DTYPE, RAY_DTYPE, VERTEX_DTYPE  # noqa: E402


def main():
    import torch
    import occlusion_oracle as oo
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = max(3, int(sys.argv[2])) if len(sys.argv) > 2 else 10
    p = Polygonizer()
    p.set_materials(synth.default_lut())
    p.create_terrain(n)
    info = p.execute(0)                         # the mirrors, and with them the sign summaries, are current
    levels = int(info.levels)
    copier = DeviceCopy()
    hip = copier.hip
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    stream = torch.cuda.Stream()
    p.set_stream(stream.cuda_stream)
    print("grid %d^3 device terrain after a full run of %d levels, %d repetitions after 2 warm-up rounds, medians;" % (n, levels, reps))
    print("the device form between two events on the context's stream, alternating with its yardsticks round after round")

    def snapshot():
        tabs = []
        for L in range(levels):
            tab, nb = p.device_block_table(L)
            t = np.zeros(nb, LISTED_BLOCK_DTYPE)
            assert nb == 0 or hip.hipMemcpy(t.ctypes.data, tab, nb * LISTED_BLOCK_DTYPE.itemsize, 2) == 0
            tabs.append(t)
        dv, _, nv, _ = p.device_meshes()
        verts = np.zeros(nv, VERTEX_DTYPE)
        assert hip.hipMemcpy(verts.ctypes.data, dv, nv * 48, 2) == 0
        return tabs, verts

    tabs, verts = snapshot()
    nv = len(verts)
    d_ao = torch.full((nv,), 0xA5, dtype=torch.uint8, device="cuda:0")

    def device_call(level, prm, array):
        def call():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            p.occlusion_device(level, prm, array.data_ptr(), array.numel(), None)
            e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)
        return call

    def alternating(call, *others):
        """call (returns its own ms) and the others (wall time) once per round -> medians"""
        rows = [[] for _ in range(1 + len(others))]
        for k in range(reps + 2):
            t = [call()] + [timed(fn)[0] for fn in others]
            if k >= 2:
                for r, v in zip(rows, t):
                    r.append(v)
        return [med(r) for r in rows]

    def moved(level, prm, table):
        q = prm[0]
        vis = oo.visited(table, prm)
        baked = sum(len(oo.entry_vertices(t, bool(int(q["flags"]) & 1))) for t, v in zip(table, vis) if v)
        edge = 16 + 2 * (int(q["steps"]) + 2) + 1
        return baked, int(vis.sum()), baked * 49 + int(vis.sum()) * edge ** 3

    def ray_yardstick(level, steps, table, pool, count=100000):
        """-> (call, rays, vertices): the probes of `count` sampled regular vertices of the level as rays on its meshes"""
        idx = np.concatenate([oo.entry_vertices(t, False) for t in table])
        rng = np.random.RandomState(level + 1)
        pick = idx[rng.randint(0, len(idx), min(count, len(idx)))]
        P, N, baked = oo.quantise(pool["pos"][pick], pool["nrm"][pick], level)
        s = 1 << level
        O = (P + 2 * N).astype(np.float64) * (s / 256.0)          # grid axes, voxels
        rows = []
        for S in oo.DIRS:
            w = (N @ S) >> 8
            k = np.nonzero((w > 0) & baked)[0]
            r = np.zeros(len(k), RAY_DTYPE)
            r["origin"] = O[k][:, [0, 2, 1]]
            r["dir"] = (S[[0, 2, 1]] * (s / 256.0)).astype(np.float32)[None, :]
            r["t_max"] = steps
            rows.append(r)
        rays = np.concatenate(rows)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1)).to("cuda:0")
        d_hits = torch.zeros(len(rays) * 48, dtype=torch.uint8, device="cuda:0")
        p.raycast_prepare(level)

        def call():
            p.raycast_device(d_rays.data_ptr(), len(rays), d_hits.data_ptr(), level)
            stream.synchronize()
        return call, len(rays), len(pick)

    def row(label, level, prm, array=None, table=None, pool=None, rays=True):
        table, pool = tabs[level] if table is None else table, verts if pool is None else pool
        array = d_ao if array is None else array
        baked, visited, nbytes = moved(level, prm, table)
        copy = Copy(copier, nbytes)
        others = [copy]
        if rays:
            ray_call, nrays, sampled = ray_yardstick(level, int(prm[0]["steps"]), table, pool)
            others.append(ray_call)
        t = alternating(device_call(level, prm, array), *others)
        copy.free()
        text = "  %s: %.4f ms for %d vertices of %d entries (%.2f ns per vertex) | memcpy of %.1f MB %.4f ms: call / memcpy %.2f" % (
            label, t[0], baked, visited, t[0] * 1e6 / max(baked, 1), nbytes / 1e6, t[1], t[0] / t[1])
        if rays:
            per_vertex = t[2] / sampled
            text += " | %d rays of %d sampled vertices %.4f ms: per vertex, rays / bake %.0f" % (nrays, sampled, t[2], per_vertex / (t[0] / max(baked, 1)))
        print(text)
        return t[0]

    for steps in (4, 8, 12):
        row("level 0, whole, %d steps" % steps, 0, occlusion_params(steps=steps), rays=steps == 8)
    for level in range(1, min(levels, 4)):
        row("level %d, whole, 8 steps" % level, level, occlusion_params(steps=8))
    row("level 0, 8 steps, with the transition meshes", 0, occlusion_params(steps=8, transitions=True), rays=False)
    p.debug_occlusion_shortcuts(False)
    row("level 0, 8 steps, sign summaries off", 0, occlusion_params(steps=8), rays=False)
    p.debug_occlusion_shortcuts(True)

    # the host form
    prm = occlusion_params(steps=8)
    ao, counts = p.occlusion(0, prm)
    t = med([timed(lambda: p.occlusion(0, prm))[0] for _ in range(reps)])
    print("  the host form of level 0, 8 steps (one byte per pool vertex copied back, %.1f MB): %.4f ms; vertices %d, mean byte %.1f, darkest %d, open %d" % (
        nv / 1e6, t, int(counts["vertices"]), int(counts["sum"]) / max(int(counts["vertices"]), 1), int(counts["darkest"]), int(counts["open"])))

    # 2 000 random vertices per level against the numpy oracle, on a part of the grid read back through a stamp
    size = min(384, n)
    lo = (n // 2 - size // 2) // 16 * 16
    st = p.capture_stamp(((lo, lo, 0), (lo + size, lo + size, n)))
    part = st.read()[0]
    st.free()
    rng = np.random.RandomState(4)
    for level in range(min(levels, 4)):
        s, steps = 1 << level, 12
        got = p.occlusion(level, occlusion_params(steps=steps, transitions=True), counts=False)[0]
        idx = np.concatenate([oo.entry_vertices(t, True) for t in tabs[level]])
        g = verts["pos"][idx][:, [0, 2]]
        margin = (steps + 2) * s
        inside = np.all((g >= lo + margin) & (g <= lo + size - 1 - margin), axis=1) if size < n else np.ones(len(idx), bool)
        pick = idx[inside]
        pick = pick[rng.permutation(len(pick))[:2000]]
        want = oo.bake(part, level, steps, verts["pos"][pick], verts["nrm"][pick], part=(n, (lo, lo, 0)))[0]
        assert len(pick) and np.array_equal(want, got[pick]), (level, int((want != got[pick]).sum()))
        print("  level %d: %d random vertices at %d steps equal the numpy oracle (mean byte %.1f, %d below 255)" % (level, len(pick), steps, want.mean(), int((want < 255).sum())))

    # the filtered re-bake after one crater
    c = n / 2.0
    h = float(p.heightmap(((n // 2, n // 2, 0), (n // 2 + 1, n // 2 + 1, n)))[0][0, 0, 0]) / 256.0
    mn, mx = p.inject_ball((c, h, c), (12, 12, 12), 10.0, 2)   # (Y up, as Grid::InjectSurface takes it)
    p.execute_dirty(mn, mx)
    tabs2, verts2 = snapshot()
    d_ao2 = torch.full((len(verts2),), 0xA5, dtype=torch.uint8, device="cuda:0")
    for level in range(min(levels, 2)):
        s = 1 << level
        grow = 8 * s + 16 * s
        box = occlusion_params(steps=8, transitions=True, box_min=np.asarray(mn, np.float32) - grow, box_max=np.asarray(mx, np.float32) + grow)
        row("level %d, 8 steps, filtered re-bake after one crater" % level, level, box, array=d_ao2, table=tabs2[level], pool=verts2, rays=False)
    p.set_stream(0)
    p.close()


if __name__ == "__main__":
    main()
