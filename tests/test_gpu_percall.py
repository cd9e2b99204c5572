"""What a full run costs outside its kernels, and what that must not break (vx_hip.hip wait_published, vx_host.inl settle_run):
vx_polygonize on the single-stream path takes its device time from two clock words of the header and returns when the header
has arrived in page-locked memory - the last kernel may still be running, and the next run is queued behind it unwaited.  Here:
runs back to back, a run that has to be repeated, every kind of call that can meet a run in flight, and device_ms itself.
32^3 with 2 levels and the 64^3 terrain with 3 levels (the smallest grid with material, regular and transition items on the
upper queue); VX_SYNC_WAIT=1 (the stream is waited for) and stage timing (the event path) are the references."""
import os
import time

import numpy as np
import pytest

import vxo

pytestmark = pytest.mark.gpu


def new_poly(**env):
    """A context created under the given environment (the knobs are read once, when a context is created)."""
    from voxels_amd import Polygonizer
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        p = Polygonizer(device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def digest_of(p):
    from voxels_amd import digest
    return digest.surface_digest(p.all_levels())


def same(a, b):
    from voxels_amd import digest
    return digest.digests_equal(a, b)


def device_sync():
    import torch
    torch.cuda.synchronize()


def signature(info):
    return (tuple(int(x) for x in info.active_blocks[:info.levels]), int(info.total_verts), int(info.total_indices))


def back_to_back(p, calls=300):
    """`calls` executes with the level limits cycling 1, 3, 2 and nothing between them; the digest behind the last one"""
    first = {}
    for i in range(calls):
        limit = (1, 3, 2)[i % 3]
        s = signature(p.execute(limit))
        assert s == first.setdefault(limit, s), (i, limit, s, first[limit])
    return digest_of(p)


def test_back_to_back_runs():
    p, q, r = new_poly(), new_poly(VX_SYNC_WAIT="1"), new_poly()
    r.set_stage_timing(True)
    try:
        for x in (p, q, r):
            x.create_terrain(64, 1337)
        d = back_to_back(p)
        assert d[0][:, 1].sum() > 0 and (d[0][1:, 3] > 0).any()  # (vertices, and transition vertices above level 0)
        assert same(d, back_to_back(q))
        assert same(d, back_to_back(r))
    finally:
        for x in (p, q, r):
            x.close()


def test_a_repeated_run():
    """Pools too small for the meshes (VX_POOL_SLACK=64, the tight pools of the edit-sequence tests): the first run of a context
    is the chain of launches (nothing is known about its surface yet), so the single-stream run that does not fit is the one
    behind a change to a larger grid - it grows the pools, while the attempt that overflowed may still be draining, and runs again."""
    p, ref = new_poly(VX_POOL_SLACK="64"), new_poly()
    try:
        p.create_terrain(32, 1337)
        assert p.execute().retries >= 1
        p.execute()
        p.create_terrain(64, 1337)
        info = p.execute()
        assert info.retries >= 1
        ref.create_terrain(64, 1337)
        want = ref.execute()
        assert signature(info) == signature(want)
        assert same(digest_of(p), digest_of(ref))
    finally:
        p.close(); ref.close()


@pytest.mark.parametrize("n", [32, 64])
def test_with_a_run_in_flight(n):
    ref = new_poly(VX_SYNC_WAIT="1")
    try:
        # close() at once
        p = new_poly()
        p.create_terrain(n, 1337)
        p.execute(); p.execute()
        p.close()
        # another grid, then a run: the new grid's surface
        p = new_poly()
        p.create_terrain(n, 1337)
        p.execute(); p.execute()
        p.create_terrain(n, 4242)
        p.execute()
        ref.create_terrain(n, 4242)
        ref.execute()
        want = digest_of(ref)
        assert same(digest_of(p), want)
        # invalidate, then a run
        p.execute()
        p.invalidate()
        p.execute()
        assert same(digest_of(p), want)
        # an edit and an incremental run, then a level's meshes: the same sequence with every run waited for, byte for byte
        got = []
        for x in (p, ref):
            x.execute(); x.execute()
            mn, mx = x.inject_ball((n / 2.0, n / 2.0, n / 2.0), (n / 4.0, n / 4.0, n / 4.0), n / 5.0, 2)
            ids = x.execute_dirty(mn, mx)
            assert ids.size > 0
            lv = x.level(0)
            got.append([ids.tobytes()] + [np.ascontiguousarray(a).tobytes() for a in (lv.infos, lv.verts, lv.idx, lv.tverts, lv.tidx)])
        assert got[0] == got[1]
        p.close()
    finally:
        ref.close()


@pytest.mark.parametrize("path", ["clock", "clock+sync", "events"])
def test_device_ms(path):
    """Positive, and not larger than the wall time around the call (between two device synchronisations) - on the timestamp
    path, on the event path (stage timing), for full and for incremental runs."""
    p = new_poly(**({"VX_SYNC_WAIT": "1"} if path == "clock+sync" else {}))
    try:
        p.set_stage_timing(path == "events")
        for n in (32, 64):
            p.create_terrain(n, 1337)
            p.execute(); p.execute()
            for _ in range(5):
                device_sync()
                t = time.perf_counter()
                info = p.execute()
                device_sync()
                wall = (time.perf_counter() - t) * 1e3
                print("%s %d^3 full: device %.4f ms, wall %.4f ms" % (path, n, info.device_ms, wall))
                assert 0.0 < info.device_ms <= wall
            mn, mx = p.inject_ball((n / 2.0, n / 2.0, n / 2.0), (n / 4.0, n / 4.0, n / 4.0), n / 5.0, 2)
            device_sync()
            t = time.perf_counter()
            p.execute_dirty(mn, mx)
            device_sync()
            wall = (time.perf_counter() - t) * 1e3
            print("%s %d^3 incremental: device %.4f ms, wall %.4f ms" % (path, n, p.info.device_ms, wall))
            assert 0.0 < p.info.device_ms <= wall
    finally:
        p.close()
