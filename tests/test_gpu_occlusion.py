"""vx_occlusion / vx_occlusion_device on the MI355X against the numpy oracle of tests/occlusion_oracle.py, byte for byte with no
tolerance, on the block tables and the vertex pool copied from the same context, against the grid as the context holds it."""
import ctypes as C

import numpy as np
import pytest

import fields
import occlusion_oracle as oo
import vxo
from occlusion_oracle import occlusion_params
from test_gpu_parity import port  # noqa: F401  (fixture)
from test_gpu_scatter import snapshot

pytestmark = pytest.mark.gpu

INVALID = -1
POISON = 0xA5
COUNT_NAMES = oo.OCCLUSION_COUNTS_DTYPE.names


@pytest.fixture(scope="module")
def torch():
    import torch
    torch.cuda.init()
    return torch


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    p.set_materials(vxo.default_lut())
    return p


def flags_of(d):
    from voxels_amd import synth
    return synth.block_empty_flags(d)


def upload(p, name):
    d = oo.grids()[name]
    n = d.shape[0]
    if name == "terrain48":
        m, b = fields.materials_for(n, 11)
    else:
        m, b = np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint8)
    p.upload(np.ascontiguousarray(d), m, b, flags_of(d))
    return d


class Resident:
    """a context with one of the shared grids polygonized, its snapshot, and the oracle's byte per pool vertex - baked once per
    (level, steps) over every range of the level and left unchanged"""

    def __init__(self, name):
        self.p = new_poly()
        self.dist = upload(self.p, name)
        self.p.execute()
        self.refresh()

    def refresh(self, dist=None):
        self.dist = self.dist if dist is None else dist
        self.tabs, self.verts, _ = snapshot(self.p)
        self.levels = min(len(self.tabs), len(oo.LEVELS))
        self.cache = {}

    def bytes_of(self, level, steps):
        """(byte, baked) per pool vertex of the level's entries, 255 / False elsewhere"""
        if (level, steps) not in self.cache:
            out, baked = np.full(len(self.verts), 255, np.uint8), np.zeros(len(self.verts), bool)
            parts = [oo.entry_vertices(t, True) for t in self.tabs[level]]
            idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
            out[idx], baked[idx] = oo.bake(self.dist, level, steps, self.verts["pos"][idx], self.verts["nrm"][idx])
            out.setflags(write=False)
            self.cache[level, steps] = (out, baked)
        return self.cache[level, steps]

    def expect(self, level, prm, fill):
        """what a call leaves in an array filled with `fill` -> (array, counts dict, pool indices baked)"""
        q = np.asarray(prm, oo.OCCLUSION_PARAMS_DTYPE).reshape(-1)[0]
        byte, baked = self.bytes_of(level, int(q["steps"]))
        vis = oo.visited(self.tabs[level], prm)
        parts = [oo.entry_vertices(t, bool(int(q["flags"]) & oo.OCCLUSION_TRANSITIONS)) for t, v in zip(self.tabs[level], vis) if v]
        idx = np.concatenate(parts) if parts else np.zeros(0, np.int64)
        out = np.full(len(self.verts), fill, np.uint8)
        out[idx] = byte[idx]
        b = byte[idx][baked[idx]]
        counts = {"vertices": int(baked[idx].sum()), "sum": int(b.astype(np.int64).sum()), "entries": len(self.tabs[level]), "visited_entries": int(vis.sum()),
                  "darkest": int(b.min()) if b.size else 255, "open": int((b == 255).sum())}
        return out, counts, idx


def as_dict(rec):
    return {k: int(rec[k]) for k in COUNT_NAMES}


def host_form(p, level, prm):
    ao, rec = p.occlusion(level, prm)
    return ao, as_dict(rec)


def device_form(torch, p, level, prm, nv, counts=True, guard=64):
    """vx_occlusion_device into poisoned torch tensors on a stream of its own -> (bytes, counts dict or None, guards intact)"""
    d_ao = torch.full((nv + guard,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((32 + guard,), POISON, dtype=torch.uint8, device="cuda") if counts else None
    s = torch.cuda.Stream()
    p.set_stream(s.cuda_stream)
    p.occlusion_device(level, prm, d_ao.data_ptr(), nv, None if d_counts is None else d_counts.data_ptr())
    s.synchronize()
    p.set_stream(0)
    ao = d_ao.cpu().numpy()
    intact = bool(np.all(ao[nv:] == POISON))
    c = None
    if counts:
        cnt = d_counts.cpu().numpy()
        intact = intact and bool(np.all(cnt[32:] == POISON))
        c = as_dict(cnt[:32].view(oo.OCCLUSION_COUNTS_DTYPE)[0])
    return ao[:nv], c, intact


def check(torch, r, level, prm, label, device=True):
    want, counts, idx = r.expect(level, prm, 255)
    ao, c = host_form(r.p, level, prm)
    assert c == counts, (label, c, counts)
    assert ao.tobytes() == want.tobytes(), (label, int((ao != want).sum()), len(idx))
    if device:
        want, _, _ = r.expect(level, prm, POISON)
        dao, dc, intact = device_form(torch, r.p, level, prm, len(r.verts))
        assert intact and dc == counts, (label, dc, counts, intact)
        assert dao.tobytes() == want.tobytes(), (label, int((dao != want).sum()))
    return ao, counts, idx


@pytest.fixture(scope="module")
def resident():
    made = {}

    def get(name):
        if name not in made:
            made[name] = Resident(name)
        return made[name]

    yield get
    for r in made.values():
        r.p.close()


# 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sphere32", "terrain48", "caves64"])
def test_bake_matches_the_oracle(torch, resident, name):
    """host form against the oracle, device form against both, with and without the transition meshes, counts included"""
    r = resident(name)
    assert r.levels >= 2
    darkened = transition_vertices = 0
    for level in range(r.levels):
        for steps in oo.STEPS:
            for transitions in (False, True):
                ao, c, idx = check(torch, r, level, occlusion_params(steps=steps, transitions=transitions), "%s L%d steps %d tr %d" % (name, level, steps, transitions))
                assert c["vertices"] == len(idx) > 0 and c["visited_entries"] == c["entries"] == len(r.tabs[level])
                darkened += c["vertices"] - c["open"]
                transition_vertices += transitions * (len(idx) - int(r.tabs[level]["v_count"].sum()))
    # (a ball is convex: every probe of every vertex leaves it, so every byte is 255 - the terrain and the caves are not)
    assert darkened == 0 if name == "sphere32" else darkened > 0
    assert transition_vertices > 0 or name != "caves64"        # (two-level grids of 32 and 48 may carry no transition mesh; the caves do)


# 2 -------------------------------------------------------------------------------------------------------------------------
def test_filter_box(torch, resident):
    r = resident("caves64")
    nv = len(r.verts)
    for level, box in ((0, dict(box_min=[2.5, 1.0, 3.0], box_max=[29.75, 40.0, 21.5])), (1, dict(box_min=[0.0, 0.0, 0.0], box_max=[20.0, 20.0, 20.0]))):
        prm = occlusion_params(steps=5, transitions=True, **box)
        full, _, _ = r.expect(level, occlusion_params(steps=5, transitions=True), POISON)
        want, counts, idx = r.expect(level, prm, POISON)
        assert 0 < counts["visited_entries"] < counts["entries"]
        dao, dc, intact = device_form(torch, r.p, level, prm, nv)
        assert intact and dc == counts
        assert dao.tobytes() == want.tobytes()
        mask = np.zeros(nv, bool)
        mask[idx] = True
        assert (dao[~mask] == POISON).all() and dao[mask].tobytes() == full[mask].tobytes()   # unvisited bytes unchanged, visited ones the full bake's
        check(torch, r, level, prm, "filter L%d" % level, device=False)
    # a box that meets nothing: nothing is written
    prm = occlusion_params(steps=5, box_min=[500, 500, 500], box_max=[600, 600, 600])
    dao, dc, intact = device_form(torch, r.p, 0, prm, nv)
    assert intact and (dao == POISON).all() and dc == dict(vertices=0, sum=0, entries=len(r.tabs[0]), visited_entries=0, darkest=255, open=0)


# 3 -------------------------------------------------------------------------------------------------------------------------
def test_shortcuts_on_and_off_are_the_same_bytes(torch, resident):
    r = resident("terrain48")
    try:
        for level in range(r.levels):
            prm = occlusion_params(steps=12, transitions=True)
            on = host_form(r.p, level, prm)
            r.p.debug_occlusion_shortcuts(False)
            off = host_form(r.p, level, prm)
            r.p.debug_occlusion_shortcuts(True)
            assert on[1] == off[1] and on[0].tobytes() == off[0].tobytes() == r.expect(level, prm, 255)[0].tobytes()
    finally:
        r.p.debug_occlusion_shortcuts(True)


# 4 -------------------------------------------------------------------------------------------------------------------------
def test_edits(torch, port):
    """after vx_grid_inject_ball WITHOUT a run: the old vertices against the new grid, in the oracle likewise (the sign summaries
    are brought up to date by the edit, so the shortcuts stay in use).  After vx_polygonize_dirty: the appended ranges are baked,
    and a re-bake filtered to the edit's box grown by steps * s + 16 * s equals a full re-bake on every visited entry.  After
    vx_compact_pools: the same bytes per entry at the new offsets."""
    r = Resident("caves64")
    p = r.p
    try:
        steps = 5
        prm = occlusion_params(steps=steps, transitions=True)
        before = [check(torch, r, L, prm, "before L%d" % L, device=False)[0] for L in range(r.levels)]
        mn, mx = p.inject_ball((20.0, 22.0, 31.0), (6, 6, 6), 5.0, 2)
        dist = port.grid_load(p.pack()).read_dense()[0]
        assert (dist != r.dist).any()
        r.refresh(np.ascontiguousarray(dist))            # (the same tables and vertices: nothing has run)
        changed = 0
        for L in range(r.levels):
            ao = check(torch, r, L, prm, "edited grid, old vertices L%d" % L)[0]
            changed += int((ao != before[L]).sum())
            p.debug_occlusion_shortcuts(False)
            assert host_form(p, L, prm)[0].tobytes() == ao.tobytes()
            p.debug_occlusion_shortcuts(True)
        assert changed > 0
        old_nv = len(r.verts)
        assert len(p.execute_dirty(mn, mx))
        r.refresh()
        assert len(r.verts) > old_nv                      # appended
        for L in range(r.levels):
            ao, c, idx = check(torch, r, L, prm, "after the incremental run L%d" % L)
            assert idx.max() >= old_nv or L > 0
            s = 1 << L
            grow = steps * s + 16 * s
            box = occlusion_params(steps=steps, transitions=True, box_min=np.asarray(mn, np.float32) - grow, box_max=np.asarray(mx, np.float32) + grow)
            want, counts, part = r.expect(L, box, POISON)
            dao, dc, intact = device_form(torch, p, L, box, len(r.verts))
            assert intact and dc == counts and dao.tobytes() == want.tobytes() and counts["visited_entries"] > 0
            assert dao[part].tobytes() == ao[part].tobytes()
        per_entry = [{int(t["coord_id"]): check(torch, r, L, prm, "", device=False)[0][oo.entry_vertices(t, True)].tobytes() for t in r.tabs[L]} for L in range(r.levels)]
        p.compact_pools()
        r.refresh()
        for L in range(r.levels):
            ao = check(torch, r, L, prm, "compacted L%d" % L)[0]
            assert {int(t["coord_id"]): ao[oo.entry_vertices(t, True)].tobytes() for t in r.tabs[L]} == per_entry[L]
    finally:
        p.close()


# 5 -------------------------------------------------------------------------------------------------------------------------
def test_behind_a_one_launch_kept_run(torch):
    """the table's count is the device's behind a full run; the bake leaves plan, store and layout alone: the run after it is
    still one launch"""
    import test_gpu_cellmap as cellmap
    from test_gpu_layout import KEPT_ONE, run, warm
    from test_gpu_matstore import make_poly
    from test_gpu_slotplan import plan_field
    d, m, b = plan_field("terrain64")
    p = make_poly()
    try:
        p.upload(d, m, b, cellmap.flags_of(d))
        warm(p)
        run(p, KEPT_ONE, label="the kept run in front of the bake")
        r = Resident.__new__(Resident)
        r.p, r.dist = p, np.ascontiguousarray(d)
        r.refresh()
        for L in range(r.levels):
            check(torch, r, L, occlusion_params(steps=5, transitions=True), "behind a one-launch run L%d" % L)
            run(p, KEPT_ONE, label="the kept run behind the bake of level %d" % L)
            tabs, verts, _ = snapshot(p)
            assert verts.tobytes() == r.verts.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(tabs, r.tabs))
    finally:
        p.close()


# 6 -------------------------------------------------------------------------------------------------------------------------
def test_nothing_changes(torch, resident):
    from voxels_amd import digest
    r = resident("terrain48")
    p = r.p
    grid, meshes = p.pack(), digest.surface_digest(p.all_levels())
    for L in range(r.levels):
        host_form(p, L, occlusion_params(steps=12, transitions=True))
        device_form(torch, p, L, occlusion_params(steps=12, transitions=True), len(r.verts))
    assert np.asarray(p.pack()).tobytes() == np.asarray(grid).tobytes()
    assert digest.digests_equal(digest.surface_digest(p.all_levels()), meshes)
    tabs, verts, _ = snapshot(p)
    assert verts.tobytes() == r.verts.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(tabs, r.tabs))


# 7 -------------------------------------------------------------------------------------------------------------------------
def test_empty_level(torch):
    n = 32
    p = new_poly()
    p.upload(np.full((n, n, n), 127, np.int8), np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint8), np.ones((n // 16) ** 3, np.uint8))
    p.execute()
    assert p.info.levels >= 1 and p.device_block_table(0)[1] == 0
    nv = int(p.device_meshes()[2])
    prm = np.ascontiguousarray(occlusion_params(steps=4), oo.OCCLUSION_PARAMS_DTYPE)
    ao, counts = np.full(16, POISON, np.uint8), np.full(32, POISON, np.uint8)
    rc = p._L.lib.vx_occlusion(p._h, 0, prm.ctypes.data_as(C.c_void_p), ao.ctypes.data_as(C.c_void_p), 16, counts.ctypes.data_as(C.c_void_p))
    assert rc == 0 and as_dict(counts.view(oo.OCCLUSION_COUNTS_DTYPE)[0]) == dict(vertices=0, sum=0, entries=0, visited_entries=0, darkest=255, open=0)
    assert (ao[nv:] == POISON).all() and (ao[:nv] == 255).all()
    dao, dc, intact = device_form(torch, p, 0, prm, 16)
    assert intact and (dao == POISON).all() and dc == dict(vertices=0, sum=0, entries=0, visited_entries=0, darkest=255, open=0)
    p.close()


# 8 -------------------------------------------------------------------------------------------------------------------------
def test_validation(torch, resident):
    r = resident("sphere32")
    p = r.p
    lib, vp = p._L.lib, C.c_void_p
    nv = len(r.verts)
    d_ao = torch.full((nv + 16,), POISON, dtype=torch.uint8, device="cuda")
    d_counts = torch.full((48,), POISON, dtype=torch.uint8, device="cuda")
    ao, counts = np.full(nv, POISON, np.uint8), np.full(32, POISON, np.uint8)

    def ptr(a):
        return a.ctypes.data_as(vp)

    def both(label, level, prm, capacity=nv, no_array=False, ctx=p):
        rec = None if prm is None else np.ascontiguousarray(prm, oo.OCCLUSION_PARAMS_DTYPE)
        rc = lib.vx_occlusion(ctx._h, level, None if rec is None else ptr(rec), None if no_array else ptr(ao), capacity, ptr(counts))
        assert rc == INVALID, ("host", label, rc)
        rc = lib.vx_occlusion_device(ctx._h, level, None if rec is None else ptr(rec), None if no_array else vp(d_ao.data_ptr()), capacity, vp(d_counts.data_ptr()))
        assert rc == INVALID, ("device", label, rc)
        assert oo.check(1, 1, p.info.levels, level, rec, not no_array, capacity, nv) == -1 or ctx is not p, label

    def changed(**kw):
        prm = occlusion_params(steps=4)
        for k, v in kw.items():
            prm[k] = v
        return prm

    good = occlusion_params(steps=4)
    nan = float("nan")
    both("level beyond the run", p.info.levels, good)
    both("null params", 0, None)
    both("null array", 0, good, no_array=True)
    both("capacity below n_verts", 0, good, capacity=nv - 1)
    for steps in (0, 13):
        both("steps %d" % steps, 0, changed(steps=steps))
    for flags in (2, 3):
        both("flags %d" % flags, 0, changed(flags=flags))
    for k in range(4):
        w = [0, 0, 0, 0]
        w[k] = 1
        both("reserved[%d]" % k, 0, changed(reserved=w))
    for field in ("box_min", "box_max"):
        for a in range(3):
            v = [0.0, 0.0, 0.0] if field == "box_min" else [8.0, 8.0, 8.0]
            v[a] = nan
            both("NaN %s[%d]" % (field, a), 0, changed(**dict(dict(box_min=[0, 0, 0], box_max=[8, 8, 8]), **{field: v})))
    for a in range(3):
        lo = [0.0, 0.0, 0.0]
        lo[a] = 9.0
        both("box_min > box_max on axis %d" % a, 0, changed(box_min=lo, box_max=[8, 8, 8]))
    rec = np.ascontiguousarray(good, oo.OCCLUSION_PARAMS_DTYPE)
    assert lib.vx_occlusion_device(p._h, 0, ptr(rec), vp(d_ao.data_ptr()), nv, vp(d_counts.data_ptr() + 4)) == INVALID   # misaligned counts
    for fn in (lib.vx_occlusion, lib.vx_occlusion_device):
        assert fn(None, 0, ptr(rec), ptr(ao), nv, None) == INVALID                                                     # a null context
    empty = new_poly()  # no grid and no surface
    both("no grid", 0, good, ctx=empty)
    n = 32
    empty.upload(np.ascontiguousarray(oo.grids()["sphere32"]), np.zeros((n, n, n), np.uint8), np.zeros((n, n, n), np.uint8), flags_of(oo.grids()["sphere32"]))
    both("no surface", 0, good, ctx=empty)
    empty.close()
    torch.cuda.synchronize()
    for a in (ao, counts, d_ao.cpu().numpy(), d_counts.cpu().numpy()):
        assert np.all(a == POISON)
    # and the same buffers are written by a valid call
    assert lib.vx_occlusion(p._h, 0, ptr(rec), ptr(ao), nv, ptr(counts)) == 0
    assert not np.all(ao == POISON) and not np.all(counts == POISON)


def test_a_context_without_a_whole_grid_is_refused(torch):
    """an attached slab is not a whole grid of the context's own: the undo_whole_grid condition"""
    from voxels_amd import synth
    from voxels_amd.slab import SlabBuffers
    n = 64
    p = new_poly()
    try:
        slab = SlabBuffers(torch, n, 0, 1, torch.device("cuda", 0), axis="z")
        d, m, b = synth.terrain(n, 0, n, 3)
        slab.fill_from_full(d, m, b, flags_of(d))
        torch.cuda.synchronize()
        slab.attach(p)
        p.execute()
        nv = int(p.device_meshes()[2])
        assert nv > 0
        rec = np.ascontiguousarray(occlusion_params(steps=4), oo.OCCLUSION_PARAMS_DTYPE)
        ao = np.full(nv, POISON, np.uint8)
        d_ao = torch.full((nv,), POISON, dtype=torch.uint8, device="cuda")
        assert p._L.lib.vx_occlusion(p._h, 0, rec.ctypes.data_as(C.c_void_p), ao.ctypes.data_as(C.c_void_p), nv, None) == INVALID
        assert p._L.lib.vx_occlusion_device(p._h, 0, rec.ctypes.data_as(C.c_void_p), C.c_void_p(d_ao.data_ptr()), nv, None) == INVALID
        torch.cuda.synchronize()
        assert (ao == POISON).all() and (d_ao.cpu().numpy() == POISON).all()
    finally:
        p.close()


# 9 -------------------------------------------------------------------------------------------------------------------------
def test_module_life(torch):
    """a bake, then vx_ctx_destroy; two contexts side by side; the working memory small, regrown and small again"""
    prm = occlusion_params(steps=5, transitions=True)

    def per_entry(r, ao):
        """(a block's meshes lie in the pools where the run's blocks reserved their room: not the same in two contexts)"""
        return {int(t["coord_id"]): ao[oo.entry_vertices(t, True)].tobytes() for t in r.tabs[0]}

    a = Resident("sphere32")
    ao, counts = host_form(a.p, 0, prm)
    first = (per_entry(a, ao), counts, len(ao))
    a.p.close()                                          # (the state goes with the context)
    a, b = Resident("sphere32"), Resident("terrain48")
    try:
        ao, counts, _ = check(torch, a, 0, prm, "a new context")
        other = check(torch, b, 0, prm, "second context")
        assert counts == first[1] and per_entry(a, ao) == first[0]
        # the same context with a larger pool, then the small one again
        upload(a.p, "caves64")
        a.p.execute()
        a.refresh(oo.grids()["caves64"])
        assert len(a.verts) > first[2]
        check(torch, a, 0, prm, "regrown")
        upload(a.p, "sphere32")
        a.p.execute()
        a.refresh(oo.grids()["sphere32"])
        ao, counts, _ = check(torch, a, 0, prm, "small again")
        assert counts == first[1] and per_entry(a, ao) == first[0]
        assert host_form(b.p, 0, prm)[0].tobytes() == other[0].tobytes()
    finally:
        a.p.close()
        b.p.close()
