"""The stamps on the MI355X against the numpy statement of the header's text (tests/stamp_oracle.py), exactly.  The state of the
device grid is read back - the packed file (vx_grid_pack) expanded by the port, and the flag bytes, which a pack recomputes, by
vx_grid_read_block - as tests/test_gpu_undo.py does; results and counts are compared as bytes.  tests/test_stamp.py anchors the
oracle to answers written by hand."""
import ctypes as C

import numpy as np
import pytest

import fields
import stamp_oracle as sto
import undo_oracle as uo
import vxo

pytestmark = pytest.mark.gpu

R, U, S, P = sto.MODES
CASES = sto.cases()


def new_poly():
    from voxels_amd import Polygonizer
    p = Polygonizer(device=0)
    assert p.backend == "hip:gfx950"
    assert p._L.has_stamps
    p.set_materials(vxo.default_lut())
    return p


def resident(g):
    """a context that holds grid g, flag bytes included (a dense upload takes them from the caller)"""
    p = new_poly()
    p.upload(g.dist, g.mat, g.blend, g.flags)
    return p


def device_flags(p):
    f = np.zeros((p.n // 16) ** 3, np.uint8)
    for bid in range(f.size):
        p._check(p._lib.vx_grid_read_block(p._h, bid, None, None, None, f[bid:bid + 1].ctypes.data), "vx_grid_read_block")
    return f


def device_grid(p):
    d, m, b = vxo.load_port().grid_load(p.pack()).read_dense()
    return uo.Grid(d, m, b, device_flags(p))


def device_stamps(p, case_or_entries, g=None):
    """the entries of a case (or a list of St / None) as Stamps of p"""
    entries = case_or_entries.entries if isinstance(case_or_entries, sto.Case) else case_or_entries
    out = []
    for e in entries:
        if e is None:
            out.append(None)
        elif isinstance(e, tuple):
            out.append(p.capture_stamp((e[1], e[2])))
        else:
            out.append(p.upload_stamp(e.dist, e.mat, e.blend))
    return out


def same_records(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (a, b)


def same_grid(p, want):
    got = device_grid(p)
    for name in ("dist", "mat", "blend", "flags"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def check_batch(p, g, stamps, dev, ps):
    """pastes on the device and in the oracle (g, in place); everything compared"""
    want_res, want_counts = sto.paste(g, stamps, ps)
    res, counts = p.paste(dev, ps)
    same_records(res, want_res)
    same_records(counts, want_counts)
    same_grid(p, g)


# ---- stamps ---------------------------------------------------------------------------------------------------------------------

def test_capture_and_upload_round_trip():
    g = sto.terrain_grid(48)
    p = resident(g)
    pack0 = p.pack()
    p.execute()
    replay0 = p.material_path_counts()
    p.execute()
    replay1 = p.material_path_counts()
    # whole rows of 16 bytes; rows that start or end off a 16-byte border; one voxel; the whole grid
    for box in (((16, 3, 5), (48, 20, 9)), ((0, 0, 0), (16, 16, 16)), ((3, 16, 16), (19, 17, 40)), ((16, 0, 0), (31, 5, 5)), ((47, 47, 47), (48, 48, 48)), ((0, 0, 0), (48, 48, 48))):
        st = p.capture_stamp(box)
        want = sto.capture(g, box)
        info = st.info()
        assert info["size"].tolist() == list(want.size) and int(info["voxels"]) == want.dist.size and int(info["bytes"]) == 3 * want.dist.size and int(info["reserved"]) == 0
        for got, w in zip(st.read(), (want.dist, want.mat, want.blend)):
            assert got.dtype == w.dtype and np.array_equal(got, w), box
        st.free()
    # a capture changes nothing, kept state included: a full run replays what it replayed before
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), g.flags)
    p.execute()
    assert p.material_path_counts() == replay1, (replay0, replay1)
    src = sto.noise_stamp((7, 3, 5), 1)
    for mat, blend in ((src.mat, src.blend), (None, src.blend), (src.mat, None), (None, None)):
        st = p.upload_stamp(src.dist, mat, blend)
        d, m, b = st.read()
        assert np.array_equal(d, src.dist) and np.array_equal(m, src.mat if mat is not None else 0 * src.mat) and np.array_equal(b, src.blend if blend is not None else 0 * src.blend)
    only_dist = np.zeros((5, 3, 7), np.int8)
    p._check(p._lib.vx_stamp_read(p._h, st._s, only_dist.ctypes.data, None, None), "vx_stamp_read")
    assert np.array_equal(only_dist, src.dist)


# ---- the case list --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_on_the_device(case):
    g = case.grid()
    p = resident(g)
    check_batch(p, g, case.stamps(g), device_stamps(p, case), case.pastes)


# ---- batching -------------------------------------------------------------------------------------------------------------------

def test_a_batch_equals_its_pastes_one_call_at_a_time_and_repeats():
    g0 = sto.terrain_grid(48)
    stamps, ps = sto.random_batch(48, 77)
    ps = np.concatenate([ps, ps[::-1]])
    want = g0.copy()
    want_res, want_counts = sto.paste(want, stamps, ps)
    packs = []
    for how in ("batch", "batch", "single", "chunked"):
        p = resident(g0)
        dev = device_stamps(p, stamps)
        if how == "single":
            res = np.concatenate([p.paste(dev, ps[k:k + 1])[0] for k in range(ps.size)])
        else:
            if how == "chunked":   # lists of at most 7 entries: chunk borders fall inside the blocks' lists
                p._lib.vx_debug_paste_list_cap.argtypes = [C.c_void_p, C.c_uint32]
                assert p._lib.vx_debug_paste_list_cap(p._h, 7) == 0
            res, counts = p.paste(dev, ps)
            same_records(counts, want_counts)
        same_records(res, want_res)
        same_grid(p, want)
        packs.append(p.pack())
    assert all(np.array_equal(packs[0], k) for k in packs[1:])


def test_a_list_longer_than_the_sort_tile():
    # 1 100 pastes on one block: its list is sorted in device memory, not in LDS
    rng = np.random.default_rng(21)
    g = sto.terrain_grid(48)
    stamps = [sto.noise_stamp((4, 3, 5), 1), sto.noise_stamp((2, 6, 3), 2)]
    ps = sto.pastes([(tuple(int(v) for v in rng.integers(16, 26, 3)), int(rng.integers(2)), int(rng.integers(8)), int(rng.integers(4))) for _ in range(1100)])
    p = resident(g)
    check_batch(p, g, stamps, device_stamps(p, stamps), ps)


def test_a_large_batch():
    rng = np.random.default_rng(22)
    g = sto.terrain_grid(64)
    stamps = [sto.noise_stamp((5, 5, 5), 3)]
    ps = sto.pastes([(tuple(int(v) for v in rng.integers(-4, 64, 3)), 0, int(rng.integers(8)), int(rng.integers(4))) for _ in range(2000)])
    p = resident(g)
    check_batch(p, g, stamps, device_stamps(p, stamps), ps)


# ---- flags ----------------------------------------------------------------------------------------------------------------------

def test_flags_change_only_where_a_paste_other_than_paint_touched():
    g = sto.terrain_grid(48)
    g.flags[:] ^= 1                        # every flag disagrees with the codec
    before = g.flags.copy()
    p = resident(g)
    stamps = [sto.noise_stamp((10, 10, 10), 4), sto.solid_stamp((20, 20, 20), 100)]
    ps = sto.pastes([((2, 2, 2), 0, 0, P), ((30, 30, 30), 0, 1, P), ((20, 4, 36), 0, 2, U), ((0, 20, 0), 1, 0, S), ((28, 0, 0), 1, 3, P)])
    check_batch(p, g, stamps, device_stamps(p, stamps), ps)
    carved = np.zeros(27, bool)
    for k in (2, 3):
        carved[sto.blocks_of_box(sto.paste_box(ps[k], stamps[int(ps[k]["stamp"])].size, 48)[1], 48)] = True
    assert np.array_equal(g.flags[~carved], before[~carved]) and (g.flags[carved] != before[carved]).any()


# ---- the incremental path -------------------------------------------------------------------------------------------------------

def level0_equals(p, fresh):
    part, full = p.all_levels()[0], fresh.all_levels()[0]
    assert len(part.infos) == len(full.infos)
    at = {tuple(c): i for c, i in zip(full.infos["min_corner"].tolist(), full.infos["id"])}
    part.infos = part.infos.copy()
    part.infos["id"] = [at[tuple(c)] for c in part.infos["min_corner"].tolist()]
    ok, msg = fields.listed_blocks_equal_by_id(part, full)
    assert ok, msg


@pytest.mark.parametrize("modes", [(R, U, S), (P, P, P)], ids=["carve", "paint only"])
def test_a_batch_feeds_the_incremental_path(modes):
    g = sto.terrain_grid(64)
    p = resident(g)
    p.execute()
    entries = [("capture", (8, 8, 2), (40, 30, 30)), sto.solid_stamp((9, 9, 9), -90, 5, 77)]
    stamps = [sto.capture(g, (entries[0][1], entries[0][2])), entries[1]]
    ps = sto.pastes([((20, 25, 12), 0, 1, modes[0]), ((3, 40, 20), 1, 0, modes[1]), ((30, 10, 22), 1, 5, modes[2])])
    want_counts = sto.paste(g, stamps, ps)[1]
    counts = p.paste(device_stamps(p, entries), ps)[1]
    same_records(counts, want_counts)
    assert int(counts["changed_voxels"]) > 0
    p.execute_dirty(counts["out_min"], counts["out_max"])
    fresh = resident(g)                    # the oracle's grid
    fresh.execute()
    level0_equals(p, fresh)
    p.execute()
    ok, msg = fields.surface_equal(p.all_levels(), fresh.all_levels())
    assert ok, msg
    assert np.array_equal(p.stats(), fresh.stats())


# ---- undo -----------------------------------------------------------------------------------------------------------------------

def test_capture_paste_trim_swap_restores_the_grid():
    from voxels_amd import paste_boxes
    g = sto.terrain_grid(48)
    p = resident(g)
    pack0, flags0 = p.pack(), device_flags(p)
    stamps = [sto.noise_stamp((17, 5, 3), 5), sto.capture(g, ((0, 0, 0), (20, 20, 14)))]
    ps = sto.pastes([((9, 12, 14), 0, 3, R), ((60, 0, 0), 0, 0, R), ((25, 25, 0), 1, 0, R), ((-3, 30, 30), 0, 6, S), ((0, 0, 0), 1, 0, U)])
    boxes = paste_boxes(ps, [st.size for st in stamps], 48)
    assert boxes.size == ps.size - 1
    rec = p.capture(boxes)
    counts = p.paste(device_stamps(p, stamps), ps)[1]
    assert int(rec.info()["blocks"]) == int(counts["touched_blocks"]) and rec.block_ids().tolist() == sto.touched_blocks(stamps, ps, 48).tolist()
    assert not np.array_equal(p.pack(), pack0)
    dropped = rec.trim()
    assert int(rec.info()["blocks"]) == int(counts["changed_blocks"]) == int(counts["touched_blocks"]) - dropped and dropped > 0
    res = rec.swap()
    assert np.array_equal(p.pack(), pack0) and np.array_equal(device_flags(p), flags0)
    assert (int(res["changed_voxels"]), int(res["flag_changes"])) == (int(counts["changed_voxels"]), int(counts["flag_changes"]))
    assert res["out_min"].tolist() == counts["out_min"].tolist() and res["out_max"].tolist() == counts["out_max"].tolist()


# ---- another grid ---------------------------------------------------------------------------------------------------------------

def test_a_stamp_survives_the_upload_of_a_grid_of_another_edge():
    g48, g64 = sto.terrain_grid(48), sto.terrain_grid(64)
    p = resident(g48)
    box = ((5, 6, 7), (37, 30, 20))
    dev = [p.capture_stamp(box), p.upload_stamp(sto.noise_stamp((6, 6, 6), 6).dist)]
    stamps = [sto.capture(g48, box), sto.St(sto.noise_stamp((6, 6, 6), 6).dist)]
    p.execute()
    p.compact_pools()
    p.upload(g64.dist, g64.mat, g64.blend, g64.flags)
    ps = sto.pastes([((40, 40, 30), 0, 7, R), ((50, 2, 3), 1, 2, U), ((0, 0, 40), 0, 1, P)])
    check_batch(p, g64, stamps, dev, ps)
    for got, w in zip(dev[0].read(), (stamps[0].dist, stamps[0].mat, stamps[0].blend)):
        assert np.array_equal(got, w)


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_every_listed_error_is_invalid_and_changes_nothing():
    from voxels_amd import Polygonizer, binding
    g = sto.terrain_grid(48)
    p = resident(g)
    other = resident(g)
    lib, h = p._lib, p._h
    src = sto.noise_stamp((3, 4, 5), 7)
    mine, theirs = p.upload_stamp(src.dist, src.mat, src.blend), other.upload_stamp(src.dist)
    out = C.c_void_p()
    box = binding.boxes([((0, 0, 0), (8, 8, 8))])
    size = np.array([3, 4, 5], np.uint32)
    d = src.dist
    info = np.zeros(1, binding.STAMP_INFO_DTYPE)
    INVALID = -1
    # capture
    assert lib.vx_stamp_capture(None, box.ctypes.data, C.byref(out)) == INVALID
    assert lib.vx_stamp_capture(h, box.ctypes.data, None) == INVALID and lib.vx_stamp_capture(h, None, C.byref(out)) == INVALID
    for lo, hi in (((4, 4, 4), (4, 8, 8)), ((0, 0, 0), (49, 8, 8)), ((0, 9, 0), (8, 8, 8))):
        assert lib.vx_stamp_capture(h, binding.boxes([(lo, hi)]).ctypes.data, C.byref(out)) == INVALID and not out.value
    bare = Polygonizer(device=0)           # owns no grid
    assert bare._lib.vx_stamp_capture(bare._h, box.ctypes.data, C.byref(out)) == INVALID
    # upload
    assert lib.vx_stamp_upload(None, size.ctypes.data, d.ctypes.data, None, None, C.byref(out)) == INVALID
    assert lib.vx_stamp_upload(h, size.ctypes.data, d.ctypes.data, None, None, None) == INVALID
    assert lib.vx_stamp_upload(h, size.ctypes.data, None, None, None, C.byref(out)) == INVALID
    assert lib.vx_stamp_upload(h, None, d.ctypes.data, None, None, C.byref(out)) == INVALID
    for bad in ((0, 4, 5), (3, 4, 0), (2049, 1, 1), (2048, 2048, 257)):
        assert lib.vx_stamp_upload(h, np.array(bad, np.uint32).ctypes.data, d.ctypes.data, None, None, C.byref(out)) == INVALID and not out.value
    # read, info
    assert lib.vx_stamp_info_get(h, mine._s, None) == INVALID and lib.vx_stamp_info_get(h, None, info.ctypes.data) == INVALID
    assert lib.vx_stamp_info_get(h, theirs._s, info.ctypes.data) == INVALID and lib.vx_stamp_info_get(None, mine._s, info.ctypes.data) == INVALID
    assert lib.vx_stamp_read(h, theirs._s, None, None, None) == INVALID and lib.vx_stamp_read(h, None, None, None, None) == INVALID
    lib.vx_stamp_free(h, None)
    lib.vx_stamp_free(h, theirs._s)        # not this context's: ignored
    assert int(theirs.info()["voxels"]) == 60
    # paste
    good = sto.pastes([((1, 2, 3), 0, 0, R)])
    arr = lambda *s: (C.c_void_p * len(s))(*s)
    results = np.zeros(4, binding.PASTE_RESULT_DTYPE)
    counts = np.zeros(1, binding.PASTE_COUNTS_DTYPE)

    def paste(ctx, stamps, n_stamps, ps, count):
        return lib.vx_grid_paste(ctx, stamps, n_stamps, None if ps is None else ps.ctypes.data, count, results.ctypes.data, counts.ctypes.data)
    assert paste(None, arr(mine._s), 1, good, 1) == INVALID
    assert paste(h, arr(mine._s), 1, None, 1) == INVALID and paste(h, None, 1, good, 1) == INVALID
    assert paste(h, arr(mine._s), 1, good, binding.PASTE_MAX_COUNT + 1) == INVALID
    assert paste(h, arr(*([mine._s] * (binding.PASTE_MAX_STAMPS + 1))), binding.PASTE_MAX_STAMPS + 1, good, 1) == INVALID
    assert paste(h, arr(mine._s), 0, good, 1) == INVALID                      # stamp >= n_stamps
    assert paste(h, arr(None, mine._s), 2, good, 1) == INVALID                # refers to a null entry
    assert paste(h, arr(theirs._s), 1, good, 1) == INVALID                    # a stamp of another context
    assert paste(bare._h, arr(mine._s), 1, good, 1) == INVALID                # no grid (and not its stamp)
    for field, value in (("orient", 8), ("mode", 4), ("reserved", (1, 0)), ("reserved", (0, 7)), ("stamp", 1)):
        bad = np.concatenate([good, good])
        bad[1][field] = value
        assert paste(h, arr(mine._s), 1, bad, 2) == INVALID, field
    same_grid(p, g)
    # legal: no pastes; an unreferenced null entry
    assert paste(h, None, 0, None, 0) == 0 and paste(h, arr(mine._s), 1, None, 0) == 0
    assert counts.tobytes() == bytes(48)
    same_grid(p, g)
    second = sto.pastes([((1, 2, 3), 1, 0, R)])
    assert paste(h, arr(None, mine._s), 2, second, 1) == 0
    sto.paste(g, [None, src], second)
    same_grid(p, g)
