"""The texture-only vertex forms against the full ones, on the CPU (tests/geomkeep/geomkeep_host.cpp): a full run
that keeps the mesh layout computes and stores only bytes 40..47 of a regular vertex (f0_vertex_tex, f1_vertex_tex), so those 8
bytes must be, byte for byte, what the full forms (f0_vertex, f1_vertex) put there - everything in them is integer arithmetic or
exact fp32.  The host library runs the CPU emulation and, behind the regular pass of every full run, walks every table-driven
regular block of every level with the serial forms and compares every vertex.

Fields: gentle64_nozero and gentle128_nozero (four levels: chains of three steps) of steady_fields.py and chunks64 of
index_keep_fields.py (a block of more than one descriptor chunk), each under the default table, the permuted table of
test_material_table_change_keeps_one_launch_and_the_indices and a table with some rows' valid byte cleared.  These fields stage no
exact zero, so no block may be left out: the vertices compared are the oracle's regular vertices of every level."""
import ctypes as C

import numpy as np
import pytest

import fields
import index_keep_fields as ikf
import steady_fields as sf
import test_gpu_cellmap as cellmap
import vxo
from voxels_amd import binding, build

FIGURES = 8
COMPARED, DIFFERENT, SAME_BRANCH, CELL_BRANCH, INVALID_ROW, DECLINED, WALKED, NOT_INTERIOR = range(FIGURES)
INVALID_IDS = (1, 5)  # two of the ids of matstore.mixed_materials {0, 1, 2, 5, 9}


def tables():
    default = vxo.default_lut()
    permuted = ((default.astype(np.uint32) * 7 + 3) % 249).astype(np.uint8)
    assert not np.array_equal(permuted, default)
    valid = np.ones(256, np.uint8)
    valid[list(INVALID_IDS)] = 0
    return {"default": (default, None), "permuted": (permuted, None), "invalid_rows": (default, valid)}


@pytest.fixture(scope="module")
def host():
    lib = binding.HipLibrary(build.build_measure_host())
    assert lib.backend.startswith("emu:") and "texture-only" in lib.backend
    lib.lib.gkh_levels.restype = C.c_uint32
    lib.lib.gkh_counts.argtypes = [C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def port():
    return vxo.load_port()


def field(name):
    return ikf.chunks64() if name == "chunks64" else sf.make(name)[:3]


def counts(host):
    out = np.zeros((int(host.lib.gkh_levels()), FIGURES), np.uint64)
    host.lib.gkh_counts(out.ctypes.data_as(C.c_void_p))
    return out.astype(np.int64)


@pytest.mark.parametrize("table", ["default", "permuted", "invalid_rows"])
@pytest.mark.parametrize("name", ["gentle64_nozero", "gentle128_nozero", "chunks64"])
def test_texture_only_forms_equal_bytes_40_to_47_of_the_full_forms(host, port, name, table):
    d, m, b = field(name)
    lut, valid = tables()[table]
    s = port.execute(port.grid_from_dense(d, m, b), lut=lut, valid=valid)
    want = s.all_levels()
    p = binding.Polygonizer(library=host)
    try:
        p.upload(d, m, b, cellmap.flags_of(d))
        p.set_materials(lut, valid)
        host.lib.gkh_reset()
        info = p.execute()
        got = counts(host)
        # (the run itself is the emulation's: the comparison changed nothing in it)
        ok, msg = fields.surface_equal(p.all_levels(), want, nrm_tol=0.0)
        assert ok, msg
    finally:
        p.close()
    levels = int(info.levels)
    assert levels == len(want) == sf.level_count(d.shape[0]) and not got[levels:].any()
    if name == "gentle128_nozero":
        assert levels == 4
    print("%s, %s: per level [compared, different, same-material branch, cell branch, invalid row, declined, walked, not interior]" % (name, table))
    for l in range(levels):
        print("  L%d %s (the oracle's regular vertices: %d)" % (l, got[l].tolist(), int(want[l].infos["n_verts"].sum())))
    for l in range(levels):
        n = int(want[l].infos["n_verts"].sum())
        assert got[l][DECLINED] == 0 and got[l][NOT_INTERIOR] == 0, "L%d: a block or a vertex was left out" % l
        assert got[l][COMPARED] == n, "L%d: %d vertices compared, the oracle has %d regular vertices" % (l, got[l][COMPARED], n)
        assert got[l][DIFFERENT] == 0, "L%d: %d of %d vertices differ in their texture bytes" % (l, got[l][DIFFERENT], n)
        assert got[l][SAME_BRANCH] + got[l][CELL_BRANCH] == n
        if n:
            assert got[l][SAME_BRANCH] > 0 and got[l][CELL_BRANCH] > 0, "L%d: one branch of the rv.mat rule was never taken" % l
            assert got[l][WALKED] == int((want[l].infos["n_verts"] > 0).sum())
    assert sum(int(want[l].infos["n_verts"].sum()) for l in range(levels)) > 0
    if name == "chunks64":
        assert int(want[0].infos["n_verts"].max()) > ikf.F0_VDESC
    if table == "invalid_rows":
        assert got[:, INVALID_ROW].sum() > 0, "no compared vertex used an invalid row"
        tex = np.concatenate([np.asarray(lv.verts["tex"]).reshape(-1, 8) for lv in want if len(lv.verts)])
        assert (tex == 0).all(axis=1).any() and tex[:, 1].any()  # (the oracle: blend forced to 0 there, kept elsewhere)
    else:
        assert got[:, INVALID_ROW].sum() == 0
