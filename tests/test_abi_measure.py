"""The ABI of the measurements (include/voxels_hip.h, "measurements"): the exports, the layout of the structs as the C compiler
sees them, the limit and the prototypes in the header, and the entry checks in the host pipeline."""
import os
import re

import numpy as np

import measure_oracle as mo
import undo_oracle as uo
from voxels_amd import binding

EXPORTS = ("vx_grid_measure", "vx_record_measure", "vx_debug_measure_chunk", "vx_debug_measure_shortcuts")


def layout(which):
    out = np.zeros(8, np.uint32)
    k = mo.load().mh_layout(which, out.ctypes.data)
    return out[:k].tolist()


def test_the_library_exports_the_measurements():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_measure and all(hasattr(lib.lib, name) for name in EXPORTS)
    assert hasattr(binding.Polygonizer, "measure") and hasattr(binding.Record, "measure")
    for name in ("MEASURE_DTYPE", "RECORD_DELTA_DTYPE", "MEASURE_MAX_BOXES"):
        assert getattr(voxels_amd, name) is getattr(binding, name) and name in voxels_amd.__all__


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/measure/measure_host.cpp includes include/voxels_hip.h)
    assert layout(0) == [48, 64, 24]
    assert [d.itemsize for d in (binding.MEASURE_DTYPE, binding.RECORD_DELTA_DTYPE, binding.BOX_DTYPE)] == [48, 64, 24]
    names = ("voxels", "solid_voxels", "min", "max", "materials", "reserved")
    assert layout(1) == [binding.MEASURE_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 28, 40, 44]
    names = ("removed_voxels", "added_voxels", "repainted_voxels", "min", "max", "blocks", "reserved")
    assert layout(2) == [binding.RECORD_DELTA_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 36, 48, 52]


def test_the_header_states_the_limit_and_the_prototypes():
    text = open(os.path.join(mo.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_MEASURE_MAX_BOXES \(1u << 16\)", text)
    assert mo.load().mh_limit(0) == binding.MEASURE_MAX_BOXES == 1 << 16
    for proto in ("int  vx_grid_measure(vx_ctx* ctx, const vx_box* boxes /* host */, uint32_t count, vx_measure* results /* host, count entries */,",
                  "                     uint64_t* tallies /* host, count * 256, may be NULL */);",
                  "int  vx_record_measure(vx_ctx* ctx, const vx_record* record, vx_record_delta* delta,",
                  "                       uint64_t* removed /* host, 256, may be NULL */, uint64_t* added /* host, 256, may be NULL */);",
                  "int  vx_debug_measure_chunk(vx_ctx* ctx, uint32_t pairs);"):
        assert proto in text, proto
    for phrase in ("2160 bytes per box", "chunks of at most 2^22", "exchange their roles", "zero is air"):
        assert phrase in text, phrase


def test_the_entry_checks_refuse_bad_arguments():
    g = mo.grids()[1][1]          # 48^3
    lib = mo.load()
    good = mo.boxes([((0, 0, 0), (48, 48, 48)), ((47, 47, 47), (48, 48, 48))])
    res = np.zeros(good.size, binding.MEASURE_DTYPE)
    assert lib.mh_check(48, good.ctypes.data, good.size, res.ctypes.data) == 0 == mo.check(48, good)
    assert lib.mh_check(48, None, 0, None) == 0                              # count = 0 is fine
    assert lib.mh_check(48, None, 1, res.ctypes.data) == -1                  # a null box array with count > 0
    assert lib.mh_check(48, good.ctypes.data, good.size, None) == -1         # null results
    many = np.repeat(good[:1], binding.MEASURE_MAX_BOXES + 1)
    big = np.zeros(many.size, binding.MEASURE_DTYPE)
    assert lib.mh_check(48, many.ctypes.data, many.size, big.ctypes.data) == -1 == mo.check(48, many)
    assert lib.mh_check(48, many.ctypes.data, many.size - 1, big.ctypes.data) == 0 == mo.check(48, many[:-1])
    for lo, hi in (((0, 0, 0), (49, 48, 48)), ((4, 4, 4), (4, 8, 8)), ((4, 9, 4), (8, 8, 8)), ((0, 0, 48), (1, 1, 49)), ((5, 5, 5), (6, 6, 5))):
        bad = mo.boxes([good[0], (lo, hi)])
        assert lib.mh_check(48, bad.ctypes.data, 2, res.ctypes.data) == -1 == mo.check(48, bad), (lo, hi)
        for path in (0, 1):
            assert mo.host_measure(path, g, bad)[0] == -1
    # the record call: a null delta, a null record, a record from a grid of another edge
    rec = uo.capture(g, [((0, 0, 0), (16, 16, 16))])
    assert mo.host_record(1, g, rec)[0] == 0
    assert mo.host_record(1, g, rec, null_delta=True)[0] == -1
    assert mo.host_record(1, g, rec, has_record=0)[0] == -1
    assert mo.host_record(1, g, rec, rec_n=64)[0] == -1
