"""The ABI of the height maps (include/voxels_hip.h, "height maps"): the exports, the layout of the structs as the C compiler
sees them, the constants and the prototypes in the header, and the entry checks in the host pipeline."""
import os
import re

import numpy as np

import height_oracle as ho
from voxels_amd import binding

EXPORTS = ("vx_grid_heightmap", "vx_grid_heightmap_device", "vx_debug_height_shortcuts")


def layout(which):
    out = np.zeros(8, np.uint32)
    k = ho.load().hh_layout(which, out.ctypes.data)
    return out[:k].tolist()


def test_the_library_exports_the_height_maps():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_height and all(hasattr(lib.lib, name) for name in EXPORTS)
    assert hasattr(binding.Polygonizer, "heightmap") and hasattr(binding.Polygonizer, "heightmap_device")
    for name in ("HEIGHT_QUERY_DTYPE", "HEIGHT_COUNTS_DTYPE", "HEIGHT_MAX_LAYERS", "HEIGHT_NONE", "HEIGHT_FROM_TOP", "HEIGHT_FROM_BOTTOM", "HEIGHT_COUNT_SURFACES"):
        assert getattr(voxels_amd, name) is getattr(binding, name) and name in voxels_amd.__all__


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/height/height_host.cpp includes include/voxels_hip.h)
    assert layout(0) == [48, 48, 24]
    assert [d.itemsize for d in (binding.HEIGHT_QUERY_DTYPE, binding.HEIGHT_COUNTS_DTYPE, binding.BOX_DTYPE)] == [48, 48, 24]
    names = ("box", "direction", "layers", "flags", "reserved")
    assert layout(1) == [binding.HEIGHT_QUERY_DTYPE.fields[k][1] for k in names] == [0, 24, 28, 32, 36]
    names = ("columns", "covered", "surfaces", "min_height", "max_height", "clipped", "max_surfaces", "reserved")
    assert layout(2) == [binding.HEIGHT_COUNTS_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 28, 32, 36, 40]


def test_the_header_states_the_constants_and_the_prototypes():
    text = open(os.path.join(ho.ROOT, "include", "voxels_hip.h")).read()
    lib = ho.load()
    for k, (name, value) in enumerate((("VX_HEIGHT_MAX_LAYERS", "8u"), ("VX_HEIGHT_NONE", "0xFFFFFFFFu"), ("VX_HEIGHT_FROM_TOP", "0u"),
                                       ("VX_HEIGHT_FROM_BOTTOM", "1u"), ("VX_HEIGHT_COUNT_SURFACES", "1u"))):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
        assert lib.hh_limit(k) == int(value[:-1], 0) == getattr(binding, name[3:])
    for proto in ("int  vx_grid_heightmap(vx_ctx* ctx, const vx_height_query* query, uint32_t* heights /* host, layers * H * W */,",
                  "int  vx_grid_heightmap_device(vx_ctx* ctx, const vx_height_query* query, uint32_t* d_heights /* device */,",
                  "int  vx_debug_height_shortcuts(vx_ctx* ctx, uint32_t enable);"):
        assert proto in text, proto
    for phrase in ("f = (256 * -d0) / (d1 - d0)", "h = z * 256 + f", "h = z * 256 - f", "can be the same number", "counts as air", "layer-major, then y, then x"):
        assert phrase in text, phrase


def test_a_null_context_is_invalid():
    lib = binding.HipLibrary().lib
    q = ho.height_query(((0, 0, 0), (8, 8, 8)))
    heights = np.full(64, 0xA5A5A5A5, np.uint32)
    for fn in (lib.vx_grid_heightmap, lib.vx_grid_heightmap_device):
        assert fn(None, q.ctypes.data, heights.ctypes.data, None, None, None) == -1
    assert lib.vx_debug_height_shortcuts(None, 1) == -1
    assert (heights == 0xA5A5A5A5).all()


def test_the_entry_checks_refuse_bad_arguments():
    g = ho.grids()[1][1]          # 48^3
    lib = ho.load()
    good = ho.height_query(((0, 0, 0), (48, 48, 48)), "bottom", 8, True)
    assert lib.hh_check(48, good.ctypes.data, 1, 1) == 0 == ho.check(48, good, True, True)
    assert lib.hh_check(48, good.ctypes.data, 1, 0) == 0 == ho.check(48, good, True, False)
    assert lib.hh_check(48, None, 1, 0) == -1 == ho.check(48, None)                       # a null query
    assert lib.hh_check(48, good.ctypes.data, 0, 0) == -1 == ho.check(48, good, False)    # null heights

    def bad(change, surfaces=False):
        q = good.copy()
        change(q)
        assert lib.hh_check(48, q.ctypes.data, 1, int(surfaces)) == -1 == ho.check(48, q, True, surfaces), q
        for path in (0, 1):
            rc, h, m, s, c, _ = ho.host_heightmap(path, g, None, count_surfaces=surfaces, query=q)
            assert rc == -1 and (h == 0xA5A5A5A5).all() and (m == 0xA5).all()             # nothing written

    for lo, hi in (((0, 0, 0), (49, 48, 48)), ((4, 4, 4), (4, 8, 8)), ((4, 9, 4), (8, 8, 8)), ((0, 0, 48), (1, 1, 49)), ((5, 5, 5), (6, 6, 5))):
        def box(q, lo=lo, hi=hi):
            q["box"]["lo"], q["box"]["hi"] = lo, hi
        bad(box)
    bad(lambda q: q.__setitem__("direction", 2))
    bad(lambda q: q.__setitem__("layers", 0))
    bad(lambda q: q.__setitem__("layers", 9))
    bad(lambda q: q.__setitem__("flags", 3))
    bad(lambda q: q.__setitem__("flags", 2))
    for k in range(3):
        def word(q, k=k):
            q["reserved"][0, k] = 1
        bad(word)
    bad(lambda q: q.__setitem__("flags", 0), surfaces=True)                               # a surfaces array without the flag
