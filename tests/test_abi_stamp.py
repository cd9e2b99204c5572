"""The ABI of the stamps (include/voxels_hip.h, "stamps"): the exports, the layout of the structs as the C compiler sees them,
the limits and the prototypes in the header, and the entry checks in the host pipeline."""
import os
import re

import numpy as np

import stamp_oracle as sto
from voxels_amd import binding

EXPORTS = ("vx_stamp_capture", "vx_stamp_upload", "vx_stamp_read", "vx_stamp_info_get", "vx_stamp_free", "vx_grid_paste", "vx_paste_box")


def layout(which):
    out = np.zeros(8, np.uint32)
    k = sto.load().sh_layout(which, out.ctypes.data)
    return out[:k].tolist()


def test_the_library_exports_the_stamps():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_stamps and all(hasattr(lib.lib, name) for name in EXPORTS)
    assert all(hasattr(binding.Stamp, m) for m in ("read", "info", "free"))
    assert all(hasattr(binding.Polygonizer, m) for m in ("capture_stamp", "upload_stamp", "paste"))
    for name in ("STAMP_INFO_DTYPE", "PASTE_DTYPE", "PASTE_RESULT_DTYPE", "PASTE_COUNTS_DTYPE", "STAMP_MAX_EDGE", "STAMP_MAX_VOXELS", "PASTE_MAX_COUNT",
                 "PASTE_MAX_STAMPS", "PASTE_REPLACE", "PASTE_UNION", "PASTE_SUBTRACT", "PASTE_PAINT", "Stamp", "paste_boxes"):
        assert getattr(voxels_amd, name) is getattr(binding, name) and name in voxels_amd.__all__


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/stamp/stamp_host.cpp includes include/voxels_hip.h)
    assert layout(0) == [32, 32, 32, 48]
    assert [d.itemsize for d in (binding.STAMP_INFO_DTYPE, binding.PASTE_DTYPE, binding.PASTE_RESULT_DTYPE, binding.PASTE_COUNTS_DTYPE)] == [32, 32, 32, 48]
    assert layout(1) == [binding.STAMP_INFO_DTYPE.fields[k][1] for k in ("size", "reserved", "voxels", "bytes")] == [0, 12, 16, 24]
    assert layout(2) == [binding.PASTE_DTYPE.fields[k][1] for k in ("origin", "stamp", "orient", "mode", "reserved")] == [0, 12, 16, 20, 24]
    assert layout(3) == [binding.PASTE_RESULT_DTYPE.fields[k][1] for k in ("box", "touched_blocks", "reserved")] == [0, 24, 28]
    names = ("out_min", "out_max", "changed_voxels", "changed_blocks", "flag_changes", "touched_blocks", "reserved")
    assert layout(4) == [binding.PASTE_COUNTS_DTYPE.fields[k][1] for k in names] == [0, 12, 24, 32, 36, 40, 44]


def test_the_header_states_the_limits_and_the_prototypes():
    text = open(os.path.join(sto.ROOT, "include", "voxels_hip.h")).read()
    for pattern in (r"#define VX_STAMP_MAX_EDGE   2048u", r"#define VX_STAMP_MAX_VOXELS \(1u << 30\)", r"#define VX_PASTE_MAX_COUNT  \(1u << 20\)",
                    r"#define VX_PASTE_MAX_STAMPS \(1u << 16\)", r"#define VX_PASTE_REPLACE  0u", r"#define VX_PASTE_UNION    1u", r"#define VX_PASTE_SUBTRACT 2u",
                    r"#define VX_PASTE_PAINT    3u"):
        assert re.search(pattern, text), pattern
    limit = sto.load().sh_limit
    assert [limit(k) for k in range(8)] == [binding.STAMP_MAX_EDGE, binding.STAMP_MAX_VOXELS, binding.PASTE_MAX_COUNT, binding.PASTE_MAX_STAMPS,
                                            binding.PASTE_REPLACE, binding.PASTE_UNION, binding.PASTE_SUBTRACT, binding.PASTE_PAINT] == [2048, 1 << 30, 1 << 20, 1 << 16, 0, 1, 2, 3]
    for proto in ("int  vx_stamp_capture(vx_ctx* ctx, const vx_box* box /* host */, vx_stamp** out);",
                  "int  vx_stamp_upload(vx_ctx* ctx, const uint32_t size[3], const int8_t* dist, const uint8_t* mat /* may be NULL: zeros */,",
                  "int  vx_stamp_read(vx_ctx* ctx, const vx_stamp* stamp, int8_t* dist, uint8_t* mat, uint8_t* blend);",
                  "int  vx_stamp_info_get(vx_ctx* ctx, const vx_stamp* stamp, vx_stamp_info* info);",
                  "void vx_stamp_free(vx_ctx* ctx, vx_stamp* stamp);",
                  "int  vx_grid_paste(vx_ctx* ctx, vx_stamp* const* stamps, uint32_t n_stamps, const vx_paste* pastes /* host */, uint32_t count,",
                  "int  vx_paste_box(const vx_paste* paste, const uint32_t stamp_size[3], uint32_t n, vx_box* out);"):
        assert proto in text, proto
    assert "3 bytes per voxel of device memory" in text


def test_the_entry_checks_refuse_bad_arrays():
    good = sto.pastes([((1, 2, 3), 1, 7, 3)])
    sizes = [None, (3, 4, 5)]
    assert sto.host_check(good, sizes) == 0 == sto.check(good, sizes)
    assert sto.host_check(sto.pastes([]), []) == 0 and sto.load().sh_check(None, 1, None, 0) == -1
    for field, value in (("stamp", 2), ("stamp", 0), ("orient", 8), ("mode", 4), ("reserved", (0, 1)), ("reserved", (1, 0))):
        bad = np.concatenate([good, good])
        bad[1][field] = value
        assert sto.host_check(bad, sizes) == -1 == sto.check(bad, sizes), (field, value)
    many = np.repeat(good, binding.PASTE_MAX_COUNT + 1)
    assert sto.host_check(many, sizes) == -1 == sto.check(many, sizes) and sto.host_check(many[:-1], sizes) == 0
    assert sto.host_check(good, sizes + [None] * (binding.PASTE_MAX_STAMPS - 1)) == -1 and sto.host_check(good, sizes + [None] * (binding.PASTE_MAX_STAMPS - 2)) == 0
    size_check = lambda s: sto.load().sh_check_size(np.array(s, np.uint32).ctypes.data)
    assert size_check((1, 1, 1)) == 0 and size_check((2048, 2048, 256)) == 0 and size_check((1024, 1024, 1024)) == 0
    for s in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (2049, 1, 1), (1, 1, 2049), (2048, 2048, 257), (1025, 1024, 1024)):
        assert size_check(s) == -1, s
    box_check = lambda n, lo, hi: sto.load().sh_check_box(n, binding.boxes([(lo, hi)]).ctypes.data)
    assert box_check(48, (0, 0, 0), (48, 48, 48)) == 0 and box_check(48, (47, 47, 47), (48, 48, 48)) == 0 and sto.load().sh_check_box(48, None) == -1
    for lo, hi in (((0, 0, 0), (49, 48, 48)), ((4, 4, 4), (4, 8, 8)), ((4, 9, 4), (8, 8, 8)), ((0, 0, 48), (1, 1, 49))):
        assert box_check(48, lo, hi) == -1, (lo, hi)
    # a refused batch changes nothing
    g = sto.terrain_grid(48)
    before = g.copy()
    bad = sto.pastes([((1, 2, 3), 0, 0, 0), ((1, 2, 3), 0, 9, 0)])
    for path in (0, 1):
        assert sto.host_paste(path, g, [sto.noise_stamp((3, 4, 5), 1)], bad)[0] == -1 and g.same_as(before)
