"""The ABI of the undo records (include/voxels_hip.h, "undo records"): the exports, the layout of the structs as the C compiler
sees them, the limits and the prototypes in the header, and the entry check of vx_grid_capture in the host pipeline."""
import os
import re

import numpy as np

import undo_oracle as uo
from voxels_amd import binding

EXPORTS = ("vx_grid_capture", "vx_record_trim", "vx_record_swap", "vx_record_info_get", "vx_record_block_ids", "vx_record_read_block",
           "vx_record_free", "vx_brush_box")


def layout(which):
    out = np.zeros(8, np.uint32)
    k = uo.load().uh_layout(which, out.ctypes.data)
    return out[:k].tolist()


def test_the_library_exports_the_undo_records():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_undo and all(hasattr(lib.lib, name) for name in EXPORTS)
    assert all(hasattr(binding.Record, m) for m in ("trim", "swap", "info", "block_ids", "read_block", "free"))
    assert hasattr(binding.Polygonizer, "capture")
    for name in ("BOX_DTYPE", "RECORD_INFO_DTYPE", "SWAP_RESULT_DTYPE", "Record", "brush_boxes"):
        assert getattr(voxels_amd, name) is getattr(binding, name) and name in voxels_amd.__all__


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/undo/undo_host.cpp includes include/voxels_hip.h)
    assert layout(0) == [24, 48, 48, 64, 12]
    assert binding.BOX_DTYPE.itemsize == 24 and binding.RECORD_INFO_DTYPE.itemsize == 48 and binding.SWAP_RESULT_DTYPE.itemsize == 48
    assert binding.BRUSH_DTYPE.itemsize == 64 and binding.BOX_DTYPE.fields["hi"][1] == 12
    names = ("n", "blocks", "bytes", "min", "max", "swaps", "reserved")
    assert layout(1) == [binding.RECORD_INFO_DTYPE.fields[k][1] for k in names] == [0, 4, 8, 16, 28, 40, 44]
    names = ("out_min", "out_max", "changed_voxels", "changed_blocks", "flag_changes", "reserved")
    assert layout(2) == [binding.SWAP_RESULT_DTYPE.fields[k][1] for k in names] == [0, 12, 24, 32, 36, 40]


def test_the_header_states_the_limits_and_the_prototypes():
    text = open(os.path.join(uo.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_RECORD_MAX_BLOCKS \(1u << 18\)", text) and re.search(r"#define VX_RECORD_MAX_BOXES  \(1u << 16\)", text)
    assert binding.RECORD_MAX_BLOCKS == 1 << 18 == uo.load().uh_limit(0) and binding.RECORD_MAX_BOXES == 1 << 16 == uo.load().uh_limit(1)
    for proto in ("int  vx_grid_capture(vx_ctx* ctx, const vx_box* boxes /* host */, uint32_t count, vx_record** out);",
                  "int  vx_record_trim(vx_ctx* ctx, vx_record* record, uint32_t* dropped /* may be NULL */);",
                  "int  vx_record_swap(vx_ctx* ctx, vx_record* record, vx_swap_result* result /* may be NULL */);",
                  "int  vx_record_info_get(vx_ctx* ctx, const vx_record* record, vx_record_info* info);",
                  "int  vx_record_block_ids(vx_ctx* ctx, const vx_record* record, uint32_t* ids, uint32_t capacity);",
                  "int  vx_record_read_block(vx_ctx* ctx, const vx_record* record, uint32_t index, int8_t* dist, uint8_t* mat, uint8_t* blend,",
                  "void vx_record_free(vx_ctx* ctx, vx_record* record);",
                  "int  vx_brush_box(const vx_brush* brush, uint32_t n, vx_box* out);"):
        assert proto in text, proto
    assert "12 293 bytes of device memory per held block" in text


def test_the_entry_check_refuses_bad_box_arrays():
    check = uo.load().uh_check
    good = uo.boxes([((0, 0, 0), (48, 48, 48))])
    assert check(48, good.ctypes.data, 1) == 0 == uo.check(48, good)
    many = np.repeat(good, binding.RECORD_MAX_BOXES + 1)
    assert check(48, many.ctypes.data, many.size) == -1 == uo.check(48, many)
    assert check(48, many.ctypes.data, binding.RECORD_MAX_BOXES) == 0
    assert check(48, None, 1) == -1 and check(48, None, 0) == 0
    for lo, hi in (((0, 0, 0), (49, 48, 48)), ((0, 0, 0), (48, 48, 64)), ((4, 4, 4), (4, 8, 8)), ((4, 9, 4), (8, 8, 8)), ((0, 0, 48), (1, 1, 49))):
        bad = uo.boxes([((0, 0, 0), (16, 16, 16)), (lo, hi)])
        assert check(48, bad.ctypes.data, 2) == -1 == uo.check(48, bad), (lo, hi)
    g = uo.noise_grid(48, 2)
    before = g.copy()
    assert uo.host_capture(g, many)[0] == -1 and uo.host_capture(g, [((0, 0, 0), (48, 48, 64))])[0] == -1 and g.same_as(before)
