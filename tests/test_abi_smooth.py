"""The ABI of vx_grid_smooth (include/voxels_hip.h, "smoothing"): the export and the sizes of its two records."""
import os
import re

import smooth_oracle as so
from voxels_amd import binding


def test_the_library_exports_vx_grid_smooth():
    lib = binding.HipLibrary()
    assert lib.has_smooth and hasattr(lib.lib, "vx_grid_smooth")
    assert hasattr(binding.Polygonizer, "smooth")


def test_record_sizes():
    # as the C compiler lays out the header's structs (tests/smooth/smooth_host.cpp includes include/voxels_hip.h)
    assert [so.load().sh_sizes(k) for k in range(2)] == [48, 32]
    assert binding.SMOOTH_DTYPE.itemsize == 48 and binding.SMOOTH_RESULT_DTYPE.itemsize == 32
    assert binding.SMOOTH_DTYPE.fields["hi"][1] == 12 and binding.SMOOTH_DTYPE.fields["center"][1] == 24
    assert binding.SMOOTH_DTYPE.fields["radius"][1] == 36 and binding.SMOOTH_DTYPE.fields["iterations"][1] == 44
    assert binding.SMOOTH_RESULT_DTYPE.fields["out_max"][1] == 12 and binding.SMOOTH_RESULT_DTYPE.fields["changed_voxels"][1] == 24


def test_the_header_states_the_limits_and_the_prototype():
    text = open(os.path.join(so.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_SMOOTH_MAX_ITERATIONS 64u", text) and re.search(r"#define VX_SMOOTH_MAX_COUNT \(1u << 16\)", text)
    assert binding.SMOOTH_MAX_ITERATIONS == 64 and binding.SMOOTH_MAX_COUNT == 1 << 16
    assert "int vx_grid_smooth(vx_ctx* ctx, const vx_smooth* ops, uint32_t count, vx_smooth_result* results /* may be NULL */," in text
    assert "float union_min[3], float union_max[3] /* may be NULL */, uint64_t* changed_voxels /* may be NULL */);" in text
