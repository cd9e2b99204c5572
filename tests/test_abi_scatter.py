"""The ABI of vx_scatter (include/voxels_hip.h, "scattering"): the two exports and the sizes of its four records."""
import os
import re

import scatter_oracle as so
import voxels_amd
from voxels_amd import binding


def test_the_library_exports_vx_scatter():
    lib = binding.HipLibrary()
    assert lib.has_scatter and hasattr(lib.lib, "vx_scatter") and hasattr(lib.lib, "vx_scatter_device")
    assert hasattr(binding.Polygonizer, "scatter") and hasattr(binding.Polygonizer, "scatter_device")
    for name in ("SCATTER_PARAMS_DTYPE", "SCATTER_POINT_DTYPE", "SCATTER_RANGE_DTYPE", "SCATTER_COUNTS_DTYPE", "scatter_params"):
        assert name in voxels_amd.__all__ and getattr(voxels_amd, name) is getattr(binding, name)


def test_record_sizes():
    # as the C compiler lays out the header's structs (tests/scatter/scatter_host.cpp includes include/voxels_hip.h)
    assert [so.load().sc_sizes(k) for k in range(6)] == [80, 48, 8, 32, 48, 156]
    P, Q, R, K = binding.SCATTER_PARAMS_DTYPE, binding.SCATTER_POINT_DTYPE, binding.SCATTER_RANGE_DTYPE, binding.SCATTER_COUNTS_DTYPE
    assert [P.itemsize, Q.itemsize, R.itemsize, K.itemsize] == [80, 48, 8, 32]
    assert binding.VERTEX_DTYPE.itemsize == 48 and binding.LISTED_BLOCK_DTYPE.itemsize == 156
    assert [P.fields[k][1] for k in P.names] == [0, 4, 8, 12, 16, 28, 40, 44, 76]
    assert [Q.fields[k][1] for k in Q.names] == [0, 12, 16, 28, 32, 36, 40]
    assert [K.fields[k][1] for k in K.names] == [0, 8, 16, 20, 24, 28]


def test_the_default_parameters_filter_nothing():
    p = binding.scatter_params()[0]
    assert p["min_up"] == -1 and p["max_up"] == 1 and all(p["box_min"] == -float("inf")) and all(p["box_max"] == float("inf"))
    assert all(p["texture_mask"] == 0xFFFFFFFF) and p["reserved"] == 0 and p["density"] == 1
    q = binding.scatter_params(texture_slot=5, texture_values=[3, 40, 255])[0]
    assert q["texture_mask"].tolist() == [8, 256, 0, 0, 0, 0, 0, 1 << 31] and q["texture_slot"] == 5


def test_the_header_states_the_limits_and_the_prototypes():
    text = open(os.path.join(so.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_SCATTER_MAX_DENSITY 64\.0f", text) and re.search(r"#define VX_SCATTER_MAX_PER_TRIANGLE 65535u", text)
    assert binding.SCATTER_MAX_DENSITY == 64.0 and binding.SCATTER_MAX_PER_TRIANGLE == 65535
    assert "int vx_scatter_device(vx_ctx*, uint32_t level, const vx_scatter_params* params /* host */, uint32_t capacity," in text
    assert "int vx_scatter(vx_ctx*, uint32_t level, const vx_scatter_params* params, uint32_t capacity," in text
    assert "a floor has nrm.y > 0" in text  # the direction of the normals is part of the specification
