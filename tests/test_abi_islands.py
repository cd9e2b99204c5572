"""The ABI of vx_grid_islands (include/voxels_hip.h, "detached solid pieces"): the export and the sizes of its three records."""
import ctypes as C
import re

import island_oracle as io
from voxels_amd import binding


def test_the_library_exports_vx_grid_islands():
    lib = binding.HipLibrary()
    assert lib.has_islands and hasattr(lib.lib, "vx_grid_islands")
    assert hasattr(binding.Polygonizer, "islands")


def test_record_sizes():
    # as the C compiler lays out the header's structs (tests/island/island_host.cpp includes include/voxels_hip.h)
    assert [io.load().ih_sizes(k) for k in range(3)] == [48, 40, 48]
    assert binding.ISLAND_QUERY_DTYPE.itemsize == 48 and binding.ISLAND_DTYPE.itemsize == 40 and binding.ISLAND_COUNTS_DTYPE.itemsize == 48
    assert binding.ISLAND_DTYPE.fields["voxels"][1] == 8 and binding.ISLAND_DTYPE.fields["min"][1] == 16
    assert binding.ISLAND_QUERY_DTYPE.fields["max_voxels"][1] == 40 and binding.ISLAND_COUNTS_DTYPE.fields["components"][1] == 24


def test_the_header_states_the_flags_and_sizes():
    import os
    text = open(os.path.join(io.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_ISLANDS_DETACHED_ONLY 1u", text) and re.search(r"#define VX_ISLANDS_REMOVE\s+2u", text)
    assert binding.ISLANDS_DETACHED_ONLY == 1 and binding.ISLANDS_REMOVE == 2
    assert "int vx_grid_islands(vx_ctx* ctx, const vx_island_query* query, vx_island* islands, uint32_t capacity," in text
    assert C.sizeof(C.c_uint64) == 8
