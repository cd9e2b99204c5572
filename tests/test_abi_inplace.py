"""The ABI of vx_material_inplace_counts (include/voxels_hip.h) and of the knob VX_MAT_INPLACE: the header declares the entry
point and documents the knob, INTEGRATION.md lists it, the HIP library exports it and the binding binds it; the CPU emulation -
which keeps neither material store nor slot plan: its host code is the same file without the backend macros - is without it, and
the binding says so instead of calling into nothing."""
import os
import re

import pytest

from emu_lib import ROOT, emu_library
from voxels_amd import binding


def test_the_header_declares_the_entry_point_and_documents_the_knob():
    text = open(os.path.join(ROOT, "include", "voxels_hip.h")).read()
    assert "int vx_material_inplace_counts(vx_ctx* ctx, uint64_t out[2]);" in text
    assert re.search(r"VX_MAT_INPLACE=0 \(read at context creation\)", text)
    # next to vx_material_path_counts: the knob is part of that comment, and "replayed" covers both ways into the slot
    at = text.index("int vx_material_path_counts(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "VX_MAT_INPLACE=0" in comment and "copied from the store" in comment and "left in the slot" in comment


def test_the_knob_table_lists_it():
    knobs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in knobs.splitlines() if l.startswith("| `VX_MAT_INPLACE` |")]
    assert len(rows) == 1, rows
    assert "tests/test_gpu_inplace.py" in rows[0] and "vx_material_inplace_counts" in rows[0]


def test_the_library_exports_it_and_the_binding_binds_it():
    lib = binding.HipLibrary()
    assert lib.has_material_inplace and hasattr(lib.lib, "vx_material_inplace_counts")
    assert len(lib.lib.vx_material_inplace_counts.argtypes) == 2
    assert hasattr(binding.Polygonizer, "material_inplace_counts")


def test_the_knob_is_read_at_context_creation_with_the_others():
    hip = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_hip.hip")).read()
    assert 'env_u32("VX_MAT_INPLACE", 1)' in hip
    host = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_host.inl")).read()
    at = host.index("int vx_material_inplace_counts(")
    guard = host.rindex("#if", 0, at)
    assert host[guard:].startswith("#if defined(VX_BACKEND_SLOT_PLAN)")


def test_the_emulation_is_without_it_and_the_binding_says_so():
    emu = emu_library()
    assert not emu.has_material_inplace and not hasattr(emu.lib, "vx_material_inplace_counts")
    p = binding.Polygonizer(library=emu)
    try:
        with pytest.raises(binding.VoxelsHipError, match="vx_material_inplace_counts"):
            p.material_inplace_counts()
    finally:
        p.close()
