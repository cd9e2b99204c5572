"""The ABI of the slot plan's one entry point (include/voxels_hip.h, vx_slot_plan_counts): the header declares it, the HIP
library exports it and the binding binds it; the CPU emulation - which keeps no plan: its host code is the same file without
VX_BACKEND_SLOT_PLAN - is without it, and the binding says so instead of calling into nothing."""
import os
import re

import pytest

from emu_lib import ROOT, emu_library
from voxels_amd import binding


def test_the_header_declares_the_entry_point_and_the_knob():
    text = open(os.path.join(ROOT, "include", "voxels_hip.h")).read()
    assert "int vx_slot_plan_counts(vx_ctx* ctx, uint64_t out[2]);" in text
    assert re.search(r"VX_PLAN=0 \(read at context creation\)", text)
    knobs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`VX_PLAN`" in knobs and "tests/test_gpu_slotplan.py" in knobs


def test_the_library_exports_it_and_the_binding_binds_it():
    lib = binding.HipLibrary()
    assert lib.has_slot_plan and hasattr(lib.lib, "vx_slot_plan_counts")
    assert len(lib.lib.vx_slot_plan_counts.argtypes) == 2
    assert hasattr(binding.Polygonizer, "slot_plan_counts")


def test_the_host_code_keeps_the_plan_behind_the_backend_macro():
    host = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_host.inl")).read()
    at = host.index("int vx_slot_plan_counts(")
    guard = host.rindex("#if", 0, at)
    assert host[guard:at].strip() == "#if defined(VX_BACKEND_SLOT_PLAN)"
    assert "#define VX_BACKEND_SLOT_PLAN 1" in open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_hip.hip")).read()
    for name in os.listdir(os.path.join(ROOT, "tests", "emu")):
        if name.endswith((".cpp", ".inl", ".h")):
            assert "VX_BACKEND_SLOT_PLAN" not in open(os.path.join(ROOT, "tests", "emu", name)).read(), name


def test_the_emulation_is_without_it_and_the_binding_says_so():
    emu = emu_library()
    assert not emu.has_slot_plan and not hasattr(emu.lib, "vx_slot_plan_counts")
    p = binding.Polygonizer(library=emu)
    try:
        with pytest.raises(binding.VoxelsHipError, match="vx_slot_plan_counts"):
            p.slot_plan_counts()
    finally:
        p.close()
