"""The ABI of vx_geometry_keep_counts (include/voxels_hip.h) and of the knob VX_KEEP_GEOMETRY: the header declares the entry point
and documents the knob, INTEGRATION.md lists it, the HIP library exports it and the binding binds it; the host code sits behind
the slot plan's backend macro, so the CPU emulation - the same file without the backend macros: no plan, no layout, no kept
geometry - is without it, and the binding says so instead of calling into nothing."""
import os
import re

import pytest

from emu_lib import ROOT, emu_library
from voxels_amd import binding


def test_the_header_declares_the_entry_point_and_documents_the_knob():
    text = open(os.path.join(ROOT, "include", "voxels_hip.h")).read()
    assert "int vx_geometry_keep_counts(vx_ctx* ctx, uint64_t out[2]);" in text
    assert re.search(r"VX_KEEP_GEOMETRY=0 \(read at context creation\)", text)
    at = text.index("int vx_geometry_keep_counts(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "vx_layout_keep_counts" in comment and "material table" in comment and "HIP builds only" in comment
    assert "texture bytes" in comment and "Transition vertices" in comment
    # what a kept run does with the pools, and that they are the library's to write
    comment = text[text.index("/* Device-resident hand-off"):text.index("int vx_device_meshes(")]
    assert "leaves the index pool's bytes alone" in comment and "read-only for the caller" in comment
    assert "only the texture bytes" in comment and "vx_geometry_keep_counts" in comment


def test_the_knob_table_lists_it():
    knobs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in knobs.splitlines() if l.startswith("| `VX_KEEP_GEOMETRY` |")]
    assert len(rows) == 1, rows
    assert "tests/test_gpu_geometry_keep.py" in rows[0] and "vx_geometry_keep_counts" in rows[0] and "profiles/geometry_keep_ab_bench.txt" in rows[0]


def test_the_library_exports_it_and_the_binding_binds_it():
    lib = binding.HipLibrary()
    assert lib.has_geometry_keep and hasattr(lib.lib, "vx_geometry_keep_counts")
    assert len(lib.lib.vx_geometry_keep_counts.argtypes) == 2
    assert hasattr(binding.Polygonizer, "geometry_keep_counts")


def test_the_knob_is_read_at_context_creation_and_the_host_code_sits_behind_the_backend_macro():
    hip = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_hip.hip")).read()
    assert 'env_u32("VX_KEEP_GEOMETRY", 1)' in hip
    host = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_host.inl")).read()
    at = host.index("int vx_geometry_keep_counts(")
    guard = host.rindex("#if", 0, at)
    assert host[guard:].startswith("#if defined(VX_BACKEND_SLOT_PLAN)")
    assert "#endif" not in host[guard:at], "the entry point is outside the slot plan's guard"
    for name in os.listdir(os.path.join(ROOT, "tests", "emu")):
        if name.endswith((".cpp", ".inl", ".h")):
            assert "vx_geometry_keep_counts" not in open(os.path.join(ROOT, "tests", "emu", name)).read(), name


def test_the_plan_field_needs_no_kernel_argument_and_no_instantiation():
    """MainPlan::geometry is a field of its own, read through the kernarg mirror: k_main keeps its four parameters and its four
    instantiations, MainPlan::layout its values and main_indices_kept its text."""
    main = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_main.inl")).read()
    assert "void k_main(ExecParamsDev pArg, MainPlan plan, u32* clockStart, LayoutEnd endArg)" in main
    assert "main_kernargs().plan.layout) == 2u" in main
    assert "bool main_geometry_kept() { return r0_uniform(main_kernargs().plan.geometry) != 0u; }" in main
    hip = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_hip.hip")).read()
    code = "\n".join(l.split("//")[0] for l in (main + hip).splitlines())
    assert set(re.findall(r"k_main<([^>]*)>", code)) == {"false, false, true", "true", "false, true", "false"}
    # the branch stands in the two trip loops, around the call of the vertex body
    for name, body in (("vx_fast0.inl", "f0_vertex_tex("), ("vx_fast1.inl", "f1_vertex_tex(")):
        text = open(os.path.join(ROOT, "voxels_amd", "csrc", name)).read()
        assert text.count("main_geometry_kept()") == 1 and body in text, name
    fastt = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_fastt.inl")).read()
    assert "main_geometry_kept" not in fastt  # (transition vertices are written whole)


def test_one_definition_of_the_texture_bytes():
    core = open(os.path.join(ROOT, "voxels_amd", "csrc", "tv_core.h")).read()
    assert core.count("__builtin_amdgcn_perm(hi, lo, 0x01040C0Cu)") == 1 and core.count("pack_tex_dwords(") >= 3
    for name in ("tv_fast0.h", "tv_fast1.h"):
        assert "pack_tex_dwords(" in open(os.path.join(ROOT, "voxels_amd", "csrc", name)).read(), name


def test_the_emulation_is_without_it_and_the_binding_says_so():
    emu = emu_library()
    assert not emu.has_geometry_keep and not hasattr(emu.lib, "vx_geometry_keep_counts")
    p = binding.Polygonizer(library=emu)
    try:
        with pytest.raises(binding.VoxelsHipError, match="vx_geometry_keep_counts"):
            p.geometry_keep_counts()
    finally:
        p.close()
