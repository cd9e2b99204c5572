"""The ABI of vx_layout_keep_counts (include/voxels_hip.h) and of the knob VX_LAYOUT: the header declares the entry point and
documents the knob, INTEGRATION.md lists it, the HIP library exports it and the binding binds it; the host code sits behind the
slot plan's backend macro, so the CPU emulation - the same file without the backend macros: no plan, no layout - is without
it, and the binding says so instead of calling into nothing."""
import os
import re

import pytest

from emu_lib import ROOT, emu_library
from voxels_amd import binding


def test_the_header_declares_the_entry_point_and_documents_the_knob():
    text = open(os.path.join(ROOT, "include", "voxels_hip.h")).read()
    assert "int vx_layout_keep_counts(vx_ctx* ctx, uint64_t out[2]);" in text
    assert re.search(r"VX_LAYOUT=0 \(read at context creation\)", text)
    at = text.index("int vx_layout_keep_counts(")
    comment = text[text.rindex("/*", 0, at):at]
    assert "VX_LAYOUT=0" in comment and "vx_compact_pools" in comment and "vx_material_lut" in comment and "HIP builds only" in comment


def test_the_knob_table_lists_it():
    knobs = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = [l for l in knobs.splitlines() if l.startswith("| `VX_LAYOUT` |")]
    assert len(rows) == 1, rows
    assert "tests/test_gpu_layout.py" in rows[0] and "vx_layout_keep_counts" in rows[0] and "profiles/layout_ab_bench.txt" in rows[0]


def test_the_library_exports_it_and_the_binding_binds_it():
    lib = binding.HipLibrary()
    assert lib.has_layout_keep and hasattr(lib.lib, "vx_layout_keep_counts")
    assert len(lib.lib.vx_layout_keep_counts.argtypes) == 2
    assert hasattr(binding.Polygonizer, "layout_keep_counts")


def test_the_knob_is_read_at_context_creation_and_the_host_code_sits_behind_the_backend_macro():
    hip = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_hip.hip")).read()
    assert 'env_u32("VX_LAYOUT", 1)' in hip
    host = open(os.path.join(ROOT, "voxels_amd", "csrc", "vx_host.inl")).read()
    at = host.index("int vx_layout_keep_counts(")
    guard = host.rindex("#if", 0, at)
    assert host[guard:].startswith("#if defined(VX_BACKEND_SLOT_PLAN)")
    assert "#endif" not in host[guard:at], "the entry point is outside the slot plan's guard"
    # ... and so does every use of the layout's state inside vx_polygonize: whatever names one of these identifiers in code (comments
    # stripped; any spelling of the statement) sits inside a conditional block that asks for the backend macro.  (The emulation's
    # build is the stronger check of the same thing: its Backend has neither set_layout_end nor layoutRan.)
    names = re.compile(r"\b(layoutValid|layoutLevels|layoutCursors|layoutTotals|layoutRuns|layoutOn|layoutRan|set_layout_end|STAT_LAYOUT_MISS|LAYOUT_MISS_OFF)\b")
    body = host[host.index("int vx_polygonize_from("):host.index("int vx_compact_pools(")]
    depth, seen = [], 0
    for line in body.splitlines():
        code = line.split("//")[0].strip()
        if code.startswith("#if"):
            depth.append("VX_BACKEND_SLOT_PLAN" in code)
        elif code.startswith("#endif"):
            depth.pop()
        elif names.search(code):
            seen += 1
            assert any(depth), "outside the backend macro: " + code
    assert not depth and seen >= 8, "the scan did not find the layout's code in vx_polygonize_from (%d lines)" % seen
    for name in os.listdir(os.path.join(ROOT, "tests", "emu")):
        if name.endswith((".cpp", ".inl", ".h")):
            assert "vx_layout_keep_counts" not in open(os.path.join(ROOT, "tests", "emu", name)).read(), name


def test_the_emulation_is_without_it_and_the_binding_says_so():
    emu = emu_library()
    assert not emu.has_layout_keep and not hasattr(emu.lib, "vx_layout_keep_counts")
    p = binding.Polygonizer(library=emu)
    try:
        with pytest.raises(binding.VoxelsHipError, match="vx_layout_keep_counts"):
            p.layout_keep_counts()
    finally:
        p.close()
