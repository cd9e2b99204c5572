"""The ABI of vx_grid_walk_field (include/voxels_hip.h, "walk fields"): the export, the layout of its three records as the C
compiler sees them, and the limits and the prototype the header states."""
import os
import re

import walk_oracle as wo
from voxels_amd import binding


def test_the_library_exports_vx_grid_walk_field():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_walk_field and hasattr(lib.lib, "vx_grid_walk_field")
    assert hasattr(binding.Polygonizer, "walk_field")
    for name in ("WALK_QUERY_DTYPE", "WALK_GOAL_DTYPE", "WALK_COUNTS_DTYPE", "WALK_UNREACHED", "WALK_MAX_GOALS", "walk_query"):
        assert hasattr(voxels_amd, name), name


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/walk/walk_host.cpp includes include/voxels_hip.h)
    lib = wo.load()
    assert [lib.wh_sizes(k) for k in range(3)] == [64, 16, 32]
    for which, dt in enumerate((binding.WALK_QUERY_DTYPE, binding.WALK_GOAL_DTYPE, binding.WALK_COUNTS_DTYPE)):
        assert dt.itemsize == lib.wh_sizes(which)
        assert [lib.wh_offset(which, k) for k in range(len(dt.names))] == [dt.fields[name][1] for name in dt.names], dt
        assert lib.wh_offset(which, len(dt.names)) == 0xFFFFFFFF
    assert binding.WALK_QUERY_DTYPE.names == ("lo", "hi", "whole_grid", "clearance", "step_up", "step_down", "cost_axial", "cost_diagonal",
                                              "cost_climb", "max_cost", "flags", "reserved")
    assert binding.WALK_COUNTS_DTYPE.names == ("standable", "reached", "goals_used", "goals_ignored", "max_distance", "sweeps")


def test_the_header_states_the_limits_and_the_prototype():
    text = open(os.path.join(wo.ROOT, "include", "voxels_hip.h")).read()
    assert re.search(r"#define VX_WALK_UNREACHED 0xFFFFFFFFu", text) and re.search(r"#define VX_WALK_MAX_GOALS 65536u", text)
    assert binding.WALK_UNREACHED == 0xFFFFFFFF and binding.WALK_MAX_GOALS == 65536
    assert "int vx_grid_walk_field(vx_ctx* ctx, const vx_walk_query* query, const vx_walk_goal* goals /* host */, uint32_t goal_count," in text
    section = text[text.index("---- walk fields"):text.index("#define VX_WALK_UNREACHED")]
    for limit in ("clearance 1..32", "step_up, step_down 0..4", "cost_axial 1..65535", "cost_diagonal 0..65535", "cost_climb 0..65535",
                  "max_cost 0..2^30", "<= 2^28", "no sum wraps a uint32", "NOT part of the deterministic result"):
        assert limit in section, limit
    # the limits as the entry points enforce them: the largest legal values pass, one more does not
    flat = wo.floor(32, 8)
    top = dict(clearance=32, step_up=4, step_down=4, cost_axial=65535, cost_diagonal=65535, cost_climb=65535, max_cost=1 << 30)
    for kind in ("oracle", "emulate"):
        assert wo.run(kind, flat, goals=[(5, 7, 8)], **dict(top, clearance=24)).rc == 0
        for name, value in top.items():
            assert wo.run(kind, flat, goals=[(5, 7, 8)], **{name: value}).rc == 0, name
            assert wo.run(kind, flat, goals=[(5, 7, 8)], **{name: value + 1}).rc == -1, name
