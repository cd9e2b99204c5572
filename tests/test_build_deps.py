"""voxels_amd/build.py rebuilds a native piece when a file it is made from is newer: the files come from the sources' quoted
#include lines, not from lists kept by hand.  Checked here against a scan of the test's own."""
import os
import re
import time

import pytest

from voxels_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxels_amd", "csrc")
TARGETS = sorted(list(build.HIP_TARGETS) + list(build.GXX_TARGETS) + list(build.EXE_TARGETS))


def closure(sources):
    """The test's own scan: breadth first, by line, over real paths."""
    todo, seen = [os.path.realpath(s) for s in sources], set()
    while todo:
        path = todo.pop(0)
        if path in seen:
            continue
        seen.add(path)
        with open(path, errors="replace") as f:
            for line in f:
                m = re.match(r'\s*#\s*include\s+"([^"]+)"', line)
                if m:
                    todo.append(os.path.realpath(os.path.join(os.path.dirname(path), m.group(1))))
    return seen


def test_every_target_is_known():
    # every public build_<name> but the oracle's (a Makefile) and the drop-in tests (two programs) is a target of that name
    names = {n[len("build_"):] for n in dir(build) if n.startswith("build_")}
    assert names - {"oracle", "dropin_tests"} == set(TARGETS) - {"dropin_ours", "mirror_ours"}
    assert len(TARGETS) == 20


@pytest.mark.parametrize("name", TARGETS)
def test_deps_are_the_include_closure(name):
    sources = build.target_sources(name)
    assert sources and all(os.path.isfile(s) for s in sources)
    deps = build.target_deps(name)
    assert len(deps) == len(set(deps))
    built = {os.path.realpath(d) for d in deps if d.endswith(".so")}  # link-time dependencies: libraries this module builds
    assert built <= {os.path.realpath(os.path.join(CSRC, f)) for f in ("libvoxels_hip.so", "libVoxels.so")}
    assert {os.path.realpath(d) for d in deps} - built == closure(sources)


def test_link_time_dependencies_stay():
    assert os.path.join(CSRC, "libvoxels_hip.so") in build.target_deps("cpp_api")
    for name in ("dropin_ours", "mirror_ours", "dropin_bench"):
        assert os.path.join(CSRC, "libVoxels.so") in build.target_deps(name)


def test_hip_closure_holds_what_the_hand_lists_missed():
    for name in ("hip", "hip_casedump", "hip_conservative"):
        deps = set(build.target_deps(name))
        assert os.path.join(CSRC, "vx_terrain_math.h") in deps
        assert os.path.join(ROOT, "include", "voxels_hip.h") in deps
        inl = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.startswith("vx_") and f.endswith(".inl")]
        assert len(inl) >= 18 and set(inl) <= deps
    for name in ("emu", "trfast_host"):
        deps = set(build.target_deps(name))
        assert os.path.join(CSRC, "vx_terrain_math.h") in deps and os.path.join(ROOT, "include", "voxels_hip.h") in deps


def test_missing_include_raises(tmp_path):
    src = tmp_path / "a.cpp"
    src.write_text('#include <vector>\n#include "b.h"\n')
    (tmp_path / "b.h").write_text('  #  include "sub/c.h"\n// #include "commented_out.h"\n')
    with pytest.raises(FileNotFoundError, match="c.h"):
        build.include_closure(str(src))
    (tmp_path / "sub").mkdir()
    (tmp_path / "sub" / "c.h").write_text('#include "../b.h"\n')  # (a cycle ends)
    assert build.include_closure(str(src)) == [str(src), str(tmp_path / "b.h"), str(tmp_path / "sub" / "c.h")]


def test_touched_header_makes_target_stale(tmp_path):
    src, hdr, out = tmp_path / "a.cpp", tmp_path / "a.h", tmp_path / "liba.so"
    hdr.write_text("int f();\n")
    src.write_text('#include "a.h"\nint f() { return 1; }\n')
    out.write_text("")
    now = time.time()
    os.utime(str(src), (now - 30, now - 30))
    os.utime(str(hdr), (now - 30, now - 30))
    os.utime(str(out), (now - 20, now - 20))
    assert not build._newer(str(out), build.deps([str(src)]))
    os.utime(str(hdr), (now - 10, now - 10))
    assert build._newer(str(out), build.deps([str(src)]))
    assert not build._newer(str(out), [str(src)])  # (the source alone would not have shown it)
