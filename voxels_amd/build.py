"""Build helpers: compile the HIP library for gfx950 in-tree (the .so travels with the repo snapshot)."""
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")

HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-ldl"]


def _newer(target, sources):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources)


def include_closure(path, found=None):
    """`path` and every file it reaches through quoted #include lines, each resolved relative to the including file.
    A quoted include that names no file is an error: a dependency nobody watches means a stale library under test."""
    found = [] if found is None else found
    path = os.path.normpath(path)
    if path in found:
        return found
    found.append(path)
    with open(path, errors="replace") as f:
        names = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read(), re.M)
    for name in names:
        inc = os.path.join(os.path.dirname(path), name)
        if not os.path.isfile(inc):
            raise FileNotFoundError('%s: #include "%s" names no file' % (path, name))
        include_closure(inc, found)
    return found


def deps(sources):
    """What a target built from `sources` has to be rebuilt for: the sources and everything they include."""
    found = []
    for src in sources:
        include_closure(src, found)
    return found


def _path(rel):
    return os.path.join(ROOT, *rel.split("/"))


# The g++ targets: name -> (output, .cpp files, extra compiler flags, extra link arguments, built libraries linked against).
# What each one is for stands at its build_<name> function below.
GXX_TARGETS = {
    "synth": ("voxels_amd/csrc/libvoxels_synth.so", ["voxels_amd/csrc/vx_synth.cpp"], ["-fopenmp", "-ffp-contract=off"], [], []),
    "cpp_api": ("voxels_amd/csrc/libVoxels.so", ["voxels_amd/csrc/vx_api_cpp.cpp", "voxels_amd/csrc/vx_grid_host.cpp"], ["-fvisibility=hidden"],
                ["-L" + CSRC, "-lvoxels_hip", "-Wl,-rpath,$ORIGIN"], ["voxels_amd/csrc/libvoxels_hip.so"]),
    "emu": ("tests/emu/libvoxels_emu.so", ["tests/emu/emu.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-subobject-linkage"], [], []),
    "shape_host": ("tests/shape/libvoxels_shape_host.so", ["tests/shape/shape_host.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas"], [], []),
    "brush_host": ("tests/brush/libvoxels_brush_host.so", ["tests/brush/brush_host.cpp", "voxels_amd/csrc/vx_grid_host.cpp"], ["-ffp-contract=off"], [], []),
    "island_host": ("tests/island/libvoxels_island_host.so", ["tests/island/island_host.cpp"], [], [], []),
    "walk_host": ("tests/walk/libvoxels_walk_host.so", ["tests/walk/walk_host.cpp"], [], [], []),
    "undo_host": ("tests/undo/libvoxels_undo_host.so", ["tests/undo/undo_host.cpp"], ["-ffp-contract=off"], [], []),
    "stamp_host": ("tests/stamp/libvoxels_stamp_host.so", ["tests/stamp/stamp_host.cpp"], ["-ffp-contract=off"], [], []),
    "measure_host": ("tests/measure/libvoxels_measure_host.so", ["tests/measure/measure_host.cpp", "tests/height/height_host.cpp", "tests/occlusion/occlusion_host.cpp", "tests/geomkeep/geomkeep_host.cpp"],
                     ["-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-subobject-linkage"], [], []),
    "smooth_host": ("tests/smooth/libvoxels_smooth_host.so", ["tests/smooth/smooth_host.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas"], [], []),
    "scatter_host": ("tests/scatter/libvoxels_scatter_host.so", ["tests/scatter/scatter_host.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas"], [], []),
    "overlap_host": ("tests/overlap/libvoxels_overlap_host.so", ["tests/overlap/overlap_host.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas"], [], []),
    "trfast_host": ("tests/trfast/libvoxels_trfast_host.so", ["tests/trfast/trfast_host.cpp"], ["-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-subobject-linkage"], [], []),
}
# The hipcc builds of vx_hip.hip: name -> (output, extra defines)
HIP_TARGETS = {
    "hip": ("voxels_amd/csrc/libvoxels_hip.so", []),
    "hip_casedump": ("voxels_amd/csrc/libvoxels_hip_casedump.so", ["-DVX_CASE_DUMP"]),
    "hip_conservative": ("voxels_amd/csrc/libvoxels_hip_conservative.so", ["-DVX_CONSERVATIVE_SYNC"]),
}
# The test and benchmark programs that link libVoxels.so: name -> (output, source)
EXE_TARGETS = {
    "dropin_ours": ("tests/cpp/dropin_ours", "tests/cpp/dropin_test.cpp"),
    "mirror_ours": ("tests/cpp/mirror_ours", "tests/cpp/mirror_test.cpp"),
    "dropin_bench": ("tools/dropin_bench", "tools/dropin_bench.cpp"),
}


def target_sources(name):
    """The source files target `name` is compiled from."""
    if name in HIP_TARGETS:
        return [os.path.join(CSRC, "vx_hip.hip")]
    if name in EXE_TARGETS:
        return [_path(EXE_TARGETS[name][1])]
    return [_path(f) for f in GXX_TARGETS[name][1]]


def target_deps(name):
    """Every file a change of which rebuilds target `name`: its sources, what they include, and the built libraries it links."""
    libs = GXX_TARGETS[name][4] if name in GXX_TARGETS else ["voxels_amd/csrc/libVoxels.so"] if name in EXE_TARGETS else []
    return deps(target_sources(name)) + [_path(f) for f in libs]


def _build_shared(name, force):
    """g++ shared library of GXX_TARGETS[name]."""
    out, _, flags, link, _ = GXX_TARGETS[name]
    out, srcs = _path(out), target_sources(name)
    if force or _newer(out, target_deps(name)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-fPIC", "-shared"] + flags + ["-o", out] + srcs + link, cwd=os.path.dirname(srcs[0]))
    return out


def _build_exe(name, force):
    """g++ program of EXE_TARGETS[name] against include/ and libVoxels.so."""
    out, src = _path(EXE_TARGETS[name][0]), target_sources(name)[0]
    if force or _newer(out, target_deps(name)):
        subprocess.check_call(["g++", "-std=c++14", "-O2", "-o", out, src, "-I" + os.path.join(ROOT, "include"),
                               "-L" + CSRC, "-lVoxels", "-Wl,-rpath," + CSRC])
    return out


def _build_vx_hip(name, force, extra=(), verbose=False):
    """hipcc build of vx_hip.hip with the defines of HIP_TARGETS[name] (and `extra` flags) -> (output, the finished compiler run;
    None where the library was up to date)."""
    out, defines = HIP_TARGETS[name]
    out = _path(out)
    if not force and not _newer(out, target_deps(name)):
        return out, None
    cmd = [_hipcc()] + HIP_FLAGS + defines + list(extra) + ["-o", out, os.path.join(CSRC, "vx_hip.hip")]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed:\n" + "\n".join(l for l in r.stderr.splitlines() if "remark:" not in l)[-4000:])
    return out, r


def _hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def build_hip(force=False, verbose=True):
    """hipcc --offload-arch=gfx950 ... -o voxels_amd/csrc/libvoxels_hip.so (cross-compiles without a GPU)."""
    out, r = _build_vx_hip("hip", force, ["-Rpass-analysis=kernel-resource-usage"], verbose)
    if r is None:
        return out
    table = kernel_resources(r.stderr)
    # Policy: no kernel of the library spills or keeps arrays in scratch memory (a spilled variant of k_regular produced
    # wrong vertices now and then).  VX_ALLOW_SCRATCH=1 lifts the check for experiments.
    bad = [(k, v["ScratchSize"]) for k, v in table.items() if v.get("ScratchSize", 0)]
    # the gate must not pass because the remark format changed and nothing was parsed
    missing = [k for k in ("k_regular0", "k_regular", "k_transition", "k_classify", "k_material", "k_main", "k_tail", "k_run_head", "k_cell_map", "k_dirty_head", "k_dirty_tail",
                           "k_spherecast", "k_closest_point", "k_brush_apply",
                           "k_isl_local", "k_isl_merge", "k_isl_flatten", "k_isl_scan", "k_isl_roots", "k_isl_stats", "k_isl_mark", "k_isl_compact", "k_isl_remove",
                           "k_smooth_eval", "k_smooth_commit", "k_smooth_results",
                           "k_walk_stand", "k_walk_seed", "k_walk_relax", "k_walk_finish",
                           "k_scatter_count", "k_scatter_scan", "k_scatter_write",
                           "k_overlap_count", "k_overlap_scan", "k_overlap_write",
                           "k_rec_mark", "k_rec_scan", "k_rec_list", "k_rec_capture", "k_rec_diff", "k_rec_pack", "k_rec_swap",
                           "k_stamp_capture", "k_paste_count", "k_paste_fill", "k_paste_apply",
                           "k_measure_pairs", "k_measure_finish", "k_rec_measure",
                           "k_height_tiles",
                           "k_occlusion_bake", "k_occlusion_counts")
               if not any(k in name and "ScratchSize" in v for name, v in table.items())]
    if missing:
        os.remove(out)
        raise RuntimeError("kernel resource remarks not found for %s: the no-scratch policy cannot be checked (hipcc remark format changed?)" % missing)
    with open(os.path.join(CSRC, "kernel_resources.txt"), "w") as f:
        f.write("%-72s %6s %8s %10s %10s\n" % ("kernel", "VGPRs", "scratch", "occupancy", "staticLDS"))
        for k, v in sorted(table.items()):
            f.write("%-72s %6d %8d %10d %10d\n" % (k[:72], v.get("VGPRs", 0), v.get("ScratchSize", 0), v.get("Occupancy", 0), v.get("LDS Size", 0)))
    if bad and not os.environ.get("VX_ALLOW_SCRATCH"):
        # A frame can be reserved without ever being touched (spill slots of scalar registers that were all turned into
        # vector-register lanes afterwards): what the policy forbids is scratch TRAFFIC, so a flagged kernel passes if its
        # code holds no instruction that can reach the private segment.  One device-only compile to assembly serves all
        # flagged kernels.
        touching = _kernels_touching_scratch(_hipcc(), [k for k, _ in bad])
        bad = [(k, n) for k, n in bad if k in touching]
    if bad and not os.environ.get("VX_ALLOW_SCRATCH"):
        os.remove(out)
        raise RuntimeError("kernels using scratch memory: %s" % bad)
    return out


def _kernels_touching_scratch(hipcc, kernels):
    """Which of `kernels` (mangled names) hold an instruction that can reach the private segment: any scratch_* instruction,
    or any buffer_* access whose resource is the private-segment descriptor (s[0:3] under the default calling convention -
    also the constant-offset forms without `offen`).  A kernel whose code cannot be found counts as touching."""
    import tempfile
    touching = set(kernels)
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "vx.s")
        flags = [f for f in HIP_FLAGS if f not in ("-shared", "-fPIC", "-ldl")]
        r = subprocess.run([hipcc] + flags + ["-S", "--cuda-device-only", "-o", asm, os.path.join(CSRC, "vx_hip.hip")], cwd=CSRC, capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(asm):
            return touching
        current, dirty, seen = None, False, set()
        with open(asm) as f:
            for line in f:
                m = re.match(r"^(\S+):", line)
                if m and m.group(1) in touching | seen:
                    current, dirty = m.group(1), False
                    seen.add(current)
                    continue
                if current is None:
                    continue
                if line.startswith(".Lfunc_end"):
                    if not dirty:
                        touching.discard(current)
                    current = None
                    continue
                code = line.split(";")[0]
                if "scratch_" in code or (re.search(r"\bbuffer_(load|store|atomic)", code) and re.search(r"s\[0:3\]", code)):
                    dirty = True
    return touching


def kernel_resources(remarks):
    """-Rpass-analysis=kernel-resource-usage remarks -> {kernel: {VGPRs, SGPRs, ScratchSize, Occupancy, LDS Size}}"""
    table, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = table.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+(VGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return table


def build_hip_casedump(force=False):
    """Test build of the HIP library that also records the case codes it looks up (tests/test_case_codes.py)."""
    return _build_vx_hip("hip_casedump", force)[0]


def build_hip_conservative(force=False):
    """Test build of the HIP library whose in-kernel dependency flags use release / acquire fences instead of write-through
    stores and loads (-DVX_CONSERVATIVE_SYNC, vx_hip.hip): tests/test_gpu_parity.py compares it with the product library."""
    return _build_vx_hip("hip_conservative", force)[0]


def build_synth(force=False):
    """Host-side synthetic input generator (include/voxels_synth.h)."""
    return _build_shared("synth", force)


def build_cpp_api(force=False):
    """libVoxels.so: the reference's public C++ API (include/Voxels.h) on top of libvoxels_hip.so."""
    return _build_shared("cpp_api", force)


def build_dropin_tests(force=False):
    """tests/cpp/dropin_test.cpp compiled against OUR headers + libVoxels.so, and (where /root/reference exists)
    the very same source against the REFERENCE headers + the unmodified reference library (oracle/_ref)."""
    src = target_sources("dropin_ours")[0]
    out = _build_exe("dropin_ours", force)
    _build_exe("mirror_ours", force)
    ref_out = os.path.join(ROOT, "oracle", "_ref", "dropin_ref")
    ref_lib = os.path.join(ROOT, "oracle", "_ref", "libvoxels_ref.so")
    if os.path.isdir("/root/reference/include") and os.path.exists(ref_lib) and (force or _newer(ref_out, [src, ref_lib])):
        subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++14", "-O2", "-w", "-fms-extensions", "-fdeclspec",
                               "-DVOXELS_API=", "-DVOXELS_CDECL=", "-o", ref_out, src, "-I/root/reference/include",
                               "-L" + os.path.dirname(ref_lib), "-lvoxels_ref", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib/llvm/lib"])
    return out, ref_out


def build_dropin_bench(force=False):
    """tools/dropin_bench.cpp: end-to-end Polygonizer::Execute through libVoxels.so (used by bench.py's e2e figure)."""
    return _build_exe("dropin_bench", force)


def build_emu(force=False):
    """CPU emulation of the device phases — tests only (tests/emu)."""
    return _build_shared("emu", force)


def build_shape_host(force=False):
    """The sphere-triangle arithmetic of the sphere casts (csrc/tv_shape.h) compiled for the host, the same float32 operations
    as the kernels (-ffp-contract=off) — tests only (tests/test_shapecast.py)."""
    return _build_shared("shape_host", force)


def build_brush_host(force=False):
    """Host oracle of vx_grid_inject_brushes: the host grid class (csrc/vx_grid_host.cpp) applying a brush array one call at a
    time, with the sample functions of csrc/tv_brush.h, the same float32 operations as the kernels (-ffp-contract=off) — tests
    only (tests/test_brushes.py, tests/test_gpu_brushes.py)."""
    return _build_shared("brush_host", force)


def build_island_host(force=False):
    """Host side of the tests of vx_grid_islands: a flood-fill oracle that shares nothing with the device path, and the tile
    pipeline of csrc/tv_island.h run sequentially (the algorithm of the kernels, testable without a GPU) — tests only
    (tests/test_islands.py, tests/test_gpu_islands.py)."""
    return _build_shared("island_host", force)


def build_walk_host(force=False):
    """Host side of the tests of vx_grid_walk_field: a Dijkstra oracle that shares nothing with the device path, and the tile
    pipeline of csrc/tv_walk.h run sequentially, sweep loop included (the algorithm of the kernels, testable without a GPU) -
    tests only (tests/test_walk.py, tests/test_gpu_walk.py, tests/test_abi_walk.py)."""
    return _build_shared("walk_host", force)


def build_undo_host(force=False):
    """Host side of the tests of the undo records: the kernels' pipeline of csrc/tv_undo.h run sequentially (mark, scan, list,
    capture, diff, pack, swap), the entry checks and the layout of the header's structs - tests only (tests/test_undo.py,
    tests/test_abi_undo.py)."""
    return _build_shared("undo_host", force)


def build_stamp_host(force=False):
    """Host side of the tests of the stamps: csrc/tv_stamp.h in a plain sequential loop, and the kernels' pipeline (bin, sort,
    per-block apply from a tile, flags, reduction) run on the CPU with the list capacity as a parameter, the entry checks and the
    layout of the header's structs - tests only (tests/test_stamp.py, tests/test_abi_stamp.py)."""
    return _build_shared("stamp_host", force)


def build_measure_host(force=False):
    """Host side of the tests of the measurements: csrc/tv_measure.h in a plain triple loop, and the kernels' pipeline (rows, block
    partials, merges into box results, finish) run on the CPU with the chunk size as a parameter, the entry checks and the layout of
    the header's structs - tests only (tests/test_measure.py, tests/test_abi_measure.py).  The same library holds the host side of
    the tests of the height maps, which walk the same rows (tests/height/height_host.cpp): csrc/tv_height.h in a plain loop over
    columns, and the kernel's tile pipeline (row masks, column bits, the carry, the early exit, sign summaries given or withheld)
    run on the CPU, the entry checks and the layout of the header's structs (tests/test_height.py, tests/test_abi_height.py).  And
    the host side of the tests of vx_occlusion, whose staging reads the same 16-byte rows and sign summaries
    (tests/occlusion/occlusion_host.cpp): the rule of csrc/tv_occlusion.h in a plain loop over vertices and the dense grid, and the
    kernel's pipeline - staged row masks of a block's neighbourhood, then the probes, with the region's reach as a parameter so that
    the reads from the grid itself are reached - the entry checks and the layout of the header's structs (tests/test_occlusion.py,
    tests/test_abi_occlusion.py).  And the comparison of the texture-only vertex forms with the full ones
    (tests/geomkeep/geomkeep_host.cpp): the CPU emulation of tests/emu, whose every full run walks its table-driven regular blocks
    once more with the serial forms and compares, vertex by vertex, the 8 bytes of f0_vertex_tex / f1_vertex_tex with bytes 40..47
    of the full form (tests/test_geometry_keep_host.py)."""
    return _build_shared("measure_host", force)


def build_smooth_host(force=False):
    """Host side of the tests of vx_grid_smooth: the arithmetic of csrc/tv_smooth.h in a plain loop over a dense array, and the
    tile pipeline of the kernels run sequentially, the same float32 operations as the kernels (-ffp-contract=off) - tests only
    (tests/test_smooth.py, tests/test_abi_smooth.py)."""
    return _build_shared("smooth_host", force)


def build_scatter_host(force=False):
    """Host side of the tests of vx_scatter: the arithmetic of csrc/tv_scatter.h in a plain loop over a level's table and meshes, the
    same float32 operations as the kernels (-ffp-contract=off) - tests only (tests/test_scatter.py, tests/test_abi_scatter.py)."""
    return _build_shared("scatter_host", force)


def build_overlap_host(force=False):
    """Host side of the tests of the overlap queries: a level's ray-cast index built on the host by the rule of k_ray_index
    (csrc/tv_ray.h) and the count, scan and write passes run sequentially with the functions of csrc/tv_overlap.h, with a seed that
    shuffles every bucket's slice of the permutation - tests only (tests/test_overlap.py, tests/test_abi_overlap.py)."""
    return _build_shared("overlap_host", force)


def build_trfast_host(force=False):
    """Host side of the tests of the table-driven transition body (csrc/tv_fastt.h): the CPU emulation of tests/emu with a
    transition pass that runs either body, and the exhaustive check of the derived case rows - tests only
    (tests/test_trfast_tables.py)."""
    return _build_shared("trfast_host", force)


def build_oracle(with_reference=True):
    """The CPU checkers (test infrastructure): the port always, the unmodified reference when /root/reference exists."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "port"])
    if with_reference and os.path.isdir("/root/reference/src"):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "ref"])
