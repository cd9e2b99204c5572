"""ctypes binding of include/voxels_hip.h (libvoxels_hip.so)."""
import ctypes as C
import os
import sys

import numpy as np

LISTED_BLOCK_DTYPE = np.dtype([
    ("coord_id", "<u4"), ("v_off", "<u4"), ("v_count", "<u4"), ("i_off", "<u4"), ("i_count", "<u4"),
    ("tv_off", "<u4", 6), ("tv_count", "<u4", 6), ("ti_off", "<u4", 6), ("ti_count", "<u4", 6),
    ("degenerate", "<u4"), ("nt_cells", "<u4"), ("reserved", "<u4"), ("id", "<u4"),
    ("min_corner", "<f4", 3), ("max_corner", "<f4", 3)])
VERTEX_DTYPE = np.dtype([("pos", "<f4", 3), ("sec", "<f4", 4), ("nrm", "<f4", 3), ("tex", "u1", 8)])
BLOCK_INFO_DTYPE = np.dtype([
    ("id", "<u4"), ("n_verts", "<u4"), ("n_idx", "<u4"),
    ("n_tverts", "<u4", 6), ("n_tidx", "<u4", 6),
    ("min_corner", "<f4", 3), ("max_corner", "<f4", 3)])
assert VERTEX_DTYPE.itemsize == 48 and BLOCK_INFO_DTYPE.itemsize == 84
# vx_ray / vx_ray_hit (include/voxels_hip.h, ray casts)
RAY_DTYPE = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4")])
HIT_DTYPE = np.dtype([("t", "<f4"), ("pos", "<f4", 3), ("nrm", "<f4", 3), ("bary", "<f4", 2),
                      ("entry", "<u4"), ("block_id", "<u4"), ("tri", "<u4")])
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 48
RAY_NONE = 0xFFFFFFFF
# vx_sphere_cast / vx_sphere_hit / vx_point_query / vx_point_hit (include/voxels_hip.h, sphere casts and closest points)
SPHERE_CAST_DTYPE = np.dtype([("origin", "<f4", 3), ("t_min", "<f4"), ("dir", "<f4", 3), ("t_max", "<f4"), ("radius", "<f4"),
                              ("reserved", "<f4", 3)])
SPHERE_HIT_DTYPE = np.dtype([("t", "<f4"), ("center", "<f4", 3), ("contact", "<f4", 3), ("nrm", "<f4", 3), ("depth", "<f4"),
                             ("entry", "<u4"), ("block_id", "<u4"), ("tri", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
POINT_QUERY_DTYPE = np.dtype([("pos", "<f4", 3), ("max_dist", "<f4")])
POINT_HIT_DTYPE = np.dtype([("dist", "<f4"), ("point", "<f4", 3), ("nrm", "<f4", 3), ("bary", "<f4", 2),
                            ("entry", "<u4"), ("block_id", "<u4"), ("tri", "<u4")])
assert SPHERE_CAST_DTYPE.itemsize == 48 and SPHERE_HIT_DTYPE.itemsize == 64
# vx_brush / vx_brush_result (include/voxels_hip.h, "edits on the device")
BRUSH_BALL, BRUSH_CAPSULE, BRUSH_BOX, BRUSH_MATERIAL = 0, 1, 2, 3
BRUSH_DTYPE = np.dtype([("position", "<f4", 3), ("shape", "<u4"), ("extents", "<f4", 3), ("type", "<u4"),
                        ("a", "<f4", 3), ("radius", "<f4"), ("b", "<f4", 3), ("material", "<u4")])
BRUSH_RESULT_DTYPE = np.dtype([("out_min", "<f4", 3), ("out_max", "<f4", 3), ("touched_blocks", "<u4"), ("reserved", "<u4")])
assert BRUSH_DTYPE.itemsize == 64 and BRUSH_RESULT_DTYPE.itemsize == 32
# vx_island_query / vx_island / vx_island_counts (include/voxels_hip.h, "detached solid pieces")
ISLANDS_DETACHED_ONLY, ISLANDS_REMOVE = 1, 2
ISLAND_QUERY_DTYPE = np.dtype([("lo", "<u4", 3), ("hi", "<u4", 3), ("whole_grid", "<u4"), ("flags", "<u4"), ("anchor_faces", "<u4"),
                               ("air_value", "<i4"), ("max_voxels", "<u8")])
ISLAND_DTYPE = np.dtype([("label", "<u4"), ("faces", "<u4"), ("voxels", "<u8"), ("min", "<u4", 3), ("max", "<u4", 3)])
ISLAND_COUNTS_DTYPE = np.dtype([("solid_voxels", "<u8"), ("detached_voxels", "<u8"), ("removed_voxels", "<u8"), ("components", "<u4"),
                                ("detached", "<u4"), ("listed", "<u4"), ("removed", "<u4"), ("touched_blocks", "<u4"), ("reserved", "<u4")])
assert ISLAND_QUERY_DTYPE.itemsize == 48 and ISLAND_DTYPE.itemsize == 40 and ISLAND_COUNTS_DTYPE.itemsize == 48
# vx_smooth / vx_smooth_result (include/voxels_hip.h, "smoothing")
SMOOTH_MAX_ITERATIONS, SMOOTH_MAX_COUNT = 64, 1 << 16
SMOOTH_DTYPE = np.dtype([("lo", "<u4", 3), ("hi", "<u4", 3), ("center", "<f4", 3), ("radius", "<f4"), ("strength", "<f4"), ("iterations", "<u4")])
SMOOTH_RESULT_DTYPE = np.dtype([("out_min", "<f4", 3), ("out_max", "<f4", 3), ("changed_voxels", "<u8")])
assert SMOOTH_DTYPE.itemsize == 48 and SMOOTH_RESULT_DTYPE.itemsize == 32
assert POINT_QUERY_DTYPE.itemsize == 16 and POINT_HIT_DTYPE.itemsize == 48
# vx_walk_query / vx_walk_goal / vx_walk_counts (include/voxels_hip.h, "walk fields")
WALK_UNREACHED, WALK_MAX_GOALS = 0xFFFFFFFF, 65536
WALK_QUERY_DTYPE = np.dtype([("lo", "<u4", 3), ("hi", "<u4", 3), ("whole_grid", "<u4"), ("clearance", "<u4"), ("step_up", "<u4"),
                             ("step_down", "<u4"), ("cost_axial", "<u4"), ("cost_diagonal", "<u4"), ("cost_climb", "<u4"),
                             ("max_cost", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
WALK_GOAL_DTYPE = np.dtype([("x", "<u4"), ("y", "<u4"), ("z", "<u4"), ("cost", "<u4")])
WALK_COUNTS_DTYPE = np.dtype([("standable", "<u8"), ("reached", "<u8"), ("goals_used", "<u4"), ("goals_ignored", "<u4"),
                              ("max_distance", "<u4"), ("sweeps", "<u4")])
assert WALK_QUERY_DTYPE.itemsize == 64 and WALK_GOAL_DTYPE.itemsize == 16 and WALK_COUNTS_DTYPE.itemsize == 32

# undo records (include/voxels_hip.h, "undo records")
BOX_DTYPE = np.dtype([("lo", "<u4", 3), ("hi", "<u4", 3)])
RECORD_INFO_DTYPE = np.dtype([("n", "<u4"), ("blocks", "<u4"), ("bytes", "<u8"), ("min", "<u4", 3), ("max", "<u4", 3), ("swaps", "<u4"), ("reserved", "<u4")])
SWAP_RESULT_DTYPE = np.dtype([("out_min", "<f4", 3), ("out_max", "<f4", 3), ("changed_voxels", "<u8"), ("changed_blocks", "<u4"), ("flag_changes", "<u4"),
                              ("reserved", "<u8")])
assert BOX_DTYPE.itemsize == 24 and RECORD_INFO_DTYPE.itemsize == 48 and SWAP_RESULT_DTYPE.itemsize == 48
# stamps (include/voxels_hip.h, "stamps")
STAMP_INFO_DTYPE = np.dtype([("size", "<u4", 3), ("reserved", "<u4"), ("voxels", "<u8"), ("bytes", "<u8")])
PASTE_DTYPE = np.dtype([("origin", "<i4", 3), ("stamp", "<u4"), ("orient", "<u4"), ("mode", "<u4"), ("reserved", "<u4", 2)])
PASTE_RESULT_DTYPE = np.dtype([("box", BOX_DTYPE), ("touched_blocks", "<u4"), ("reserved", "<u4")])
PASTE_COUNTS_DTYPE = np.dtype([("out_min", "<f4", 3), ("out_max", "<f4", 3), ("changed_voxels", "<u8"), ("changed_blocks", "<u4"), ("flag_changes", "<u4"),
                               ("touched_blocks", "<u4"), ("reserved", "<u4")])
assert STAMP_INFO_DTYPE.itemsize == 32 and PASTE_DTYPE.itemsize == 32 and PASTE_RESULT_DTYPE.itemsize == 32 and PASTE_COUNTS_DTYPE.itemsize == 48
STAMP_MAX_EDGE, STAMP_MAX_VOXELS, PASTE_MAX_COUNT, PASTE_MAX_STAMPS = 2048, 1 << 30, 1 << 20, 1 << 16
PASTE_REPLACE, PASTE_UNION, PASTE_SUBTRACT, PASTE_PAINT = 0, 1, 2, 3
RECORD_MAX_BLOCKS = 1 << 18
RECORD_MAX_BOXES = 1 << 16
# measurements (include/voxels_hip.h, "measurements")
MEASURE_DTYPE = np.dtype([("voxels", "<u8"), ("solid_voxels", "<u8"), ("min", "<u4", 3), ("max", "<u4", 3), ("materials", "<u4"), ("reserved", "<u4")])
RECORD_DELTA_DTYPE = np.dtype([("removed_voxels", "<u8"), ("added_voxels", "<u8"), ("repainted_voxels", "<u8"), ("min", "<u4", 3), ("max", "<u4", 3),
                               ("blocks", "<u4"), ("reserved", "<u4", 3)])
assert MEASURE_DTYPE.itemsize == 48 and RECORD_DELTA_DTYPE.itemsize == 64
MEASURE_MAX_BOXES = 1 << 16
# height maps (include/voxels_hip.h, "height maps")
HEIGHT_QUERY_DTYPE = np.dtype([("box", BOX_DTYPE), ("direction", "<u4"), ("layers", "<u4"), ("flags", "<u4"), ("reserved", "<u4", 3)])
HEIGHT_COUNTS_DTYPE = np.dtype([("columns", "<u8"), ("covered", "<u8"), ("surfaces", "<u8"), ("min_height", "<u4"), ("max_height", "<u4"),
                                ("clipped", "<u4"), ("max_surfaces", "<u4"), ("reserved", "<u4", 2)])
assert HEIGHT_QUERY_DTYPE.itemsize == 48 and HEIGHT_COUNTS_DTYPE.itemsize == 48
HEIGHT_MAX_LAYERS, HEIGHT_NONE = 8, 0xFFFFFFFF
HEIGHT_FROM_TOP, HEIGHT_FROM_BOTTOM, HEIGHT_COUNT_SURFACES = 0, 1, 1
# ambient occlusion (include/voxels_hip.h, "ambient occlusion")
OCCLUSION_PARAMS_DTYPE = np.dtype([("steps", "<u4"), ("flags", "<u4"), ("box_min", "<f4", 3), ("box_max", "<f4", 3), ("reserved", "<u4", 4)])
OCCLUSION_COUNTS_DTYPE = np.dtype([("vertices", "<u8"), ("sum", "<u8"), ("entries", "<u4"), ("visited_entries", "<u4"), ("darkest", "<u4"), ("open", "<u4")])
assert OCCLUSION_PARAMS_DTYPE.itemsize == 48 and OCCLUSION_COUNTS_DTYPE.itemsize == 32
OCCLUSION_MAX_STEPS, OCCLUSION_TRANSITIONS = 12, 1
SPHERE_STARTED_IN_CONTACT = 1
# vx_lod_params / vx_lod_draw / vx_draw_indexed / vx_lod_counts (include/voxels_hip.h, LOD selection)
LOD_PARAMS_DTYPE = np.dtype([("camera", "<f4", 3), ("n_planes", "<u4"), ("planes", "<f4", (6, 4)), ("ranges", "<f4", 16)])
LOD_DRAW_DTYPE = np.dtype([("level", "<u4"), ("entry", "<u4"), ("block_id", "<u4"), ("coord_id", "<u4"), ("transitions", "<u4"),
                           ("adjacency", "<u4"), ("reserved", "<u4", 2)])
DRAW_INDEXED_DTYPE = np.dtype([("index_count", "<u4"), ("instance_count", "<u4"), ("first_index", "<u4"), ("vertex_offset", "<i4"),
                               ("first_instance", "<u4")])
LOD_COUNTS_DTYPE = np.dtype([("records", "<u4"), ("regular", "<u4"), ("transition", "<u4"), ("leaves", "<u4"),
                             ("meshed_leaves", "<u4"), ("culled_leaves", "<u4"), ("leaf_volume", "<u8")])
assert LOD_PARAMS_DTYPE.itemsize == 176 and LOD_DRAW_DTYPE.itemsize == 32
assert DRAW_INDEXED_DTYPE.itemsize == 20 and LOD_COUNTS_DTYPE.itemsize == 32


def lod_ranges(factor=4.0, levels=16):
    """ranges[L] = factor * 16 * 2^L: a level-L block is split while the camera is closer than `factor` of its edges"""
    r = np.zeros(16, np.float32)
    r[:levels] = [factor * 16.0 * (1 << L) for L in range(levels)]
    return r


def lod_params(camera, ranges=None, planes=None):
    """one LOD_PARAMS_DTYPE record (ranges: 16 floats, default lod_ranges(); planes: up to 6 (a, b, c, d) rows)"""
    prm = np.zeros(1, LOD_PARAMS_DTYPE)
    prm["camera"] = np.asarray(camera, np.float32).reshape(3)
    r = lod_ranges() if ranges is None else np.asarray(ranges, np.float32).reshape(-1)
    prm["ranges"][0, :len(r)] = r
    if planes is not None:
        pl = np.asarray(planes, np.float32).reshape(-1, 4)
        prm["n_planes"] = len(pl)
        prm["planes"][0, :min(len(pl), 6)] = pl[:6]
    return prm


# vx_scatter_* (include/voxels_hip.h, scattering)
SCATTER_PARAMS_DTYPE = np.dtype([("seed", "<u4"), ("density", "<f4"), ("min_up", "<f4"), ("max_up", "<f4"), ("box_min", "<f4", 3),
                                 ("box_max", "<f4", 3), ("texture_slot", "<u4"), ("texture_mask", "<u4", 8), ("reserved", "<u4")])
SCATTER_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("rand", "<f4"), ("nrm", "<f4", 3), ("entry", "<u4"), ("block_id", "<u4"),
                                ("tri", "<u4"), ("tex", "<u4", 2)])
SCATTER_RANGE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4")])
SCATTER_COUNTS_DTYPE = np.dtype([("points", "<u8"), ("candidates", "<u8"), ("triangles", "<u4"), ("entries", "<u4"),
                                 ("visited_entries", "<u4"), ("reserved", "<u4")])
assert SCATTER_PARAMS_DTYPE.itemsize == 80 and SCATTER_POINT_DTYPE.itemsize == 48
assert SCATTER_RANGE_DTYPE.itemsize == 8 and SCATTER_COUNTS_DTYPE.itemsize == 32
SCATTER_MAX_DENSITY = 64.0
SCATTER_MAX_PER_TRIANGLE = 65535


def scatter_params(seed=0, density=1.0, min_up=-1.0, max_up=1.0, box_min=None, box_max=None, texture_slot=0, texture_values=None):
    """one SCATTER_PARAMS_DTYPE record; the defaults mean "no filter": any slope, an infinite box, every texture value.
    texture_values: the values of vertex tex byte `texture_slot` (of a triangle's first vertex) that take part, None = all"""
    prm = np.zeros(1, SCATTER_PARAMS_DTYPE)
    prm["seed"], prm["density"], prm["min_up"], prm["max_up"] = seed, density, min_up, max_up
    prm["box_min"] = -np.inf if box_min is None else box_min
    prm["box_max"] = np.inf if box_max is None else box_max
    prm["texture_slot"] = texture_slot
    if texture_values is None:
        prm["texture_mask"] = 0xFFFFFFFF
    else:
        for v in texture_values:
            prm["texture_mask"][0, int(v) >> 5] |= np.uint32(1 << (int(v) & 31))
    return prm


# vx_overlap_* (include/voxels_hip.h, overlap queries)
OVERLAP_BOX_DTYPE = np.dtype([("lo", "<f4", 3), ("reserved0", "<u4"), ("hi", "<f4", 3), ("reserved1", "<u4")])
OVERLAP_TRI_DTYPE = np.dtype([("query", "<u4"), ("entry", "<u4"), ("block_id", "<u4"), ("tri", "<u4")])
OVERLAP_RANGE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4")])
OVERLAP_COUNTS_DTYPE = np.dtype([("triangles", "<u8"), ("pairs", "<u8"), ("queries", "<u4"), ("hit_queries", "<u4"),
                                 ("max_per_query", "<u4"), ("reserved", "<u4")])
assert OVERLAP_BOX_DTYPE.itemsize == 32 and OVERLAP_TRI_DTYPE.itemsize == 16
assert OVERLAP_RANGE_DTYPE.itemsize == 8 and OVERLAP_COUNTS_DTYPE.itemsize == 32
OVERLAP_MAX_QUERIES = 1 << 20


def overlap_boxes(lo, hi):
    """an OVERLAP_BOX_DTYPE array from corners lo, hi of shape [n, 3] (or [3]: one box): closed boxes, mesh space (Y-up, voxels)"""
    lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
    boxes = np.zeros(max(len(lo), len(hi)), OVERLAP_BOX_DTYPE)
    boxes["lo"], boxes["hi"] = lo, hi
    return boxes


class VoxelsHipError(RuntimeError):
    pass


class _HostMeshesStruct(C.Structure):
    _fields_ = [("verts", C.c_void_p), ("indices", C.c_void_p), ("n_verts", C.c_uint64), ("n_indices", C.c_uint64),
                ("arena", C.c_void_p)]


class HostMeshes:
    """Owner of one arena (include/voxels_hip.h vx_host_meshes): .verts / .indices are views into page-locked memory,
    valid until release() (or garbage collection of this object)."""

    def __init__(self, lib, m):
        self._lib, self._arena = lib, m.arena
        nv, ni = int(m.n_verts), int(m.n_indices)
        self.verts = (np.ctypeslib.as_array(C.cast(m.verts, C.POINTER(C.c_uint8)), (nv * VERTEX_DTYPE.itemsize,)).view(VERTEX_DTYPE)
                      if nv else np.zeros(0, VERTEX_DTYPE))
        self.indices = (np.ctypeslib.as_array(C.cast(m.indices, C.POINTER(C.c_uint32)), (ni,)) if ni else np.zeros(0, np.uint32))

    def _take(self):
        a, self._arena = self._arena, None
        self.verts = self.indices = None
        return a

    def release(self):
        a = self._take()
        if a:
            self._lib.vx_host_meshes_release(a)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class RayIndexInfo(C.Structure):
    _fields_ = [("triangles", C.c_uint64), ("bytes", C.c_uint64), ("blocks", C.c_uint32), ("straddling", C.c_uint32),
                ("build_ms", C.c_float)]


class ExecInfo(C.Structure):
    _fields_ = [("levels", C.c_uint32), ("retries", C.c_uint32), ("device_ms", C.c_float),
                ("total_verts", C.c_uint64), ("total_indices", C.c_uint64),
                ("active_blocks", C.c_uint32 * 8), ("algorithmic_bytes", C.c_uint64),
                ("blocks_read", C.c_uint32), ("mirror_ms", C.c_float), ("first_meshed_level", C.c_uint32)]


def hip_library_path():
    """The in-tree HIP build.  VOXELS_HIP_LIBRARY names another build of the SAME library (A/B measurements of kernel
    variants compiled from the same sources with different -D switches, tools/ab_build.py) — never a different backend."""
    return os.environ.get("VOXELS_HIP_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libvoxels_hip.so")


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class HipLibrary:
    """Loads the C-ABI library.  The default is the in-tree HIP build; a missing library is an error."""

    def __init__(self, path=None):
        path = path or hip_library_path()
        if not os.path.exists(path):
            raise VoxelsHipError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
        # torch wheels bundle their own HIP runtime; when torch is in the process it has to initialise before the
        # system runtime this library links (the other order leaves torch without a visible GPU)
        torch = sys.modules.get("torch")
        if torch is not None and torch.cuda.is_available():
            torch.cuda.init()
        lib = C.CDLL(path)
        vp, u32, i32 = C.c_void_p, C.c_uint32, C.c_int32
        lib.vx_backend.restype = C.c_char_p
        lib.vx_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        lib.vx_ctx_destroy.argtypes = [vp]
        lib.vx_last_error.restype = C.c_char_p
        lib.vx_last_error.argtypes = [vp]
        lib.vx_set_stream.argtypes = [vp, vp]
        lib.vx_grid_upload.argtypes = [vp, u32, vp, vp, vp, vp]
        lib.vx_grid_upload_packed.argtypes = [vp, vp, C.c_uint64]
        lib.vx_grid_attach_y.argtypes = [vp, u32, u32, u32, vp, C.c_int32, u32, vp, vp, C.c_int32, u32, vp]
        lib.vx_device_meshes.argtypes = [vp, vp, vp, vp, vp]
        lib.vx_export_meshes.argtypes = [vp, vp]
        lib.vx_compact_pools.argtypes = [vp]
        lib.vx_grid_pack.argtypes = [vp, vp, C.c_uint64, vp]
        lib.vx_grid_create_heightmap.argtypes = [vp, u32, vp]
        lib.vx_grid_create_terrain.argtypes = [vp, u32, u32]
        lib.vx_grid_create_terrain_ex.argtypes = [vp, u32, u32, u32]
        lib.vx_grid_fill_terrain.argtypes = [vp, u32]
        lib.vx_grid_inject_ball.argtypes = [vp, vp, vp, C.c_float, C.c_int, vp, vp]
        lib.vx_grid_inject_material.argtypes = [vp, vp, vp, C.c_uint8, C.c_int, vp, vp]
        lib.vx_level_ranges.argtypes = [vp, u32, vp]
        lib.vx_device_block_table.argtypes = [vp, u32, vp, vp]
        lib.vx_comm_unique_id.argtypes = [vp]
        lib.vx_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
        lib.vx_comm_destroy.argtypes = [vp]
        lib.vx_halo_exchange.argtypes = [vp]
        lib.vx_halo_exchange_group.argtypes = [vp, C.c_int]
        lib.vx_grid_read_block.argtypes = [vp, u32, vp, vp, vp, vp]
        lib.vx_grid_attach.argtypes = [vp, u32, u32, u32, vp, i32, vp, vp, i32, vp]
        lib.vx_grid_update_blocks.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        lib.vx_grid_invalidate.argtypes = [vp]
        lib.vx_ctx_forget_hints.argtypes = [vp]
        lib.vx_material_lut.argtypes = [vp, vp, vp]
        lib.vx_polygonize.argtypes = [vp, u32, C.POINTER(ExecInfo)]
        lib.vx_polygonize_from.argtypes = [vp, u32, u32, C.POINTER(ExecInfo)]
        lib.vx_polygonize_dirty.argtypes = [vp, vp, vp, C.POINTER(ExecInfo), vp, u32, C.POINTER(u32)]
        lib.vx_level_counts.argtypes = [vp, u32, C.POINTER(u32), vp]
        lib.vx_download_level.argtypes = [vp, u32, vp, vp, vp, vp, vp]
        lib.vx_host_meshes_acquire.argtypes = [vp, vp]
        lib.vx_host_meshes_release.argtypes = [vp]
        lib.vx_host_meshes_release.restype = None
        lib.vx_host_meshes_trim.argtypes = []
        lib.vx_host_meshes_trim.restype = None
        lib.vx_host_meshes_reserve.argtypes = [vp, C.c_uint64, C.c_uint64]
        lib.vx_stats.argtypes = [vp, vp]
        lib.vx_transition_path_counts.argtypes = [vp, vp]
        # (absent from builds of the library made before the material store: VOXELS_HIP_LIBRARY may name one, for A/B measurements)
        self.has_material_path_counts = hasattr(lib, "vx_material_path_counts")
        if self.has_material_path_counts:
            lib.vx_material_path_counts.argtypes = [vp, vp]
        # (the slot plan: HIP builds only, and absent from builds made before it)
        self.has_slot_plan = hasattr(lib, "vx_slot_plan_counts")
        if self.has_slot_plan:
            lib.vx_slot_plan_counts.argtypes = [vp, vp]
        # (material caches left in place by the runs that keep the plan: HIP builds only - the CPU emulation has neither store
        # nor plan - and absent from builds made before it)
        self.has_material_inplace = hasattr(lib, "vx_material_inplace_counts")
        if self.has_material_inplace:
            lib.vx_material_inplace_counts.argtypes = [vp, vp]
        # (the mesh layout kept by runs in place - one launch: HIP builds only, and absent from builds made before it)
        self.has_layout_keep = hasattr(lib, "vx_layout_keep_counts")
        if self.has_layout_keep:
            lib.vx_layout_keep_counts.argtypes = [vp, vp]
        # (the index pool kept by runs that keep the layout: HIP builds only, and absent from builds made before it)
        self.has_index_keep = hasattr(lib, "vx_index_keep_counts")
        if self.has_index_keep:
            lib.vx_index_keep_counts.argtypes = [vp, vp]
        # (the regular vertices' geometry kept by runs that keep the layout: HIP builds only, and absent from builds made before it)
        self.has_geometry_keep = hasattr(lib, "vx_geometry_keep_counts")
        if self.has_geometry_keep:
            lib.vx_geometry_keep_counts.argtypes = [vp, vp]
        lib.vx_selftest.argtypes = [vp, vp]
        lib.vx_stage_layout.argtypes = [vp, C.POINTER(C.c_int)]
        lib.vx_set_stage_timing.argtypes = [vp, C.c_int]
        lib.vx_stage_times.argtypes = [vp, vp]
        # ray casts: HIP builds only (the CPU emulation library of the tests does not have them)
        self.has_raycast = hasattr(lib, "vx_raycast")
        if self.has_raycast:
            lib.vx_raycast_prepare.argtypes = [vp, u32, vp]
            lib.vx_raycast_device.argtypes = [vp, u32, vp, u32, vp]
            lib.vx_raycast.argtypes = [vp, u32, vp, u32, vp]
        # LOD selection: HIP builds only, likewise
        # sphere casts and closest points: HIP builds only, like the ray casts
        self.has_shapecast = hasattr(lib, "vx_spherecast") and hasattr(lib, "vx_closest_point")
        if self.has_shapecast:
            for name in ("vx_spherecast_device", "vx_spherecast", "vx_closest_point_device", "vx_closest_point"):
                getattr(lib, name).argtypes = [vp, u32, vp, u32, vp]
                getattr(lib, name).restype = C.c_int
        # brush batches: HIP builds only, likewise
        self.has_brushes = hasattr(lib, "vx_grid_inject_brushes")
        if self.has_brushes:
            lib.vx_grid_inject_brushes.argtypes = [vp, vp, u32, vp, vp, vp, vp]
            lib.vx_grid_inject_brushes.restype = C.c_int
        # detached solid pieces: HIP builds only, likewise
        self.has_islands = hasattr(lib, "vx_grid_islands")
        if self.has_islands:
            lib.vx_grid_islands.argtypes = [vp, vp, vp, u32, vp, vp, vp, vp]
            lib.vx_grid_islands.restype = C.c_int
        # the cell map's read-back: libraries that keep the map
        self.has_cell_map = hasattr(lib, "vx_grid_cell_map")
        if self.has_cell_map:
            lib.vx_grid_cell_map.argtypes = [vp, u32, u32, u32, vp, vp]
        # smoothing: HIP builds only, likewise
        self.has_smooth = hasattr(lib, "vx_grid_smooth")
        if self.has_smooth:
            lib.vx_grid_smooth.argtypes = [vp, vp, u32, vp, vp, vp, vp]
            lib.vx_grid_smooth.restype = C.c_int
        # walk fields: HIP builds only, likewise
        self.has_walk_field = hasattr(lib, "vx_grid_walk_field")
        if self.has_walk_field:
            lib.vx_grid_walk_field.argtypes = [vp, vp, vp, u32, vp, vp, vp]
            lib.vx_grid_walk_field.restype = C.c_int
        # undo records: HIP builds only, likewise
        self.has_undo = all(hasattr(lib, name) for name in ("vx_grid_capture", "vx_record_trim", "vx_record_swap", "vx_record_info_get", "vx_record_block_ids",
                                                            "vx_record_read_block", "vx_record_free", "vx_brush_box"))
        if self.has_undo:
            lib.vx_grid_capture.argtypes = [vp, vp, u32, C.POINTER(vp)]
            lib.vx_record_trim.argtypes = [vp, vp, vp]
            lib.vx_record_swap.argtypes = [vp, vp, vp]
            lib.vx_record_info_get.argtypes = [vp, vp, vp]
            lib.vx_record_block_ids.argtypes = [vp, vp, vp, u32]
            lib.vx_record_read_block.argtypes = [vp, vp, u32, vp, vp, vp, vp]
            lib.vx_record_free.argtypes = [vp, vp]
            lib.vx_record_free.restype = None
            lib.vx_brush_box.argtypes = [vp, u32, vp]
            for name in ("vx_grid_capture", "vx_record_trim", "vx_record_swap", "vx_record_info_get", "vx_record_block_ids", "vx_record_read_block", "vx_brush_box"):
                getattr(lib, name).restype = C.c_int
        # stamps: HIP builds only, likewise
        stamp_calls = ("vx_stamp_capture", "vx_stamp_upload", "vx_stamp_read", "vx_stamp_info_get", "vx_grid_paste", "vx_paste_box")
        self.has_stamps = all(hasattr(lib, name) for name in stamp_calls + ("vx_stamp_free",))
        if self.has_stamps:
            lib.vx_stamp_capture.argtypes = [vp, vp, C.POINTER(vp)]
            lib.vx_stamp_upload.argtypes = [vp, vp, vp, vp, vp, C.POINTER(vp)]
            lib.vx_stamp_read.argtypes = [vp, vp, vp, vp, vp]
            lib.vx_stamp_info_get.argtypes = [vp, vp, vp]
            lib.vx_stamp_free.argtypes = [vp, vp]
            lib.vx_stamp_free.restype = None
            lib.vx_grid_paste.argtypes = [vp, vp, u32, vp, u32, vp, vp]
            lib.vx_paste_box.argtypes = [vp, vp, u32, vp]
            for name in stamp_calls:
                getattr(lib, name).restype = C.c_int
        # measurements: HIP builds only, likewise
        measure_calls = ("vx_grid_measure", "vx_record_measure", "vx_debug_measure_chunk", "vx_debug_measure_shortcuts")
        self.has_measure = all(hasattr(lib, name) for name in measure_calls)
        if self.has_measure:
            lib.vx_grid_measure.argtypes = [vp, vp, u32, vp, vp]
            lib.vx_record_measure.argtypes = [vp, vp, vp, vp, vp]
            lib.vx_debug_measure_chunk.argtypes = [vp, u32]
            lib.vx_debug_measure_shortcuts.argtypes = [vp, u32]
            for name in measure_calls:
                getattr(lib, name).restype = C.c_int
        # height maps: HIP builds only, likewise
        height_calls = ("vx_grid_heightmap", "vx_grid_heightmap_device", "vx_debug_height_shortcuts")
        self.has_height = all(hasattr(lib, name) for name in height_calls)
        if self.has_height:
            lib.vx_grid_heightmap.argtypes = [vp, vp, vp, vp, vp, vp]
            lib.vx_grid_heightmap_device.argtypes = [vp, vp, vp, vp, vp, vp]
            lib.vx_debug_height_shortcuts.argtypes = [vp, u32]
            for name in height_calls:
                getattr(lib, name).restype = C.c_int
        # ambient occlusion: HIP builds only, likewise
        occlusion_calls = ("vx_occlusion", "vx_occlusion_device", "vx_debug_occlusion_shortcuts")
        self.has_occlusion = all(hasattr(lib, name) for name in occlusion_calls)
        if self.has_occlusion:
            lib.vx_occlusion.argtypes = [vp, u32, vp, vp, C.c_uint64, vp]
            lib.vx_occlusion_device.argtypes = [vp, u32, vp, vp, C.c_uint64, vp]
            lib.vx_debug_occlusion_shortcuts.argtypes = [vp, u32]
            for name in occlusion_calls:
                getattr(lib, name).restype = C.c_int
        self.has_lod = hasattr(lib, "vx_lod_select")
        if self.has_lod:
            lib.vx_lod_select_device.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
            lib.vx_lod_select.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
        # scattering: HIP builds only, likewise
        self.has_scatter = hasattr(lib, "vx_scatter")
        if self.has_scatter:
            lib.vx_scatter_device.argtypes = [vp, u32, vp, u32, vp, vp, vp]
            lib.vx_scatter.argtypes = [vp, u32, vp, u32, vp, vp, vp]
        # overlap queries: HIP builds only, likewise
        self.has_overlap = hasattr(lib, "vx_overlap_boxes")
        if self.has_overlap:
            lib.vx_overlap_boxes_device.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, vp]
            lib.vx_overlap_boxes.argtypes = [vp, u32, vp, u32, u32, vp, vp, vp, vp]
        self.lib = lib
        self.path = path
        self.backend = lib.vx_backend().decode()


def island_query(box=None, detached_only=False, remove=False, anchor_faces=0x3F, max_voxels=0, air_value=127):
    """one ISLAND_QUERY_DTYPE record; box = (lo, hi) in grid coordinates (internal axes, Z up), None = the whole grid"""
    q = np.zeros(1, ISLAND_QUERY_DTYPE)
    if box is None:
        q["whole_grid"] = 1
    else:
        q["lo"], q["hi"] = np.asarray(box[0], np.uint32), np.asarray(box[1], np.uint32)
    q["flags"] = (ISLANDS_DETACHED_ONLY if detached_only else 0) | (ISLANDS_REMOVE if remove else 0)
    q["anchor_faces"] = anchor_faces
    q["max_voxels"] = max_voxels
    q["air_value"] = air_value
    return q


def height_query(box, direction="top", layers=1, count_surfaces=False):
    """one HEIGHT_QUERY_DTYPE record; box = (lo, hi) in grid coordinates (internal axes, Z up); direction "top" / "bottom" (or
    HEIGHT_FROM_TOP / HEIGHT_FROM_BOTTOM)"""
    q = np.zeros(1, HEIGHT_QUERY_DTYPE)
    q["box"]["lo"], q["box"]["hi"] = np.asarray(box[0], np.uint32), np.asarray(box[1], np.uint32)
    q["direction"] = {"top": HEIGHT_FROM_TOP, "bottom": HEIGHT_FROM_BOTTOM}.get(direction, direction)
    q["layers"] = layers
    q["flags"] = HEIGHT_COUNT_SURFACES if count_surfaces else 0
    return q


def occlusion_params(steps=8, transitions=False, box_min=None, box_max=None):
    """one OCCLUSION_PARAMS_DTYPE record; the filter box in mesh space (Y up), None = unbounded"""
    prm = np.zeros(1, OCCLUSION_PARAMS_DTYPE)
    prm["steps"] = steps
    prm["flags"] = OCCLUSION_TRANSITIONS if transitions else 0
    prm["box_min"] = -np.inf if box_min is None else np.asarray(box_min, np.float32)
    prm["box_max"] = np.inf if box_max is None else np.asarray(box_max, np.float32)
    return prm


def walk_query(box=None, clearance=2, step_up=1, step_down=1, cost_axial=10, cost_diagonal=14, cost_climb=0, max_cost=1 << 30):
    """one WALK_QUERY_DTYPE record; box = (lo, hi) in grid coordinates (internal axes, Z up), None = the whole grid"""
    q = np.zeros(1, WALK_QUERY_DTYPE)
    if box is None:
        q["whole_grid"] = 1
    else:
        q["lo"], q["hi"] = np.asarray(box[0], np.uint32), np.asarray(box[1], np.uint32)
    q["clearance"], q["step_up"], q["step_down"] = clearance, step_up, step_down
    q["cost_axial"], q["cost_diagonal"], q["cost_climb"], q["max_cost"] = cost_axial, cost_diagonal, cost_climb, max_cost
    return q


def walk_goals(goals):
    """a WALK_GOAL_DTYPE array from one, or from rows of (x, y, z) or (x, y, z, cost)"""
    if isinstance(goals, np.ndarray) and goals.dtype == WALK_GOAL_DTYPE:
        return np.ascontiguousarray(goals).reshape(-1)
    g = np.zeros(len(goals), WALK_GOAL_DTYPE)
    for k, row in enumerate(goals):
        g[k] = tuple(int(v) for v in row) + (0,) * (4 - len(row))
    return g


def smooth_op(box, center=None, radius=0.0, strength=1.0, iterations=1):
    """one SMOOTH_DTYPE record; box = (lo, hi) in grid coordinates (internal axes, Z up); center defaults to the middle of the
    box (it only matters with radius > 0: the ball falloff)"""
    op = np.zeros(1, SMOOTH_DTYPE)
    lo, hi = np.asarray(box[0], np.uint32), np.asarray(box[1], np.uint32)
    op["lo"], op["hi"] = lo, hi
    op["center"] = (lo.astype(np.float32) + hi.astype(np.float32)) * np.float32(0.5) if center is None else np.asarray(center, np.float32)
    op["radius"], op["strength"], op["iterations"] = radius, strength, iterations
    return op


def boxes(rows):
    """a BOX_DTYPE array from one, or from rows of (lo, hi) in grid coordinates (internal axes, Z up)"""
    if isinstance(rows, np.ndarray) and rows.dtype == BOX_DTYPE:
        return np.ascontiguousarray(rows).reshape(-1)
    b = np.zeros(len(rows), BOX_DTYPE)
    for k, (lo, hi) in enumerate(rows):
        b[k]["lo"], b[k]["hi"] = np.asarray(lo, np.uint32), np.asarray(hi, np.uint32)
    return b


def brush_boxes(brushes, n, library=None):
    """vx_brush_box over a BRUSH_DTYPE array: the BOX_DTYPE array of the brushes that touch a grid of edge n, in array order -
    capture it before vx_grid_inject_brushes and the record holds exactly the blocks the batch touches"""
    L = library or HipLibrary()
    if not L.has_undo:
        raise VoxelsHipError("this library has no undo records (HIP builds only)")
    brushes = np.ascontiguousarray(brushes, BRUSH_DTYPE).reshape(-1)
    out = np.zeros(brushes.size, BOX_DTYPE)
    keep = np.zeros(brushes.size, bool)
    for k in range(brushes.size):
        rc = L.lib.vx_brush_box(_ptr(brushes[k:k + 1]), int(n), _ptr(out[k:k + 1]))
        if rc < 0:
            raise VoxelsHipError("vx_brush_box failed (%d)" % rc)
        keep[k] = rc == 1
    return out[keep]


def pastes(rows):
    """a PASTE_DTYPE array from one, or from rows of (origin, stamp, orient, mode)"""
    if isinstance(rows, np.ndarray) and rows.dtype == PASTE_DTYPE:
        return np.ascontiguousarray(rows).reshape(-1)
    p = np.zeros(len(rows), PASTE_DTYPE)
    for k, (origin, stamp, orient, mode) in enumerate(rows):
        p[k]["origin"], p[k]["stamp"], p[k]["orient"], p[k]["mode"] = np.asarray(origin, np.int32), stamp, orient, mode
    return p


def paste_boxes(paste_rows, sizes, n, library=None):
    """vx_paste_box over a PASTE_DTYPE array; sizes = the (sx, sy, sz) of every stamp of the stamp array: the BOX_DTYPE array of the
    pastes that touch a grid of edge n, in array order - capture it before vx_grid_paste and the record holds exactly the blocks
    the batch touches"""
    L = library or HipLibrary()
    if not L.has_stamps:
        raise VoxelsHipError("this library has no stamps (HIP builds only)")
    ps = pastes(paste_rows)
    sizes = np.ascontiguousarray(sizes, np.uint32).reshape(-1, 3)
    out = np.zeros(ps.size, BOX_DTYPE)
    keep = np.zeros(ps.size, bool)
    for k in range(ps.size):
        rc = L.lib.vx_paste_box(_ptr(ps[k:k + 1]), _ptr(sizes[int(ps[k]["stamp"])]), int(n), _ptr(out[k:k + 1]))
        if rc < 0:
            raise VoxelsHipError("vx_paste_box failed (%d)" % rc)
        keep[k] = rc == 1
    return out[keep]


def capsule_stroke(p0, p1, radius, inj_type=2, margin=2.0):
    """One capsule brush for a tool of `radius` moved from p0 to p1 (grid coordinates, Z up): positioned at the middle of the
    segment, the ends relative to it, rewriting the segment's box grown by radius + margin on every side."""
    p0 = np.asarray(p0, np.float32); p1 = np.asarray(p1, np.float32)
    b = np.zeros(1, BRUSH_DTYPE)
    mid = (p0 + p1) * np.float32(0.5)
    b["position"] = mid
    b["shape"] = BRUSH_CAPSULE
    b["extents"] = np.abs(p1 - p0) + np.float32(2.0 * (radius + margin))
    b["type"] = inj_type
    b["a"] = p0 - mid
    b["b"] = p1 - mid
    b["radius"] = radius
    return b[0]


class Level:
    """One LOD level: blocks in PolygonSurface::GetBlockForLevel order, arrays concatenated."""

    def __init__(self, infos, verts, idx, tverts, tidx):
        self.infos, self.verts, self.idx, self.tverts, self.tidx = infos, verts, idx, tverts, tidx

    def totals(self):
        return (len(self.infos), len(self.verts), len(self.idx), len(self.tverts), len(self.tidx))


class Record:
    """An undo record (include/voxels_hip.h, "undo records") of a Polygonizer: made by Polygonizer.capture, freed by free() or
    when it is collected while the polygonizer that owns it lives."""

    def __init__(self, poly, handle):
        self._p, self._r = poly, handle

    def _call(self, fn, *args):
        if not self._r:
            raise VoxelsHipError("the record has been freed")
        p = self._p
        p._check(getattr(p._lib, fn)(p._h, self._r, *args), fn)

    def trim(self):
        """vx_record_trim -> the number of blocks dropped"""
        dropped = C.c_uint32()
        self._call("vx_record_trim", C.byref(dropped))
        return int(dropped.value)

    def swap(self):
        """vx_record_swap -> the SWAP_RESULT_DTYPE record"""
        res = np.zeros(1, SWAP_RESULT_DTYPE)
        self._call("vx_record_swap", _ptr(res))
        return res[0]

    def info(self):
        """vx_record_info_get -> the RECORD_INFO_DTYPE record"""
        info = np.zeros(1, RECORD_INFO_DTYPE)
        self._call("vx_record_info_get", _ptr(info))
        return info[0]

    def block_ids(self):
        """vx_record_block_ids -> the held block ids, ascending"""
        ids = np.zeros(int(self.info()["blocks"]), np.uint32)
        self._call("vx_record_block_ids", _ptr(ids) if ids.size else None, ids.size)
        return ids

    def read_block(self, index):
        """(dist int8[16,16,16] (z,y,x), mat, blend, BF_Empty) of entry `index`, as Polygonizer.read_block"""
        d = np.zeros((16, 16, 16), np.int8)
        m = np.zeros((16, 16, 16), np.uint8)
        b = np.zeros((16, 16, 16), np.uint8)
        f = np.zeros(1, np.uint8)
        self._call("vx_record_read_block", int(index), _ptr(d), _ptr(m), _ptr(b), _ptr(f))
        return d, m, b, int(f[0])

    def measure(self, tallies=True):
        """vx_record_measure: what changed between the record and the grid as it is now -> (the RECORD_DELTA_DTYPE record,
        removed uint64[256] by the record's materials, added uint64[256] by the grid's); tallies=False: (delta, None, None)"""
        if not self._p._L.has_measure:
            raise VoxelsHipError("this library has no measurements (HIP builds only)")
        delta = np.zeros(1, RECORD_DELTA_DTYPE)
        removed, added = (np.zeros(256, np.uint64), np.zeros(256, np.uint64)) if tallies else (None, None)
        self._call("vx_record_measure", _ptr(delta), _ptr(removed), _ptr(added))
        return delta[0], removed, added

    def free(self):
        if self._r and getattr(self._p, "_h", None):
            self._p._lib.vx_record_free(self._p._h, self._r)
        self._r = None

    def __del__(self):
        self.free()


class Stamp:
    """A stamp (include/voxels_hip.h, "stamps") of a Polygonizer: made by Polygonizer.capture_stamp / upload_stamp, freed by
    free() or when it is collected while the polygonizer that owns it lives."""

    def __init__(self, poly, handle):
        self._p, self._s = poly, handle

    def _call(self, fn, *args):
        if not self._s:
            raise VoxelsHipError("the stamp has been freed")
        p = self._p
        p._check(getattr(p._lib, fn)(p._h, self._s, *args), fn)

    def info(self):
        """vx_stamp_info_get -> the STAMP_INFO_DTYPE record"""
        info = np.zeros(1, STAMP_INFO_DTYPE)
        self._call("vx_stamp_info_get", _ptr(info))
        return info[0]

    @property
    def size(self):
        return tuple(int(v) for v in self.info()["size"])

    def read(self):
        """vx_stamp_read -> (dist int8[sz, sy, sx], mat, blend)"""
        sx, sy, sz = self.size
        d, m, b = np.zeros((sz, sy, sx), np.int8), np.zeros((sz, sy, sx), np.uint8), np.zeros((sz, sy, sx), np.uint8)
        self._call("vx_stamp_read", _ptr(d), _ptr(m), _ptr(b))
        return d, m, b

    def free(self):
        if self._s and getattr(self._p, "_h", None):
            self._p._lib.vx_stamp_free(self._p._h, self._s)
        self._s = None

    def __del__(self):
        self.free()


class Polygonizer:
    """Host-side mirror of Voxels::Polygonizer for the device path.

    upload(dist, mat, blend, empty_flags)  ~ the Grid the reference's Execute reads
    execute(num_levels=0)                   ~ Polygonizer::Execute (full run); returns exec info
    level(l) / stats()                      ~ PolygonSurface accessors
    """

    def __init__(self, device=0, library=None):
        self._L = library or HipLibrary()
        self._lib = self._L.lib
        h = C.c_void_p()
        rc = self._lib.vx_ctx_create(int(device), C.byref(h))
        if rc != 0:
            raise VoxelsHipError("vx_ctx_create failed (%d): no usable HIP device?" % rc)
        self._h = h
        self.n = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.vx_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            raise VoxelsHipError("%s failed (%d): %s" % (what, rc, self._lib.vx_last_error(self._h).decode()))

    @property
    def backend(self):
        return self._L.backend

    def set_stream(self, stream_handle):
        self._check(self._lib.vx_set_stream(self._h, C.c_void_p(stream_handle)), "vx_set_stream")

    def upload(self, dist, mat, blend, empty_flags):
        n = dist.shape[0]
        assert dist.shape == (n, n, n) and dist.dtype == np.int8 and dist.flags.c_contiguous
        for a in (mat, blend):
            assert a is None or (a.shape == (n, n, n) and a.dtype == np.uint8 and a.flags.c_contiguous)
        empty_flags = np.ascontiguousarray(empty_flags, np.uint8)
        assert empty_flags.size == (n // 16) ** 3
        self._keep = (dist, mat, blend, empty_flags)
        self._check(self._lib.vx_grid_upload(self._h, n, _ptr(dist), _ptr(mat), _ptr(blend), _ptr(empty_flags)), "vx_grid_upload")
        self.n = n

    def upload_packed(self, blob):
        """Grid file format v1 (Grid::PackForSave) straight to the device; expanded there."""
        blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if not isinstance(blob, np.ndarray) else blob.view(np.uint8))
        self._check(self._lib.vx_grid_upload_packed(self._h, _ptr(blob), blob.size), "vx_grid_upload_packed")
        self.n = int(np.frombuffer(blob[4:8].tobytes(), np.uint32)[0])

    def create_heightmap(self, heightmap):
        """Grid::Create(w, heightmap) evaluated on the device; heightmap int8 [w, w] (row = y)."""
        hm = np.ascontiguousarray(heightmap, np.int8)
        assert hm.ndim == 2 and hm.shape[0] == hm.shape[1]
        self._check(self._lib.vx_grid_create_heightmap(self._h, hm.shape[0], _ptr(hm)), "vx_grid_create_heightmap")
        self.n = hm.shape[0]

    def pack(self):
        """Grid::PackForSave of the resident grid (encoded on the device) -> uint8 array."""
        size = C.c_uint64()
        self._check(self._lib.vx_grid_pack(self._h, None, 0, C.byref(size)), "vx_grid_pack")
        out = np.zeros(size.value, np.uint8)
        self._check(self._lib.vx_grid_pack(self._h, _ptr(out), out.size, C.byref(size)), "vx_grid_pack")
        return out

    def read_block(self, block_id):
        """(dist int8[16,16,16] (z,y,x), mat, blend, BF_Empty) of one resident block."""
        d = np.zeros((16, 16, 16), np.int8)
        m = np.zeros((16, 16, 16), np.uint8)
        b = np.zeros((16, 16, 16), np.uint8)
        f = np.zeros(1, np.uint8)
        self._check(self._lib.vx_grid_read_block(self._h, int(block_id), _ptr(d), _ptr(m), _ptr(b), _ptr(f)), "vx_grid_read_block")
        return d, m, b, int(f[0])

    def column(self, n, x, y):
        """The n distance samples of the voxel column (x, y) of the resident grid (all z), read block by block: what tools use
        to find the surface without generating the grid on the host a second time."""
        nb = n // 16
        return np.concatenate([self.read_block((bz * nb + y // 16) * nb + x // 16)[0][:, y % 16, x % 16] for bz in range(nb)])

    def inject_ball(self, pos, ext, radius, inj_type):
        """Grid::InjectSurface with the analytic ball brush, on the device; returns the modified box (output order)."""
        pos = np.ascontiguousarray(pos, np.float32); ext = np.ascontiguousarray(ext, np.float32)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self._lib.vx_grid_inject_ball(self._h, _ptr(pos), _ptr(ext), C.c_float(radius), int(inj_type), _ptr(mn), _ptr(mx)), "vx_grid_inject_ball")
        return mn, mx

    def inject_material(self, pos, ext, material, add):
        pos = np.ascontiguousarray(pos, np.float32); ext = np.ascontiguousarray(ext, np.float32)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        self._check(self._lib.vx_grid_inject_material(self._h, _ptr(pos), _ptr(ext), int(material), int(bool(add)), _ptr(mn), _ptr(mx)), "vx_grid_inject_material")
        return mn, mx

    def inject_brushes(self, brushes):
        """vx_grid_inject_brushes: a BRUSH_DTYPE array applied in array order in one device pass ->
        (results BRUSH_RESULT_DTYPE array, union_min, union_max, distinct touched blocks)."""
        if not self._L.has_brushes:
            raise VoxelsHipError("this library has no brush batches (HIP builds only)")
        brushes = np.ascontiguousarray(brushes, BRUSH_DTYPE)
        results = np.zeros(brushes.size, BRUSH_RESULT_DTYPE)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        touched = C.c_uint32()
        self._check(self._lib.vx_grid_inject_brushes(self._h, _ptr(brushes) if brushes.size else None, brushes.size,
                                                     _ptr(results) if brushes.size else None, _ptr(mn), _ptr(mx), C.byref(touched)),
                    "vx_grid_inject_brushes")
        return results, mn, mx, int(touched.value)

    def smooth(self, ops):
        """vx_grid_smooth: a SMOOTH_DTYPE array applied in array order ->
        (results SMOOTH_RESULT_DTYPE array, union_min, union_max, changed voxels)."""
        if not self._L.has_smooth:
            raise VoxelsHipError("this library has no vx_grid_smooth (HIP builds only)")
        ops = np.ascontiguousarray(ops, SMOOTH_DTYPE).reshape(-1)
        results = np.zeros(ops.size, SMOOTH_RESULT_DTYPE)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)
        changed = C.c_uint64()
        self._check(self._lib.vx_grid_smooth(self._h, _ptr(ops) if ops.size else None, ops.size, _ptr(results) if ops.size else None,
                                             _ptr(mn), _ptr(mx), C.byref(changed)), "vx_grid_smooth")
        return results, mn, mx, int(changed.value)

    def capture(self, box_rows):
        """vx_grid_capture: the blocks that a BOX_DTYPE array (or rows of (lo, hi)) intersects -> a Record"""
        if not self._L.has_undo:
            raise VoxelsHipError("this library has no undo records (HIP builds only)")
        b = boxes(box_rows)
        h = C.c_void_p()
        self._check(self._lib.vx_grid_capture(self._h, _ptr(b) if b.size else None, b.size, C.byref(h)), "vx_grid_capture")
        return Record(self, h)

    def measure(self, box_rows, tallies=True):
        """vx_grid_measure: a BOX_DTYPE array (or rows of (lo, hi)) -> (the MEASURE_DTYPE array, uint64[count, 256] solid voxels
        per box and material byte, or None with tallies=False)"""
        if not self._L.has_measure:
            raise VoxelsHipError("this library has no measurements (HIP builds only)")
        b = boxes(box_rows)
        results = np.zeros(b.size, MEASURE_DTYPE)
        per_material = np.zeros((b.size, 256), np.uint64) if tallies else None
        self._check(self._lib.vx_grid_measure(self._h, _ptr(b) if b.size else None, b.size, _ptr(results) if b.size else None,
                                              _ptr(per_material) if tallies and b.size else None), "vx_grid_measure")
        return results, per_material

    def heightmap(self, box, direction="top", layers=1, materials=True, count_surfaces=False):
        """vx_grid_heightmap: the surfaces of the columns of box = (lo, hi) in grid coordinates (internal axes, Z up) ->
        (heights uint32 [layers, H, W] in 24.8 fixed point, HEIGHT_NONE where a column has fewer surfaces; materials uint8
        [layers, H, W] or None; surfaces uint16 [H, W] with count_surfaces, else None; the HEIGHT_COUNTS_DTYPE record)"""
        if not self._L.has_height:
            raise VoxelsHipError("this library has no height maps (HIP builds only)")
        q = height_query(box, direction, layers, count_surfaces)
        w, h = (int(q["box"]["hi"][0][k]) - int(q["box"]["lo"][0][k]) for k in (0, 1))
        shape = (int(layers), max(h, 0), max(w, 0))
        heights = np.zeros(shape, np.uint32)
        mats = np.zeros(shape, np.uint8) if materials else None
        surfaces = np.zeros(shape[1:], np.uint16) if count_surfaces else None
        counts = np.zeros(1, HEIGHT_COUNTS_DTYPE)
        self._check(self._lib.vx_grid_heightmap(self._h, _ptr(q), _ptr(heights), _ptr(mats), _ptr(surfaces), _ptr(counts)), "vx_grid_heightmap")
        return heights, mats, surfaces, counts[0]

    def heightmap_device(self, box, heights, direction="top", layers=1, materials=None, surfaces=None, counts=True):
        """vx_grid_heightmap_device: as heightmap(), into device memory - heights (layers * H * W uint32), materials (as many
        uint8, or None) and surfaces (H * W uint16, or None: given, it sets VX_HEIGHT_COUNT_SURFACES) are torch device tensors or
        device addresses (ints).  counts=True: waits and returns the HEIGHT_COUNTS_DTYPE record; counts=False: only queued on the
        context's stream (set_stream), returns None."""
        if not self._L.has_height:
            raise VoxelsHipError("this library has no height maps (HIP builds only)")
        q = height_query(box, direction, layers, surfaces is not None)
        cells = int(np.prod([max(int(q["box"]["hi"][0][k]) - int(q["box"]["lo"][0][k]), 0) for k in (0, 1)]))

        def address(a, size, entries):
            if a is None or isinstance(a, int):
                return C.c_void_p(a)
            assert a.is_cuda and a.is_contiguous() and a.element_size() == size and a.numel() == entries
            return C.c_void_p(a.data_ptr())

        rec = np.zeros(1, HEIGHT_COUNTS_DTYPE) if counts else None
        self._check(self._lib.vx_grid_heightmap_device(self._h, _ptr(q), address(heights, 4, cells * int(layers)), address(materials, 1, cells * int(layers)),
                                                       address(surfaces, 2, cells), _ptr(rec)), "vx_grid_heightmap_device")
        return rec[0] if counts else None

    def _occlusion_lib(self):
        if not self._L.has_occlusion:
            raise VoxelsHipError("%s has no ambient occlusion (vx_occlusion*)" % self._L.path)
        return self._L.lib

    def occlusion(self, level, params=None, counts=True):
        """vx_occlusion: an OCCLUSION_PARAMS_DTYPE record (occlusion_params(), the default when None) -> (uint8 array parallel to
        the vertex pool of device_meshes(), 255 where the call baked nothing; the OCCLUSION_COUNTS_DTYPE record, or None)"""
        lib = self._occlusion_lib()
        prm = np.ascontiguousarray(occlusion_params() if params is None else params, OCCLUSION_PARAMS_DTYPE)
        nv = int(self.device_meshes()[2])
        ao = np.zeros(nv, np.uint8)
        rec = np.zeros(1, OCCLUSION_COUNTS_DTYPE) if counts else None
        self._check(lib.vx_occlusion(self._h, int(level), _ptr(prm), C.c_void_p(ao.ctypes.data if nv else None), nv, _ptr(rec)), "vx_occlusion")
        return ao, (rec[0] if counts else None)

    def occlusion_device(self, level, params, d_ao, capacity=None, d_counts=None):
        """vx_occlusion_device: d_ao (uint8, at least the pool's n_verts entries) and d_counts (32 bytes, 8-byte aligned, or None) are
        torch device tensors or device addresses (ints; then give the capacity); queued on the context's stream (set_stream),
        returns without waiting."""
        lib = self._occlusion_lib()
        prm = np.ascontiguousarray(params, OCCLUSION_PARAMS_DTYPE)

        def address(a):
            return C.c_void_p(a if a is None or isinstance(a, int) else a.data_ptr())

        if capacity is None:
            assert not isinstance(d_ao, int) and d_ao.is_cuda and d_ao.is_contiguous() and d_ao.element_size() == 1
            capacity = d_ao.numel()
        self._check(lib.vx_occlusion_device(self._h, int(level), _ptr(prm), address(d_ao), int(capacity), address(d_counts)), "vx_occlusion_device")

    def debug_occlusion_shortcuts(self, enable):
        self._check(self._occlusion_lib().vx_debug_occlusion_shortcuts(self._h, 1 if enable else 0), "vx_debug_occlusion_shortcuts")

    def capture_stamp(self, box):
        """vx_stamp_capture: the voxels of box = (lo, hi) in grid coordinates (internal axes, Z up) -> a Stamp"""
        if not self._L.has_stamps:
            raise VoxelsHipError("this library has no stamps (HIP builds only)")
        b = boxes([box])
        h = C.c_void_p()
        self._check(self._lib.vx_stamp_capture(self._h, _ptr(b), C.byref(h)), "vx_stamp_capture")
        return Stamp(self, h)

    def upload_stamp(self, dist, mat=None, blend=None):
        """vx_stamp_upload: dist int8 [sz, sy, sx] (and mat, blend uint8 of the same shape, None = zeros) -> a Stamp"""
        if not self._L.has_stamps:
            raise VoxelsHipError("this library has no stamps (HIP builds only)")
        dist = np.ascontiguousarray(dist, np.int8)
        assert dist.ndim == 3
        mat, blend = (None if a is None else np.ascontiguousarray(a, np.uint8) for a in (mat, blend))
        assert all(a is None or a.shape == dist.shape for a in (mat, blend))
        size = np.array(dist.shape[::-1], np.uint32)
        h = C.c_void_p()
        self._check(self._lib.vx_stamp_upload(self._h, _ptr(size), _ptr(dist), _ptr(mat), _ptr(blend), C.byref(h)), "vx_stamp_upload")
        return Stamp(self, h)

    def paste(self, stamps, paste_rows):
        """vx_grid_paste: a list of Stamps (None entries allowed) and a PASTE_DTYPE array (or rows of (origin, stamp, orient, mode))
        applied in array order in one device pass -> (results PASTE_RESULT_DTYPE array, counts PASTE_COUNTS_DTYPE record)"""
        if not self._L.has_stamps:
            raise VoxelsHipError("this library has no stamps (HIP builds only)")
        ps = pastes(paste_rows)
        handles = (C.c_void_p * max(len(stamps), 1))(*[None if s is None else s._s for s in stamps])
        results = np.zeros(ps.size, PASTE_RESULT_DTYPE)
        counts = np.zeros(1, PASTE_COUNTS_DTYPE)
        self._check(self._lib.vx_grid_paste(self._h, C.cast(handles, C.c_void_p) if len(stamps) else None, len(stamps), _ptr(ps) if ps.size else None, ps.size,
                                            _ptr(results) if ps.size else None, _ptr(counts)), "vx_grid_paste")
        return results, counts[0]

    def islands(self, box=None, detached_only=False, remove=False, anchor_faces=0x3F, max_voxels=0, air_value=127, labels=None, capacity=None):
        """vx_grid_islands: the connected components of the solid voxels of `box` ((lo, hi), None = the whole grid) ->
        (records ISLAND_DTYPE array in label order, counts ISLAND_COUNTS_DTYPE record, out_min, out_max).  labels: optional torch
        device tensor of V int32 / uint32 that receives the label volume.  capacity=None: one call with no room (and without the
        removal) to learn `listed`, then the call proper with exactly that room."""
        if not self._L.has_islands:
            raise VoxelsHipError("this library has no vx_grid_islands (HIP builds only)")
        q = island_query(box, detached_only, remove, anchor_faces, max_voxels, air_value)
        lp = None
        if labels is not None:
            assert labels.is_cuda and labels.is_contiguous() and labels.element_size() == 4
            ext = [self.n] * 3 if box is None else [int(h) - int(l) for l, h in zip(box[0], box[1])]
            assert labels.numel() == ext[0] * ext[1] * ext[2]
            lp = C.c_void_p(labels.data_ptr())
        counts = np.zeros(1, ISLAND_COUNTS_DTYPE)
        mn, mx = np.zeros(3, np.float32), np.zeros(3, np.float32)

        def call(query, room):
            recs = np.zeros(room, ISLAND_DTYPE)
            rc = self._lib.vx_grid_islands(self._h, _ptr(query), _ptr(recs) if room else None, room, _ptr(counts), lp, _ptr(mn), _ptr(mx))
            return rc, recs

        if capacity is None:
            # learn `listed` from a query that changes nothing, then make the call with exactly that room
            probe = q.copy()
            probe["flags"] &= ~np.uint32(ISLANDS_REMOVE)
            rc, _ = call(probe, 0)
            if rc not in (0, -3):
                self._check(rc, "vx_grid_islands")
            capacity = int(counts["listed"][0])
        rc, recs = call(q, int(capacity))
        listed = int(counts["listed"][0])
        if rc == -3:
            raise VoxelsHipError("vx_grid_islands failed (-3): %d records listed, room for %d" % (listed, capacity))
        self._check(rc, "vx_grid_islands")
        return recs[:min(listed, int(capacity))], counts[0].copy(), mn, mx

    def walk_field(self, box, goals, clearance=2, step_up=1, step_down=1, cost_axial=10, cost_diagonal=14, cost_climb=0, max_cost=1 << 30,
                   field=None, dirs=None):
        """vx_grid_walk_field: the cost of the cheapest walk from every standable voxel of `box` ((lo, hi), None = the whole
        grid) to the nearest goal (a WALK_GOAL_DTYPE array, or rows of (x, y, z[, cost])) -> the counts WALK_COUNTS_DTYPE record.
        field: optional torch device tensor of V int32 / uint32 that receives the field (WALK_UNREACHED where there is no walk);
        dirs: optional torch device tensor of V uint8 that receives the direction bytes."""
        if not self._L.has_walk_field:
            raise VoxelsHipError("this library has no vx_grid_walk_field (HIP builds only)")
        q = walk_query(box, clearance, step_up, step_down, cost_axial, cost_diagonal, cost_climb, max_cost)
        g = walk_goals(goals)
        ext = [self.n] * 3 if box is None else [int(h) - int(l) for l, h in zip(box[0], box[1])]
        fp = dp = None
        if field is not None:
            assert field.is_cuda and field.is_contiguous() and field.element_size() == 4 and field.numel() == ext[0] * ext[1] * ext[2]
            fp = C.c_void_p(field.data_ptr())
        if dirs is not None:
            assert dirs.is_cuda and dirs.is_contiguous() and dirs.element_size() == 1 and dirs.numel() == ext[0] * ext[1] * ext[2]
            dp = C.c_void_p(dirs.data_ptr())
        counts = np.zeros(1, WALK_COUNTS_DTYPE)
        self._check(self._lib.vx_grid_walk_field(self._h, _ptr(q), _ptr(g) if g.size else None, g.size, fp, dp, _ptr(counts)), "vx_grid_walk_field")
        return counts[0].copy()

    def compact_pools(self):
        self._check(self._lib.vx_compact_pools(self._h), "vx_compact_pools")

    def device_meshes(self):
        """(device pointer of the vertex pool, of the index pool, vertices, indices) of the last full run."""
        dv, di = C.c_void_p(), C.c_void_p()
        nv, ni = C.c_uint64(), C.c_uint64()
        self._check(self._lib.vx_device_meshes(self._h, C.byref(dv), C.byref(di), C.byref(nv), C.byref(ni)), "vx_device_meshes")
        return dv.value, di.value, nv.value, ni.value

    def export_meshes(self):
        """Inter-process handles of the two pools (vx_export_meshes): dict with the two 64-byte handles, the counts, the
        capacities and the pools' generation."""
        class IpcMeshes(C.Structure):
            _fields_ = [("verts_handle", C.c_uint8 * 64), ("indices_handle", C.c_uint8 * 64), ("n_verts", C.c_uint64), ("n_indices", C.c_uint64),
                        ("verts_capacity", C.c_uint64), ("indices_capacity", C.c_uint64), ("generation", C.c_uint64)]
        m = IpcMeshes()
        self._check(self._lib.vx_export_meshes(self._h, C.byref(m)), "vx_export_meshes")
        return {"verts_handle": bytes(m.verts_handle), "indices_handle": bytes(m.indices_handle), "n_verts": int(m.n_verts), "n_indices": int(m.n_indices),
                "verts_capacity": int(m.verts_capacity), "indices_capacity": int(m.indices_capacity), "generation": int(m.generation)}

    def create_terrain(self, n, seed=1337, style=0):
        """The synthetic noise terrain (voxels_amd.synth.terrain) generated on the device into a grid the context owns."""
        self._check(self._lib.vx_grid_create_terrain_ex(self._h, int(n), int(seed), int(style)), "vx_grid_create_terrain_ex")
        self.n = n

    def fill_terrain(self, seed=1337):
        """The same into the attached slab (own layers + halo) with the BF_Empty flags of the rank's own blocks."""
        self._check(self._lib.vx_grid_fill_terrain(self._h, int(seed)), "vx_grid_fill_terrain")

    def comm_unique_id(self):
        """128-byte RCCL id (rank 0 creates it, every rank passes it to comm_init)."""
        buf = np.zeros(128, np.uint8)
        rc = self._lib.vx_comm_unique_id(_ptr(buf))
        if rc != 0:
            raise VoxelsHipError("vx_comm_unique_id failed (%d): RCCL not available?" % rc)
        return buf

    def comm_init(self, nranks, rank, unique_id):
        uid = np.ascontiguousarray(unique_id, np.uint8)
        assert uid.size == 128
        self._check(self._lib.vx_comm_init(self._h, int(nranks), int(rank), _ptr(uid)), "vx_comm_init")

    def halo_exchange(self):
        """Halo of the attached slab over RCCL (queued on the context's stream, no host wait)."""
        self._check(self._lib.vx_halo_exchange(self._h), "vx_halo_exchange")

    @staticmethod
    def halo_exchange_group(polys):
        """The same between several contexts of this process (slab order)."""
        arr = (C.c_void_p * len(polys))(*[p._h for p in polys])
        rc = polys[0]._lib.vx_halo_exchange_group(arr, len(polys))
        if rc != 0:
            bad = next((p for p in polys if p._lib.vx_last_error(p._h)), polys[0])
            raise VoxelsHipError("vx_halo_exchange_group failed (%d): %s" % (rc, bad._lib.vx_last_error(bad._h).decode()))

    def device_block_table(self, lvl):
        """(device pointer, count) of the level's block table (vx_listed_block records, GetBlockForLevel order)."""
        tab, nb = C.c_void_p(), C.c_uint32()
        self._check(self._lib.vx_device_block_table(self._h, int(lvl), C.byref(tab), C.byref(nb)), "vx_device_block_table")
        return tab.value, nb.value

    def level_ranges(self, lvl):
        """Per block (download order): offsets of its meshes in the device pools."""
        nb = self.level(lvl, with_data=False).infos.size
        dt = np.dtype([("v_off", np.uint32), ("i_off", np.uint32), ("tv_off", np.uint32, 6), ("ti_off", np.uint32, 6)])
        r = np.zeros(nb, dt)
        self._check(self._lib.vx_level_ranges(self._h, int(lvl), _ptr(r)), "vx_level_ranges")
        return r

    def attach(self, n, z_begin, z_end, d_dist, dist_z0, d_mat, d_blend, mat_z0, d_flags):
        """Device pointers (ints), e.g. torch tensors' data_ptr().  The library mirrors the fields for its gathers: after
        rewriting the tensors in place call invalidate() (or attach again), or the next execute() sees the old contents."""
        self._check(self._lib.vx_grid_attach(self._h, n, z_begin, z_end, C.c_void_p(d_dist), dist_z0,
                                             C.c_void_p(d_mat), C.c_void_p(d_blend), mat_z0, C.c_void_p(d_flags)),
                    "vx_grid_attach")
        self.n = n

    def attach_y(self, n, y_begin, y_end, d_dist, dist_y0, dist_rows, d_mat, d_blend, mat_y0, mat_rows, d_flags):
        """Slab cut along y: device arrays [n][rows][n] (see vx_grid_attach_y)."""
        self._check(self._lib.vx_grid_attach_y(self._h, n, y_begin, y_end, C.c_void_p(d_dist), dist_y0, dist_rows,
                                               C.c_void_p(d_mat), C.c_void_p(d_blend), mat_y0, mat_rows, C.c_void_p(d_flags)),
                    "vx_grid_attach_y")
        self.n = n

    def invalidate(self):
        """The attached tensors were rewritten in place by the caller: the library's mirrors of them are rebuilt by the
        next execute().  Without this call (or a new attach) a run after an in-place edit polygonizes the OLD contents."""
        self._check(self._lib.vx_grid_invalidate(self._h), "vx_grid_invalidate")

    def cell_map(self, bx, by, bz):
        """vx_grid_cell_map: (128 uint32 words, count) - the bitmap of the non-trivial cells of level-0 block (bx, by, bz), bit
        x | y << 4 | z << 8, from the cell map the library keeps with its mirrors (brought up to date first if it is stale)."""
        if not self._L.has_cell_map:
            raise VoxelsHipError("this library has no vx_grid_cell_map")
        out = np.zeros(128, np.uint32)
        count = C.c_uint32()
        self._check(self._lib.vx_grid_cell_map(self._h, int(bx), int(by), int(bz), _ptr(out), C.byref(count)), "vx_grid_cell_map")
        return out, int(count.value)

    def forget_hints(self):
        """What earlier runs taught this context about its surfaces (capacity classes, launch sizes) is forgotten: the next run
        starts from a new context's conservative defaults (vx_ctx_forget_hints)."""
        self._check(self._lib.vx_ctx_forget_hints(self._h), "vx_ctx_forget_hints")

    def update_blocks(self, block_ids, dist, mat, blend, empty_flags):
        block_ids = np.ascontiguousarray(block_ids, np.uint32)
        self._check(self._lib.vx_grid_update_blocks(self._h, block_ids.size, _ptr(block_ids), _ptr(dist), _ptr(mat),
                                                    _ptr(blend), _ptr(np.ascontiguousarray(empty_flags, np.uint8))),
                    "vx_grid_update_blocks")

    def set_materials(self, lut, valid=None):
        lut = np.ascontiguousarray(lut, np.uint8)
        assert lut.shape == (256, 6)
        valid = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        self._check(self._lib.vx_material_lut(self._h, _ptr(lut), _ptr(valid)), "vx_material_lut")

    def execute(self, num_levels=0):
        info = ExecInfo()
        self._check(self._lib.vx_polygonize(self._h, int(num_levels), C.byref(info)), "vx_polygonize")
        self.info = info
        return info

    def execute_from(self, num_levels, first_meshed_level):
        """vx_polygonize_from: caches and bitmaps of every level, meshes only from first_meshed_level up (info.first_meshed_level
        tells what the run really did)."""
        info = ExecInfo()
        self._check(self._lib.vx_polygonize_from(self._h, int(num_levels), int(first_meshed_level), C.byref(info)), "vx_polygonize_from")
        self.info = info
        return info

    def execute_dirty(self, min_corner, max_corner):
        """Polygonizer::Execute with a Modification: re-polygonize the dirty box (output, Y-up, coordinates).
        Returns the ids of the rebuilt blocks (Modification::GetModifiedBlocks)."""
        mn = np.ascontiguousarray(min_corner, np.float32)
        mx = np.ascontiguousarray(max_corner, np.float32)
        info = ExecInfo()
        cap = 1 << 20
        ids = getattr(self, "_dirty_ids", None)  # (kept: allocating and zeroing 4 MB per call cost more than a small incremental run)
        if ids is None:
            ids = self._dirty_ids = np.zeros(cap, np.uint32)
        cnt = C.c_uint32()
        self._check(self._lib.vx_polygonize_dirty(self._h, _ptr(mn), _ptr(mx), C.byref(info), _ptr(ids), cap, C.byref(cnt)),
                    "vx_polygonize_dirty")
        self.info = info
        return ids[:cnt.value].copy()

    def debug_header(self, count=352):
        """vx_debug_header: the device copy of the run's header words (diagnostics)"""
        out = np.zeros(count, np.uint32)
        self._check(self._lib.vx_debug_header(self._h, _ptr(out), int(count)), "vx_debug_header")
        return out

    def level(self, lvl, with_data=True):
        nb = C.c_uint32()
        tot = np.zeros(4, np.uint64)
        self._check(self._lib.vx_level_counts(self._h, lvl, C.byref(nb), _ptr(tot)), "vx_level_counts")
        infos = np.zeros(nb.value, BLOCK_INFO_DTYPE)
        if not with_data:
            self._check(self._lib.vx_download_level(self._h, lvl, _ptr(infos), None, None, None, None), "vx_download_level")
            return Level(infos, np.zeros(0, VERTEX_DTYPE), np.zeros(0, np.uint32), np.zeros(0, VERTEX_DTYPE), np.zeros(0, np.uint32))
        verts = np.zeros(int(tot[0]), VERTEX_DTYPE)
        idx = np.zeros(int(tot[1]), np.uint32)
        tverts = np.zeros(int(tot[2]), VERTEX_DTYPE)
        tidx = np.zeros(int(tot[3]), np.uint32)
        self._check(self._lib.vx_download_level(self._h, lvl, _ptr(infos), _ptr(verts), _ptr(idx), _ptr(tverts), _ptr(tidx)),
                    "vx_download_level")
        return Level(infos, verts, idx, tverts, tidx)

    def reserve_host_meshes(self, n_verts, n_indices):
        """vx_host_meshes_reserve: page-lock an arena of that size ahead of time (it waits in the recycling list)."""
        self._check(self._lib.vx_host_meshes_reserve(self._h, int(n_verts), int(n_indices)), "vx_host_meshes_reserve")

    def host_meshes(self, previous=None):
        """vx_host_meshes_acquire: both pools on the host (page-locked, one DMA), as numpy views.  Block k of level l owns
        verts[level_ranges(l)[k]['v_off'] : ... + level(l, False).infos[k]['n_verts']] etc.  `previous`: a HostMeshes of an
        earlier acquire on this context, brought up to date instead (incremental runs); do not use it afterwards."""
        m = _HostMeshesStruct()
        if previous is not None:
            m.arena = previous._take()
        rc = self._lib.vx_host_meshes_acquire(self._h, C.byref(m))
        if rc != 0 and m.arena:
            # the C side always writes the arena back (possibly a different one): nothing owns it on this path, so it goes
            # back to the library's recycling list instead of leaking page-locked memory (`previous` is spent either way)
            self._lib.vx_host_meshes_release(m.arena)
            m.arena = None
        self._check(rc, "vx_host_meshes_acquire")
        return HostMeshes(self._lib, m)

    def all_levels(self):
        return [self.level(l) for l in range(self.info.levels)]

    def set_stage_timing(self, enable):
        self._check(self._lib.vx_set_stage_timing(self._h, int(bool(enable))), "vx_set_stage_timing")


    def stage_layout(self):
        """vx_stage_layout: 1 if the last run with stage timing used the single-stream form (k_main), else 0"""
        v = C.c_int(0)
        self._check(self._lib.vx_stage_layout(self._h, C.byref(v)), "vx_stage_layout")
        return v.value

    def stage_times(self):
        """ms of (reset, classify, hierarchy, material, regular level 0, regular levels >= 1, transition, block lists) of the last run."""
        out = np.zeros(8, np.float32)
        self._check(self._lib.vx_stage_times(self._h, _ptr(out)), "vx_stage_times")
        return out

    def selftest(self):
        """vx_selftest: mismatch counts of the device arithmetic against its definition, exhaustively ([0..2], [11] must be 0)."""
        r = np.zeros(16, np.uint32)
        self._check(self._lib.vx_selftest(self._h, _ptr(r)), "vx_selftest")
        return r

    def _ray_lib(self):
        if not self._L.has_raycast:
            raise VoxelsHipError("%s has no ray casts (vx_raycast*)" % self._L.path)
        return self._lib

    def raycast_prepare(self, level=0):
        """vx_raycast_prepare: build the level's ray-cast index (or keep it if current); its figures as a dict."""
        info = RayIndexInfo()
        self._check(self._ray_lib().vx_raycast_prepare(self._h, int(level), C.byref(info)), "vx_raycast_prepare")
        return {"triangles": int(info.triangles), "bytes": int(info.bytes), "blocks": int(info.blocks),
                "straddling": int(info.straddling), "build_ms": float(info.build_ms)}

    def raycast_device(self, d_rays, n, d_hits, level=0):
        """vx_raycast_device: n rays at device address d_rays (RAY_DTYPE records, 16-byte aligned) -> d_hits (HIT_DTYPE), queued on
        the context's stream (set_stream) without waiting.  Addresses are ints, e.g. tensor.data_ptr()."""
        self._check(self._ray_lib().vx_raycast_device(self._h, int(level), C.c_void_p(d_rays), int(n), C.c_void_p(d_hits)), "vx_raycast_device")

    def raycast_rays(self, rays, level=0):
        """vx_raycast on a RAY_DTYPE array -> HIT_DTYPE array (synchronous)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(rays.size, HIT_DTYPE)
        self._check(self._ray_lib().vx_raycast(self._h, int(level), _ptr(rays) if rays.size else None, rays.size,
                                               _ptr(hits) if rays.size else None), "vx_raycast")
        return hits

    def raycast(self, origins, dirs, t_min=0.0, t_max=float("inf"), level=0):
        """Nearest hit of each ray o + t d (t_min <= t <= t_max, t in units of |d|) with the regular meshes of one level, in
        mesh space (Y-up, voxels): a HIT_DTYPE array (misses: t = inf, entry = block_id = tri = RAY_NONE)."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        n = max(len(origins), len(dirs))
        rays = np.zeros(n, RAY_DTYPE)
        rays["origin"], rays["dir"] = origins, dirs
        rays["t_min"], rays["t_max"] = t_min, t_max
        return self.raycast_rays(rays, level)

    def _shape_lib(self):
        if not self._L.has_shapecast:
            raise VoxelsHipError("%s has no sphere casts or closest points (vx_spherecast*, vx_closest_point*)" % self._L.path)
        return self._L.lib

    def spherecast_device(self, d_casts, n, d_hits, level=0):
        """vx_spherecast_device: n casts at device address d_casts (SPHERE_CAST_DTYPE records, 16-byte aligned) -> d_hits
        (SPHERE_HIT_DTYPE), queued on the context's stream."""
        self._check(self._shape_lib().vx_spherecast_device(self._h, int(level), C.c_void_p(d_casts), int(n), C.c_void_p(d_hits)),
                    "vx_spherecast_device")

    def spherecast_casts(self, casts, level=0):
        """vx_spherecast on a SPHERE_CAST_DTYPE array -> SPHERE_HIT_DTYPE array (synchronous)."""
        casts = np.ascontiguousarray(casts, SPHERE_CAST_DTYPE)
        hits = np.zeros(casts.size, SPHERE_HIT_DTYPE)
        self._check(self._shape_lib().vx_spherecast(self._h, int(level), _ptr(casts) if casts.size else None, casts.size,
                                                    _ptr(hits) if casts.size else None), "vx_spherecast")
        return hits

    def spherecast(self, origins, dirs, radius, t_min=0.0, t_max=float("inf"), level=0):
        """First contact of a sphere of `radius` (a scalar or one per cast) whose centre moves along o + t d (t_min <= t <= t_max,
        t in units of |d|) with the regular meshes of one level, in mesh space (Y-up, voxels): a SPHERE_HIT_DTYPE array (misses:
        t = inf, entry = block_id = tri = RAY_NONE)."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        n = max(len(origins), len(dirs))
        casts = np.zeros(n, SPHERE_CAST_DTYPE)
        casts["origin"], casts["dir"] = origins, dirs
        casts["t_min"], casts["t_max"], casts["radius"] = t_min, t_max, radius
        return self.spherecast_casts(casts, level)

    def closest_points_device(self, d_queries, n, d_hits, level=0):
        """vx_closest_point_device: n queries at device address d_queries (POINT_QUERY_DTYPE, 16-byte aligned) -> d_hits
        (POINT_HIT_DTYPE), queued on the context's stream."""
        self._check(self._shape_lib().vx_closest_point_device(self._h, int(level), C.c_void_p(d_queries), int(n), C.c_void_p(d_hits)),
                    "vx_closest_point_device")

    def closest_points_queries(self, queries, level=0):
        """vx_closest_point on a POINT_QUERY_DTYPE array -> POINT_HIT_DTYPE array (synchronous)."""
        queries = np.ascontiguousarray(queries, POINT_QUERY_DTYPE)
        hits = np.zeros(queries.size, POINT_HIT_DTYPE)
        self._check(self._shape_lib().vx_closest_point(self._h, int(level), _ptr(queries) if queries.size else None, queries.size,
                                                       _ptr(hits) if queries.size else None), "vx_closest_point")
        return hits

    def closest_points(self, points, max_dist=float("inf"), level=0):
        """Nearest point of the regular meshes of one level to each point, if within max_dist (a scalar or one per point), in mesh
        space: a POINT_HIT_DTYPE array (nothing within max_dist: dist = inf, entry = block_id = tri = RAY_NONE)."""
        points = np.asarray(points, np.float32).reshape(-1, 3)
        q = np.zeros(len(points), POINT_QUERY_DTYPE)
        q["pos"], q["max_dist"] = points, max_dist
        return self.closest_points_queries(q, level)

    def _lod_lib(self):
        if not self._L.has_lod:
            raise VoxelsHipError("%s has no LOD selection (vx_lod_select*)" % self._L.path)
        return self._L.lib

    def lod_select(self, camera, ranges=None, planes=None):
        """vx_lod_select: (draws LOD_DRAW_DTYPE, regular DRAW_INDEXED_DTYPE, transition DRAW_INDEXED_DTYPE, counts dict) for a
        mesh-space camera, ranges (16 floats, default lod_ranges()) and up to 6 frustum planes (a, b, c, d)."""
        lib = self._lod_lib()
        prm = lod_params(camera, ranges, planes)
        cap = sum(self.device_block_table(L)[1] for L in range(self.info.levels)) if getattr(self, "info", None) else 0
        tcap = cap
        for attempt in range(2):
            draws, regular = np.zeros(cap, LOD_DRAW_DTYPE), np.zeros(cap, DRAW_INDEXED_DTYPE)
            transition, counts = np.zeros(tcap, DRAW_INDEXED_DTYPE), np.zeros(1, LOD_COUNTS_DTYPE)
            rc = lib.vx_lod_select(self._h, _ptr(prm), cap, tcap, _ptr(draws) if cap else None, _ptr(regular) if cap else None,
                                   _ptr(transition) if tcap else None, _ptr(counts))
            if rc == -3 and attempt == 0:
                cap, tcap = max(cap, int(counts["records"][0])), max(tcap, int(counts["transition"][0]))
                continue
            self._check(rc, "vx_lod_select")
            break
        c = {k: int(counts[k][0]) for k in LOD_COUNTS_DTYPE.names}
        return draws[:c["records"]], regular[:c["records"]], transition[:c["transition"]], c

    def lod_select_device(self, params, draw_capacity, transition_capacity, d_draws, d_regular, d_transition, d_counts):
        """vx_lod_select_device: params = a LOD_PARAMS_DTYPE record (lod_params()), arrays at device addresses (ints, 16-byte
        aligned); queued on the context's stream (set_stream), returns without waiting."""
        prm = np.ascontiguousarray(params, LOD_PARAMS_DTYPE)
        self._check(self._lod_lib().vx_lod_select_device(self._h, _ptr(prm), int(draw_capacity), int(transition_capacity),
                                                         C.c_void_p(d_draws), C.c_void_p(d_regular), C.c_void_p(d_transition),
                                                         C.c_void_p(d_counts)), "vx_lod_select_device")

    def _scatter_lib(self):
        if not self._L.has_scatter:
            raise VoxelsHipError("%s has no scattering (vx_scatter*)" % self._L.path)
        return self._L.lib

    def scatter_raw(self, level, params, capacity):
        """one vx_scatter call: (return code, points SCATTER_POINT_DTYPE[capacity], ranges SCATTER_RANGE_DTYPE, counts record)"""
        lib = self._scatter_lib()
        prm = np.ascontiguousarray(params, SCATTER_PARAMS_DTYPE)
        points, counts = np.zeros(int(capacity), SCATTER_POINT_DTYPE), np.zeros(1, SCATTER_COUNTS_DTYPE)
        ranges = np.zeros(self.device_block_table(level)[1], SCATTER_RANGE_DTYPE)
        rc = lib.vx_scatter(self._h, int(level), _ptr(prm), int(capacity), _ptr(points) if capacity else None, _ptr(ranges), _ptr(counts))
        return rc, points, ranges, counts[0]

    def scatter(self, level, params, capacity=None):
        """vx_scatter: (points SCATTER_POINT_DTYPE, ranges SCATTER_RANGE_DTYPE per table entry, counts dict) for a
        SCATTER_PARAMS_DTYPE record (scatter_params()).  capacity None: two calls, the counts first, then the fill; with a
        capacity, at most that many points come back (counts["points"] says how many there are)."""
        cap = capacity
        if cap is None:
            rc, _, _, counts = self.scatter_raw(level, params, 0)
            if rc != -3:
                self._check(rc, "vx_scatter")
            if int(counts["points"]) > 0xFFFFFFFF:
                raise VoxelsHipError("vx_scatter: %d points do not fit a 32-bit capacity" % int(counts["points"]))
            cap = int(counts["points"])
        rc, points, ranges, counts = self.scatter_raw(level, params, cap)
        if rc != -3 or capacity is None:
            self._check(rc, "vx_scatter")
        c = {k: int(counts[k]) for k in SCATTER_COUNTS_DTYPE.names}
        return points[:min(c["points"], cap)], ranges, c

    def scatter_device(self, level, params, capacity, d_points, d_ranges, d_counts):
        """vx_scatter_device: params = a SCATTER_PARAMS_DTYPE record (scatter_params()), arrays at device addresses (ints, 16-byte
        aligned, d_ranges 8 or None); queued on the context's stream (set_stream), returns without waiting."""
        prm = np.ascontiguousarray(params, SCATTER_PARAMS_DTYPE)
        self._check(self._scatter_lib().vx_scatter_device(self._h, int(level), _ptr(prm), int(capacity), C.c_void_p(d_points),
                                                          C.c_void_p(d_ranges), C.c_void_p(d_counts)), "vx_scatter_device")

    def _overlap_lib(self):
        if not self._L.has_overlap:
            raise VoxelsHipError("%s has no overlap queries (vx_overlap_boxes*)" % self._L.path)
        return self._L.lib

    def overlap_boxes_raw(self, level, boxes, capacity, corners=False):
        """one vx_overlap_boxes call: (return code, tris OVERLAP_TRI_DTYPE[capacity], corners float32 [capacity, 3, 4] or None,
        ranges OVERLAP_RANGE_DTYPE per query, counts record); capacity 0 is the count-only form"""
        lib = self._overlap_lib()
        boxes = np.ascontiguousarray(boxes, OVERLAP_BOX_DTYPE).reshape(-1)
        cap = int(capacity)
        tris, counts = np.zeros(cap, OVERLAP_TRI_DTYPE), np.zeros(1, OVERLAP_COUNTS_DTYPE)
        crn = np.zeros((cap, 3, 4), np.float32) if corners and cap else None
        ranges = np.zeros(boxes.size, OVERLAP_RANGE_DTYPE)
        rc = lib.vx_overlap_boxes(self._h, int(level), _ptr(boxes) if boxes.size else None, boxes.size, cap, _ptr(tris) if cap else None,
                                  None if crn is None else _ptr(crn), _ptr(ranges) if boxes.size else None, _ptr(counts))
        return rc, tris, crn, ranges, counts[0]

    def overlap_boxes(self, level, boxes, capacity=None, corners=False):
        """vx_overlap_boxes: the regular triangles of a level whose bounding boxes meet each of the closed query boxes
        (overlap_boxes(lo, hi)), ordered by query, coord_id, tri: (tris OVERLAP_TRI_DTYPE, corners float32 [k, 3, 4] or None,
        ranges OVERLAP_RANGE_DTYPE per query, counts dict).  capacity None: two calls, the counts first, then the fill; with
        a capacity, at most that many results come back (counts["triangles"] says how many there are)."""
        cap = capacity
        if cap is None:
            rc, _, _, _, counts = self.overlap_boxes_raw(level, boxes, 0)
            if rc != -3:
                self._check(rc, "vx_overlap_boxes")
            if int(counts["triangles"]) > 0xFFFFFFFF:
                raise VoxelsHipError("vx_overlap_boxes: %d results do not fit a 32-bit capacity" % int(counts["triangles"]))
            cap = int(counts["triangles"])
        rc, tris, crn, ranges, counts = self.overlap_boxes_raw(level, boxes, cap, corners)
        if rc != -3 or capacity is None:
            self._check(rc, "vx_overlap_boxes")
        c = {k: int(counts[k]) for k in OVERLAP_COUNTS_DTYPE.names}
        filled = min(c["triangles"], cap)
        if corners and crn is None:
            crn = np.zeros((0, 3, 4), np.float32)
        return tris[:filled], None if crn is None else crn[:filled], ranges, c

    def overlap_boxes_device(self, level, d_boxes, n, capacity, d_tris, d_corners, d_ranges, d_counts):
        """vx_overlap_boxes_device: n OVERLAP_BOX_DTYPE boxes at device address d_boxes, arrays at device addresses (ints, 16-byte
        aligned, d_ranges 8; d_corners and d_ranges may be None, d_tris with capacity 0); queued on the context's stream
        (set_stream), returns without waiting."""
        self._check(self._overlap_lib().vx_overlap_boxes_device(self._h, int(level), C.c_void_p(d_boxes), int(n), int(capacity),
                                                                C.c_void_p(d_tris), C.c_void_p(d_corners), C.c_void_p(d_ranges),
                                                                C.c_void_p(d_counts)), "vx_overlap_boxes_device")

    def stats(self):
        out = np.zeros(20, np.uint32)
        self._check(self._lib.vx_stats(self._h, _ptr(out)), "vx_stats")
        return out

    def transition_path_counts(self):
        """vx_transition_path_counts: (table_driven, fallback) transition blocks of the last run."""
        out = np.zeros(2, np.uint32)
        self._check(self._lib.vx_transition_path_counts(self._h, _ptr(out)), "vx_transition_path_counts")
        return int(out[0]), int(out[1])

    def material_path_counts(self):
        """vx_material_path_counts: (voted, replayed) material blocks of the last full run."""
        if not self._L.has_material_path_counts:
            raise VoxelsHipError("this library has no vx_material_path_counts")
        out = np.zeros(2, np.uint32)
        self._check(self._lib.vx_material_path_counts(self._h, _ptr(out)), "vx_material_path_counts")
        return int(out[0]), int(out[1])

    def slot_plan_counts(self):
        """vx_slot_plan_counts: (handed out, kept) - the full runs of this context by where their slots came from, cumulative."""
        if not self._L.has_slot_plan:
            raise VoxelsHipError("this library has no vx_slot_plan_counts")
        out = np.zeros(2, np.uint64)
        self._check(self._lib.vx_slot_plan_counts(self._h, _ptr(out)), "vx_slot_plan_counts")
        return int(out[0]), int(out[1])

    def material_inplace_counts(self):
        """vx_material_inplace_counts: (copied, left in place) - the full-run attempts of this context whose material blocks were
        replayed, by how, cumulative.  HIP builds only: the CPU emulation library has no such entry point."""
        if not self._L.has_material_inplace:
            raise VoxelsHipError("this library has no vx_material_inplace_counts")
        out = np.zeros(2, np.uint64)
        self._check(self._lib.vx_material_inplace_counts(self._h, _ptr(out)), "vx_material_inplace_counts")
        return int(out[0]), int(out[1])

    def layout_keep_counts(self):
        """vx_layout_keep_counts: (two launches, one launch) - the full-run attempts of this context that kept the slot plan, by
        whether they also kept the mesh layout, cumulative.  HIP builds only: the CPU emulation library has no such entry point."""
        if not self._L.has_layout_keep:
            raise VoxelsHipError("this library has no vx_layout_keep_counts")
        out = np.zeros(2, np.uint64)
        self._check(self._lib.vx_layout_keep_counts(self._h, _ptr(out)), "vx_layout_keep_counts")
        return int(out[0]), int(out[1])

    def index_keep_counts(self):
        """vx_index_keep_counts: (indices rewritten, indices kept) - the full-run attempts of this context that kept the mesh layout,
        by what they did with the index pool, cumulative.  HIP builds only: the CPU emulation library has no such entry point."""
        if not self._L.has_index_keep:
            raise VoxelsHipError("this library has no vx_index_keep_counts")
        out = np.zeros(2, np.uint64)
        self._check(self._lib.vx_index_keep_counts(self._h, _ptr(out)), "vx_index_keep_counts")
        return int(out[0]), int(out[1])

    def geometry_keep_counts(self):
        """vx_geometry_keep_counts: (whole vertices stored, texture bytes only) - the full-run attempts of this context that kept the
        mesh layout, by what they did with the regular vertices, cumulative.  HIP builds only: the CPU emulation library has no such
        entry point."""
        if not self._L.has_geometry_keep:
            raise VoxelsHipError("this library has no vx_geometry_keep_counts")
        out = np.zeros(2, np.uint64)
        self._check(self._lib.vx_geometry_keep_counts(self._h, _ptr(out)), "vx_geometry_keep_counts")
        return int(out[0]), int(out[1])
