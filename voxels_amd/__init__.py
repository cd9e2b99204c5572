"""voxels_amd — MI355X-native TransVoxel polygonizer (drop-in for stoyannk/voxels' Polygonizer::Execute path).

The compute path is hand-written HIP for gfx950 in voxels_amd/csrc (libvoxels_hip.so, C ABI in
include/voxels_hip.h).  This package is the thin Python host side used by tests and bench.py: it mirrors
the reference's operator interface for the path (Grid -> Polygonizer.Execute -> PolygonSurface levels/blocks)
and fails loudly when the HIP library is missing — there is no CPU fallback.
"""
from .binding import (BLOCK_INFO_DTYPE, BOX_DTYPE, DRAW_INDEXED_DTYPE, HIT_DTYPE, LOD_COUNTS_DTYPE, LOD_DRAW_DTYPE, OVERLAP_BOX_DTYPE, OVERLAP_COUNTS_DTYPE,
                      OVERLAP_MAX_QUERIES, OVERLAP_RANGE_DTYPE, OVERLAP_TRI_DTYPE, POINT_HIT_DTYPE,
                      POINT_QUERY_DTYPE, RAY_DTYPE, RECORD_INFO_DTYPE, RECORD_MAX_BLOCKS, RECORD_MAX_BOXES, SCATTER_COUNTS_DTYPE, SCATTER_PARAMS_DTYPE, SCATTER_POINT_DTYPE,
                      SCATTER_RANGE_DTYPE, SPHERE_CAST_DTYPE, SPHERE_HIT_DTYPE, SWAP_RESULT_DTYPE, VERTEX_DTYPE, WALK_COUNTS_DTYPE,
                      WALK_GOAL_DTYPE, WALK_MAX_GOALS, WALK_QUERY_DTYPE, WALK_UNREACHED, HipLibrary, Level, Polygonizer, Record, VoxelsHipError,
                      brush_boxes, hip_library_path, lod_params, lod_ranges, overlap_boxes, scatter_params, walk_query,
                      PASTE_COUNTS_DTYPE, PASTE_DTYPE, PASTE_MAX_COUNT, PASTE_MAX_STAMPS, PASTE_PAINT, PASTE_REPLACE, PASTE_RESULT_DTYPE, PASTE_SUBTRACT, PASTE_UNION,
                      STAMP_INFO_DTYPE, STAMP_MAX_EDGE, STAMP_MAX_VOXELS, Stamp, paste_boxes, pastes,
                      MEASURE_DTYPE, MEASURE_MAX_BOXES, RECORD_DELTA_DTYPE,
                      HEIGHT_COUNTS_DTYPE, HEIGHT_COUNT_SURFACES, HEIGHT_FROM_BOTTOM, HEIGHT_FROM_TOP, HEIGHT_MAX_LAYERS, HEIGHT_NONE, HEIGHT_QUERY_DTYPE, height_query,
                      OCCLUSION_COUNTS_DTYPE, OCCLUSION_MAX_STEPS, OCCLUSION_PARAMS_DTYPE, OCCLUSION_TRANSITIONS, occlusion_params)

__all__ = ["BLOCK_INFO_DTYPE", "BOX_DTYPE", "DRAW_INDEXED_DTYPE", "HIT_DTYPE", "LOD_COUNTS_DTYPE", "LOD_DRAW_DTYPE", "POINT_HIT_DTYPE", "POINT_QUERY_DTYPE",
           "RAY_DTYPE", "SCATTER_COUNTS_DTYPE", "SCATTER_PARAMS_DTYPE", "SCATTER_POINT_DTYPE", "SCATTER_RANGE_DTYPE", "SPHERE_CAST_DTYPE", "SPHERE_HIT_DTYPE", "VERTEX_DTYPE",
           "WALK_COUNTS_DTYPE", "WALK_GOAL_DTYPE", "WALK_MAX_GOALS", "WALK_QUERY_DTYPE", "WALK_UNREACHED",
           "RECORD_INFO_DTYPE", "RECORD_MAX_BLOCKS", "RECORD_MAX_BOXES", "SWAP_RESULT_DTYPE", "Record", "brush_boxes",
           "HipLibrary", "Level", "Polygonizer", "VoxelsHipError", "hip_library_path", "lod_params", "lod_ranges", "scatter_params", "walk_query",
           "OVERLAP_BOX_DTYPE", "OVERLAP_TRI_DTYPE", "OVERLAP_RANGE_DTYPE", "OVERLAP_COUNTS_DTYPE", "OVERLAP_MAX_QUERIES", "overlap_boxes",
           "STAMP_INFO_DTYPE", "PASTE_DTYPE", "PASTE_RESULT_DTYPE", "PASTE_COUNTS_DTYPE", "STAMP_MAX_EDGE", "STAMP_MAX_VOXELS", "PASTE_MAX_COUNT", "PASTE_MAX_STAMPS",
           "PASTE_REPLACE", "PASTE_UNION", "PASTE_SUBTRACT", "PASTE_PAINT", "Stamp", "paste_boxes", "pastes",
           "MEASURE_DTYPE", "RECORD_DELTA_DTYPE", "MEASURE_MAX_BOXES",
           "HEIGHT_QUERY_DTYPE", "HEIGHT_COUNTS_DTYPE", "HEIGHT_MAX_LAYERS", "HEIGHT_NONE", "HEIGHT_FROM_TOP", "HEIGHT_FROM_BOTTOM", "HEIGHT_COUNT_SURFACES", "height_query",
           "OCCLUSION_PARAMS_DTYPE", "OCCLUSION_COUNTS_DTYPE", "OCCLUSION_MAX_STEPS", "OCCLUSION_TRANSITIONS", "occlusion_params"]
