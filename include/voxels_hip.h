/* voxels_hip.h — C ABI of libvoxels_hip.so, the MI355X (gfx950) TransVoxel polygonizer.
 *
 * This is the drop-in boundary for the reference's polygonization path.  The reference has no C interface
 * below Polygonizer::Execute (include/Polygonizer.h:230-232 -> src/TransVoxelImpl.cpp:74-79, :2153-2169,
 * TransVoxelRun::Execute :468-538); the entry points below are what a host binding of that call needs:
 * the C++ host layer of this repo (include/Voxels.h, voxels_amd/csrc/vx_api_cpp.cpp) implements
 * Voxels::Polygonizer::Execute on top of them, and INTEGRATION.md shows the equivalent patch to the
 * reference's own TransVoxelImpl::Execute.
 *
 * Conventions: plain pointers and sizes only; every function returns VX_OK (0) or a negative VX_ERR_* code and
 * never throws; vx_last_error() gives a message.  Grids are cubes of edge n (multiple of 16), Z-up, dense,
 * x fastest: index (z*n + y)*n + x (reference: src/VoxelGrid.h:31-35).  Output is Y-up, exactly the bytes of
 * Voxels::PolygonVertex / BlockPolygons (include/Polygonizer.h:14-106).  One polygonization at a time per
 * context (the reference has the same restriction, src/TransVoxelImpl.cpp:2144).
 */
#ifndef VOXELS_HIP_H
#define VOXELS_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_OK 0
#define VX_ERR_INVALID (-1)   /* bad argument or call order */
#define VX_ERR_DEVICE (-2)    /* HIP runtime error (no GPU, out of memory, launch failure) */
#define VX_ERR_OVERFLOW (-3)  /* output pools could not be grown */

typedef struct vx_ctx vx_ctx;

/* 48 bytes, bit-identical to Voxels::PolygonVertex (include/Polygonizer.h:14-48) */
typedef struct vx_vertex {
	float pos[3];
	float sec[4];     /* sec[3]: transition-face adjacency mask as raw integer bits */
	float nrm[3];
	uint8_t tex[8];   /* Reserved, Blend, Uxz, Txz, Uny, Upy, Tny, Tpy */
} vx_vertex;

/* One emitted block = one Voxels::BlockPolygons (include/Polygonizer.h:52-106) */
typedef struct vx_block_info {
	uint32_t id;            /* BlockPolygons::GetId */
	uint32_t n_verts;       /* GetVertices count */
	uint32_t n_idx;         /* GetIndices count */
	uint32_t n_tverts[6];   /* GetTransitionVertices count per TransitionFaceId */
	uint32_t n_tidx[6];     /* GetTransitionIndices count per TransitionFaceId */
	float min_corner[3];    /* GetMinimalCorner */
	float max_corner[3];    /* GetMaximalCorner */
} vx_block_info;

typedef struct vx_exec_info {
	uint32_t levels;            /* LOD levels produced (PolygonSurface::GetLevelsCount) */
	uint32_t retries;           /* re-runs after growing the output pools */
	float device_ms;            /* device time of the last run, always > 0.  A full run on the single-stream path (three launches,
	                             * or two while the slot plan is kept - then the first kernel is k_main, vx_slot_plan_counts -
	                             * or k_main alone, vx_layout_keep_counts; stage timing off): the device's constant 100 MHz clock, from the moment the first workgroup of
	                             * the first kernel starts to the publication of the run's header by the last kernel - a few
	                             * microseconds less than the interval between two HIP events around the same launches, which also
	                             * holds the first kernel's dispatch and the rest of the last kernel after the publication.  Every
	                             * other run (the chain of launches, stage timing, VX_HOST_TIMING, incremental runs): that pair of
	                             * HIP events on the context's stream. */
	uint64_t total_verts;       /* the vertex pool's cursor: vertices of all meshes (regular + transition, incl. blocks dropped as
	                             * empty) PLUS the ranges a table-driven block of a level >= 1 had reserved when it turned out to
	                             * hold a zero sample and was handed to the general pass (a handful of blocks per run; the
	                             * general pass reserves again).  Byte figures derived from meshes - bench.py's roofline,
	                             * mesh_bytes - sum the blocks' own counts (vx_download_level / vx_level_counts), not this. */
	uint64_t total_indices;     /* the index pool's cursor, likewise */
	uint32_t active_blocks[8];  /* surface-bearing blocks per level */
	uint64_t algorithmic_bytes; /* n^3 + 2*4096*surface blocks + 48*V + 4*I */
	uint32_t blocks_read;       /* level-0 blocks whose distance samples the run had to read (the others are proven
	                               surface-free by the BF_Empty flags of their 27-neighbourhood); 0 for incremental runs */
	float mirror_ms;            /* device time this call spent bringing the library's mirrors of the grid up to date (brick
	                               order, lattice copies, sign summaries: the one place where all n^3 samples are read) —
	                               0 when the grid did not change since the last run; not part of device_ms */
	uint32_t first_meshed_level; /* 0 for an ordinary run; vx_polygonize_from: the first level whose meshes the run produced */
} vx_exec_info;

/* ---- context ------------------------------------------------------------------------------------------- */
/* Number of HIP devices this process sees (0 and VX_ERR_DEVICE when there is none). */
int vx_device_count(int* count);
int vx_ctx_create(int device_index, vx_ctx** out);
void vx_ctx_destroy(vx_ctx* ctx);
const char* vx_last_error(const vx_ctx* ctx);
/* Run on a caller-provided hipStream_t (e.g. PyTorch's current stream); NULL = the context's own stream. */
int vx_set_stream(vx_ctx* ctx, void* hip_stream);

/* ---- grid residency (what TransVoxelRun reads through VoxelGrid::GetBlockData / GetMaterialBlockData /
 *      IsBlockEmpty, src/VoxelGrid.cpp:586-608) ------------------------------------------------------------ */
/* Copy a whole host grid to the device. empty_flags[(n/16)^3] = BF_Empty of every block in block-id order
 * (src/VoxelGrid.h:139-144); mat/blend may be NULL (all zero). */
int vx_grid_upload(vx_ctx* ctx, uint32_t n, const int8_t* dist, const uint8_t* mat, const uint8_t* blend,
                   const uint8_t* empty_flags);
/* Grid::Create(w, heightmap) (src/VoxelGrid.cpp:159-213) evaluated on the device: heightmap = w*w signed bytes, row = y;
 * distance(x,y,z) = clamp((z - 127) - heightmap[y][x], -127, 127) squeezed to the grid's +-4 range, materials 0; BF_Empty of
 * every block by the codec's rule.  Only the w*w bytes cross PCIe. */
int vx_grid_create_heightmap(vx_ctx* ctx, uint32_t w, const int8_t* heightmap);
/* The same, from the Grid file format v1 (what Grid::PackForSave writes and Grid::Load reads, src/VoxelGrid.cpp:215-315):
 * header {1, w, d, h}, 3 stream sizes per block, then per block in id order {flags, distance stream, material stream,
 * blend stream}; a stream is RLE pairs (u8 run length, value) or 4096 raw bytes when its BF_*Uncompressed flag is set
 * (CompressBlock / DecompressBlock, :610-694).  The blob goes to the device as it is and is expanded there; BF_Empty
 * comes from the per-block flags.  Replaces Grid::Load + vx_grid_upload (no host decode, no 3 bytes/voxel transfer). */
int vx_grid_upload_packed(vx_ctx* ctx, const void* blob, uint64_t size);
/* The resident grid as a Grid file (Grid::PackForSave, src/VoxelGrid.cpp:269-315): every block is run-length encoded on
 * the device by the codec's rules (runs of at most 255; a stream whose code would exceed 4096 bytes is stored raw and
 * flagged), the file is assembled in `out`.  Byte-identical to what the reference writes for the same grid.
 * *size receives the file size; with out == NULL (or capacity too small: VX_ERR_INVALID) nothing is written. */
int vx_grid_pack(vx_ctx* ctx, void* out, uint64_t capacity, uint64_t* size);
/* One 16^3 block of the resident grid back to the host, x fastest (Grid::GetBlockDistanceData / GetBlockMaterialData,
 * src/VoxelGrid.cpp:586-608); any output may be NULL.  empty_flag receives BF_Empty. */
int vx_grid_read_block(vx_ctx* ctx, uint32_t block_id, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* empty_flag);
/* Use caller-owned DEVICE memory (multi-GPU slabs, PyTorch tensors).  This rank polygonizes the z-range
 * [z_begin, z_end) of the global n^3 grid.  d_dist holds the z-planes [dist_z0, ...) and must cover
 * [z_begin-1, z_end+1] clamped to the grid; d_mat/d_blend hold planes [mat_z0, ...) covering [z_begin, z_end]
 * clamped.  d_empty_flags is the FULL (n/16)^3 flag array (neighbour layers of other ranks included). */
/* The library keeps brick-ordered mirrors of the fields for its gathers and refreshes them where IT changes
 * the grid (vx_grid_fill_terrain, vx_halo_exchange*).  A caller that rewrites attached memory itself after a
 * polygonization has run must call vx_grid_invalidate (below) — or attach again — before the next one; otherwise that run
 * silently polygonizes the OLD contents (nothing detects the staleness). */
int vx_grid_attach(vx_ctx* ctx, uint32_t n, uint32_t z_begin, uint32_t z_end,
                   const void* d_dist, int32_t dist_z0, const void* d_mat, const void* d_blend, int32_t mat_z0,
                   const void* d_empty_flags);
/* The same for a slab cut along y (the usual choice for terrains: a height field puts nearly all of its surface into a
 * few z-layers, so z-slabs leave most ranks idle): this rank polygonizes the rows [y_begin, y_end) of every z-plane.
 * d_dist is [n planes][dist_rows rows][n] with row 0 = global y dist_y0 and must cover [y_begin-1, y_end+1] clamped;
 * d_mat / d_blend are [n][mat_rows][n] with row 0 = global y mat_y0 covering [y_begin, y_end] clamped. */
int vx_grid_attach_y(vx_ctx* ctx, uint32_t n, uint32_t y_begin, uint32_t y_end,
                     const void* d_dist, int32_t dist_y0, uint32_t dist_rows,
                     const void* d_mat, const void* d_blend, int32_t mat_y0, uint32_t mat_rows, const void* d_empty_flags);
/* A slab of rows of a HOST grid onto the device, halo included: the context polygonizes the rows [y_begin, y_end) of every
 * z-plane of the whole n^3 host grid `dist` / `mat` / `blend` (layout of vx_grid_upload; mat / blend may be NULL) and copies
 * what that takes - distance rows [y_begin - 1, y_end + 2), material and blend rows [y_begin, y_end + 1), clamped to the grid,
 * and all BF_Empty flags - into memory of its own (strided copies straight from the host arrays: a host that owns the whole
 * Voxels::Grid needs no halo exchange between its devices).  Afterwards the context is in the state vx_grid_attach_y leaves
 * it in.  What a multi-device Polygonizer::Execute calls once per device (voxels_amd/csrc/vx_api_cpp.cpp). */
int vx_grid_upload_slab_y(vx_ctx* ctx, uint32_t n, uint32_t y_begin, uint32_t y_end, const int8_t* dist, const uint8_t* mat,
                          const uint8_t* blend, const uint8_t* empty_flags);
/* Tell the library that the caller rewrote the resident (attached) fields in place — the zero-copy use of
 * vx_grid_attach*, where the application edits its own device tensors (the reference's Grid::Modify*BlockData on
 * memory the library does not own).  The mirrors are rebuilt by the next polygonization; the emptiness flags stay the
 * caller's business, as with vx_grid_attach. */
int vx_grid_invalidate(vx_ctx* ctx);
/* One entry of the cell map, a mirror the library keeps with the others: the 4096-bit bitmap of the
 * non-trivial cells of level-0 block (bx, by, bz) - bit x | y << 4 | z << 8 of out[128], i.e. the 16-bit row (z << 4) | y - and
 * its population count.  A cell is non-trivial unless its eight corner samples agree in sign; a zero counts as >= 0,
 * coordinates are clamped to the grid; the BF_Empty flags play no part.  Full runs on the single-stream path read the map
 * instead of forming bitmaps; it is rebuilt by the first such run after the grid changed - and by this call, which brings it
 * up to date if it is stale and copies one entry.  A block whose samples and the neighbour samples its cells reach are of one
 * sign returns zeros and count 0.  Either output may be NULL.  Bringing the map up to date includes the other mirrors: on a
 * grid that changed as a whole (upload, attach, vx_grid_invalidate) this call pays their rebuild, and the next
 * vx_polygonize reports a mirror_ms without it.  VX_ERR_INVALID for a block outside the context's range and
 * for a context that keeps no map: VX_CELLMAP=0 or a knob that rules out the single-stream path (read when the context is
 * created), a grid beyond 1024^3, or a backend without mirrors.  No reference counterpart. */
int vx_grid_cell_map(vx_ctx* ctx, uint32_t bx, uint32_t by, uint32_t bz, uint32_t out[128], uint32_t* count);
/* Forget what earlier runs of this context learned about ITS surfaces - which capacity classes to launch, how many blocks the
 * general passes take over, how many upper-queue items a run has: the next run starts from the conservative defaults of a new
 * context (all capacity classes launched).  For a context that is handed to another owner with another grid (libVoxels.so:
 * the context InitializeVoxels warmed up on a toy terrain, adopted by the application's first Polygonizer).  No reference
 * counterpart: the reference keeps no state between Execute calls beyond the PolygonSurface itself. */
int vx_ctx_forget_hints(vx_ctx* ctx);
/* ---- generation on the device ------------------------------------------------------------------------------------------
 * Grid::Create(w, h, d, ..., VoxelSurface*) samples an application callback on the host (src/VoxelGrid.cpp:79-132) and
 * quantises the samples (:37-50).  For the benchmark's synthetic surface (include/voxels_synth.h, vxs_terrain) the same
 * step runs where the grid lives: the fields are byte for byte what vxs_terrain + vxs_block_empty_flags produce on the
 * host, without 3 n^3 bytes crossing PCIe.
 * vx_grid_create_terrain: a whole n^3 grid owned by the context (like vx_grid_upload).
 * vx_grid_fill_terrain: the slab attached with vx_grid_attach / vx_grid_attach_y — every resident layer that lies
 * inside the grid (the halo included) and the BF_Empty flags of the rank's own blocks (the neighbours' flag layers come
 * with vx_halo_exchange). */
int vx_grid_create_terrain(vx_ctx* ctx, uint32_t n, uint32_t seed);
/* style as in vxs_terrain_ex (include/voxels_synth.h): 0 = the terrain, 1 = "caves" (surface in a large share of all blocks) */
int vx_grid_create_terrain_ex(vx_ctx* ctx, uint32_t n, uint32_t seed, uint32_t style);
int vx_grid_fill_terrain(vx_ctx* ctx, uint32_t seed);

/* ---- multi-GPU: halo exchange of attached slabs -------------------------------------------
 * The reference has one address space and an OpenMP block loop (src/TransVoxelImpl.cpp:500-503); here the grid is cut
 * into slabs (vx_grid_attach / vx_grid_attach_y), one per GPU, rank r owning the r-th slab along the cut axis.  What a
 * rank reads beyond its own layers (a layer = a z-plane, or the y-row of every plane) comes from its neighbours:
 *   from the slab above: 2 distance layers, 1 material layer, 1 blend layer, the BF_Empty flags of its first block layer
 *   from the slab below: 1 distance layer, the BF_Empty flags of its last block layer
 * The attached buffers must have exactly that halo (dist_z0 = z_begin - 1 with 3 layers more than the slab, mat_z0 =
 * z_begin with 1 more; likewise along y), as voxels_amd/slab.py lays them out.
 *
 * vx_halo_exchange: one process per GPU.  vx_comm_init joins an RCCL communicator (the id comes from
 * vx_comm_unique_id on rank 0 and travels by whatever means the launcher has); the exchange is one grouped
 * ncclSend/ncclRecv batch per call on the context's stream with pack / unpack kernels around it — no host wait.
 * vx_halo_exchange_group: one process driving several contexts (one per GPU, or several slabs on one GPU): the same
 * packing with peer copies as transport; contexts in slab order. */
#define VX_COMM_ID_BYTES 128
int vx_comm_unique_id(void* id /* VX_COMM_ID_BYTES bytes out */);
int vx_comm_init(vx_ctx* ctx, int nranks, int rank, const void* id /* VX_COMM_ID_BYTES bytes */);
int vx_comm_destroy(vx_ctx* ctx);
int vx_halo_exchange(vx_ctx* ctx);
int vx_halo_exchange_group(vx_ctx* const* ctxs, int count);
/* Re-upload `count` edited 16^3 blocks (block ids, x-fastest 4096-byte blocks) + the full flag array. */
int vx_grid_update_blocks(vx_ctx* ctx, uint32_t count, const uint32_t* block_ids, const int8_t* dist,
                          const uint8_t* mat, const uint8_t* blend, const uint8_t* empty_flags);
/* ---- edits on the device (Grid::InjectSurface / Grid::InjectMaterial, src/VoxelGrid.cpp:388-584) -------------------
 * For a grid that lives on the device only (vx_grid_upload / vx_grid_upload_packed): the same arithmetic per voxel, the
 * same per-block sections and the same "touched block" rule as the reference, BF_Empty of every touched block
 * recomputed by the codec's rule (CompressBlock, :610-672).  out_min / out_max receive the modified box exactly as
 * Grid::Inject* returns it (output, Y-up, order) — feed it to vx_polygonize_dirty.
 * vx_grid_inject_ball: InjectSurface with the analytic VoxelSurface  f(x,y,z) = sqrt(x^2 + y^2 + z^2) - radius  sampled
 * relative to `position` (the sphere brush of doc_source/Modification.md); type = InjectionType (0 IT_Add,
 * 1 IT_SubtractAddInner, 2 IT_Subtract). */
int vx_grid_inject_ball(vx_ctx* ctx, const float position[3], const float extents[3], float radius, int type,
                        float out_min[3], float out_max[3]);
int vx_grid_inject_material(vx_ctx* ctx, const float position[3], const float extents[3], uint8_t material,
                            int add_subtract_blend, float out_min[3], float out_max[3]);

/* vx_grid_inject_brushes: an ORDERED batch of brushes applied in one device pass (HIP library only).  The grid afterwards -
 * distances, materials, blends - and the BF_Empty flags are byte for byte what `count` single-brush calls in array order
 * leave; for the shapes without a single-brush entry point that call is Grid::InjectSurface with a VoxelSurface that
 * evaluates f below at the sample positions p (relative to `position`, grid axes, Z up).  Float32, one rounding per
 * operation, dot(u, v) = (u.x*v.x + u.y*v.y) + u.z*v.z (voxels_amd/csrc/tv_brush.h is the specification):
 *   VX_BRUSH_BALL      f = sqrt(dot(p, p)) - radius                                     (= vx_grid_inject_ball)
 *   VX_BRUSH_CAPSULE   pa = p - a, ba = b - a, h = clamp(dot(pa, ba) / dot(ba, ba), 0, 1), h = 0 when dot(ba, ba) == 0,
 *                      v = pa - ba * h, f = sqrt(dot(v, v)) - radius                    (a, b relative to `position`)
 *   VX_BRUSH_BOX       q = |p| - a, m = max(q, 0), f = (sqrt(dot(m, m)) + min(max(q.x, max(q.y, q.z)), 0)) - radius
 *   VX_BRUSH_MATERIAL  Grid::InjectMaterial                                             (= vx_grid_inject_material)
 * `extents` is the box the brush rewrites (position -+ extents / 2), as in the single-brush calls; a distance brush only
 * changes what lies inside it, whatever the shape.  BF_Empty is recomputed for every block that at least one distance brush
 * touches (the position -+ extents block test); blocks that only material brushes touch keep their flag.
 * results (may be NULL) receives per brush the box the single-brush call hands back and the number of blocks it touched;
 * union_min / union_max (may be NULL) the componentwise min / max of those boxes over the brushes that touched a block - one
 * box to feed to vx_polygonize_dirty - or zeros when no brush touched the grid (the call then changes nothing);
 * touched_blocks (may be NULL) the number of distinct blocks touched.
 * Every brush is checked before anything is launched: VX_ERR_INVALID, with the grid untouched, for an unknown shape or type
 * (MATERIAL: type is add_subtract_blend, 0 or 1), a float field that is not finite, a material above 255, a NULL array with
 * count > 0, or a context that does not own a whole grid (vx_grid_upload / vx_grid_upload_packed).  count = 0 is VX_OK and
 * does nothing.  Accepted count: up to VX_BRUSH_MAX_COUNT (2^24).  The call waits for the device once, at its end. */
#define VX_BRUSH_BALL     0u
#define VX_BRUSH_CAPSULE  1u
#define VX_BRUSH_BOX      2u
#define VX_BRUSH_MATERIAL 3u
#define VX_BRUSH_MAX_COUNT (1u << 24)
typedef struct vx_brush {          /* 64 bytes */
    float position[3]; uint32_t shape;      /* VX_BRUSH_* */
    float extents[3];  uint32_t type;       /* InjectionType 0..2; MATERIAL: add_subtract_blend 0 / 1 */
    float a[3];        float radius;        /* CAPSULE: segment start; BOX: half sizes | BALL, CAPSULE: radius; BOX: rounding */
    float b[3];        uint32_t material;   /* CAPSULE: segment end | MATERIAL: the material id */
} vx_brush;
typedef struct vx_brush_result {   /* 32 bytes */
    float out_min[3], out_max[3];           /* exactly what the single-brush call hands back (output order, Y-up) */
    uint32_t touched_blocks;                /* blocks of the position -+ extents test; 0 = the brush missed the grid */
    uint32_t reserved;
} vx_brush_result;
int vx_grid_inject_brushes(vx_ctx* ctx, const vx_brush* brushes, uint32_t count, vx_brush_result* results,
                           float union_min[3], float union_max[3], uint32_t* touched_blocks);

/* ---- detached solid pieces (HIP library only) -------------------------------------------------------------------------
 * vx_grid_islands answers "did that carve cut something loose?" on the resident grid: the connected components of the solid
 * voxels of a box, which of them hang in the air, and - on request - their removal.  The reference has nothing like it.
 *   Solid      a voxel whose distance sample is < 0 (the sign bit the case codes read); zero is air.
 *   Region     a box of voxels [lo, hi) in grid coordinates (internal axes, Z up, as vx_grid_inject_ball takes them),
 *              lo < hi <= n per axis, not necessarily aligned to blocks; whole_grid != 0 means the whole grid.  Its volume
 *              V = ex * ey * ez must be <= 2^30 (a whole 1024^3 grid fits; larger grids are queried box by box).
 *   Component  a maximal set of solid voxels of the region connected through shared faces (6-connectivity) by paths INSIDE
 *              the region.  Edge and corner contact does not connect; two arms that only join outside the region are two
 *              components.
 *   Label      the least region-local linear index ((z - lo.z) * ey + (y - lo.y)) * ex + (x - lo.x) over the component's
 *              voxels.  Records are sorted by label ascending.  Nothing in the result depends on scheduling.
 *   Faces      bit k of `faces` is set when a voxel of the component lies on region face k; order -x, +x, -y, +y, -z, +z.
 *   Detached   (faces & anchor_faces) == 0.  0x3F: any face anchors; an application that treats only the bottom and the
 *              sides of a box around a carve as "the world" clears the +z bit (0x1F).
 *   Removal    (VX_ISLANDS_REMOVE) every detached component with voxels <= max_voxels (0 = no limit) has the distance of
 *              each of its voxels set to air_value (1..127).  Materials and blends stay.  BF_Empty is recomputed by the
 *              codec's rule for every block that held a removed voxel and for no other block, and the brick mirrors follow.
 *              out_min / out_max (may be NULL) receive the dirty box in the convention of the edits: output order
 *              (x, z, y), floats; for removed voxels spanning a..b inclusive per internal axis it is [a, b + 1] clamped to
 *              [0, n] - feed it to vx_polygonize_dirty.  Zeros when nothing was removed; the call then changes nothing.
 *              Removal does not depend on `capacity`.
 * islands (host array; may be NULL when capacity is 0) receives the first `capacity` listed records in label order: all
 * components, or only the detached ones with VX_ISLANDS_DETACHED_ONLY.  counts is always written; counts->listed is what an
 * unlimited capacity would hold.  VX_ERR_OVERFLOW when listed > capacity, after everything else has been done (as
 * vx_lod_select).  d_labels (optional; device memory, V uint32, 16-byte aligned) receives the label of every region voxel, x
 * fastest inside the region, UINT32_MAX for air; the labels describe the grid BEFORE a removal.  The library uses the buffer as
 * its working volume.
 * VX_ERR_INVALID, with the grid untouched and before anything is launched, for: a null query or null counts, a bad or too
 * large box, unknown flag bits, anchor_faces > 0x3F, air_value outside 1..127 while VX_ISLANDS_REMOVE is set, a capacity
 * without an array, a misaligned d_labels, a context that does not own a whole grid.  VX_ERR_DEVICE, grid untouched, when
 * working memory cannot be allocated.
 * Working memory, kept with the context and only ever grown: 4 bytes per region voxel (none of that when d_labels is given -
 * a whole 1024^3 query without d_labels takes 4 GiB), 4 bytes per x-row of the region (ey * ez), 4 bytes per block of the
 * region and about 100 bytes per component.
 * The call is synchronous and runs on the context's stream (vx_set_stream).  It waits for the device when it has counted the
 * components (the records are sized by that number), at its end, and once more between the two when a removal changed
 * blocks (their number sizes the flag and mirror pass). */
#define VX_ISLANDS_DETACHED_ONLY 1u   /* list only detached components */
#define VX_ISLANDS_REMOVE        2u
typedef struct vx_island_query {     /* 48 bytes */
    uint32_t lo[3], hi[3];           /* ignored when whole_grid != 0 */
    uint32_t whole_grid, flags, anchor_faces;
    int32_t  air_value;
    uint64_t max_voxels;
} vx_island_query;
typedef struct vx_island {           /* 40 bytes */
    uint32_t label, faces;
    uint64_t voxels;
    uint32_t min[3], max[3];         /* grid coordinates, inclusive */
} vx_island;
typedef struct vx_island_counts {    /* 48 bytes */
    uint64_t solid_voxels, detached_voxels, removed_voxels;
    uint32_t components, detached, listed /* what unlimited capacity would hold */, removed;
    uint32_t touched_blocks /* blocks rewritten by removal */, reserved;
} vx_island_counts;
int vx_grid_islands(vx_ctx* ctx, const vx_island_query* query, vx_island* islands, uint32_t capacity,
                    vx_island_counts* counts, uint32_t* d_labels, float out_min[3], float out_max[3]);

/* ---- smoothing (HIP library only) -------------------------------------------------------------------------------------
 * vx_grid_smooth softens what is there: an ORDERED batch of smoothing ops on the distance samples of the resident grid, each
 * a number of Jacobi iterations of a 3x3x3 binomial filter over a box, blended in by a weight.  The reference has nothing like
 * it.  voxels_amd/csrc/tv_smooth.h is the arithmetic; tests/smooth_oracle.py states this text again in numpy.
 *   One iteration of one op.  Every read sees the grid as it was before this iteration.  For each voxel v of the box [lo, hi):
 *     S      = sum over dx, dy, dz in {-1, 0, 1} of k(dx) k(dy) k(dz) d(clamp(v + (dx, dy, dz), 0, n - 1)), k = (1, 2, 1): an
 *              exact integer.  d is the int8 distance sample as stored (-128 is legal input).  Neighbours outside the BOX are
 *              read from the grid - fixed boundary values; neighbours outside the GRID clamp to the edge voxel.
 *     w      = strength when radius == 0; otherwise, in float32 with one rounding per written operation:
 *              p = (float)v - center, r = sqrtf((p.x p.x + p.y p.y) + p.z p.z), q = 1.0f - r / radius,
 *              w = strength * (q > 0 ? q : 0)
 *     new    = (int8) clamp(rintf(f), -128, 127), t = (float)S * 0.015625f, f = (float)d + w * (t - (float)d); rintf rounds
 *              to nearest, ties to even; the clamp is never active for strength in 0..1; a result of -0 is 0, which is air.
 *     Materials and blends are untouched.
 *   Iterations `iterations` repeats the step on the same box: iteration i + 1 reads the result of iteration i inside the box
 *              and the unchanged grid outside it.
 *   Batches    the ops are applied in array order; the grid afterwards is byte for byte what `count` single-op calls leave.
 *              An op with iterations == 0 or strength == 0 changes nothing and reports a zero box.
 *   Flags      BF_Empty is recomputed by the codec's rule for every block that the box of an op with iterations >= 1 and
 *              strength > 0 intersects, and for no other block; the brick mirrors follow: a polygonization after the call
 *              needs no vx_grid_invalidate.
 *   Results    results[i] (may be NULL) receives the box of the voxels whose value op i actually changed - the end of the op
 *              compared with its beginning - in the convention of vx_grid_islands: output order (x, z, y), floats; for changed
 *              voxels spanning a..b inclusive per internal axis it is [a, b + 1] clamped to [0, n]; zeros when nothing changed;
 *              and the number of those voxels.  union_min / union_max (may be NULL): the componentwise union over the ops that
 *              changed something - the one box to feed to vx_polygonize_dirty - or zeros.  changed_voxels (may be NULL): the
 *              sum of the per-op counts.
 * Everything is checked before anything is launched: VX_ERR_INVALID, with the grid untouched, for a NULL array with count > 0,
 * lo >= hi or hi > n on any axis, a center, radius or strength that is not finite, radius < 0, strength outside [0, 1],
 * iterations > VX_SMOOTH_MAX_ITERATIONS, count > VX_SMOOTH_MAX_COUNT, or a context that does not own a whole grid
 * (vx_grid_upload / vx_grid_upload_packed).  count = 0 is VX_OK and does nothing.  VX_ERR_DEVICE, grid untouched, when working
 * memory cannot be allocated.
 * The call runs on the context's stream (vx_set_stream) and waits for the device once, at its end, to read the results.
 * Working memory, kept with the context and only ever grown: one byte per voxel of the largest box rounded up to whole 16^3
 * grid blocks (twice that when an op has more than one iteration: its original values are kept for the comparison), 4 bytes
 * per block of that box and 64 bytes per op. */
#define VX_SMOOTH_MAX_ITERATIONS 64u
#define VX_SMOOTH_MAX_COUNT (1u << 16)
typedef struct vx_smooth {          /* 48 bytes */
    uint32_t lo[3], hi[3];          /* box [lo, hi) in grid coordinates, internal axes (Z up), as vx_island_query */
    float    center[3];             /* falloff centre, grid coordinates, may be fractional / outside the box */
    float    radius;                /* > 0: ball falloff; == 0: uniform weight over the box */
    float    strength;              /* 0..1 */
    uint32_t iterations;            /* 0..VX_SMOOTH_MAX_ITERATIONS */
} vx_smooth;
typedef struct vx_smooth_result {   /* 32 bytes */
    float    out_min[3], out_max[3];
    uint64_t changed_voxels;
} vx_smooth_result;
int vx_grid_smooth(vx_ctx* ctx, const vx_smooth* ops, uint32_t count, vx_smooth_result* results /* may be NULL */,
                   float union_min[3], float union_max[3] /* may be NULL */, uint64_t* changed_voxels /* may be NULL */);

/* ---- walk fields (HIP library only) -----------------------------------------------------------------------------------
 * vx_grid_walk_field answers "where can my agents still walk, and which way?" on the resident grid: for every voxel of a box
 * the cost of the cheapest walk to the nearest of a set of goals, and - derived from it - the move to take: the flow field a
 * crowd reads with one lookup per agent.  The reference has nothing like it.  All arithmetic is in integers and the result is
 * the unique least solution of the recurrence below: nothing in it depends on scheduling (`sweeps` excepted).
 * Internal axes with Z up, as vx_island_query; d is the int8 distance sample as stored.
 *   Solid / air  solid(x, y, z): 0 <= z < n and d < 0.  air(x, y, z): z >= n, or 0 <= z < n and d >= 0.  Below the grid
 *              (z < 0) is neither.
 *   Region     a box of voxels [lo, hi), lo < hi <= n per axis, not necessarily aligned to blocks; whole_grid != 0 means the
 *              whole grid.  Its volume V = ex * ey * ez must be <= 2^28; larger areas are queried box by box.  That bounds the
 *              field at 1 GiB and the rest of the working memory (below) at 32 MiB for a block-aligned box, about 0.5 GiB for a
 *              box one voxel thick (every 16^3 block it touches counts whole).
 *   Standable  a region voxel c = (x, y, z) with z >= 1, solid(x, y, z - 1) and air(x, y, z + k) for k = 0 .. clearance - 1.
 *              The column is read from the GRID, also below lo.z and above hi.z.  Materials, blends and BF_Empty play no part.
 *   Moves      c -> c' where c' is standable and inside the region, dz = c'.z - c.z lies in [-step_down, +step_up], and the
 *              horizontal offset is one of the codes 0..7, in this order: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1)
 *              (-1,-1).  A diagonal move (dx, dy) exists only when cost_diagonal != 0 and BOTH columns (x + dx, y) and
 *              (x, y + dy) hold at least one standable in-region cell c'' with c''.z - c.z in [-step_down, +step_up]: there is
 *              no cutting of corners.  A column can hold several targets (a bridge over a cave floor): each is a move of its
 *              own.  Weight w = (axial ? cost_axial : cost_diagonal) + |dz| * cost_climb.
 *   Goals      a host array of vx_walk_goal, at most VX_WALK_MAX_GOALS.  A goal is USED when its cell (grid coordinates) is
 *              standable, inside the region, and cost <= max_cost; every other goal is IGNORED and counted.  Duplicates are
 *              legal; the least cost wins.
 *   Field      F(c) = min(least cost of a used goal at c, min over the moves c -> c' of w + F(c')), the least solution: the cost
 *              of the cheapest walk from c to a goal.  A cell with F(c) > max_cost, a voxel that is not standable, and a cell
 *              with no walk to a goal all read VX_WALK_UNREACHED; a cell with F == max_cost is reached.  Dropping every
 *              candidate above max_cost while relaxing is exact: weights are positive, so every cell further along a cheapest
 *              walk has a smaller F - a walk whose cost is within max_cost never passes through a cell that was dropped.
 *   Direction  one byte per region voxel: 0xFF where the field is UNREACHED; 0xFE where no move gives w + F(c') == F(c) (a goal
 *              cell that is its own best); otherwise the move code offset | (dz + 4) << 3 of a move with w + F(c') == F(c) -
 *              among several, the least code.
 *   Limits     clearance 1..32; step_up, step_down 0..4; cost_axial 1..65535; cost_diagonal 0..65535 (0 = no diagonals);
 *              cost_climb 0..65535; max_cost 0..2^30; flags 0.  With these the largest sum ever formed is
 *              2^30 + 65535 + 4 * 65535 < 2^31: no sum wraps a uint32.
 * d_field (optional; device memory, V uint32, x fastest inside the region, 16-byte aligned) receives F; without it the library
 * uses a working volume of its own.  d_dirs (optional; device memory, V bytes, same order) receives the direction bytes.
 * counts is always written, also with both outputs NULL: standable cells of the region, reached cells, used and ignored goals,
 * max_distance = the largest reached F (0 when nothing is reached), and sweeps = how many relaxation sweeps the call ran -
 * the one field that is NOT part of the deterministic result (it depends on the order the hardware served the tiles in).  Sweeps
 * are launched in batches of 8 and every launch counts, also the idle ones behind the sweep that changed the last cell: the
 * number is a multiple of the batch (unless the cap of the loop cuts a batch short), not a measure of convergence.
 * With no used goal the field is all UNREACHED, reached = 0, and the call returns VX_OK.
 * VX_ERR_INVALID, with nothing launched and nothing written to d_field / d_dirs (counts, when it is not NULL, is zeroed on
 * entry, so it reads all zero after such a call), for: a null query or null counts, a bad or too
 * large box, a limit violated, non-zero flags, goal_count > VX_WALK_MAX_GOALS, a null goal array with a count, a misaligned
 * d_field, a context that does not own a whole grid (vx_grid_upload / vx_grid_upload_packed).  VX_ERR_DEVICE when working memory
 * cannot be allocated.  The call never changes the grid, the flags or the mirrors.
 * Working memory, kept with the context and only ever grown: 4 bytes per region voxel (none of that when d_field is given),
 * 524 bytes per 16^3 block the region touches (one standable bit per voxel, a count and two sweep flags) and 16 bytes per goal.
 * The call is synchronous and runs on the context's stream (vx_set_stream).  It waits for the device when the standable cells
 * are counted, once per batch of relaxation sweeps, and at its end. */
#define VX_WALK_UNREACHED 0xFFFFFFFFu
#define VX_WALK_MAX_GOALS 65536u
typedef struct vx_walk_query {      /* 64 bytes */
    uint32_t lo[3], hi[3];          /* ignored when whole_grid != 0 */
    uint32_t whole_grid, clearance, step_up, step_down;
    uint32_t cost_axial, cost_diagonal, cost_climb, max_cost;
    uint32_t flags /* 0 */, reserved;
} vx_walk_query;
typedef struct vx_walk_goal {       /* 16 bytes */
    uint32_t x, y, z, cost;
} vx_walk_goal;
typedef struct vx_walk_counts {     /* 32 bytes */
    uint64_t standable, reached;
    uint32_t goals_used, goals_ignored, max_distance;
    uint32_t sweeps;                /* not part of the deterministic result */
} vx_walk_counts;
int vx_grid_walk_field(vx_ctx* ctx, const vx_walk_query* query, const vx_walk_goal* goals /* host */, uint32_t goal_count,
                       uint32_t* d_field /* device, may be NULL */, uint8_t* d_dirs /* device, may be NULL */,
                       vx_walk_counts* counts);

/* ---- undo records (HIP library only) ----------------------------------------------------------------------------------
 * Every edit of the resident grid - vx_grid_inject_ball / _material / _brushes, vx_grid_smooth, vx_grid_islands with
 * VX_ISLANDS_REMOVE - is destructive.  An undo record is a device-resident copy of a set of whole 16^3 grid blocks, byte for
 * byte, owned by the context that made it: CAPTURE the blocks an edit may touch, edit, TRIM the record to the blocks the edit
 * did change, and SWAP it with the grid to take the edit back.  A swap exchanges, so the same record is the undo of the edit,
 * then its redo, then its undo again; a stack of records is an undo history.  The edit entry points do not capture by
 * themselves.  voxels_amd/csrc/tv_undo.h is the per-block logic; tests/undo_oracle.py states this text again in numpy.
 * Boxes are voxel boxes [lo, hi) in grid coordinates, internal axes (Z up), as vx_island_query; block ids number the blocks as
 * vx_grid_read_block does: (bz * nb + by) * nb + bx, nb = n / 16.
 *   Capture    vx_grid_capture: the record holds every block that at least one box intersects - block coordinates lo / 16 ..
 *              (hi - 1) / 16 per axis - each once, in ascending id, whatever the order or the overlap of the boxes.  Per block
 *              it holds the 4096 distances, 4096 materials and 4096 blends as the dense fields hold them (the mirrors play no
 *              part) and the block's BF_Empty byte as the grid's flag array holds it: the flag is stored, not recomputed - a
 *              block that only material brushes touched keeps its flag, and vx_grid_upload takes flags from the caller, so the
 *              flag is not a function of the voxels.  count = 0 gives a valid empty record.  More than VX_RECORD_MAX_BLOCKS
 *              distinct blocks is VX_ERR_INVALID.  The call never changes the grid, the flags or the mirrors, and a full run
 *              afterwards replays what it replayed before.
 *   Trim       vx_record_trim compares every held block with the grid as it is now, drops the blocks whose 12 288 bytes and
 *              flag byte are all equal and packs the rest, in their order, into a right-sized allocation; *dropped (may be
 *              NULL) receives the number of blocks dropped.  Legal at any time, also after swaps.  Never changes the grid.
 *   Swap       vx_record_swap: for every held block the grid receives the record's three fields and flag byte and the record
 *              receives what the grid held.  The brick mirrors follow, as after any edit: a polygonization after the call needs
 *              no vx_grid_invalidate.  result (may be NULL) receives
 *                out_min / out_max   the box of the voxels that differed in distance, material or blend, in the convention of
 *                                    vx_grid_islands and vx_grid_smooth: output order (x, z, y), floats; for differing voxels
 *                                    spanning a..b inclusive per internal axis it is [a, b + 1] clamped to [0, n]; zeros when no
 *                                    voxel differed.  Feed it to vx_polygonize_dirty - no margin is needed, also where only
 *                                    materials or blends differed.
 *                changed_voxels      the number of those voxels
 *                changed_blocks      blocks with such a voxel or a different flag byte
 *                flag_changes        blocks whose BF_Empty byte differed (such a block counts as changed and moves no box)
 *              A swap of an empty record, or of a record equal to the grid, is VX_OK, returns zeros, and a full run afterwards
 *              replays what it replayed before.
 *   Reading    vx_record_info_get; vx_record_block_ids (the held ids, ascending; capacity >= the block count);
 *              vx_record_read_block (entry `index` in the layout of vx_grid_read_block: rows z-major, 16 bytes each; every
 *              output may be NULL).
 *   Brushes    vx_brush_box (host only, no context): the voxel box [16 * first, 16 * (first + cnt)) per internal axis of the
 *              blocks the position -+ extents block test of the edits finds for the brush - the same float32 expressions per
 *              block and axis - for a grid of edge n.  1 = the brush touches the grid, 0 = it misses it (the box is zeroed:
 *              leave it out).  Capturing the boxes of a brush array captures exactly the blocks vx_grid_inject_brushes touches.
 *   Lifetime   vx_record_free releases a record (NULL is legal); vx_ctx_destroy frees what is left.  A record survives full
 *              and incremental runs, vx_compact_pools and further edits; it can be used while the context owns a whole grid
 *              of the edge it was captured from.
 * Everything is checked before anything is launched: VX_ERR_INVALID, with nothing changed, for a null context, record, out
 * pointer or info, a null box array with count > 0, count > VX_RECORD_MAX_BOXES, lo >= hi or hi > n on any axis, a context
 * that does not own a whole grid (vx_grid_upload / vx_grid_upload_packed; capture, trim, swap), a record made by another
 * context, a record whose n differs from the context's grid now (trim, swap), an index or a capacity out of range.
 * vx_brush_box returns VX_ERR_INVALID for a null argument or an n that is not a multiple of 16 in 16..2048.  VX_ERR_DEVICE,
 * with the grid untouched, when memory cannot be allocated.
 * All calls are synchronous and run on the context's stream (vx_set_stream).  Capture waits for the device once: the number of
 * distinct blocks sizes the allocation.  Trim waits once: the kept count sizes the new allocation (the one it replaces is
 * released behind the next wait of one of these calls, or with the context).  Swap waits once, at its end, for the result.
 * Memory: 12 293 bytes of device memory per held block - 12 288 of fields, 1 flag, 4 id - in one allocation per record, rounded
 * as the allocator rounds; vx_record_info.bytes is that product.  Working memory, kept with the context and only ever grown:
 * one bit and 4 bytes per 32 blocks of the grid (capture) or of the record (trim), 24 bytes per box, 4 bytes per held block. */
typedef struct vx_record vx_record;                 /* opaque; belongs to the context that made it */
typedef struct vx_box { uint32_t lo[3], hi[3]; } vx_box;         /* 24 bytes; [lo, hi), grid coordinates, internal axes (Z up) */
typedef struct vx_record_info {                                   /* 48 bytes */
    uint32_t n, blocks;            /* grid edge at capture; blocks held now */
    uint64_t bytes;                /* device memory held now */
    uint32_t min[3], max[3];       /* block coordinates of the held blocks, inclusive; zeros when blocks == 0 */
    uint32_t swaps, reserved;      /* successful vx_record_swap calls so far */
} vx_record_info;
typedef struct vx_swap_result {                                   /* 48 bytes */
    float    out_min[3], out_max[3];
    uint64_t changed_voxels;       /* voxels that differed in distance, material or blend */
    uint32_t changed_blocks;       /* blocks with such a voxel or a different flag byte */
    uint32_t flag_changes;         /* blocks whose BF_Empty byte differed */
    uint64_t reserved;
} vx_swap_result;
#define VX_RECORD_MAX_BLOCKS (1u << 18)   /* a whole 1024^3 grid */
#define VX_RECORD_MAX_BOXES  (1u << 16)
int  vx_grid_capture(vx_ctx* ctx, const vx_box* boxes /* host */, uint32_t count, vx_record** out);
int  vx_record_trim(vx_ctx* ctx, vx_record* record, uint32_t* dropped /* may be NULL */);
int  vx_record_swap(vx_ctx* ctx, vx_record* record, vx_swap_result* result /* may be NULL */);
int  vx_record_info_get(vx_ctx* ctx, const vx_record* record, vx_record_info* info);
int  vx_record_block_ids(vx_ctx* ctx, const vx_record* record, uint32_t* ids, uint32_t capacity);
int  vx_record_read_block(vx_ctx* ctx, const vx_record* record, uint32_t index, int8_t* dist, uint8_t* mat, uint8_t* blend,
                          uint8_t* empty_flag);
void vx_record_free(vx_ctx* ctx, vx_record* record);
int  vx_brush_box(const vx_brush* brush, uint32_t n, vx_box* out);

/* ---- stamps (HIP library only) ------------------------------------------------------------------------------------------
 * Copy part of the resident grid and put it somewhere else, or place a prefab kept as voxels, without a trip through the host.
 * A STAMP is a device-resident dense copy of a voxel box: a size (sx, sy, sz) and three byte fields - distance, material,
 * blend - x fastest, then y, then z (internal axes, Z up).  It belongs to the context that made it and does not depend on the
 * grid's edge.  A PASTE puts a stamp into the grid at an integer origin, in one of the eight orientations that keep Z up, under
 * one of four combine modes; vx_grid_paste applies an ordered batch of them in one device pass.  Everything is integer and every
 * byte of the result is defined.  voxels_amd/csrc/tv_stamp.h is the per-voxel logic; tests/stamp_oracle.py states this text
 * again in numpy.  Needs a context that owns a whole grid (vx_grid_upload / vx_grid_upload_packed / vx_grid_create_*), as the
 * brushes.
 *   Capture    vx_stamp_capture copies the voxels of `box` ([lo, hi), grid coordinates) out of the dense fields (the mirrors
 *              play no part).  BF_Empty flags are not part of a stamp.  The call never changes the grid, the flags, the mirrors
 *              or any kept state: a full run afterwards replays what it replayed before.
 *   Upload     vx_stamp_upload makes a stamp from host arrays of size[0] * size[1] * size[2] bytes each; mat and blend may be
 *              NULL: zeros.
 *   Reading    vx_stamp_read (every output may be NULL); vx_stamp_info_get.
 *   Orient     vx_paste.orient is 0..7.  Bit 2 mirrors the stamp's x first: i' = sx-1-i.  Bits 0..1 are q quarter turns about
 *              +z, counter-clockwise seen from +z.  Stamp voxel (i, j, k) has the oriented coordinates (u, v, k):
 *                q = 0: (i', j)      q = 1: (sy-1-j, i')      q = 2: (sx-1-i', sy-1-j)      q = 3: (j, sx-1-i')
 *              The oriented size is (sy, sx, sz) for odd q, otherwise (sx, sy, sz).  Grid voxel = origin + (u, v, k): origin is
 *              the min corner of the oriented stamp, any int32; the part outside [0, n)^3 is clipped (64-bit arithmetic).
 *   Modes      per voxel, the grid holds (d, m, b) and the stamp (sd, sm, sb):
 *                VX_PASTE_REPLACE    (sd, sm, sb)
 *                VX_PASTE_UNION      (sd, sm, sb) if sd < d, otherwise unchanged
 *                VX_PASTE_SUBTRACT   c = (sd == -128 ? 127 : -sd); d = c if c > d; m and b stay
 *                VX_PASTE_PAINT      (d, sm, sb) if sd < 0, otherwise unchanged
 *   Order      the grid afterwards is byte for byte what `count` single-paste calls in array order leave.
 *   Blocks     the touched blocks of a paste are the blocks its clipped box intersects.  BF_Empty is recomputed by the codec's
 *              rule for every block that at least one paste of a mode other than VX_PASTE_PAINT touches, and for no other block
 *              (the brushes' rule).  The brick mirrors follow over the distinct touched blocks: a polygonization afterwards
 *              needs no vx_grid_invalidate.  A batch that touches no block launches nothing that writes and changes nothing.
 *   Results    results[i] (may be NULL): box = the clipped voxel box, all zeros when the paste misses the grid; touched_blocks =
 *              the number of blocks of that box.  counts (may be NULL): out_min / out_max, changed_voxels, changed_blocks and
 *              flag_changes have the meaning and the convention of vx_swap_result - the box is over the voxels that differ
 *              between the grid before and after the whole batch, output order (x, z, y), [a, b + 1] clamped, zeros when
 *              nothing differed; feed it to vx_polygonize_dirty with no margin - and touched_blocks is the number of distinct
 *              touched blocks.
 *   Boxes      vx_paste_box (host only, no context): the clipped box by the same integer expressions, for a grid of edge n.
 *              1 = the paste touches the grid, 0 = it misses it (the box is zeroed: leave it out).  Capturing the boxes of a
 *              paste array with vx_grid_capture captures exactly the touched blocks.
 *   Lifetime   vx_stamp_free releases a stamp (NULL is legal); vx_ctx_destroy frees what is left.  A stamp survives runs,
 *              vx_compact_pools, edits and the upload of another grid, of any edge.
 * Everything is checked before anything is launched: VX_ERR_INVALID, with nothing changed, for a null context, out pointer or
 * info, a null array with a non-zero count, a box with lo >= hi or hi > n, a size of 0, above VX_STAMP_MAX_EDGE or with a
 * product above VX_STAMP_MAX_VOXELS, a null dist in upload, count > VX_PASTE_MAX_COUNT, n_stamps > VX_PASTE_MAX_STAMPS,
 * stamp >= n_stamps, a null entry that a paste refers to (an unreferenced null entry is legal), a stamp of another context,
 * orient > 7, mode > 3, non-zero reserved words, a context that does not own a whole grid (capture, paste).  vx_paste_box
 * returns VX_ERR_INVALID for a null argument, a zero size, orient > 7 or an n that is not a multiple of 16 in 16..2048.
 * VX_ERR_DEVICE, with the grid untouched, when memory cannot be allocated.  count = 0 is VX_OK.
 * All calls are synchronous and run on the context's stream (vx_set_stream): capture and upload do not wait for the device,
 * vx_grid_paste waits once, at its end, vx_stamp_read waits for its copies.
 * Memory: 3 bytes per voxel of device memory, in one allocation per stamp; vx_stamp_info.bytes is that product.  Working memory
 * of a batch, kept with the context and only ever grown: 32 bytes per paste, 24 per stamp of the array, 8 per block of the grid,
 * 12 per distinct touched block and 4 per (paste, block) pair, in chunks of at most 2^22 pairs; a batch that needs several chunks
 * adds 12 bytes per block of the grid and 12 289 per block that more than one chunk touches. */
typedef struct vx_stamp vx_stamp;                       /* opaque; belongs to the context that made it */
typedef struct vx_stamp_info { uint32_t size[3], reserved; uint64_t voxels, bytes; } vx_stamp_info;   /* 32 bytes */
#define VX_STAMP_MAX_EDGE   2048u
#define VX_STAMP_MAX_VOXELS (1u << 30)
#define VX_PASTE_REPLACE  0u
#define VX_PASTE_UNION    1u
#define VX_PASTE_SUBTRACT 2u
#define VX_PASTE_PAINT    3u
#define VX_PASTE_MAX_COUNT  (1u << 20)
#define VX_PASTE_MAX_STAMPS (1u << 16)
typedef struct vx_paste { int32_t origin[3]; uint32_t stamp; uint32_t orient; uint32_t mode; uint32_t reserved[2]; } vx_paste;   /* 32 bytes */
typedef struct vx_paste_result { vx_box box; uint32_t touched_blocks, reserved; } vx_paste_result;                             /* 32 bytes */
typedef struct vx_paste_counts { float out_min[3], out_max[3]; uint64_t changed_voxels;
                                 uint32_t changed_blocks, flag_changes, touched_blocks, reserved; } vx_paste_counts;           /* 48 bytes */
int  vx_stamp_capture(vx_ctx* ctx, const vx_box* box /* host */, vx_stamp** out);
int  vx_stamp_upload(vx_ctx* ctx, const uint32_t size[3], const int8_t* dist, const uint8_t* mat /* may be NULL: zeros */,
                     const uint8_t* blend /* may be NULL: zeros */, vx_stamp** out);
int  vx_stamp_read(vx_ctx* ctx, const vx_stamp* stamp, int8_t* dist, uint8_t* mat, uint8_t* blend);
int  vx_stamp_info_get(vx_ctx* ctx, const vx_stamp* stamp, vx_stamp_info* info);
void vx_stamp_free(vx_ctx* ctx, vx_stamp* stamp);
int  vx_grid_paste(vx_ctx* ctx, vx_stamp* const* stamps, uint32_t n_stamps, const vx_paste* pastes /* host */, uint32_t count,
                   vx_paste_result* results /* may be NULL */, vx_paste_counts* counts /* may be NULL */);
int  vx_paste_box(const vx_paste* paste, const uint32_t stamp_size[3], uint32_t n, vx_box* out);
/* tests: the capacity of the (paste, block) lists of this context's batches, 0 = the default (2^22); nothing of a batch's
 * result depends on it */
int  vx_debug_paste_list_cap(vx_ctx* ctx, uint32_t capacity);

/* ---- measurements (HIP library only) ------------------------------------------------------------------------------------
 * How much of what is in there: the solid volume, the tight bounds of the solid voxels and the count per material of voxel
 * boxes of the resident grid, and what an edit removed, added and repainted, read off the undo record captured around it -
 * a few integers per box instead of the voxels over the link.  Everything is integer and exact; no result depends on an order
 * or a schedule.  voxels_amd/csrc/tv_measure.h is the per-row logic; tests/measure_oracle.py states this text again in numpy.
 * Needs a context that owns a whole grid (vx_grid_upload / vx_grid_upload_packed / vx_grid_create_*), as the brushes.
 *   Solid      a voxel whose distance sample is < 0; zero is air (the definition of vx_grid_islands).
 *   Box        a vx_box: [lo, hi) in grid coordinates, internal axes (Z up), lo < hi <= n per axis.  A box need not be aligned
 *              to blocks.  The boxes of a batch may overlap or repeat; every box is answered on its own.
 *   Fields     the dense fields are what is measured; the mirrors and the BF_Empty flags play no part in the result.
 *   Measure    vx_grid_measure: results[i] describes box i - voxels = its volume; solid_voxels; min / max = the grid
 *              coordinates of its solid voxels per internal axis, inclusive, zeros when it holds none; materials = the number
 *              of distinct material bytes among its solid voxels.  tallies (may be NULL): tallies[i * 256 + m] = the solid
 *              voxels of box i whose material byte is m; the 256 entries of a box sum to its solid_voxels.
 *   Record     vx_record_measure compares every held block of an undo record with the grid as it is now: removed_voxels are
 *              solid in the record and not in the grid, added_voxels the other way round, repainted_voxels solid in both with
 *              different material bytes; min / max = the inclusive bounds of the removed and the added voxels, zeros when there
 *              are none; blocks = held blocks with a removed, added or repainted voxel.  removed[m] (may be NULL, 256 entries)
 *              counts the removed voxels by the material the RECORD holds for them, added[m] the added voxels by the material
 *              the GRID holds now.  A record captured before an edit so reports what the edit did.  After a vx_record_swap the
 *              record holds the edited state and the grid the earlier one, so the same call reports the redo's effect: removed
 *              and added exchange their roles.  An empty record gives zeros.
 * Neither call changes the grid, the flags, the mirrors, a record or any kept state: a full run afterwards replays what it
 * replayed before.
 * Everything is checked before anything is launched: VX_ERR_INVALID for a null context, results, delta or record, a null box
 * array with count > 0, count > VX_MEASURE_MAX_BOXES, lo >= hi or hi > n on any axis, a context that does not own a whole
 * grid, a record of another context or one whose n differs from the grid's now.  count = 0 is VX_OK and writes nothing.
 * VX_ERR_DEVICE when working memory cannot be allocated.
 * Both calls are synchronous, run on the context's stream (vx_set_stream) and wait for the device once, at their end.  Grids up
 * to 2048^3 are covered and every count is 64-bit: a whole-grid box holds 2^33 voxels.
 * Working memory, kept with the context and only ever grown: 2160 bytes per box - 24 of box, 8 of running block count, 32 of
 * count and bounds, 2048 of tallies (they exist whether or not the caller asks for them: materials is counted from them), 48 of
 * result.  The work item is a (box, block) pair; pairs are launched in chunks of at most 2^22 and a chunk needs no memory of
 * its own.  vx_record_measure uses 4352 bytes. */
#define VX_MEASURE_MAX_BOXES (1u << 16)
typedef struct vx_measure {            /* 48 bytes */
    uint64_t voxels;                   /* volume of the box */
    uint64_t solid_voxels;
    uint32_t min[3], max[3];           /* grid coordinates of the solid voxels, inclusive; zeros when solid_voxels == 0 */
    uint32_t materials;                /* distinct material bytes among the solid voxels */
    uint32_t reserved;                 /* 0 */
} vx_measure;
int  vx_grid_measure(vx_ctx* ctx, const vx_box* boxes /* host */, uint32_t count, vx_measure* results /* host, count entries */,
                     uint64_t* tallies /* host, count * 256, may be NULL */);
typedef struct vx_record_delta {       /* 64 bytes */
    uint64_t removed_voxels;           /* solid in the record, not solid in the grid now */
    uint64_t added_voxels;             /* not solid in the record, solid in the grid now */
    uint64_t repainted_voxels;         /* solid in both, material bytes differ */
    uint32_t min[3], max[3];           /* inclusive bounds of the removed and added voxels; zeros when there are none */
    uint32_t blocks;                   /* held blocks with a removed, added or repainted voxel */
    uint32_t reserved[3];              /* 0 */
} vx_record_delta;
int  vx_record_measure(vx_ctx* ctx, const vx_record* record, vx_record_delta* delta,
                       uint64_t* removed /* host, 256, may be NULL */, uint64_t* added /* host, 256, may be NULL */);
/* tests: the (box, block) pairs per launch of this context's measurements, 0 = the default (2^22), and whether the per-block
 * sign summaries may stand in for distance rows (the default: yes); nothing of a result depends on either */
int  vx_debug_measure_chunk(vx_ctx* ctx, uint32_t pairs);
int  vx_debug_measure_shortcuts(vx_ctx* ctx, uint32_t enable);

/* ---- height maps (HIP library only) -------------------------------------------------------------------------------------
 * How high is the ground at (x, y), and what is it made of: the surface heights per column of a voxel box of the resident grid,
 * from the top or from the bottom, up to VX_HEIGHT_MAX_LAYERS surfaces per column, with the material byte of each - what
 * vx_grid_create_heightmap takes, given back after brushes, pastes, smoothing and island removal.  Everything is integer and
 * exact; no result depends on an order or a schedule.  voxels_amd/csrc/tv_height.h is the per-row and per-column logic;
 * tests/height_oracle.py states this text again in numpy.  Needs a context that owns a whole grid (vx_grid_upload /
 * vx_grid_upload_packed / vx_grid_create_*), as the brushes.
 *   Solid      a voxel whose distance sample is < 0; zero is air (the definition of vx_grid_islands and vx_grid_measure).  The
 *              dense fields are what is read; the mirrors and the BF_Empty flags play no part in the result.
 *   Query      box = [lo, hi) in grid coordinates, internal axes (Z up), lo < hi <= n per axis, not necessarily aligned to
 *              blocks; direction = VX_HEIGHT_FROM_TOP or VX_HEIGHT_FROM_BOTTOM; layers = 1..VX_HEIGHT_MAX_LAYERS; flags = 0 or
 *              VX_HEIGHT_COUNT_SURFACES; the reserved words are zero.
 *   Column     the samples (x, y, z0 .. z1 - 1) of the box for one (x, y), z0 = lo[2], z1 = hi[2].  Whatever lies outside
 *              [z0, z1) counts as air, also where the grid goes on.
 *   Surface    from the top: a z of the column that is solid, with z + 1 == z1 or sample z + 1 not solid; the surfaces of a
 *              column are ordered by descending z.  From the bottom: a z that is solid, with z == z0 or sample z - 1 not solid;
 *              ordered by ascending z.  Layer j is the j-th of them.
 *   Height     a uint32_t in 24.8 fixed point.  With d0 (-128..-1) the surface sample and d1 (0..127) its air neighbour in the
 *              scan direction, f = (256 * -d0) / (d1 - d0) in integer division, 2..256; from the top h = z * 256 + f, from the
 *              bottom h = z * 256 - f.  A clipped surface is one whose air neighbour is the box's end: h = z * 256.
 *              VX_HEIGHT_NONE stands where the column has fewer surfaces than the layer asks for.  A clipped height and a
 *              crossing with d1 = 0 one sample further in can be the same number (from the top: clipped at z gives z * 256, and
 *              so does a surface at z - 1 with d1 = 0); counts.clipped tells whether layer 0 holds any clipped surface.
 *   Outputs    heights, layers * H * W entries with W = hi[0] - lo[0] and H = hi[1] - lo[1], layer-major, then y, then x.
 *              materials (may be NULL), as many bytes: the material byte of the surface voxel, 0 where the height is
 *              VX_HEIGHT_NONE.  surfaces (may be NULL; must be NULL unless VX_HEIGHT_COUNT_SURFACES is set), H * W entries: the
 *              number of surfaces in the column.
 *   Counts     (may be NULL) columns = W * H; covered = columns with at least one surface; surfaces = the sum over the
 *              columns; min_height / max_height over layer 0 of the covered columns, zeros when there are none; clipped =
 *              columns whose layer 0 is clipped; max_surfaces = the most surfaces in one column.  Without
 *              VX_HEIGHT_COUNT_SURFACES surfaces and max_surfaces are 0, and the walk may stop as soon as every column of a
 *              tile has its layers.
 * vx_grid_heightmap takes host arrays, is synchronous, runs on the context's stream (vx_set_stream) and waits for the device
 * once, at its end.  vx_grid_heightmap_device takes the three arrays as device pointers (heights 4-byte aligned, surfaces
 * 2-byte) and counts on the host; with counts == NULL it only enqueues on the context's stream and does not wait - the
 * per-frame form.
 * Neither call changes the grid, the flags, the mirrors or any kept state: a full run afterwards replays what it replayed
 * before.
 * Everything is checked before anything is launched and nothing is written on an error: VX_ERR_INVALID for a null context,
 * query or heights array, lo >= hi or hi > n on any axis, direction > 1, layers of 0 or above VX_HEIGHT_MAX_LAYERS, an unknown
 * flag bit, a non-zero reserved word, a surfaces array without VX_HEIGHT_COUNT_SURFACES, a misaligned device array, a context
 * that does not own a whole grid (slab and attached contexts, as for the brushes).  VX_ERR_DEVICE when working memory cannot be
 * allocated.
 * Working memory, kept with the context, grown when a call needs more and released with the context: 256 bytes for the counts,
 * and for vx_grid_heightmap the staging of its results on the device - 4 bytes per entry of heights, 1 per entry of materials
 * and 2 per column of surfaces where they are asked for, each part rounded up to 256 bytes.  vx_grid_heightmap_device with
 * counts == NULL uses none. */
#define VX_HEIGHT_MAX_LAYERS 8u
#define VX_HEIGHT_NONE 0xFFFFFFFFu
#define VX_HEIGHT_FROM_TOP 0u
#define VX_HEIGHT_FROM_BOTTOM 1u
#define VX_HEIGHT_COUNT_SURFACES 1u
typedef struct vx_height_query {       /* 48 bytes */
    vx_box   box;                      /* [lo, hi), grid coordinates, internal axes */
    uint32_t direction;                /* VX_HEIGHT_FROM_TOP / VX_HEIGHT_FROM_BOTTOM */
    uint32_t layers;                   /* 1..VX_HEIGHT_MAX_LAYERS */
    uint32_t flags;                    /* VX_HEIGHT_COUNT_SURFACES */
    uint32_t reserved[3];              /* 0 */
} vx_height_query;
typedef struct vx_height_counts {      /* 48 bytes */
    uint64_t columns;                  /* W * H */
    uint64_t covered;                  /* columns with at least one surface */
    uint64_t surfaces;                 /* the sum over the columns; 0 without VX_HEIGHT_COUNT_SURFACES */
    uint32_t min_height, max_height;   /* over layer 0 of the covered columns; zeros when there are none */
    uint32_t clipped;                  /* columns whose layer 0 is clipped */
    uint32_t max_surfaces;             /* 0 without VX_HEIGHT_COUNT_SURFACES */
    uint32_t reserved[2];              /* 0 */
} vx_height_counts;
int  vx_grid_heightmap(vx_ctx* ctx, const vx_height_query* query, uint32_t* heights /* host, layers * H * W */,
                       uint8_t* materials /* host, layers * H * W, may be NULL */, uint16_t* surfaces /* host, H * W, may be NULL */,
                       vx_height_counts* counts /* host, may be NULL */);
int  vx_grid_heightmap_device(vx_ctx* ctx, const vx_height_query* query, uint32_t* d_heights /* device */,
                              uint8_t* d_materials /* device, may be NULL */, uint16_t* d_surfaces /* device, may be NULL */,
                              vx_height_counts* counts /* host, may be NULL: enqueue only */);
/* tests: whether the per-block sign summaries may stand in for distance rows (the default: yes); nothing of a result depends on
 * it */
int  vx_debug_height_shortcuts(vx_ctx* ctx, uint32_t enable);

/* ---- ambient occlusion (HIP library only) --------------------------------------------------------------------------------
 * One byte per vertex of a level's meshes: how open the grid is around the vertex, on the side its normal points to - 255 is
 * fully open.  The vertex stays the reference's 48 bytes; the bytes are an array of their own, parallel to the vertex pool:
 * byte i belongs to pool vertex i of vx_device_meshes, so a renderer binds the array as a second vertex stream with the
 * offsets it already has.  The rule is integer arithmetic and exact: the device result is the same bytes as
 * tests/occlusion_oracle.py, which states this text again in numpy; voxels_amd/csrc/tv_occlusion.h is the one place where the
 * library writes it down.  Needs a context that owns a whole grid (vx_grid_upload / vx_grid_upload_packed) and has a surface.
 *
 * The rule.  All arithmetic is int32 unless stated otherwise.  Shifts of negative numbers are arithmetic.  Float operations are
 * float32 with one rounding per written operation and no contraction.
 *   Space.       s = 1 << level.  A vertex's grid-axis position is g = (pos[0], pos[2], pos[1]) and its normal is
 *                m = (nrm[0], nrm[2], nrm[1]): mesh space is Y-up and the grid is Z-up.  A voxel is solid where its distance
 *                sample is < 0, the definition used everywhere else.  Lattice point c of the level is grid sample c * s.  It is
 *                air if any coordinate is < 0 or c[a] * s >= n.
 *   Quantise.    P[a] = (int32)floorf(g[a] * (256.0f / s) + 0.5f): 24.8 fixed point in voxels of the level.
 *                N[a] = (int32)floorf(m[a] * 127.0f + 0.5f).  A vertex with a g[a] that is not finite or has |g[a]| > 4096 is
 *                not baked: it writes 255 and counts nowhere.  A normal component that is not finite gives N[a] = 0.  Clamp
 *                N[a] to [-127, 127] (the clamp is applied to the floored float, so an overflowing product ends at +-127).
 *   Directions.  There are 98 of them: the integer vectors d with max(|dx|, |dy|, |dz|) == 2, in ascending order of
 *                ((dz + 2) * 5 + (dy + 2)) * 5 + (dx + 2).  The step vector is S[a] = floor(256 * d[a] / |d| + 0.5), written
 *                out as a literal table.  Up to sign and permutation its entries are (256,0,0), (229,114,0), (181,181,0),
 *                (209,105,105), (171,171,85) and (148,148,148).
 *   Weight.      w_k = max(0, (N . S_k) >> 8).
 *   Origin.      O = P + 2 * N: just under one voxel of the level along the normal, out of the surface.
 *   Probe.       For a direction k with w_k > 0 and j = 1..steps, form Q = O + j * S_k and c[a] = (Q[a] + 128) >> 8.  The probe
 *                ends unoccluded at the first c outside the grid, in the sense above.  It ends occluded at the first solid c,
 *                with hit = j.  It ends unoccluded after `steps` air samples.
 *   Byte.        tot = steps * sum of w_k.  occ = sum over occluded k of w_k * (steps + 1 - hit_k).
 *                ao = tot ? 255 - (255 * occ) / tot : 255, as uint32 with integer division.
 *
 *   Parameters  steps = 1..VX_OCCLUSION_MAX_STEPS, the reach of a probe in voxels of the level; flags = 0 or
 *               VX_OCCLUSION_TRANSITIONS (bake the vertices of the six transition meshes too); box_min / box_max in mesh space:
 *               a table entry is visited by the rule of vx_scatter - its min_corner / max_corner box meets the filter box on
 *               every axis, -INF / +INF allowed; the reserved words are zero.
 *   Baked       the regular vertex range of every visited entry of vx_device_block_table(level), plus its six transition ranges
 *               with the flag.  Only these bytes are written; every other byte of the array keeps its value, which is what makes
 *               a re-bake after vx_polygonize_dirty with the edit's box (grown by the reach) as filter cheap.
 *   Counts      vertices = vertices baked by this call, sum = the sum of their bytes, entries / visited_entries of the table,
 *               darkest = the least byte written (255 when none), open = baked vertices whose byte is 255.  Integer sums and
 *               maxima only (the least byte is kept as the greatest complement): nothing depends on an order or a schedule.
 *   Scope       Meshes and tables are those of the last run, as for vx_scatter.  The grid is the grid as it is NOW: after an edit
 *               and before the next run, the bake uses the old vertices against the new samples.
 * vx_occlusion_device takes d_ao and d_counts (8-byte aligned, may be NULL) as device pointers, is enqueued on the context's
 * stream (vx_set_stream) and returns without waiting: one kernel launch, and with d_counts a clear of 32 bytes before it and a
 * launch of one lane behind it.  It allocates nothing once the working memory exists.  vx_occlusion takes host arrays and is
 * synchronous: it bakes into a staging buffer kept with the context, pre-filled with 255, and copies the pool's n_verts bytes
 * back, so bytes of vertices the call did not bake read 255.  capacity (in bytes = vertices) must be at least the pool's
 * n_verts.  A level with an empty table gives VX_OK with zero counts and darkest = 255.
 * Neither call changes the grid, the pools, the tables or any kept state: a full run afterwards is what it would have been.
 * Everything is checked before anything is launched and nothing is written on an error: VX_ERR_INVALID for a null context, a
 * context that does not own a whole grid (slab and attached contexts, as for the brushes), no surface, level >= the levels of
 * the last run, null params, steps outside 1..VX_OCCLUSION_MAX_STEPS, an unknown flag bit, a non-zero reserved word, a NaN in a
 * box, box_min > box_max on an axis, a null array, capacity < n_verts, misaligned device counts.  VX_ERR_DEVICE when working
 * memory cannot be allocated.
 * Working memory, kept with the context, grown when a call needs more and released with the context: 256 bytes for the counts,
 * and for vx_occlusion one byte per pool vertex.  vx_occlusion_device with d_counts == NULL uses none. */
#define VX_OCCLUSION_MAX_STEPS 12
#define VX_OCCLUSION_TRANSITIONS 1u      /* flags: bake the six transition meshes' vertices too */
typedef struct vx_occlusion_params {     /* 48 bytes */
    uint32_t steps;                      /* 1..VX_OCCLUSION_MAX_STEPS: reach of a probe, in voxels of the level */
    uint32_t flags;
    float    box_min[3], box_max[3];     /* mesh space; an entry is visited by the rule of vx_scatter ("visited"); -INF/+INF allowed */
    uint32_t reserved[4];                /* 0 */
} vx_occlusion_params;
typedef struct vx_occlusion_counts {     /* 32 bytes */
    uint64_t vertices;                   /* vertices baked by this call */
    uint64_t sum;                        /* sum of their bytes */
    uint32_t entries, visited_entries;
    uint32_t darkest;                    /* least byte written, 255 when none */
    uint32_t open;                       /* baked vertices whose byte is 255 */
} vx_occlusion_counts;
int  vx_occlusion_device(vx_ctx* ctx, uint32_t level, const vx_occlusion_params* params /* host */,
                         uint8_t* d_ao /* device */, uint64_t capacity, vx_occlusion_counts* d_counts /* device, may be NULL */);
int  vx_occlusion(vx_ctx* ctx, uint32_t level, const vx_occlusion_params* params,
                  uint8_t* ao /* host */, uint64_t capacity, vx_occlusion_counts* counts /* host, may be NULL */);
/* tests: whether the per-block sign summaries may stand in for distance rows (the default: yes); nothing of a result depends on
 * it */
int  vx_debug_occlusion_shortcuts(vx_ctx* ctx, uint32_t enable);

/* MaterialMap::GetMaterial resolved on the host (include/MaterialMap.h:19-30): lut[id] = {DiffuseIds0[3],
 * DiffuseIds1[3]}, valid[id] == 0 means GetMaterial returned NULL (texture bytes stay 0). */
int vx_material_lut(vx_ctx* ctx, const uint8_t* lut /*256*6*/, const uint8_t* valid /*256*/);

/* ---- polygonization = TransVoxelRun::Execute (src/TransVoxelImpl.cpp:468-538) ------------------------ */
/* num_levels = 0: all log2(n/16)+1 levels like the reference; otherwise only levels 0..num_levels-1 (the
 * "last level has no transitions" rule still uses the reference's level count). */
/* When the call returns, the run's header (info, vx_stats) is complete and every mesh is in the pools; on the single-stream path
 * the run's last kernel may still be writing the device block tables.  Whatever is queued on the context's stream afterwards is
 * ordered behind it, another vx_polygonize included (which does not wait for the stream), and every other entry point of the
 * context waits for it first.  Only work of the caller's own on ANOTHER stream that reads the block tables has to order itself
 * behind the context's stream.  VX_SYNC_WAIT=1 (read when the context is created) makes every run wait for its stream. */
int vx_polygonize(vx_ctx* ctx, uint32_t num_levels, vx_exec_info* info);
/* The same run without the meshes of the levels below first_meshed_level - for a caller that gets those from other devices
 * (libVoxels.so with VOXELS_DEVICES = N: helper contexts polygonize the finer levels slab by slab) but needs everything a later
 * Modification continues from in THIS context: the slot maps, non-trivial / consistency bitmaps and material caches of every level
 * (the reference keeps them in the PolygonMap, src/TransVoxelImpl.h:81-133; a Modification reads the caches of blocks it does not
 * rebuild, :753-838).  Levels below first_meshed_level list no blocks and count nothing into the statistics; info->first_meshed_level
 * says what the run really did (0 where the partial form is not available - dense surfaces, stage timing: every level was meshed). */
int vx_polygonize_from(vx_ctx* ctx, uint32_t num_levels, uint32_t first_meshed_level, vx_exec_info* info);
/* Incremental re-polygonization of a dirty box (src/TransVoxelImpl.cpp:429-465); corners in OUTPUT (Y-up)
 * coordinates as Grid::InjectSurface returns them.  Returns the new block ids. */
int vx_polygonize_dirty(vx_ctx* ctx, const float min_corner[3], const float max_corner[3], vx_exec_info* info,
                        uint32_t* modified_ids, uint32_t cap, uint32_t* count);

/* Incremental runs append rebuilt blocks to the output pools and leave the replaced blocks' ranges behind.  This packs
 * the live meshes to the front of fresh pools on the device (offsets reported by vx_level_ranges change, contents and
 * order of everything downloaded do not).  vx_polygonize_dirty calls it by itself once more than half of the pools is
 * dead; applications holding device pointers may call it at a time of their choosing. */
int vx_compact_pools(vx_ctx* ctx);

/* ---- results (PolygonSurface accessors, include/Polygonizer.h:136-178) ------------------------------- */
int vx_level_counts(vx_ctx* ctx, uint32_t level, uint32_t* n_blocks, uint64_t totals[4] /* verts, idx, tverts, tidx */);
/* Blocks of one level in GetBlockForLevel order, concatenated: regular vertices/indices, then per block the
 * transition vertices/indices of faces 0..5.  Any output pointer may be NULL. */
int vx_download_level(vx_ctx* ctx, uint32_t level, vx_block_info* infos, vx_vertex* verts, uint32_t* idx,
                      vx_vertex* tverts, uint32_t* tidx);
/* Device-resident hand-off (renderer interop): the meshes stay in two device pools; a block's meshes are contiguous
 * ranges of them.  A full run that hands out pool ranges rewrites both pools; a full run that keeps the mesh layout
 * (vx_layout_keep_counts out[1]) leaves the index pool's bytes alone (vx_index_keep_counts) - they are what it would store -
 * and of the regular vertices it rewrites only the texture bytes, tex[8], where they were (vx_geometry_keep_counts; position,
 * secondary position, secW and normal are what it would store; transition vertices are rewritten whole); an incremental run appends the rebuilt blocks behind what is there
 * (ranges of kept blocks stay valid, ranges of replaced blocks become garbage until the next full run).  The pools are
 * read-only for the caller, as the const pointers say: a kept run relies on the index and geometry bytes it finds.  d_verts /
 * d_indices are valid until the next run on this context (an incremental run may move the pools when it has to grow
 * them); indices are relative to the start of their own mesh, exactly as downloaded. */
typedef struct vx_block_ranges {
	uint32_t v_off, i_off;        /* first vertex / first index of the regular mesh in the pools */
	uint32_t tv_off[6], ti_off[6]; /* the same for the six transition meshes */
} vx_block_ranges;
int vx_device_meshes(vx_ctx* ctx, const vx_vertex** d_verts, const uint32_t** d_indices, uint64_t* n_verts, uint64_t* n_indices);
int vx_level_ranges(vx_ctx* ctx, uint32_t level, vx_block_ranges* ranges /* one per block, vx_download_level order */);
/* The same two pools for a renderer in ANOTHER process (or behind another API's external-memory import): inter-process
 * handles of the two device allocations (hipIpcGetMemHandle; on this platform dmabuf-backed, HSA_ENABLE_IPC_MODE_LEGACY=0).
 * The importer maps them with hipIpcOpenMemHandle and reads n_verts vertices / n_indices indices from the mapping's start;
 * vx_level_ranges / vx_device_block_table (copied over by the application) say which ranges are which block's.  The reference
 * hands out per-block host arrays (include/Polygonizer.h:72-99); this is their device-resident, cross-process form.
 * `generation` changes whenever the pools were rewritten or replaced (every full run; an incremental run that had to pack
 * or grow them): an importer holding a mapping of an older generation must drop it and ask again.  Appending incremental
 * runs keep the generation and only raise the counts.  Exporter and importer must run on the same HIP runtime (a handle of
 * ROCm 7.0's runtime is not accepted by 7.2's hipIpcOpenMemHandle: tests/ipc_reader.py). */
typedef struct vx_ipc_meshes {
	uint8_t verts_handle[64], indices_handle[64]; /* hipIpcMemHandle_t, bytewise */
	uint64_t n_verts, n_indices;
	uint64_t verts_capacity, indices_capacity;    /* elements the allocations hold (what an appending run may still fill) */
	uint64_t generation;
} vx_ipc_meshes;
int vx_export_meshes(vx_ctx* ctx, vx_ipc_meshes* out);
/* Host copy of both pools in ONE step (what BlockPolygons::GetVertices / GetIndices, include/Voxels.h:210-231, hand out —
 * per-block arrays — as views: block k of a level owns verts[ranges[k].v_off ..] etc., with vx_level_ranges /
 * vx_download_level(infos only) giving offsets and counts).  The copy lands in page-locked memory at DMA speed and is
 * not copied again: the caller owns `arena` (and with it verts / indices) until vx_host_meshes_release, independent of
 * later runs and of the context's lifetime.  Released arenas are recycled by the next acquire (page-locking memory is
 * slow; a steady caller never pays it twice).
 * in/out: meshes->arena == NULL asks for a fresh copy; an arena returned by an earlier acquire on the same context is
 * brought up to date instead (after incremental runs only the appended part of the pools travels; it may be exchanged
 * for a larger one - always use the returned pointers). */
typedef struct vx_host_meshes {
	const vx_vertex* verts;
	const uint32_t* indices;
	uint64_t n_verts, n_indices;
	void* arena;
} vx_host_meshes;
int vx_host_meshes_acquire(vx_ctx* ctx, vx_host_meshes* meshes);
void vx_host_meshes_release(void* arena);
/* frees the recycled arenas of this process (optional; e.g. before unloading the library) */
void vx_host_meshes_trim(void);
/* Page-locks an arena for at least n_verts vertices and n_indices indices ahead of time and puts it into the process's
 * recycling list: the first vx_host_meshes_acquire of that size then finds it instead of page-locking inside the call
 * (locking 0.5 GB takes ~130 ms on the bench host, copying into it 9 ms).  What InitializeVoxels does when
 * VOXELS_PREWARM_MB is set (reference src/Voxels.cpp:35-60 is where an application pays one-time costs). */
int vx_host_meshes_reserve(vx_ctx* ctx, uint64_t n_verts, uint64_t n_indices);
/* The same lists as a device-resident table: what PushBlocksToResult (src/TransVoxelImpl.cpp:1266-1293) assembles per
 * block — ranges of its 1 + 6 meshes in the pools, id (:149-152), Y-up corners (:1283-1293) — for the blocks of one level
 * in GetBlockForLevel order (:395-401; blocks without a regular vertex are left out, :1274).  A full run writes the
 * tables on the device as its last step, so a renderer can consume a run without any host round trip beyond the
 * per-level counts; after an incremental run the (host-maintained) lists are uploaded on the first call.
 * The table is valid until the next run on this context. */
typedef struct vx_listed_block {
	uint32_t coord_id;                     /* (bz * cnt + by) * cnt + bx, internal axes (Z up) */
	uint32_t v_off, v_count, i_off, i_count;
	uint32_t tv_off[6], tv_count[6], ti_off[6], ti_count[6];
	uint32_t degenerate, nt_cells, reserved;
	uint32_t id;
	float min_corner[3], max_corner[3];
} vx_listed_block;
int vx_device_block_table(vx_ctx* ctx, uint32_t level, const vx_listed_block** d_table, uint32_t* n_blocks);

/* ---- ray casts against the device-resident meshes ---------------------------------------------------------------------
 * The nearest intersection of each ray with the triangles of the REGULAR meshes of one LOD level, as the last run on this
 * context left them (the blocks of vx_device_block_table(level), vx_download_level order).  No reference counterpart: the
 * reference leaves picking to the application over its host-resident meshes (doc_source/Rendering.md).
 *   space   mesh space, the space of vx_vertex.pos: Y-up, voxel units.  vx_grid_inject_ball takes grid coordinates (Z-up):
 *           swap y and z of a hit's pos before carving at it.
 *   range   only hits with t_min <= t <= t_max count; t is in units of |dir| (dir need not be unit length).
 *   faces   both faces of a triangle count (rays may start inside caves or inside solid); watertight test (Woop, Benthin,
 *           Wald 2013): a ray through a shared edge or vertex of a closed part of the mesh does not pass through it.
 *   ties    among hits at equal t the smallest (entry, tri) is reported.
 *   misses  zero or NaN dir, NaN origin, t_min > t_max, or no triangle hit (a ray that never enters [0, n]^3 hits
 *           nothing): t = +INF, entry = block_id = tri = UINT32_MAX, every other field 0.
 *   scope   transition meshes and secondary positions are not intersected.
 *   stale   after a grid edit, and until the next run, results describe the OLD meshes.
 * The acceleration index of a level (block-coordinate -> entry map, per block a bucket sort of its triangles over its 4^3
 * sub-bricks) is built on demand and goes stale with every full run, incremental run and vx_compact_pools on the context. */
typedef struct vx_ray {
	float origin[3];
	float t_min;
	float dir[3];
	float t_max;
} vx_ray;                 /* 32 bytes */
typedef struct vx_ray_hit {
	float t;              /* +INF on a miss */
	float pos[3];         /* origin + t*dir, mesh space */
	float nrm[3];         /* unit (v1-v0)x(v2-v0) of the hit triangle in index order, not flipped toward the ray */
	float bary[2];        /* weights of the triangle's 2nd and 3rd vertex */
	uint32_t entry;       /* index into the level's block table / vx_download_level order */
	uint32_t block_id;    /* BlockPolygons::GetId of that block */
	uint32_t tri;         /* triangle ordinal in the block's regular mesh: its indices 3*tri .. 3*tri+2 */
} vx_ray_hit;             /* 48 bytes */
typedef struct vx_ray_index_info {
	uint64_t triangles;   /* regular triangles of the level */
	uint64_t bytes;       /* device memory of the level's index (map, bucket starts, its share of the triangle permutation) */
	uint32_t blocks;      /* entries of the level's block table */
	uint32_t straddling;  /* triangles not inside the closed box of their sub-brick (+-1/256): must be 0 */
	float build_ms;       /* device time of the last build of this level's index (HIP events) */
} vx_ray_index_info;
/* Builds the level's index, or keeps it if it is current; info (may be NULL) receives its figures. */
int vx_raycast_prepare(vx_ctx* ctx, uint32_t level, vx_ray_index_info* info);
/* Device arrays: enqueued on the context's stream (vx_set_stream), returns without waiting.  With a current index: no
 * allocation, no copy, no synchronisation, one kernel launch; otherwise vx_raycast_prepare first. */
int vx_raycast_device(vx_ctx* ctx, uint32_t level, const vx_ray* d_rays, uint32_t n, vx_ray_hit* d_hits);
/* Host arrays, synchronous (picking). */
int vx_raycast(vx_ctx* ctx, uint32_t level, const vx_ray* rays, uint32_t n, vx_ray_hit* hits);
/* All three: VX_ERR_INVALID for a level at or beyond what the last run produced, a context without a surface, and null
 * pointers with n > 0; n = 0 returns VX_OK and does nothing. */

/* ---- sphere casts and closest points against the device-resident meshes ----------------------------------------------
 * Collision queries against the same triangles as the ray casts (no reference counterpart: doc_source/Rendering.md leaves
 * collision to the application): where a sphere moving along a segment first touches the surface, and the nearest surface
 * point within a distance.  They read the level's ray-cast index (vx_raycast_prepare) and need no memory of their own.
 *   space   mesh space (Y-up, voxels), against the REGULAR triangles of one level as the last run on this context left them;
 *           transition meshes are not queried.  After a grid edit, and until the next run, results describe the OLD meshes.
 *   sphere  the hit is the least t in [t_min, t_max] at which dist(origin + t*dir, triangle) <= radius, over all triangles,
 *           both faces; t is in units of |dir|.  A sphere that already touches a triangle at t_min hits at t = t_min with flag
 *           VX_SPHERE_STARTED_IN_CONTACT and depth = radius - the least distance at t_min; contact and nrm then come from the
 *           nearest triangle at t_min.  dir = 0 is allowed: a static overlap test at t_min.
 *   misses  a NaN in origin or dir, a radius that is not finite or not > 0, t_min > t_max, or no contact: t = +INF,
 *           entry = block_id = tri = UINT32_MAX, every other field 0.
 *   closest the least distance from pos to any triangle, counted only if it is <= max_dist (which may be +INF: the whole
 *           level).  NaN pos, or a NaN or negative max_dist, is a miss, encoded as for sphere casts (dist = +INF).
 *   ties    among equal t (or equal dist) the smallest (entry, tri) is reported (at t_min: the nearest triangle first).
 * Sizes are multiples of 16 bytes: device arrays must be 16-byte aligned. */
#define VX_SPHERE_STARTED_IN_CONTACT 1u
typedef struct vx_sphere_cast {
	float origin[3];
	float t_min;
	float dir[3];
	float t_max;
	float radius;
	float reserved[3];    /* 0 */
} vx_sphere_cast;         /* 48 bytes */
typedef struct vx_sphere_hit {
	float t;              /* +INF on a miss */
	float center[3];      /* origin + t*dir */
	float contact[3];     /* the touched point of the triangle */
	float nrm[3];         /* unit (center - contact); the face normal (index order) if the centre lies on the triangle */
	float depth;          /* radius - distance at t_min when the cast starts in contact, else 0 */
	uint32_t entry;       /* index into the level's block table / vx_download_level order */
	uint32_t block_id;    /* BlockPolygons::GetId of that block */
	uint32_t tri;         /* triangle ordinal in the block's regular mesh */
	uint32_t flags;       /* bit 0: VX_SPHERE_STARTED_IN_CONTACT */
	uint32_t reserved;    /* 0 */
} vx_sphere_hit;          /* 64 bytes */
typedef struct vx_point_query {
	float pos[3];
	float max_dist;
} vx_point_query;         /* 16 bytes */
typedef struct vx_point_hit {
	float dist;           /* +INF when nothing lies within max_dist */
	float point[3];       /* nearest point of the level's regular triangles */
	float nrm[3];         /* unit (v1-v0)x(v2-v0) of that triangle, as vx_ray_hit.nrm */
	float bary[2];        /* weights of its 2nd and 3rd vertex */
	uint32_t entry, block_id, tri;
} vx_point_hit;           /* 48 bytes */
/* Device arrays: enqueued on the context's stream (vx_set_stream), returns without waiting.  With a current index: no
 * allocation, no copy, no synchronisation, one kernel launch; otherwise vx_raycast_prepare first. */
int vx_spherecast_device(vx_ctx* ctx, uint32_t level, const vx_sphere_cast* d_casts, uint32_t n, vx_sphere_hit* d_hits);
/* Host arrays, synchronous. */
int vx_spherecast(vx_ctx* ctx, uint32_t level, const vx_sphere_cast* casts, uint32_t n, vx_sphere_hit* hits);
int vx_closest_point_device(vx_ctx* ctx, uint32_t level, const vx_point_query* d_q, uint32_t n, vx_point_hit* d_hits);
int vx_closest_point(vx_ctx* ctx, uint32_t level, const vx_point_query* q, uint32_t n, vx_point_hit* hits);
/* All four: VX_ERR_INVALID for a level at or beyond what the last run produced, a context without a surface, and null
 * arrays with n > 0; n = 0 returns VX_OK and does nothing. */

/* ---- LOD selection: which block of which level to draw, with indirect draw lists -----------------------------------------
 * Each frame a renderer picks, per region, one level's block, frustum-culls it and draws the transition meshes of the faces
 * where it meets a finer block (doc_source/Rendering.md of the reference leaves this to the client).  These entry points do
 * it next to the block tables and write draw-indexed-indirect commands.  Mesh space (Y-up, voxels) throughout.
 *   nodes      R = the reference's level count (log2(n/16) + 1, rounded down), T = levels of the last run - 1.  Level L has
 *              cnt_L = (n/16) >> L nodes per axis; node (L, c) covers the internal (Z-up) box [c s, (c+1) s]^3, s = 16 * 2^L,
 *              and the mesh-space box with y and z swapped (what vx_listed_block.min_corner / max_corner report).  Its parent
 *              is (L+1, c >> 1) when L < T and c >> 1 < cnt_{L+1} on every axis; otherwise it is a root.  The roots of all
 *              levels partition [0, n)^3 (sizes whose n/16 is not a power of two have bands only finer levels cover).
 *   selection  O = the least set of opened nodes (levels >= 1) with
 *              (1) distance: ranges[L] > 0 and d^2 < ranges[L] * ranges[L]  ->  node in O;
 *              (2) closure: X in O and X has a parent  ->  parent(X) in O;
 *              (3) balance: X active at level L >= 1 (a root, or its parent in O) and a leaf of level <= L - g(L) shares a face
 *                  area with X  ->  X in O; g(L) = 1 for L = R - 1 (no transition meshes), 2 otherwise.
 *              The leaves (active nodes not in O) are the selection; it is purely spatial (n, R, T, camera, ranges).
 *   distance   float32, no contraction: d_a = max(max(min_a - cam_a, 0), cam_a - max_a); d^2 = (dx dx + dy dy) + dz dz.
 *   drawn      a leaf whose level's block table has an entry for its coord_id, unless culled: for some plane (a, b, c, d)
 *              (inside: a x + b y + c z + d >= 0), ((a px + b py) + c pz) + d < 0 in float32, p = the box corner that
 *              maximises the plane (px = a >= 0 ? max.x : min.x, ...).  A culled leaf emits nothing.
 *   faces      transitions bit f (BlockPolygons::TransitionFaceId order: -Y, -Z, -X, +Y, +Z, +X) = a leaf of a smaller level
 *              (by (3): level L - 1, over the whole face) touches face f.  adjacency = the blockAdj of Rendering.md, in the bit
 *              order of vertex.sec[3]: a regular vertex with bit b set lies on transition face b, so adjacency = transitions.
 *   order      records by level, then by block-table entry.  Per record one regular command (i_count, 1, i_off, v_off,
 *              record) and, in a second array, per set bit f with ti_count[f] > 0 one transition command (ti_count[f], 1,
 *              ti_off[f], tv_off[f], record), in record order then face order.  first_instance = record index.
 *   stale      tables, offsets and counts are those of the last run (vx_device_block_table).
 * The selection keeps per-level node flags (about 1.14 (n/16)^3 bytes) and per-entry scratch on the device, allocated on first
 * use and shared by every selection on the context: calls on one context must be ordered on one stream (a call queued on
 * another stream, after vx_set_stream, may overwrite them while an earlier call still reads them). */
typedef struct vx_lod_params {
	float camera[3];          /* mesh space (Y-up), voxels */
	uint32_t n_planes;        /* 0..6; 0 = no culling */
	float planes[6][4];       /* (a, b, c, d): inside where a x + b y + c z + d >= 0 */
	float ranges[16];         /* ranges[L] for L >= 1; <= 0: never split by distance; ranges[0] ignored */
} vx_lod_params;              /* 176 bytes */
typedef struct vx_lod_draw {
	uint32_t level, entry;    /* the block: entry of vx_device_block_table(level) */
	uint32_t block_id;        /* BlockPolygons::GetId */
	uint32_t coord_id;        /* (bz * cnt + by) * cnt + bx, internal axes */
	uint32_t transitions;     /* TransitionFaceId bits: faces that meet a finer leaf */
	uint32_t adjacency;       /* blockAdj for the vertex shader (vertex.sec[3] bit order; equal to transitions) */
	uint32_t reserved[2];     /* 0 */
} vx_lod_draw;                /* 32 bytes */
typedef struct vx_draw_indexed {  /* VkDrawIndexedIndirectCommand / D3D12_DRAW_INDEXED_ARGUMENTS */
	uint32_t index_count, instance_count /* 1 */, first_index;
	int32_t vertex_offset;
	uint32_t first_instance;  /* record index */
} vx_draw_indexed;            /* 20 bytes */
typedef struct vx_lod_counts {
	uint32_t records;         /* drawn leaves (what the arrays would hold with unlimited capacity) */
	uint32_t regular;         /* regular commands (= records) */
	uint32_t transition;      /* transition commands */
	uint32_t leaves;          /* all leaves, meshed or not */
	uint32_t meshed_leaves;   /* leaves with a block-table entry */
	uint32_t culled_leaves;   /* meshed leaves the frustum culled */
	uint64_t leaf_volume;     /* sum over leaves of 8^L in level-0 blocks: always (n/16)^3 */
} vx_lod_counts;              /* 32 bytes */
/* Device arrays (16-byte aligned), enqueued on the context's stream (vx_set_stream), returns without waiting: a handful of
 * launches, no copy, no synchronisation, and no allocation once the node flags exist.  Always writes the full counts; fills
 * the arrays up to their capacities (draw_capacity for draws and regular, transition_capacity for transition). */
int vx_lod_select_device(vx_ctx* ctx, const vx_lod_params* params, uint32_t draw_capacity, uint32_t transition_capacity,
                         vx_lod_draw* d_draws, vx_draw_indexed* d_regular, vx_draw_indexed* d_transition, vx_lod_counts* d_counts);
/* Host arrays, synchronous.  VX_ERR_OVERFLOW (after writing the counts and the first `capacity` entries) when a capacity
 * was too small; the levels' table entries summed are always enough for the draws. */
int vx_lod_select(vx_ctx* ctx, const vx_lod_params* params, uint32_t draw_capacity, uint32_t transition_capacity,
                  vx_lod_draw* draws, vx_draw_indexed* regular, vx_draw_indexed* transition, vx_lod_counts* counts);
/* Both: VX_ERR_INVALID for a context without a surface, a last run that left levels unmeshed (vx_polygonize_from with
 * first_meshed_level > 0), a NaN camera, plane or range, n_planes > 6, null params or counts, and null arrays with a
 * non-zero capacity. */

/* ---- scattering: seeded instance points on a level's meshes ------------------------------------------------------------------
 * Places points (grass, rocks, trees, decals, spawn points) on the surface, next to the meshes, as an instance buffer a
 * renderer can draw from; vx_scatter_range addresses each block's points by vx_lod_draw.entry.  No reference counterpart:
 * doc_source/Rendering.md leaves everything after the vertex buffers to the client.
 *   scope      the REGULAR triangles of one level, as the last run on this context left them (the blocks of
 *              vx_device_block_table(level)): the scope and staleness of the ray casts.  Transition meshes are not scattered
 *              on.  Mesh space: Y-up, voxels.
 *   hash       mix(x): x ^= x>>16; x *= 0x7feb352d; x ^= x>>15; x *= 0x846ca68b; x ^= x>>16, uint32 arithmetic that wraps.
 *              U(h) = (float)(h >> 8) * 2^-24 (exact).  Per block hb = mix(seed ^ mix(coord_id + 0x9E3779B9 * (level + 1))); per
 *              triangle ordinal t, ht = mix(hb + t * 0x85EBCA6B); draw j of a triangle d(j) = mix(ht ^ (j * 0xC2B2AE35)), so
 *              d(0) = mix(ht).  The key is (seed, level, coord_id, t, j), all spatial - not block_id, a running counter: the
 *              same surface gives the same points whether it came from a full run or from a chain of incremental runs.
 *   visited    an entry is visited when its table box meets the filter box: min_corner[a] <= box_max[a] && max_corner[a] >=
 *              box_min[a] on every axis.  Other entries get count = 0 and none of their triangles are looked at.
 *   candidates of triangle t (vertices v0, v1, v2 in index order), in float32, one rounding per written operation, no
 *              contraction: e1 = v1 - v0, e2 = v2 - v0; c = (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x);
 *              l2 = (c.x*c.x + c.y*c.y) + c.z*c.z; m = min((0.5f * sqrtf(l2)) * density, 65535.0f); base = (uint32)m;
 *              frac = m - (float)base; count = base + (U(d(0)) < frac ? 1 : 0).  No candidates when l2 is zero or not finite,
 *              or when the texture mask rejects the triangle.
 *   candidate  k in 0..count-1: r1 = U(d(3k+1)), r2 = U(d(3k+2)); if r1 + r2 > 1.0f then r1 = 1.0f - r1, r2 = 1.0f - r2;
 *              rand = U(d(3k+3)).  Per axis pos = v0 + (e1*r1 + e2*r2) and g = n0 + ((n1 - n0)*r1 + (n2 - n0)*r2);
 *              gl = sqrtf((g.x*g.x + g.y*g.y) + g.z*g.z); nrm = g / gl when gl > 0, else zeros.  A candidate is kept when it
 *              passes the up and box comparisons given in the struct.  Filters never change a draw: the filtered output is
 *              the unfiltered output with the predicate applied.
 *   normals    vertex normals are the normalised grid gradient, so they point from solid to air: a floor has nrm.y > 0, a
 *              ceiling nrm.y < 0.
 *   order      points by entry, then triangle ordinal, then k; no atomics decide order.  ranges[e] = {points before entry e,
 *              kept points of entry e} for every entry of the table.  Arrays are filled up to `capacity`; counts is always
 *              complete.  If points > UINT32_MAX, no point or range is written.
 *   stale      tables, offsets and meshes are those of the last run (vx_device_block_table).
 * The per-entry scratch (32 bytes per entry of the largest table) is kept with the context and only ever grown; calls on one
 * context must be ordered on one stream, as for the LOD selection. */
#define VX_SCATTER_MAX_DENSITY 64.0f
#define VX_SCATTER_MAX_PER_TRIANGLE 65535u
typedef struct vx_scatter_params {      /* 80 bytes */
	uint32_t seed;
	float    density;          /* expected points per unit of mesh area (voxel^2): finite, 0 < density <= VX_SCATTER_MAX_DENSITY */
	float    min_up, max_up;   /* keep points with min_up <= nrm.y <= max_up (mesh space, Y up); -1 / +1 = any slope */
	float    box_min[3], box_max[3]; /* keep points with box_min <= pos <= box_max per axis, mesh space; -INF / +INF allowed */
	uint32_t texture_slot;     /* 0..7: which byte of vx_vertex.tex the mask reads */
	uint32_t texture_mask[8];  /* 256 bits; a triangle takes part when bit tex[texture_slot] of its FIRST vertex is set; all ones = any */
	uint32_t reserved;         /* 0 */
} vx_scatter_params;
typedef struct vx_scatter_point {       /* 48 bytes */
	float pos[3];  float rand;          /* rand in [0,1): for the application's scale / rotation / variant */
	float nrm[3];  uint32_t entry;      /* interpolated vertex normal, unit; entry of vx_device_block_table(level) */
	uint32_t block_id, tri, tex[2];     /* BlockPolygons::GetId; triangle ordinal; the first vertex's 8 tex bytes as TI[0], TI[1] */
} vx_scatter_point;
typedef struct vx_scatter_range { uint32_t first, count; } vx_scatter_range;   /* per table entry */
typedef struct vx_scatter_counts {      /* 32 bytes */
	uint64_t points;            /* what unlimited capacity would hold */
	uint64_t candidates;        /* candidate points evaluated, before the per-point filters */
	uint32_t triangles;         /* triangles of visited entries that pass the texture mask */
	uint32_t entries, visited_entries, reserved;
} vx_scatter_counts;
/* Device arrays (16-byte aligned; d_ranges: 8), enqueued on the context's stream (vx_set_stream), returns without waiting:
 * three launches, no copy, no synchronisation, and no allocation once the per-entry scratch exists. */
int vx_scatter_device(vx_ctx*, uint32_t level, const vx_scatter_params* params /* host */, uint32_t capacity,
                      vx_scatter_point* d_points, vx_scatter_range* d_ranges /* may be NULL */, vx_scatter_counts* d_counts);
/* Host arrays, synchronous.  VX_ERR_OVERFLOW when points > capacity, after writing the counts, the ranges and the first
 * `capacity` points (as vx_lod_select does). */
int vx_scatter(vx_ctx*, uint32_t level, const vx_scatter_params* params, uint32_t capacity,
               vx_scatter_point* points, vx_scatter_range* ranges /* may be NULL */, vx_scatter_counts* counts);
/* Both: VX_ERR_INVALID, before anything is launched, for a context without a surface, a level at or beyond what the last run
 * produced, null params or counts, a null point array with a non-zero capacity, a density that is not finite or outside
 * (0, VX_SCATTER_MAX_DENSITY], a NaN in any float field, min_up > max_up, box_min > box_max on an axis, texture_slot > 7,
 * reserved != 0, and (device form) misaligned arrays.  A level with an empty table is VX_OK with zero counts (written). */

/* ---- overlap queries: a level's triangles that meet query boxes --------------------------------------------------------------
 * Which triangles are near this body: what a physics engine asks its triangle-mesh collider before narrow phase (Bullet's
 * processAllTriangles(aabbMin, aabbMax), the custom mesh shapes of PhysX and Jolt), and also "is this spot free" (count only),
 * "the surface under this decal", "the meshes of this region".  No reference counterpart: doc_source/Rendering.md leaves
 * collision to the application.
 *   scope      the REGULAR triangles of one level, as the last run on this context left them (the blocks of
 *              vx_device_block_table(level)): the scope and staleness of the ray casts.  Transition meshes are not queried.
 *              Mesh space: Y-up, voxels.  The calls read the level's ray-cast index (vx_raycast_prepare) and build it on
 *              demand, as the sphere casts do.
 *   box        closed, [lo, hi] per axis; lo == hi is allowed (a plane, a line, a point), and so is +-INF.  A NaN in lo or hi,
 *              or lo[a] > hi[a] on any axis, makes an EMPTY query: count 0, not an error (the device form cannot validate
 *              device arrays).  The reserved words are ignored.
 *   match      triangle t of an entry, vertices v0, v1, v2 in index order, matches the box when on every axis a
 *              min(v0[a], v1[a], v2[a]) <= hi[a] and max(v0[a], v1[a], v2[a]) >= lo[a]: float32 comparisons of the stored
 *              positions and nothing else.  This is the triangle's bounding box against the query box, what the engines'
 *              callbacks deliver; regular triangles lie within one cell of their level, so the bounding box is never looser
 *              than a cell.  A separating-axis refinement is out of scope.
 *   result     one vx_overlap_tri per match: the query's index, the entry of vx_device_block_table(level), that entry's id,
 *              and the triangle's ordinal in the block's regular mesh (its indices 3*tri .. 3*tri+2).
 *   corners    with a non-null corners array, triangle k of the result also gets 48 bytes at corners + 12 k floats:
 *              v0.xyz, 0.0f, v1.xyz, 0.0f, v2.xyz, 0.0f - the position bytes of the vertex pool, so that a narrow phase needs
 *              no second gather.
 *   order      matches by query index, then by the block's coord_id ascending, then by tri ascending; no atomic decides
 *              order.  By coord_id and not by entry: after incremental runs the table's order is no function of position,
 *              and the result is the same list, up to entry and block_id, whether the surface came from a full run or from a
 *              chain of incremental ones (as vx_scatter promises of its points).  ranges[q] = {matches before query q,
 *              matches of query q} for every query.  Arrays are filled up to `capacity`; ranges and counts are always
 *              complete.  If the total exceeds UINT32_MAX, no match, corner or range is written.
 *   counts     triangles = what unlimited capacity would hold; pairs = the (query, entry) pairs with at least one match;
 *              hit_queries = the queries with at least one match; max_per_query = the largest ranges[q].count.  All are
 *              functions of the result set, none a count of work done.
 *   stale      tables, offsets and meshes are those of the last run (vx_device_block_table).
 * capacity == 0 with null output arrays is the count-only form.  The per-query scratch (16 bytes per query) is kept with the
 * context and only ever grown; calls on one context must be ordered on one stream, as for the LOD selection. */
#define VX_OVERLAP_MAX_QUERIES (1u << 20)
typedef struct vx_overlap_box { float lo[3]; uint32_t reserved0; float hi[3]; uint32_t reserved1; } vx_overlap_box;   /* 32 bytes */
typedef struct vx_overlap_tri { uint32_t query, entry, block_id, tri; } vx_overlap_tri;                               /* 16 bytes */
typedef struct vx_overlap_range { uint32_t first, count; } vx_overlap_range;                                          /* per query */
typedef struct vx_overlap_counts {      /* 32 bytes */
	uint64_t triangles;         /* what unlimited capacity would hold */
	uint64_t pairs;             /* (query, entry) pairs with at least one match */
	uint32_t queries, hit_queries, max_per_query, reserved;
} vx_overlap_counts;
/* Device arrays (16-byte aligned; d_ranges: 8), enqueued on the context's stream (vx_set_stream), returns without waiting.
 * With a current index: three launches, no copy, no synchronisation, and no allocation once the per-query scratch fits. */
int vx_overlap_boxes_device(vx_ctx*, uint32_t level, const vx_overlap_box* d_boxes, uint32_t n, uint32_t capacity,
                            vx_overlap_tri* d_tris, float* d_corners /* may be NULL */,
                            vx_overlap_range* d_ranges /* may be NULL */, vx_overlap_counts* d_counts);
/* Host arrays, synchronous.  VX_ERR_OVERFLOW when triangles > capacity, after writing the counts, the ranges and the first
 * `capacity` results (and their corners). */
int vx_overlap_boxes(vx_ctx*, uint32_t level, const vx_overlap_box* boxes, uint32_t n, uint32_t capacity,
                     vx_overlap_tri* tris, float* corners, vx_overlap_range* ranges, vx_overlap_counts* counts);
/* Both: VX_ERR_INVALID, before anything is launched, for a context without a surface, a level at or beyond what the last run
 * produced, null counts, null boxes with n > 0, n > VX_OVERLAP_MAX_QUERIES, a null tris with a non-zero capacity, non-null
 * corners with null tris, and (device form) misaligned arrays.  n == 0 is VX_OK with zero counts written; so is a level with
 * an empty table, with zero ranges as well. */

/* stats[0..3] = BlocksCalculated, TrivialCells, NonTrivialCells, DegenerateTrianglesRemoved; stats[4..19] =
 * PerCaseCellsCount (include/Polygonizer.h:110-132) */
int vx_stats(vx_ctx* ctx, uint32_t stats[20]);

/* Transition blocks of the last run (full or incremental) by the body that meshed them: out[0] = through the table-driven
 * body (no exact zero on the block's staged boundary planes, all its non-trivial transition cells in one batch), out[1] = through
 * the general phases although the table-driven body is on (VX_FAST bit 2).  Both 0 with the body off.  Diagnostics: the
 * meshes are the same either way. */
int vx_transition_path_counts(vx_ctx* ctx, uint32_t out[2]);

/* Material blocks (active blocks of the levels >= 1) of the last full run by how their material cache came about (both 0
 * behind an incremental run, which counts none): out[0] = voted from the children, out[1] = replayed - taken over from the
 * run that filled the material store (the last full single-stream run on this grid) where nothing the votes read has changed
 * since (distances, materials, blends, BF_Empty flags, the context's range): either copied from the store into the block's
 * slot or, in a run that keeps the slot plan (vx_slot_plan_counts), left in the slot, which still holds it.
 * VX_MATSTORE=0 (read at context creation) keeps no store: every run votes.  VX_MAT_INPLACE=0 (read at context creation)
 * leaves nothing in place: a run that keeps the slot plan copies from the store like every other replaying run.
 * Diagnostics: caches, meshes and statistics are the same either way. */
int vx_material_path_counts(vx_ctx* ctx, uint32_t out[2]);

/* Full-run attempts of this context (since it was created) whose material blocks were replayed, by how: out[0] = copied from
 * the material store into their slots (a run that hands out its slots, or VX_MAT_INPLACE=0), out[1] = left in place (a run
 * that keeps the slot plan: its upper queue has no material items, and its regular and transition blocks wait for nobody).
 * Attempts that voted count in neither.  Diagnostics: caches, meshes, statistics and vx_material_path_counts are the same
 * either way.  HIP builds only. */
int vx_material_inplace_counts(vx_ctx* ctx, uint64_t out[2]);

/* Full runs of this context (every attempt of vx_polygonize / vx_polygonize_from, since the context was created) by where their
 * slots came from: out[0] = handed out by the run itself (k_run_head, or the classification pass of the chain of launches),
 * out[1] = kept - a full single-stream run that read the cell map has handed them out, nothing they depend on has changed
 * since (BF_Empty flags, distances through the sign summaries and the cell counts, the context's range, the level count) and
 * nobody has handed out slots in between (incremental and partial runs do): the run launches no k_run_head, and its
 * device_ms starts with k_main.  VX_PLAN=0 (read at context creation) keeps no plan: every run hands out its slots.
 * Diagnostics: tables, meshes, statistics and vx_exec_info are the same either way.  HIP builds only. */
int vx_slot_plan_counts(vx_ctx* ctx, uint64_t out[2]);

/* Full-run attempts of this context that kept the slot plan (vx_slot_plan_counts out[1], since the context was created) by their
 * launches: out[0] = two, k_main and k_tail, out[1] = one, k_main alone - a run in place (vx_material_inplace_counts out[1]) on
 * slots whose last accepted run left its mesh layout behind: every block's record, the block lists with their totals and the
 * pool cursors, which depend on the grid, the BF_Empty flags, the level count and the slot plan alone (not on the material
 * table: vx_material_lut keeps the layout).  Such a run rewrites the texture bytes of every regular vertex, and every
 * transition vertex whole, where its record says they were (vx_geometry_keep_counts), leaves the index pool's bytes alone (vx_index_keep_counts; the pools are read-only for the caller), rebuilds no list, and
 * its last workgroup publishes the header.  Whatever drops the slot plan drops the layout, and so do vx_compact_pools, pools
 * that had to grow, and a run that handed a block to the general passes or met the large capacity class.
 * VX_LAYOUT=0 (read at context creation) keeps no layout: every kept run is two launches.
 * Diagnostics: block tables, mesh contents, statistics and vx_exec_info are the same either way.  The meshes' places in the pools
 * (vx_level_ranges) are not: a run of two launches reserves them anew, in the order its blocks arrive, while a run of one launch
 * writes every mesh where the run before left it - so with the layout kept the offsets stay the same from run to run.  HIP builds only. */
int vx_layout_keep_counts(vx_ctx* ctx, uint64_t out[2]);

/* Full-run attempts of this context that kept the mesh layout (vx_layout_keep_counts out[1], since the context was created) by
 * what they did with the index pool: out[0] = rewrote every index, out[1] = kept the indices - the pool already holds, byte for
 * byte, what the run would store: an index is a vertex base of the kept layout plus an ordinal that follows from the signs and
 * material ids of the unchanged grid, and nothing in it depends on the material table.  Such a run computes and stores the
 * texture bytes of every vertex (they do depend on the table; the rest of a vertex: vx_geometry_keep_counts), checks every block's index count against its record,
 * and neither forms nor stores the indices of the table-driven blocks; a transition block with an exact zero on a staged plane
 * still writes its (unchanged) indices.  Whatever drops the layout ends it: the next run rewrites the pool.
 * VX_KEEP_INDICES=0 (read at context creation): every run that keeps the layout rewrites the indices.
 * Diagnostics: pool contents, block tables, statistics and vx_exec_info are the same either way.  HIP builds only. */
int vx_index_keep_counts(vx_ctx* ctx, uint64_t out[2]);

/* Full-run attempts of this context that kept the mesh layout (vx_layout_keep_counts out[1], since the context was created) by
 * what they did with the regular vertices: out[0] = computed and stored whole vertices, out[1] = texture bytes only - bytes
 * 0..39 of a vertex (position, secondary position, secW, normal) are a function of the grid alone, which cannot have changed
 * while a layout is valid, and the pool holds them where the block's record says; bytes 40..47 (tex[8]) are the one part the
 * material table enters, and vx_material_lut is the real-use reason to run again on an unchanged grid.  Such a run computes the
 * texture bytes of every regular vertex afresh - the blend byte too: an invalid table row forces it to 0 - and rewrites them
 * with one 8-byte store per vertex; it reads no gradient, normalises nothing and forms no position.  Transition vertices
 * (8.6 % of all on the bench terrain) are written whole as ever, the same bytes.  Whatever drops the layout ends it: the next
 * run rewrites every vertex whole.
 * VX_KEEP_GEOMETRY=0 (read at context creation): every run that keeps the layout computes and stores whole vertices.
 * Diagnostics: pool contents, block tables, statistics and vx_exec_info are the same either way.  HIP builds only. */
int vx_geometry_keep_counts(vx_ctx* ctx, uint64_t out[2]);

/* The device forms of the exactness-critical arithmetic checked exhaustively on the GPU they run on (the reference does
 * this arithmetic on the host: t = (v1 << 8) / (v1 - v0), src/TransVoxelImpl.cpp:1591; normalizeFixZero, :93-103):
 * results[0] = crossed int8 sample pairs whose t differs from the truncated quotient, results[1] = gradients whose normal
 * changes when the gradient is scaled by 0.5, results[2] = gradients whose normal differs from fp32 sqrt + division;
 * results[11] = gradients whose normal differs between normalize_gradient (the cheaper form the fast passes use for the
 * end-point normals, valid for integer gradients only) and normalizeFixZero; all four must be 0.  results[3..10] count
 * mismatches of other candidate forms (informational). */
int vx_selftest(vx_ctx* ctx, uint32_t results[16]);

/* Optional per-stage device timing (HIP events between the kernels of vx_polygonize; adds a few event records).
 * ms[0..7] = reset + block classes, classify, hierarchy, material (all levels), regular cells of level 0, of the levels >= 1,
 * transition cells, block lists of the LAST run. */
int vx_set_stage_timing(vx_ctx* ctx, int enable);
/* What the eight slots of vx_stage_times meant in the last run with stage timing: 0 = the chain of launches (reset + block
 * classes, classify, hierarchy, material, regular level 0, regular levels >= 1, transition, block lists); 1 = the single-stream
 * form (k_reset + k_run_head, nothing, nothing, k_main, what follows k_main for level 0, ... for the levels >= 1, nothing,
 * block lists - with stage timing the parts of k_tail are launches of their own, so that they can be timed). */
int vx_stage_layout(vx_ctx* ctx, int* layout);
/* Diagnostics: the first `count` 32-bit words of the run's device header (queue heads, counters), copied on a stream of
 * its own so that it also works - from another host thread - while a run is in flight. */
int vx_debug_header(vx_ctx* ctx, uint32_t* out, uint32_t count);
int vx_stage_times(vx_ctx* ctx, float ms[8]);

/* name of the code object actually running the kernels ("hip:gfx950") — lets callers assert the native path */
const char* vx_backend(void);

#ifdef __cplusplus
}
#endif
#endif
