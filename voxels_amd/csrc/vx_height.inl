// vx_height.inl — the height maps (include/voxels_hip.h, "height maps"): vx_grid_heightmap and vx_grid_heightmap_device, the
// surface heights and materials per column of a voxel box of the resident grid, from the top or from the bottom, up to eight
// layers; included by vx_hip.hip after vx_overlap.inl (HIP only).  DESIGN.md §24.  The per-row and per-column logic is tv_height.h,
// shared with the host build of the tests.
//
// The work item is a tile: the 16 x 16 columns of one block column that the box's footprint meets, and the stack of blocks
// between the box's lowest and highest z.  One launch, nothing binned:
//   k_height_tiles   one workgroup of 256 lanes per tile.  The stack's sign summaries go to LDS first (one read per block), then
//                    the workgroup walks the stack in the scan direction, a step per block: a lane per 16-byte distance row -
//                    sign mask, clipped to the box, into LDS; behind the barrier a lane per column - its 16 samples in scan
//                    order from the masks, the surface bits with the bit carried from the step before, and for each surface it
//                    still lacks three bytes gathered from the dense fields (the sample, its air neighbour, the material) and
//                    one store per output array.  The next step's distance row is on its way while a step is worked on.  An
//                    all-air block is no step at all; an all-solid one reads no row and exchanges nothing (a column's bits
//                    are the box's z range).  Without VX_HEIGHT_COUNT_SURFACES the workgroup votes after every step and
//                    leaves once every column of the tile has its layers; with it a step has one barrier, or none.  The
//                    counts are reduced per workgroup and go out as two 64-bit adds, one 32-bit add and three 32-bit maxima.
// Every atomic is an integer sum or maximum, so the results do not depend on an order or a schedule.  The calls only read the
// grid; the host form waits once, at its end, for the copies back.
#include "tv_height.h"

namespace {

struct HeightState {
	void* buf = nullptr;       // the slot, and the host form's staging of the results
	size_t bufCap = 0;
	bool shortcuts = true;     // the sign summaries may stand in for the distance rows (vx_debug_height_shortcuts)

	void release(vx_ctx* c)
	{
		c->be.free(buf);
	}
};

// slot = nullptr: no counts are gathered.  materials, surfaces: may be null.
__global__ __launch_bounds__(WG) void k_height_tiles(RecGrid g, HeightQuery q, const u16* sign, u32* heights, u8* materials, u16* surfaces, HeightSlot* slot)
{
	__shared__ u32 sMask[2][256];
	__shared__ u32 sRed[WG / 64][9];
	__shared__ u32 sSum[HEIGHT_MAX_STEPS];
	const u32 t = threadIdx.x, nb = g.n >> 4, tile = blockIdx.x;
	const bool top = q.direction == HEIGHT_FROM_TOP, countAll = (q.flags & HEIGHT_COUNT_SURFACES) != 0u;
	const HeightTiles T = height_tiles(q.box);
	if (t < T.steps) sSum[t] = sign ? ((u32)sign[height_step_block(T, nb, tile, t, top)] & 3u) : 0u;
	__syncthreads();

	// the lane as a column
	const u32 x = (T.bx0 + tile % T.tx) * 16u + (t & 15u), y = (T.by0 + tile / T.tx) * 16u + (t >> 4);
	const bool inBox = x >= q.box.lo[0] && x < q.box.hi[0] && y >= q.box.lo[1] && y < q.box.hi[1];
	const u32 W = q.box.hi[0] - q.box.lo[0];
	const size_t cells = (size_t)W * (q.box.hi[1] - q.box.lo[1]);
	const size_t cell = inBox ? (size_t)(y - q.box.lo[1]) * W + (x - q.box.lo[0]) : 0u;
	HeightColumn c = height_column();

	// the lane as a row: the clip mask and, where it is needed, the distance row of a step (everything that steers this is uniform
	// but the row's own place in the box)
	auto fetch = [&](u32 step, u32& clip, RecRow& row) {
		clip = 0u;
		if (sSum[step] != 0u) return;                               // a block of one sign: no rows
		const u32 id = height_step_block(T, nb, tile, step, top);
		clip = height_row_clip(q.box, nb, id, t);
		if (clip) row = rec_load16(g.dist + rec_grid_row(g.n, id, t));
	};
	u32 clip, nextClip = 0u, side = 0u;
	RecRow row = { { 0u, 0u, 0u, 0u } }, nextRow = { { 0u, 0u, 0u, 0u } };
	fetch(0u, clip, row);
	for (u32 step = 0; step < T.steps; ++step) {                   // (uniform)
		if (step + 1u < T.steps) fetch(step + 1u, nextClip, nextRow);
		const u32 summary = sSum[step];
		if (summary == 1u) c.carry = 0u;                            // no sample of the block is negative
		else {
			const u32 z0 = (top ? T.bz0 + T.steps - 1u - step : T.bz0 + step) * 16u;
			u32 bits;
			if (summary == 2u) bits = inBox ? height_solid_bits(q.box, z0, top) : 0u;   // every sample is: no rows, no exchange
			else {
				// The masks of consecutive exchanges go to the two halves of sMask in turn, so one barrier per exchange is enough:
				// a lane writes a half again only behind the barrier of the exchange in between, which every lane reaches with
				// its reads of that half done.
				sMask[side][t] = height_row_mask(clip, row);
				__syncthreads();
				bits = height_column_bits(sMask[side], t, top);
				side ^= 1u;
			}
			const u32 surf = height_surface_bits(bits, c.carry);
			height_take(surf, z0, top, q.layers, c, [&](u32 layer, u32 z) {   // (a column outside the box has no bits)
				const HeightHit h = height_hit(g.dist, g.mat, g.n, q.box, x, y, z, top);
				heights[layer * cells + cell] = h.height;
				if (materials) materials[layer * cells + cell] = (u8)h.material;
				return h;
			});
			if (!countAll && __syncthreads_and(height_column_done(c, inBox, q.layers, countAll) ? 1 : 0)) break;
		}
		clip = nextClip; row = nextRow;
	}

	if (inBox) {
		for (u32 layer = c.have; layer < q.layers; ++layer) {
			heights[layer * cells + cell] = HEIGHT_NONE;
			if (materials) materials[layer * cells + cell] = 0;
		}
		if (surfaces) surfaces[cell] = (u16)c.total;
	}
	if (!slot) return;                                              // (uniform)
	u32 v[9];
	height_column_counts(c, countAll, v);
	measure_reduce<3>(v, sRed, t);
	if (t < 9) {
		const u32 a = v[0];
		if (a) {
			if (t == 0) atomicMax(&slot->notMin, a);
			else if (t == 1) atomicMax(&slot->max, a);
			else if (t == 2) atomicMax(&slot->maxSurfaces, a);
			else if (t == 6) atomicAdd(&slot->covered, (u64)a);
			else if (t == 7) atomicAdd(&slot->surfaces, (u64)a);
			else if (t == 8) atomicAdd(&slot->clipped, a);
		}
	}
}

// the checks of both forms; VX_OK = go on
int height_check_call(vx_ctx* c, const vx_height_query* q, const void* heights, const void* surfaces, const std::string& what)
{
	if (!c) return VX_ERR_INVALID;
	if (!undo_whole_grid(c)) return fail(c, VX_ERR_INVALID, what + "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (const char* bad = height_check(c->n, (const HeightQuery*)q, heights, surfaces)) return fail(c, VX_ERR_INVALID, what + bad);
	return VX_OK;
}

bool height_launch(vx_ctx* c, const HeightState* s, const HeightQuery& q, u32* dHeights, u8* dMaterials, u16* dSurfaces, HeightSlot* dSlot)
{
	const HeightTiles T = height_tiles(q.box);
	const u16* sign = s->shortcuts ? grid_block_signs(c) : nullptr;
	hipLaunchKernelGGL(k_height_tiles, dim3(T.tx * T.ty), dim3(WG), 0, c->be.stream, undo_grid(c), q, sign, dHeights, dMaterials, dSurfaces, dSlot);
	return c->be.check(hipGetLastError(), "k_height_tiles launch");
}

} // namespace

extern "C" {

static_assert(sizeof(vx_height_query) == 48 && sizeof(vx_height_counts) == 48, "vx_height_query / vx_height_counts layout");
static_assert(sizeof(HeightQuery) == sizeof(vx_height_query) && sizeof(HeightCounts) == sizeof(vx_height_counts) && sizeof(HeightSlot) == 32, "tv_height.h records");
static_assert(VX_HEIGHT_MAX_LAYERS == tv::HEIGHT_MAX_LAYERS && VX_HEIGHT_NONE == tv::HEIGHT_NONE && VX_HEIGHT_FROM_TOP == tv::HEIGHT_FROM_TOP
              && VX_HEIGHT_FROM_BOTTOM == tv::HEIGHT_FROM_BOTTOM && VX_HEIGHT_COUNT_SURFACES == tv::HEIGHT_COUNT_SURFACES, "height map constants");
static_assert(VX_MAX_GRID / 16 <= tv::HEIGHT_MAX_STEPS, "a stack of the largest grid");

// test hook: whether the sign summaries may stand in for distance rows (the default); nothing of a result depends on it
int vx_debug_height_shortcuts(vx_ctx* c, uint32_t enable)
{
	if (!c) return VX_ERR_INVALID;
	module_state<HeightState>(c, MOD_HEIGHT)->shortcuts = enable != 0;
	return VX_OK;
}

int vx_grid_heightmap_device(vx_ctx* c, const vx_height_query* query, uint32_t* d_heights, uint8_t* d_materials, uint16_t* d_surfaces, vx_height_counts* counts)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_heightmap_device: ";
	const int rc = height_check_call(c, query, d_heights, d_surfaces, what);
	if (rc != VX_OK) return rc;
	if (((uintptr_t)d_heights & 3u) || ((uintptr_t)d_surfaces & 1u)) return fail(c, VX_ERR_INVALID, what + "heights must be 4-byte aligned, surfaces 2-byte");
	const HeightQuery q = *(const HeightQuery*)query;
	HeightState* s = module_state<HeightState>(c, MOD_HEIGHT);
	if (!counts) {                                                  // the per-frame form: queued, not waited for
		if (!height_launch(c, s, q, d_heights, d_materials, d_surfaces, nullptr)) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error());
		return VX_OK;
	}
	if (!dev_grow(c, s->buf, s->bufCap, 256)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	HeightSlot slot;
	memset(&slot, 0, sizeof(slot));
	bool ok = c->be.fill(s->buf, 0, sizeof(HeightSlot)) && height_launch(c, s, q, d_heights, d_materials, d_surfaces, (HeightSlot*)s->buf);
	ok = ok && c->be.d2h_async(&slot, s->buf, sizeof(slot));
	if (!ok) { c->be.sync(); return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	if (!c->be.sync_ok()) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); // (the call's one wait)
	const HeightCounts res = height_finish(q, slot);
	memcpy(counts, &res, sizeof(res));
	return VX_OK;
}

int vx_grid_heightmap(vx_ctx* c, const vx_height_query* query, uint32_t* heights, uint8_t* materials, uint16_t* surfaces, vx_height_counts* counts)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_heightmap: ";
	const int rc = height_check_call(c, query, heights, surfaces, what);
	if (rc != VX_OK) return rc;
	const HeightQuery q = *(const HeightQuery*)query;
	HeightState* s = module_state<HeightState>(c, MOD_HEIGHT);

	// one buffer: the slot | heights | materials | surfaces
	auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t cells = (size_t)(q.box.hi[0] - q.box.lo[0]) * (q.box.hi[1] - q.box.lo[1]), entries = cells * q.layers;
	const size_t atHeights = 256, atMaterials = atHeights + pad(entries * 4u), atSurfaces = atMaterials + (materials ? pad(entries) : 0u);
	const size_t need = atSurfaces + (surfaces ? pad(cells * 2u) : 0u);
	if (!dev_grow(c, s->buf, s->bufCap, need)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	char* base = (char*)s->buf;
	u32* dHeights = (u32*)(base + atHeights);
	u8* dMaterials = materials ? (u8*)(base + atMaterials) : nullptr;
	u16* dSurfaces = surfaces ? (u16*)(base + atSurfaces) : nullptr;
	HeightSlot slot;
	memset(&slot, 0, sizeof(slot));
	bool ok = (!counts || c->be.fill(base, 0, sizeof(HeightSlot))) && height_launch(c, s, q, dHeights, dMaterials, dSurfaces, counts ? (HeightSlot*)base : nullptr);
	ok = ok && c->be.d2h_async(heights, dHeights, entries * 4u);
	if (materials) ok = ok && c->be.d2h_async(materials, dMaterials, entries);
	if (surfaces) ok = ok && c->be.d2h_async(surfaces, dSurfaces, cells * 2u);
	if (counts) ok = ok && c->be.d2h_async(&slot, base, sizeof(slot));
	if (!ok) { c->be.sync(); return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	if (!c->be.sync_ok()) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); // (the call's one wait)
	if (counts) {
		const HeightCounts res = height_finish(q, slot);
		memcpy(counts, &res, sizeof(res));
	}
	return VX_OK;
}

} // extern "C"
