// height_host.cpp — host side of the tests of the height maps (tests only; built by voxels_amd/build.py
// build_measure_host() into the measurements' host library, whose rows these walks share).
//
// voxels_amd/csrc/tv_height.h compiled for the host behind one C interface, with two paths through a query:
//   path 0   a plain loop: column after column, sample after sample in the scan direction
//   path 1   the pipeline of vx_height.inl - a workgroup per tile of 16 x 16 columns, the stack's sign summaries first, then a
//            step per block in scan order: the 256 row masks, behind them the 256 columns (bits in scan order, the surface bits
//            with the carried bit, the surfaces still lacking resolved and written), the vote that ends the walk early, the
//            tail that writes VX_HEIGHT_NONE, and the counts reduced per workgroup and merged into the slot - with the lanes of
//            a workgroup as loops.  `skip` = 1 lets the per-block sign summaries (formed here from the grid, by the rule of the
//            mirrors: 1 = no sample < 0, 2 = every sample < 0) stand in for distance rows, as the kernel does.  *walked
//            receives the steps in which rows were looked at: what the early exit and the summaries save.
//   hh_value    the height formula alone          hh_layout   sizes and offsets of the header's structs as this compiler lays
//   them out; hh_limit the constants
// A grid is dist / mat (n^3 bytes each, x fastest, Z up).
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_height.h"

using namespace tv;

namespace {

static_assert(sizeof(HeightQuery) == sizeof(vx_height_query) && sizeof(HeightCounts) == sizeof(vx_height_counts) && sizeof(RecBox) == sizeof(vx_box), "tv_height.h records");

struct Out {
	u32* heights;
	u8* materials;
	uint16_t* surfaces;
	size_t cells, width;
};

// what the device does with atomics
void merge(HeightSlot& s, const u32 v[9])
{
	s.notMin = std::max(s.notMin, v[0]); s.max = std::max(s.max, v[1]); s.maxSurfaces = std::max(s.maxSurfaces, v[2]);
	s.covered += v[6]; s.surfaces += v[7]; s.clipped += v[8];
}

void plain(u32 n, const u8* dist, const u8* mat, const HeightQuery& q, const Out& o, HeightSlot& slot)
{
	const bool top = q.direction == HEIGHT_FROM_TOP, countAll = (q.flags & HEIGHT_COUNT_SURFACES) != 0u;
	const RecBox& b = q.box;
	for (u32 y = b.lo[1]; y < b.hi[1]; ++y)
		for (u32 x = b.lo[0]; x < b.hi[0]; ++x) {
			const size_t cell = (size_t)(y - b.lo[1]) * o.width + (x - b.lo[0]);
			HeightColumn c = height_column();
			bool before = false;                                     // air at the box's end
			for (u32 k = 0; k < b.hi[2] - b.lo[2]; ++k) {
				const u32 z = top ? b.hi[2] - 1u - k : b.lo[2] + k;
				const bool solid = (i8)dist[((size_t)z * n + y) * n + x] < 0;
				if (solid && !before) {
					if (c.have < q.layers) {
						const HeightHit h = height_hit(dist, mat, n, b, x, y, z, top);
						o.heights[c.have * o.cells + cell] = h.height;
						if (o.materials) o.materials[c.have * o.cells + cell] = (u8)h.material;
						if (!c.have) { c.h0 = h.height; c.clipped0 = h.clipped; }
						++c.have;
					}
					++c.total;
				}
				before = solid;
			}
			for (u32 layer = c.have; layer < q.layers; ++layer) {
				o.heights[layer * o.cells + cell] = HEIGHT_NONE;
				if (o.materials) o.materials[layer * o.cells + cell] = 0;
			}
			if (o.surfaces) o.surfaces[cell] = (uint16_t)c.total;
			u32 v[9];
			height_column_counts(c, countAll, v);
			merge(slot, v);
		}
}

u32 block_summary(u32 n, const u8* dist, u32 id)
{
	bool neg = false, pos = false;
	for (u32 row = 0; row < 256; ++row) {
		const i8* p = (const i8*)dist + rec_grid_row(n, id, row);
		for (u32 x = 0; x < 16; ++x) { if (p[x] < 0) neg = true; else pos = true; }
	}
	return neg && pos ? 0u : neg ? 2u : 1u;
}

void pipeline(u32 n, const u8* dist, const u8* mat, const HeightQuery& q, u32 skip, const Out& o, HeightSlot& slot, u64& walked)
{
	const u32 nb = n >> 4;
	const bool top = q.direction == HEIGHT_FROM_TOP, countAll = (q.flags & HEIGHT_COUNT_SURFACES) != 0u;
	const HeightTiles T = height_tiles(q.box);
	for (u32 tile = 0; tile < T.tx * T.ty; ++tile) {                 // k_height_tiles: a workgroup
		u32 sum[HEIGHT_MAX_STEPS];
		for (u32 t = 0; t < T.steps; ++t) sum[t] = skip ? block_summary(n, dist, height_step_block(T, nb, tile, t, top)) : 0u;
		HeightColumn col[256];
		u32 xs[256], ys[256];
		bool in[256];
		for (u32 t = 0; t < 256; ++t) {
			col[t] = height_column();
			xs[t] = (T.bx0 + tile % T.tx) * 16u + (t & 15u); ys[t] = (T.by0 + tile / T.tx) * 16u + (t >> 4);
			in[t] = xs[t] >= q.box.lo[0] && xs[t] < q.box.hi[0] && ys[t] >= q.box.lo[1] && ys[t] < q.box.hi[1];
		}
		for (u32 step = 0; step < T.steps; ++step) {
			if (sum[step] == 1u) { for (u32 t = 0; t < 256; ++t) col[t].carry = 0u; continue; }
			const u32 id = height_step_block(T, nb, tile, step, top);
			const u32 z0 = (top ? T.bz0 + T.steps - 1u - step : T.bz0 + step) * 16u;
			u32 masks[256];
			if (sum[step] == 0u) {
				++walked;
				for (u32 t = 0; t < 256; ++t) {                      // a lane as a row
					const u32 clip = height_row_clip(q.box, nb, id, t);
					RecRow row = { { 0u, 0u, 0u, 0u } };
					if (clip) row = rec_load16(dist + rec_grid_row(n, id, t));
					masks[t] = height_row_mask(clip, row);
				}
			}
			bool all = true;
			for (u32 t = 0; t < 256; ++t) {                          // a lane as a column
				const u32 bits = sum[step] == 2u ? (in[t] ? height_solid_bits(q.box, z0, top) : 0u) : height_column_bits(masks, t, top);
				const u32 surf = height_surface_bits(bits, col[t].carry);
				const size_t cell = in[t] ? (size_t)(ys[t] - q.box.lo[1]) * o.width + (xs[t] - q.box.lo[0]) : 0u;
				height_take(surf, z0, top, q.layers, col[t], [&](u32 layer, u32 z) {
					const HeightHit h = height_hit(dist, mat, n, q.box, xs[t], ys[t], z, top);
					o.heights[layer * o.cells + cell] = h.height;
					if (o.materials) o.materials[layer * o.cells + cell] = (u8)h.material;
					return h;
				});
				all = all && height_column_done(col[t], in[t], q.layers, countAll);
			}
			if (all) break;
		}
		u32 wg[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
		for (u32 t = 0; t < 256; ++t) {
			if (in[t]) {
				const size_t cell = (size_t)(ys[t] - q.box.lo[1]) * o.width + (xs[t] - q.box.lo[0]);
				for (u32 layer = col[t].have; layer < q.layers; ++layer) {
					o.heights[layer * o.cells + cell] = HEIGHT_NONE;
					if (o.materials) o.materials[layer * o.cells + cell] = 0;
				}
				if (o.surfaces) o.surfaces[cell] = (uint16_t)col[t].total;
			}
			u32 v[9];
			height_column_counts(col[t], countAll, v);
			for (int k = 0; k < 6; ++k) wg[k] = std::max(wg[k], v[k]);
			for (int k = 6; k < 9; ++k) wg[k] += v[k];
		}
		merge(slot, wg);
	}
}

} // namespace

extern "C" {

int hh_check(uint32_t n, const vx_height_query* q, uint32_t has_heights, uint32_t has_surfaces)
{
	static const char some = 0;
	return height_check(n, (const HeightQuery*)q, has_heights ? &some : nullptr, has_surfaces ? &some : nullptr) ? VX_ERR_INVALID : VX_OK;
}

// what vx_grid_heightmap returns for bad arguments (everything but the context), else VX_OK with the answers written
int hh_heightmap(uint32_t path, uint32_t n, const uint8_t* dist, const uint8_t* mat, const vx_height_query* query, uint32_t skip,
                 uint32_t* heights, uint8_t* materials, uint16_t* surfaces, vx_height_counts* counts, uint64_t* walked)
{
	if (height_check(n, (const HeightQuery*)query, heights, surfaces)) return VX_ERR_INVALID;
	const HeightQuery q = *(const HeightQuery*)query;
	Out o;
	o.heights = heights; o.materials = materials; o.surfaces = surfaces;
	o.width = q.box.hi[0] - q.box.lo[0];
	o.cells = o.width * (q.box.hi[1] - q.box.lo[1]);
	HeightSlot slot;
	memset(&slot, 0, sizeof(slot));
	u64 steps = 0;
	if (path == 0) plain(n, dist, mat, q, o, slot);
	else pipeline(n, dist, mat, q, skip, o, slot, steps);
	if (counts) {
		const HeightCounts r = height_finish(q, slot);
		memcpy(counts, &r, sizeof(r));
	}
	if (walked) *walked = steps;
	return VX_OK;
}

uint32_t hh_value(uint32_t z, int32_t d0, int32_t d1, uint32_t top, uint32_t clipped) { return height_value(z, d0, d1, top != 0, clipped != 0); }

// which: 0 = sizes of vx_height_query, vx_height_counts, vx_box; 1 = offsets inside vx_height_query; 2 = inside vx_height_counts
uint32_t hh_layout(uint32_t which, uint32_t* out)
{
	if (which == 0) { const uint32_t v[] = { sizeof(vx_height_query), sizeof(vx_height_counts), sizeof(vx_box) }; memcpy(out, v, sizeof(v)); return 3; }
	if (which == 1) {
		const uint32_t v[] = { offsetof(vx_height_query, box), offsetof(vx_height_query, direction), offsetof(vx_height_query, layers), offsetof(vx_height_query, flags), offsetof(vx_height_query, reserved) };
		memcpy(out, v, sizeof(v)); return 5;
	}
	const uint32_t v[] = { offsetof(vx_height_counts, columns), offsetof(vx_height_counts, covered), offsetof(vx_height_counts, surfaces), offsetof(vx_height_counts, min_height),
	                       offsetof(vx_height_counts, max_height), offsetof(vx_height_counts, clipped), offsetof(vx_height_counts, max_surfaces), offsetof(vx_height_counts, reserved) };
	memcpy(out, v, sizeof(v)); return 8;
}

// 0 = VX_HEIGHT_MAX_LAYERS, 1 = VX_HEIGHT_NONE, 2 = VX_HEIGHT_FROM_TOP, 3 = VX_HEIGHT_FROM_BOTTOM, 4 = VX_HEIGHT_COUNT_SURFACES
uint32_t hh_limit(uint32_t which)
{
	const uint32_t v[] = { VX_HEIGHT_MAX_LAYERS, VX_HEIGHT_NONE, VX_HEIGHT_FROM_TOP, VX_HEIGHT_FROM_BOTTOM, VX_HEIGHT_COUNT_SURFACES };
	return which < 5 ? v[which] : 0;
}

} // extern "C"
