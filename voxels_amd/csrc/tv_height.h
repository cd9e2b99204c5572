// tv_height.h — the per-row and per-column logic of the height maps (include/voxels_hip.h, "height maps").  DESIGN.md §24.
//
// This header is the one place where that logic is written down, shared by the device kernel (vx_height.inl) and the host build
// of the tests (tests/height/height_host.cpp).  Everything is integer arithmetic; counts are summed, the extremes are combined
// by maxima (a minimum is kept as the maximum of its complement, as MeasureSlot does), so no result depends on an order.
//
// The work item is a TILE: the 16 x 16 columns of one block column of the grid that the query's footprint meets, with the
// STACK of blocks between the box's lowest and highest z, walked in the scan direction, one STEP per block.  In a step a lane is
// first a row (row = z * 16 + y inside the block, tv_undo.h): the sign bits of its 16 distances as a mask over x, clipped to the
// box.  The 256 masks are exchanged, and the lane is a column (col = y * 16 + x): its 16 samples as bits in SCAN ORDER (bit i is
// the i-th sample the walk meets in this block), the surface bits from them and one bit carried from the block before, then the
// surfaces it still lacks, each resolved to a height and a material byte from the dense fields.
//
// The caller supplies the lanes (a workgroup, or a loop), the exchange and the reductions between them.
#pragma once

#include "tv_measure.h"

namespace tv {

enum : u32 { HEIGHT_FROM_TOP = 0, HEIGHT_FROM_BOTTOM = 1, HEIGHT_COUNT_SURFACES = 1, HEIGHT_MAX_LAYERS = 8, HEIGHT_NONE = 0xFFFFFFFFu };
enum : u32 { HEIGHT_MAX_STEPS = 128 };   // the blocks of a stack of the largest grid (2048 / 16)

struct HeightQuery {         // = vx_height_query
	RecBox box;
	u32 direction, layers, flags, reserved[3];
};

struct HeightCounts {        // = vx_height_counts
	u64 columns, covered, surfaces;
	u32 min_height, max_height, clipped, max_surfaces, reserved[2];
};

// per call, accumulated with integer maxima and sums: zero = no covered column met yet
struct HeightSlot {          // 32 bytes
	u64 covered, surfaces;
	u32 notMin;              // ~(least layer-0 height)
	u32 max;                 // greatest layer-0 height
	u32 maxSurfaces, clipped;
};

// ---- the entry check ------------------------------------------------------------------------------------------------------------

// what vx_grid_heightmap refuses before anything is launched (everything but the context); nullptr = fine
TV_HD const char* height_check(u32 n, const HeightQuery* q, const void* heights, const void* surfaces)
{
	if (!q) return "null query";
	if (!heights) return "null heights array";
	for (int k = 0; k < 3; ++k)
		if (!(q->box.lo[k] < q->box.hi[k] && q->box.hi[k] <= n)) return "the box needs lo < hi <= n on every axis";
	if (q->direction > HEIGHT_FROM_BOTTOM) return "direction is neither VX_HEIGHT_FROM_TOP nor VX_HEIGHT_FROM_BOTTOM";
	if (q->layers < 1u || q->layers > HEIGHT_MAX_LAYERS) return "layers must be 1..VX_HEIGHT_MAX_LAYERS";
	if (q->flags & ~(u32)HEIGHT_COUNT_SURFACES) return "unknown flag bits";
	if (q->reserved[0] | q->reserved[1] | q->reserved[2]) return "reserved words must be zero";
	if (surfaces && !(q->flags & HEIGHT_COUNT_SURFACES)) return "a surfaces array needs VX_HEIGHT_COUNT_SURFACES";
	return nullptr;
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------------

struct HeightTiles {
	u32 bx0, by0, tx, ty;    // the block columns the footprint meets: first and count per axis
	u32 bz0, steps;          // the stack: its lowest block plane and its height in blocks
};

TV_HD HeightTiles height_tiles(const RecBox& b)
{
	u32 first[3], cnt[3];
	measure_box_blocks(b, first, cnt);
	HeightTiles t;
	t.bx0 = first[0]; t.by0 = first[1]; t.tx = cnt[0]; t.ty = cnt[1];
	t.bz0 = first[2]; t.steps = cnt[2];
	return t;
}

// the grid block id of step `step` of tile `tile` (tiles x fastest; steps in scan order)
TV_HD u32 height_step_block(const HeightTiles& t, u32 nb, u32 tile, u32 step, bool top)
{
	const u32 bx = t.bx0 + tile % t.tx, by = t.by0 + tile / t.tx, bz = top ? t.bz0 + t.steps - 1u - step : t.bz0 + step;
	return (bz * nb + by) * nb + bx;
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------

// Row `row` of block `id` (a block that holds both signs, or one nothing is known about): `clip` = its voxels inside the box as
// a mask over x; 0 = the row is outside and its distances need not be read
TV_HD u32 height_row_clip(const RecBox& b, u32 nb, u32 id, u32 row) { return measure_clip_mask(b, nb, id, row); }
// ... and the solid voxels of the row inside the box
TV_HD u32 height_row_mask(u32 clip, const RecRow& dist) { return clip ? clip & measure_sign_mask(dist) : 0u; }

// ---- columns --------------------------------------------------------------------------------------------------------------------

// the 16 samples of column `col` (y * 16 + x) of a block out of its 256 row masks (row = z * 16 + y), in scan order
TV_HD u32 height_column_bits(const u32* masks, u32 col, bool top)
{
	const u32 x = col & 15u, y = col >> 4;
	u32 bits = 0;
	for (u32 i = 0; i < 16u; ++i) {
		const u32 z = top ? 15u - i : i;
		bits |= ((masks[z * 16u + y] >> x) & 1u) << i;
	}
	return bits;
}

// The same for a column inside the footprint of a block whose every sample is solid (summary 2), without rows or masks: the
// samples of the block's planes [z0, z0 + 16) that lie in the box's z range, a run of bits.
TV_HD u32 height_solid_bits(const RecBox& b, u32 z0, bool top)
{
	const u32 za = b.lo[2] > z0 ? b.lo[2] - z0 : 0u, zb = b.hi[2] < z0 + 16u ? b.hi[2] - z0 : 16u;   // (za < zb <= 16: the stack's blocks meet the box)
	const u32 first = top ? 16u - zb : za, last = top ? 16u - za : zb;                                // in scan order
	return ((1u << last) - 1u) & ~((1u << first) - 1u);
}

// what a column carries from step to step and gathers for the counts
struct HeightColumn {
	u32 carry;               // 1 = the sample walked just before this block is solid; air at the box's end
	u32 have;                // layers found so far
	u32 total;               // surfaces met so far
	u32 h0, clipped0;        // layer 0: its height, and whether it is clipped
};
TV_HD HeightColumn height_column() { HeightColumn c; c.carry = c.have = c.total = c.h0 = c.clipped0 = 0; return c; }

// the surface bits of a block's samples in scan order: solid, and the sample met just before it is not
TV_HD u32 height_surface_bits(u32 bits, u32& carry)
{
	const u32 before = ((bits << 1) | carry) & 0xFFFFu;
	carry = bits >> 15;
	return bits & ~before;
}

// the grid z of bit i of a block whose lowest plane is z0
TV_HD u32 height_bit_z(u32 z0, u32 i, bool top) { return z0 + (top ? 15u - i : i); }

// 24.8 fixed point: d0 (-128..-1) the surface sample, d1 (0..127) its air neighbour in the scan direction
TV_HD u32 height_value(u32 z, int d0, int d1, bool top, bool clipped)
{
	if (clipped) return z * 256u;
	const u32 f = (u32)(256 * -d0) / (u32)(d1 - d0);   // 2..256
	return top ? z * 256u + f : z * 256u - f;
}

struct HeightHit { u32 height, material, clipped; };

// the surface at (x, y, z) of the dense fields of edge n resolved: a few bytes gathered, its air neighbour only where the box
// does not end there
TV_HD HeightHit height_hit(const u8* dist, const u8* mat, u32 n, const RecBox& b, u32 x, u32 y, u32 z, bool top)
{
	const size_t plane = (size_t)n * n, at = (size_t)z * plane + (size_t)y * n + x;
	HeightHit h;
	h.clipped = (top ? z + 1u == b.hi[2] : z == b.lo[2]) ? 1u : 0u;
	const int d0 = (i8)dist[at], d1 = h.clipped ? 0 : (int)(i8)dist[top ? at + plane : at - plane];
	h.height = height_value(z, d0, d1, top, h.clipped != 0u);
	h.material = mat[at];
	return h;
}

// One step of a column: the surfaces of `surf` counted, and those the column still lacks taken in scan order -
// emit(layer, z) once per taken surface resolves it (height_hit), writes it out and returns it.
template <class Emit> TV_HD void height_take(u32 surf, u32 z0, bool top, u32 layers, HeightColumn& c, const Emit& emit)
{
	c.total += (u32)__builtin_popcount(surf);
	while (surf && c.have < layers) {
		const u32 i = (u32)__builtin_ctz(surf);
		surf &= surf - 1u;
		const HeightHit h = emit(c.have, height_bit_z(z0, i, top));
		if (!c.have) { c.h0 = h.height; c.clipped0 = h.clipped; }
		++c.have;
	}
}

// may the walk leave this column: nothing of the result depends on the steps behind
TV_HD bool height_column_done(const HeightColumn& c, bool inBox, u32 layers, bool countAll) { return !countAll && (!inBox || c.have >= layers); }

// What one column adds to the slot: v[0] ~min, v[1] max, v[2] max surfaces, v[3..5] unused (the layout of measure_reduce: six
// maxima, then sums), v[6] covered, v[7] surfaces, v[8] clipped - zeros where the column has no surface.
TV_HD void height_column_counts(const HeightColumn& c, bool countAll, u32 v[9])
{
	for (int k = 0; k < 9; ++k) v[k] = 0;
	if (!c.have) return;
	v[0] = ~c.h0; v[1] = c.h0;
	v[2] = countAll ? c.total : 0u;
	v[6] = 1u; v[7] = v[2]; v[8] = c.clipped0;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------

TV_HD HeightCounts height_finish(const HeightQuery& q, const HeightSlot& s)
{
	const bool countAll = (q.flags & HEIGHT_COUNT_SURFACES) != 0u;
	HeightCounts r;
	r.columns = (u64)(q.box.hi[0] - q.box.lo[0]) * (q.box.hi[1] - q.box.lo[1]);
	r.covered = s.covered;
	r.surfaces = countAll ? s.surfaces : 0u;
	r.min_height = s.covered ? ~s.notMin : 0u;
	r.max_height = s.covered ? s.max : 0u;
	r.clipped = s.clipped;
	r.max_surfaces = countAll ? s.maxSurfaces : 0u;
	r.reserved[0] = r.reserved[1] = 0;
	return r;
}

} // namespace tv
