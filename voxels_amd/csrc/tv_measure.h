// tv_measure.h — the per-row and per-block logic of the measurements (include/voxels_hip.h, "measurements").  DESIGN.md §23.
//
// This header is the one place where that logic is written down, shared by the device kernels (vx_measure.inl) and the host
// build of the tests (tests/measure/measure_host.cpp).  Everything is integer arithmetic: counts are summed, bounds are combined
// by maxima (a minimum is kept as the maximum of its complement, as RecSwapSlot does), so no result depends on an order.
//
// The work item is a (box, block) PAIR: pair p of a batch belongs to the box b with prefix[b] <= p < prefix[b + 1], where
// prefix holds the running sums of the boxes' block counts, and is block p - prefix[b] of that box, x fastest.  A block is 256
// rows of 16 bytes (row = z * 16 + y inside the block, tv_undo.h); a lane takes one row: the sign bits of its 16 distances as a
// mask, clipped to the box, then the materials of the solid voxels as runs of equal bytes.
//
// The caller supplies the lanes (a workgroup, or a loop) and the reductions between them.
#pragma once

#include "tv_undo.h"

namespace tv {

typedef unsigned long long u64;

enum : u32 { MEASURE_MAX_BOXES = 1u << 16, MEASURE_CHUNK_PAIRS = 1u << 22 };
enum : u32 { MEASURE_GROUP = 16 };   // consecutive pairs of a launch that one workgroup walks (vx_measure.inl)

struct MeasureResult {       // = vx_measure
	u64 voxels, solid_voxels;
	u32 min[3], max[3];
	u32 materials, reserved;
};

struct RecordDelta {         // = vx_record_delta
	u64 removed_voxels, added_voxels, repainted_voxels;
	u32 min[3], max[3];
	u32 blocks, reserved[3];
};

// per box, accumulated with integer maxima and sums: zero = no solid voxel met yet
struct MeasureSlot {         // 32 bytes
	u64 solid;
	u32 notMin[3];           // ~(least solid coordinate) per internal axis
	u32 max[3];              // greatest solid coordinate
};

// per vx_record_measure call, likewise
struct DeltaSlot {           // 56 bytes
	u64 removed, added, repainted;
	u32 notMin[3], max[3];   // over the removed and the added voxels
	u32 blocks, pad;
};

// ---- the entry checks -----------------------------------------------------------------------------------------------------------

// what vx_grid_measure refuses before anything is launched; nullptr = fine
TV_HD const char* measure_check(u32 n, const RecBox* boxes, u32 count, const void* results)
{
	if (count > MEASURE_MAX_BOXES) return "more than VX_MEASURE_MAX_BOXES boxes";
	if (count && !boxes) return "null box array";
	if (count && !results) return "null result array";
	for (u32 i = 0; i < count; ++i)
		for (int k = 0; k < 3; ++k)
			if (!(boxes[i].lo[k] < boxes[i].hi[k] && boxes[i].hi[k] <= n)) return "a box needs lo < hi <= n on every axis";
	return nullptr;
}

// ---- pairs ----------------------------------------------------------------------------------------------------------------------

// the blocks a box intersects: first block and count per axis
TV_HD void measure_box_blocks(const RecBox& b, u32 first[3], u32 cnt[3])
{
	for (int k = 0; k < 3; ++k) { first[k] = b.lo[k] >> 4; cnt[k] = ((b.hi[k] + 15u) >> 4) - first[k]; }
}
TV_HD u64 measure_box_pairs(const RecBox& b)
{
	u32 first[3], cnt[3];
	measure_box_blocks(b, first, cnt);
	return (u64)cnt[0] * cnt[1] * cnt[2];
}
TV_HD u64 measure_box_volume(const RecBox& b) { return (u64)(b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1]) * (b.hi[2] - b.lo[2]); }

// the box of pair p: the last b in [0, count) with prefix[b] <= p (prefix ascends, prefix[0] = 0, p < prefix[count])
TV_HD u32 measure_pair_box(const u64* prefix, u32 count, u64 p)
{
	u32 lo = 0, hi = count;
	while (hi - lo > 1u) {
		const u32 mid = lo + ((hi - lo) >> 1);
		if (prefix[mid] <= p) lo = mid; else hi = mid;
	}
	return lo;
}

// the grid block id of block q of a box (x fastest, then y, then z)
TV_HD u32 measure_pair_block(const RecBox& b, u32 nb, u32 q)
{
	u32 first[3], cnt[3];
	measure_box_blocks(b, first, cnt);
	const u32 x = first[0] + q % cnt[0], y = first[1] + (q / cnt[0]) % cnt[1], z = first[2] + q / (cnt[0] * cnt[1]);
	return (z * nb + y) * nb + x;
}

// is block `id` wholly inside the box
TV_HD bool measure_block_inside(const RecBox& b, u32 nb, u32 id)
{
	const u32 c[3] = { (id % nb) * 16u, ((id / nb) % nb) * 16u, (id / (nb * nb)) * 16u };
	return b.lo[0] <= c[0] && c[0] + 16u <= b.hi[0] && b.lo[1] <= c[1] && c[1] + 16u <= b.hi[1] && b.lo[2] <= c[2] && c[2] + 16u <= b.hi[2];
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------

// bit x set where distance x of the row is < 0: the four sign bits of a word gathered by one multiplication (the partial
// products fall on distinct bits: nothing carries)
TV_HD u32 measure_sign_mask(const RecRow& d)
{
	u32 m = 0;
	for (u32 k = 0; k < 4; ++k) m |= (((((d.w[k] >> 7) & 0x01010101u) * 0x00204081u) >> 21) & 0xFu) << (k * 4u);
	return m;
}

// the voxels of row `row` of block `id` that lie in the box, as a mask over x; 0 = the row is outside
TV_HD u32 measure_clip_mask(const RecBox& b, u32 nb, u32 id, u32 row)
{
	const u32 x0 = (id % nb) * 16u, y = ((id / nb) % nb) * 16u + (row & 15u), z = (id / (nb * nb)) * 16u + (row >> 4);
	if (y < b.lo[1] || y >= b.hi[1] || z < b.lo[2] || z >= b.hi[2]) return 0u;
	const u32 xa = b.lo[0] > x0 ? b.lo[0] - x0 : 0u, xb = b.hi[0] < x0 + 16u ? b.hi[0] - x0 : 16u;
	return ((1u << xb) - 1u) & ~((1u << xa) - 1u);   // (xa < xb <= 16: the block intersects the box)
}

// byte x of a row given as its four words, by selects: words indexed by a variable would leave the registers
TV_HD u32 measure_row_byte(u32 w0, u32 w1, u32 w2, u32 w3, u32 x)
{
	const u32 w = x < 8u ? (x < 4u ? w0 : w1) : (x < 12u ? w2 : w3);
	return (w >> ((x & 3u) * 8u)) & 0xFFu;
}

// bit x (1..15) set where material x equals material x - 1
TV_HD u32 measure_same_as_left(const RecRow& m)
{
	u32 same = 0;
	for (u32 k = 0; k < 4; ++k) {
		// bytes 1..3 of the word against bytes 0..2; byte 0 against byte 3 of the word before
		const u32 x = m.w[k] ^ (m.w[k] << 8);
		for (u32 j = 1; j < 4; ++j) if (!((x >> (j * 8u)) & 0xFFu)) same |= 1u << (k * 4u + j);
		if (k && !(((m.w[k] ^ (m.w[k - 1] >> 24)) & 0xFFu))) same |= 1u << (k * 4u);
	}
	return same;
}

// The materials of the voxels of `mask`, as runs: add(material, voxels) once per run of adjacent voxels of the mask that hold
// the same byte - a terrain row is usually one run.
template <class Add> TV_HD void measure_row_materials(const RecRow& m, u32 mask, const Add& add)
{
	const u32 joined = measure_same_as_left(m) & mask & (mask << 1);   // bit x: voxel x continues the run of voxel x - 1
	u32 starts = mask & ~joined;
	const u32 w0 = m.w[0], w1 = m.w[1], w2 = m.w[2], w3 = m.w[3];
	while (starts) {
		const u32 x = (u32)__builtin_ctz(starts);
		starts &= starts - 1u;
		const u32 len = 1u + (u32)__builtin_ctz(~(joined >> (x + 1u)));   // (bit 15 of the shifted word is clear: the count ends)
		add(measure_row_byte(w0, w1, w2, w3, x), len);
	}
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------

TV_HD MeasureResult measure_finish(const RecBox& b, const MeasureSlot& s, u32 materials)
{
	MeasureResult r;
	r.voxels = measure_box_volume(b);
	r.solid_voxels = s.solid;
	for (int k = 0; k < 3; ++k) { r.min[k] = s.solid ? ~s.notMin[k] : 0u; r.max[k] = s.solid ? s.max[k] : 0u; }
	r.materials = s.solid ? materials : 0u;
	r.reserved = 0;
	return r;
}

TV_HD RecordDelta measure_delta_finish(const DeltaSlot& s)
{
	RecordDelta r;
	const bool moved = s.removed || s.added;
	r.removed_voxels = s.removed; r.added_voxels = s.added; r.repainted_voxels = s.repainted;
	for (int k = 0; k < 3; ++k) { r.min[k] = moved ? ~s.notMin[k] : 0u; r.max[k] = moved ? s.max[k] : 0u; }
	r.blocks = s.blocks;
	r.reserved[0] = r.reserved[1] = r.reserved[2] = 0;
	return r;
}

// ---- the record's rows ----------------------------------------------------------------------------------------------------------

// one row of a held block beside the grid's: the masks of the removed, added and repainted voxels from the sign masks of the
// record's row (was) and the grid's (is); the material rows are read only where one of the two masks is not empty
struct DeltaRow { u32 removed, added, repainted; };
TV_HD DeltaRow measure_delta_row(u32 was, u32 is, const RecRow& recMat, const RecRow& gridMat)
{
	DeltaRow r;
	r.removed = was & ~is; r.added = is & ~was;
	r.repainted = was & is & rec_row_diff(recMat, gridMat);
	return r;
}

} // namespace tv
