// tv_undo.h — the per-lane and per-block logic of the undo records (include/voxels_hip.h, "undo records").  DESIGN.md §20.
//
// This header is the one place where that logic is written down, shared by the device kernels (vx_undo.inl) and the host build
// of the tests (tests/undo/undo_host.cpp).  A record holds whole 16^3 grid blocks, byte for byte; nothing here is arithmetic.
//
// The copy passes (capture, diff, pack, swap) share one tiling.  A workgroup of REC_LANES lanes takes a GROUP of REC_GROUP
// consecutive entries of the record and walks their 256 x-rows in REC_STEPS steps; in a step lane t has
//   entry = t & 7, row = (t >> 3) + 32 * step        (row = z * 16 + y inside the block; a row is 16 bytes in every field)
// The ids of a record ascend with x fastest, so the entries of a group are x-neighbours wherever the record holds a run of
// them: 8 adjacent lanes then read 8 x 16 adjacent bytes of a dense-field row - one whole 128-byte line - and the 8 lanes of a
// wave that share an entry cover 8 consecutive rows of it, 128 contiguous bytes of the record.  Where the entries are no
// neighbours the pass is as correct and reads 16 bytes per line, as a block-at-a-time copy would everywhere.
//
// The caller supplies the lanes (a workgroup, or a loop) and the reductions between them.
#pragma once

#include <stdint.h>
#include <stddef.h>
#include <string.h>

#if !defined(TV_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TV_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define TV_HD inline
#endif
#endif

namespace tv {

typedef uint8_t u8;
typedef uint32_t u32;
typedef int8_t i8;

enum : u32 { REC_MAX_BLOCKS = 1u << 18, REC_MAX_BOXES = 1u << 16 };
enum : u32 { REC_LANES = 256, REC_GROUP = 8, REC_STEPS = 8, REC_BLOCK_BYTES = 12293 /* 3 x 4096 of fields, 1 flag, 4 id */ };

struct RecBox { u32 lo[3], hi[3]; };          // = vx_box: [lo, hi), grid coordinates, internal axes

// the dense fields and the flag bytes of a whole grid
struct RecGrid {
	u8 *dist, *mat, *blend, *flags;
	u32 n;
};

// A record's one allocation: the three fields block after block (4096 bytes each, rows z-major as vx_grid_read_block hands
// them out), then the ids, then the flag bytes - 12 293 bytes per block and no padding: every section starts 4-byte aligned,
// every row 16-byte aligned.
struct RecView {
	u8 *dist, *mat, *blend, *flags;
	u32* ids;
	u32 blocks;
};

TV_HD size_t rec_bytes(u32 blocks) { return (size_t)blocks * REC_BLOCK_BYTES; }

TV_HD RecView rec_view(void* mem, u32 blocks)
{
	RecView r;
	u8* p = (u8*)mem;
	r.dist = p; r.mat = p + (size_t)blocks * 4096u; r.blend = p + (size_t)blocks * 8192u;
	r.ids = (u32*)(p + (size_t)blocks * 12288u);
	r.flags = p + (size_t)blocks * 12292u;
	r.blocks = blocks;
	return r;
}

// per swap, accumulated with integer maxima and sums (as SmoothSlot of tv_smooth.h): zero = nothing differed
struct RecSwapSlot {      // 40 bytes
	u32 notMin[3];        // ~(least differing coordinate) per internal axis
	u32 max[3];           // greatest differing coordinate
	unsigned long long changed;
	u32 blocks, flagChanges;
};

struct RecSwapResult {    // = vx_swap_result
	float out_min[3], out_max[3];
	unsigned long long changed_voxels;
	u32 changed_blocks, flag_changes;
	unsigned long long reserved;
};

// ---- the entry checks -----------------------------------------------------------------------------------------------------------

// what vx_grid_capture refuses before anything is launched; nullptr = fine
TV_HD const char* rec_check_boxes(u32 n, const RecBox* boxes, u32 count)
{
	if (count && !boxes) return "null box array";
	if (count > REC_MAX_BOXES) return "more than VX_RECORD_MAX_BOXES boxes";
	for (u32 i = 0; i < count; ++i)
		for (int k = 0; k < 3; ++k)
			if (!(boxes[i].lo[k] < boxes[i].hi[k] && boxes[i].hi[k] <= n)) return "a box needs lo < hi <= n on every axis";
	return nullptr;
}

// The voxel box of the blocks a brush at pos +- ext touches: the block test of edit_touched_box (vx_host.inl), the reference's
// float32 expressions per block and axis.  1 = touches the grid, 0 = misses it (out is zeroed).
TV_HD int rec_brush_box(const float pos[3], const float ext[3], u32 n, RecBox* out)
{
	const u32 nb = n >> 4;
	int any = 1;
	for (int k = 0; k < 3; ++k) {
		u32 lo = nb, hi = 0, hits = 0;
		for (u32 b = 0; b < nb; ++b) {
			const float bmin = (float)(b * 16u), bmax = (bmin + 8.f) + 8.f;
			if (pos[k] - ext[k] > bmax || bmin > pos[k] + ext[k]) continue;
			if (b < lo) lo = b;
			hi = b; ++hits;
		}
		if (!hits || hi - lo + 1u != hits) any = 0;
		out->lo[k] = lo * 16u; out->hi[k] = (lo + hits) * 16u;
	}
	if (!any) for (int k = 0; k < 3; ++k) out->lo[k] = out->hi[k] = 0;
	return any;
}

// ---- mark, list -----------------------------------------------------------------------------------------------------------------

// The blocks a box intersects, as runs along x: one run per (by, bz), its ids consecutive.
TV_HD u32 rec_box_run_length(const RecBox& b) { return ((b.hi[0] + 15u) >> 4) - (b.lo[0] >> 4); }
TV_HD u32 rec_box_runs(const RecBox& b) { return (((b.hi[1] + 15u) >> 4) - (b.lo[1] >> 4)) * (((b.hi[2] + 15u) >> 4) - (b.lo[2] >> 4)); }
// the id of the first block of run q (by fastest)
TV_HD u32 rec_box_run(const RecBox& b, u32 nb, u32 q)
{
	const u32 ny = ((b.hi[1] + 15u) >> 4) - (b.lo[1] >> 4);
	return (((b.lo[2] >> 4) + q / ny) * nb + (b.lo[1] >> 4) + q % ny) * nb + (b.lo[0] >> 4);
}

// the bits [first, first + count) of a bitmap, one orWord(word, mask) per word they reach
template <class Or> TV_HD void rec_mark_run(u32 first, u32 count, const Or& orWord)
{
	const u32 end = first + count;
	for (u32 at = first; at < end;) {
		const u32 lo = at & 31u, room = 32u - lo, left = end - at;
		const u32 take = left < room ? left : room;
		orWord(at >> 5, (take == 32u ? 0xFFFFFFFFu : (1u << take) - 1u) << lo);
		at += take;
	}
}

// one word of a bitmap into the ascending list of its set bits; `before` = the set bits of the words below it
TV_HD void rec_list_word(u32 bits, u32 word, u32 before, u32* out)
{
	while (bits) {
		out[before++] = word * 32u + (u32)__builtin_ctz(bits);
		bits &= bits - 1u;
	}
}

// ---- rows -----------------------------------------------------------------------------------------------------------------------

struct RecRow { u32 w[4]; };
TV_HD RecRow rec_load16(const u8* p) { RecRow r; memcpy(r.w, __builtin_assume_aligned(p, 16), 16); return r; }
TV_HD void rec_store16(u8* p, const RecRow& r) { memcpy(__builtin_assume_aligned(p, 16), r.w, 16); }

TV_HD u32 rec_lane_entry(u32 t) { return t & (REC_GROUP - 1u); }
TV_HD u32 rec_lane_row(u32 t, u32 step) { return (t >> 3) + (REC_LANES / REC_GROUP) * step; }

// byte offset of row (z * 16 + y) of block `id` in a dense field of edge n (n is a multiple of 16: every row is 16-byte aligned)
TV_HD size_t rec_grid_row(u32 n, u32 id, u32 row)
{
	const u32 nb = n >> 4;
	const u32 bx = id % nb, by = (id / nb) % nb, bz = id / (nb * nb);
	return ((size_t)(bz * 16u + (row >> 4)) * n + (by * 16u + (row & 15u))) * n + bx * 16u;
}
TV_HD size_t rec_row(u32 entry, u32 row) { return (size_t)entry * 4096u + row * 16u; }

// bit x set where byte x of the two rows differs
TV_HD u32 rec_row_diff(const RecRow& a, const RecRow& b)
{
	u32 m = 0;
	for (u32 k = 0; k < 4; ++k) {
		const u32 x = a.w[k] ^ b.w[k];
		for (u32 j = 0; j < 4; ++j) if ((x >> (j * 8u)) & 0xFFu) m |= 1u << (k * 4u + j);
	}
	return m;
}
TV_HD bool rec_row_equal(const RecRow& a, const RecRow& b) { return ((a.w[0] ^ b.w[0]) | (a.w[1] ^ b.w[1]) | (a.w[2] ^ b.w[2]) | (a.w[3] ^ b.w[3])) == 0u; }

// grid -> record: one row of the three fields (id = the entry's block, read once by the lane)
TV_HD void rec_capture_row(const RecGrid& g, const RecView& r, u32 entry, u32 id, u32 row)
{
	const size_t src = rec_grid_row(g.n, id, row), dst = rec_row(entry, row);
	const RecRow d = rec_load16(g.dist + src), m = rec_load16(g.mat + src), b = rec_load16(g.blend + src);
	rec_store16(r.dist + dst, d); rec_store16(r.mat + dst, m); rec_store16(r.blend + dst, b);
}

// does one row of the record differ from the grid in any of its 48 bytes
TV_HD bool rec_differs_row(const RecGrid& g, const RecView& r, u32 entry, u32 id, u32 row)
{
	const size_t at = rec_grid_row(g.n, id, row), in = rec_row(entry, row);
	return !(rec_row_equal(rec_load16(g.dist + at), rec_load16(r.dist + in)) && rec_row_equal(rec_load16(g.mat + at), rec_load16(r.mat + in))
	         && rec_row_equal(rec_load16(g.blend + at), rec_load16(r.blend + in)));
}

// record -> record: one row of entry `from` of src into entry `to` of dst
TV_HD void rec_pack_row(const RecView& src, const RecView& dst, u32 from, u32 to, u32 row)
{
	const size_t a = rec_row(from, row), b = rec_row(to, row);
	const RecRow d = rec_load16(src.dist + a), m = rec_load16(src.mat + a), l = rec_load16(src.blend + a);
	rec_store16(dst.dist + b, d); rec_store16(dst.mat + b, m); rec_store16(dst.blend + b, l);
}
TV_HD void rec_pack_entry(const RecView& src, const RecView& dst, u32 from, u32 to) { dst.ids[to] = src.ids[from]; dst.flags[to] = src.flags[from]; }

// grid <-> record: one row of the three fields exchanged; bit x set where voxel x differed in distance, material or blend
TV_HD u32 rec_swap_row(const RecGrid& g, const RecView& r, u32 entry, u32 id, u32 row)
{
	const size_t at = rec_grid_row(g.n, id, row), in = rec_row(entry, row);
	const RecRow gd = rec_load16(g.dist + at), gm = rec_load16(g.mat + at), gb = rec_load16(g.blend + at);
	const RecRow rd = rec_load16(r.dist + in), rm = rec_load16(r.mat + in), rb = rec_load16(r.blend + in);
	rec_store16(g.dist + at, rd); rec_store16(g.mat + at, rm); rec_store16(g.blend + at, rb);
	rec_store16(r.dist + in, gd); rec_store16(r.mat + in, gm); rec_store16(r.blend + in, gb);
	return rec_row_diff(gd, rd) | rec_row_diff(gm, rm) | rec_row_diff(gb, rb);
}

// the flag byte of an entry exchanged; true where it differed
TV_HD bool rec_swap_flag(const RecGrid& g, const RecView& r, u32 entry, u32 id)
{
	const u8 a = g.flags[id], b = r.flags[entry];
	g.flags[id] = b; r.flags[entry] = a;
	return a != b;
}

// What one lane adds to the slot for a row whose differing voxels are `mask`: v[0..2] ~min, v[3..5] max, v[6] count - zeros
// where nothing differed, combined by max / sum (the kernels reduce per wave and per workgroup before the atomics).
TV_HD void rec_row_bounds(u32 n, u32 id, u32 row, u32 mask, u32 v[7])
{
	if (!mask) return;
	const u32 nb = n >> 4;
	const u32 x0 = (id % nb) * 16u, y = ((id / nb) % nb) * 16u + (row & 15u), z = (id / (nb * nb)) * 16u + (row >> 4);
	const u32 a = ~(x0 + (u32)__builtin_ctz(mask)), b = x0 + 31u - (u32)__builtin_clz(mask);
	if (a > v[0]) v[0] = a;
	if (~y > v[1]) v[1] = ~y;
	if (~z > v[2]) v[2] = ~z;
	if (b > v[3]) v[3] = b;
	if (y > v[4]) v[4] = y;
	if (z > v[5]) v[5] = z;
	v[6] += (u32)__builtin_popcount(mask);
}

// a slot as the result record: output order (x, z, y); differing voxels a..b inclusive -> [a, b + 1] clamped to [0, n]
TV_HD RecSwapResult rec_swap_result(u32 n, const RecSwapSlot& s)
{
	RecSwapResult r;
	const int order[3] = { 0, 2, 1 };
	for (int k = 0; k < 3; ++k) {
		const u32 a = ~s.notMin[order[k]], b = s.max[order[k]] + 1u;
		r.out_min[k] = s.changed ? (float)(a < n ? a : n) : 0.f;
		r.out_max[k] = s.changed ? (float)(b < n ? b : n) : 0.f;
	}
	r.changed_voxels = s.changed;
	r.changed_blocks = s.blocks; r.flag_changes = s.flagChanges;
	r.reserved = 0;
	return r;
}

} // namespace tv
