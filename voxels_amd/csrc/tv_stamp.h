// tv_stamp.h — the per-voxel and per-block logic of the stamps (include/voxels_hip.h, "stamps").  DESIGN.md §22.
//
// This header is the one place where that logic is written down, shared by the device kernels (vx_stamp.inl) and the host build
// of the tests (tests/stamp/stamp_host.cpp).  Everything here is integer arithmetic on bytes and coordinates.
//
// A stamp is a dense box of voxels, three byte fields, x fastest.  A paste puts an oriented stamp at an integer origin.  The eight
// orientations map boxes to boxes, and a stamp coordinate depends on one oriented coordinate only (PasteMap), so the part of a
// stamp that one 16^3 grid block needs is a box of at most 16^3 stamp voxels (PasteSection): a workgroup reads that box along the
// stamp's x into a tile and applies from the tile with the permuted index (paste_tile_index).
//
// The caller supplies the lanes (a workgroup, or a loop) and the reductions between them; the comparison with what the grid held
// and the result record are tv_undo.h's (rec_row_diff, rec_row_bounds, RecSwapSlot, rec_swap_result).
#pragma once

#include <vector>
#include "tv_undo.h"

namespace tv {

typedef int32_t i32;
typedef int64_t i64;

enum : u32 { STAMP_MAX_EDGE = 2048, STAMP_MAX_VOXELS = 1u << 30, PASTE_MAX_COUNT = 1u << 20, PASTE_MAX_STAMPS = 1u << 16 };
enum : u32 { PASTE_REPLACE = 0, PASTE_UNION = 1, PASTE_SUBTRACT = 2, PASTE_PAINT = 3, PASTE_MODES = 4 };

struct Paste { i32 origin[3]; u32 stamp, orient, mode, reserved[2]; };      // = vx_paste
struct PasteResult { RecBox box; u32 touched_blocks, reserved; };           // = vx_paste_result
struct PasteCounts {                                                        // = vx_paste_counts
	float out_min[3], out_max[3];
	unsigned long long changed_voxels;
	u32 changed_blocks, flag_changes, touched_blocks, reserved;
};

// a stamp's one allocation: distance, material, blend, `voxels` bytes each
struct StampView {
	const u8* base;
	u32 size[3], pad;
};
TV_HD size_t stamp_voxels(const u32 size[3]) { return (size_t)size[0] * size[1] * size[2]; }

// ---- the entry checks -----------------------------------------------------------------------------------------------------------

TV_HD const char* stamp_check_size(const u32 size[3])
{
	if (!size) return "null size";
	for (int k = 0; k < 3; ++k) if (!size[k] || size[k] > STAMP_MAX_EDGE) return "a stamp needs 1 <= size <= VX_STAMP_MAX_EDGE on every axis";
	if ((unsigned long long)size[0] * size[1] * size[2] > (unsigned long long)STAMP_MAX_VOXELS) return "more than VX_STAMP_MAX_VOXELS voxels";
	return nullptr;
}

TV_HD const char* stamp_check_box(u32 n, const RecBox* box)
{
	if (!box) return "null box";
	for (int k = 0; k < 3; ++k) if (!(box->lo[k] < box->hi[k] && box->hi[k] <= n)) return "the box needs lo < hi <= n on every axis";
	u32 size[3];
	for (int k = 0; k < 3; ++k) size[k] = box->hi[k] - box->lo[k];
	return stamp_check_size(size);
}

// what vx_grid_paste refuses before anything is launched; sizes[i][0] == 0 marks a null entry of the stamp array.  nullptr = fine
TV_HD const char* paste_check(const Paste* pastes, u32 count, const u32 (*sizes)[3], u32 nStamps)
{
	if (count && !pastes) return "null paste array";
	if (nStamps && !sizes) return "null stamp array";
	if (count > PASTE_MAX_COUNT) return "more than VX_PASTE_MAX_COUNT pastes";
	if (nStamps > PASTE_MAX_STAMPS) return "more than VX_PASTE_MAX_STAMPS stamps";
	for (u32 i = 0; i < count; ++i) {
		const Paste& p = pastes[i];
		if (p.stamp >= nStamps) return "a paste refers to a stamp beyond the array";
		if (!sizes[p.stamp][0]) return "a paste refers to a null stamp";
		if (p.orient > 7u) return "orient above 7";
		if (p.mode >= PASTE_MODES) return "unknown mode";
		if (p.reserved[0] || p.reserved[1]) return "non-zero reserved words";
	}
	return nullptr;
}

// ---- orientation ----------------------------------------------------------------------------------------------------------------

TV_HD void paste_oriented_size(u32 orient, const u32 size[3], u32 os[3])
{
	const bool odd = (orient & 1u) != 0u;
	os[0] = odd ? size[1] : size[0]; os[1] = odd ? size[0] : size[1]; os[2] = size[2];
}

// Oriented coordinates (u, v) -> stamp coordinates: i = i0 + iu * u + iv * v, j = j0 + ju * u + jv * v; one of iu, iv is zero and
// so is one of ju, jv.  The inverse of the header's table: with i' the mirrored i,
//   q = 0: i' = u, j = v        q = 1: i' = v, j = sy-1-u        q = 2: i' = sx-1-u, j = sy-1-v        q = 3: i' = sx-1-v, j = u
struct PasteMap { i32 i0, iu, iv, j0, ju, jv; };

TV_HD PasteMap paste_map(u32 orient, u32 sx, u32 sy)
{
	const i32 X = (i32)sx - 1, Y = (i32)sy - 1;
	PasteMap m;
	switch (orient & 3u) {
	case 0:  m.i0 = 0; m.iu = 1;  m.iv = 0;  m.j0 = 0; m.ju = 0;  m.jv = 1;  break;
	case 1:  m.i0 = 0; m.iu = 0;  m.iv = 1;  m.j0 = Y; m.ju = -1; m.jv = 0;  break;
	case 2:  m.i0 = X; m.iu = -1; m.iv = 0;  m.j0 = Y; m.ju = 0;  m.jv = -1; break;
	default: m.i0 = X; m.iu = 0;  m.iv = -1; m.j0 = 0; m.ju = 1;  m.jv = 0;  break;
	}
	if (orient & 4u) { m.i0 = X - m.i0; m.iu = -m.iu; m.iv = -m.iv; }
	return m;
}
TV_HD i32 paste_map_i(const PasteMap& m, i32 u, i32 v) { return m.i0 + m.iu * u + m.iv * v; }
TV_HD i32 paste_map_j(const PasteMap& m, i32 u, i32 v) { return m.j0 + m.ju * u + m.jv * v; }

// the clipped voxel box of a paste in a grid of edge n: 1 = touches the grid, 0 = misses it (out is zeroed)
TV_HD int paste_box(const Paste& p, const u32 size[3], u32 n, RecBox* out)
{
	u32 os[3];
	paste_oriented_size(p.orient, size, os);
	int any = 1;
	for (int k = 0; k < 3; ++k) {
		const i64 a = (i64)p.origin[k], b = a + (i64)os[k];
		const i64 lo = a > 0 ? a : 0, hi = b < (i64)n ? b : (i64)n;
		if (lo >= hi) any = 0;
		else { out->lo[k] = (u32)lo; out->hi[k] = (u32)hi; }
	}
	if (!any) for (int k = 0; k < 3; ++k) out->lo[k] = out->hi[k] = 0;
	return any;
}

// the blocks of a (non-empty) box: per axis first .. first + cnt - 1
TV_HD void paste_box_blocks(const RecBox& b, u32 first[3], u32 cnt[3])
{
	for (int k = 0; k < 3; ++k) { first[k] = b.lo[k] >> 4; cnt[k] = ((b.hi[k] + 15u) >> 4) - first[k]; }
}
TV_HD u32 paste_box_block_count(const RecBox& b) { u32 f[3], c[3]; paste_box_blocks(b, f, c); return c[0] * c[1] * c[2]; }

// ---- a paste inside one block ---------------------------------------------------------------------------------------------------

struct PasteSection {
	u32 lo[3], cnt[3];   // the voxels of the block the paste reaches, block-local
	i32 o[3];            // the oriented coordinates (u, v, k) of voxel lo
	i32 t0[3];           // the stamp box those voxels read: first (i, j, k) ...
	u32 tn[3];           // ... and extent, at most 16 each
	PasteMap map;
};

// false = the paste does not reach block bc (cannot happen for a listed block)
TV_HD bool paste_section(const Paste& p, const u32 size[3], const u32 bc[3], PasteSection& s)
{
	u32 os[3];
	paste_oriented_size(p.orient, size, os);
	for (int k = 0; k < 3; ++k) {
		const i64 a = (i64)p.origin[k], b = a + (i64)os[k], m0 = (i64)bc[k] * 16, m1 = m0 + 16;
		const i64 lo = a > m0 ? a : m0, hi = b < m1 ? b : m1;
		if (lo >= hi) return false;
		s.lo[k] = (u32)(lo - m0); s.cnt[k] = (u32)(hi - lo); s.o[k] = (i32)(lo - a);
	}
	s.map = paste_map(p.orient, size[0], size[1]);
	const i32 u1 = s.o[0] + (i32)s.cnt[0] - 1, v1 = s.o[1] + (i32)s.cnt[1] - 1;
	const i32 ia = paste_map_i(s.map, s.o[0], s.o[1]), ib = paste_map_i(s.map, u1, v1);
	const i32 ja = paste_map_j(s.map, s.o[0], s.o[1]), jb = paste_map_j(s.map, u1, v1);
	s.t0[0] = ia < ib ? ia : ib; s.tn[0] = (u32)(ia < ib ? ib - ia : ia - ib) + 1u;
	s.t0[1] = ja < jb ? ja : jb; s.tn[1] = (u32)(ja < jb ? jb - ja : ja - jb) + 1u;
	s.t0[2] = s.o[2]; s.tn[2] = s.cnt[2];
	return true;
}

// the tile: element q of the section's stamp box, i fastest (the order of the reads), and where it lies in the stamp's fields
TV_HD u32 paste_tile_count(const PasteSection& s) { return s.tn[0] * s.tn[1] * s.tn[2]; }
TV_HD size_t paste_tile_source(const PasteSection& s, const u32 size[3], u32 q, u32& at)
{
	const u32 di = q % s.tn[0], dj = (q / s.tn[0]) % s.tn[1], dk = q / (s.tn[0] * s.tn[1]);
	at = (dk * 16u + dj) * 16u + di;
	return ((size_t)((u32)s.t0[2] + dk) * size[1] + ((u32)s.t0[1] + dj)) * size[0] + ((u32)s.t0[0] + di);
}

// voxel v of the section (x fastest): its place in the block (li) and in the tile
TV_HD u32 paste_voxel_count(const PasteSection& s) { return s.cnt[0] * s.cnt[1] * s.cnt[2]; }
TV_HD u32 paste_tile_index(const PasteSection& s, u32 v, u32& li)
{
	const u32 x = v % s.cnt[0], y = (v / s.cnt[0]) % s.cnt[1], z = v / (s.cnt[0] * s.cnt[1]);
	li = ((s.lo[2] + z) * 16u + s.lo[1] + y) * 16u + s.lo[0] + x;
	const i32 u = s.o[0] + (i32)x, w = s.o[1] + (i32)y;
	const u32 di = (u32)(paste_map_i(s.map, u, w) - s.t0[0]), dj = (u32)(paste_map_j(s.map, u, w) - s.t0[1]);
	return (z * 16u + dj) * 16u + di;
}

// the four modes: the grid's (d, m, b) under the stamp's (sd, sm, sb)
TV_HD void paste_combine(u32 mode, i8 sd, u8 sm, u8 sb, i8& d, u8& m, u8& b)
{
	if (mode == PASTE_REPLACE) { d = sd; m = sm; b = sb; }
	else if (mode == PASTE_UNION) { if (sd < d) { d = sd; m = sm; b = sb; } }
	else if (mode == PASTE_SUBTRACT) { const i8 c = sd == (i8)-128 ? (i8)127 : (i8)-sd; if (c > d) d = c; }
	else { if (sd < 0) { m = sm; b = sb; } }
}
TV_HD bool paste_mode_reads_materials(u32 mode) { return mode != PASTE_SUBTRACT; }
TV_HD bool paste_mode_writes_distance(u32 mode) { return mode != PASTE_PAINT; }

// BF_Empty of a block by the codec's rule (k_edit_flags of vx_hip.hip), serially: a run starts where the value changes and every
// 255 voxels inside a constant stretch; empty <=> at most 2048 runs and every sample has strictly the sign of the first.
TV_HD u8 paste_block_empty(const i8* d /* 4096, rows z-major */)
{
	u32 runs = 0, start = 0;
	bool same = true;
	for (u32 i = 0; i < 4096u; ++i) {
		if (i == 0 || d[i] != d[i - 1]) start = i;
		if ((i - start) % 255u == 0u) ++runs;
		same = same && ((int)d[0] * (int)d[i] > 0);
	}
	return (same && runs <= 2048u) ? 1 : 0;
}

// a slot as the counts record
TV_HD PasteCounts paste_counts(u32 n, const RecSwapSlot& s, u32 touched)
{
	const RecSwapResult r = rec_swap_result(n, s);
	PasteCounts c;
	for (int k = 0; k < 3; ++k) { c.out_min[k] = r.out_min[k]; c.out_max[k] = r.out_max[k]; }
	c.changed_voxels = r.changed_voxels; c.changed_blocks = r.changed_blocks; c.flag_changes = r.flag_changes;
	c.touched_blocks = touched; c.reserved = 0;
	return c;
}

// ---- the plan of a batch (host) -------------------------------------------------------------------------------------------------

// Chunks of consecutive pastes whose (paste, block) lists fit `listCap` entries (a chunk of one paste may exceed it: the lists
// are sized by the largest chunk).  A block that more than one chunk touches is compared, at its last chunk, with a snapshot its
// first chunk took: first / last = the chunks, snapOf = the snapshot's index (~0 = none needed).
struct PasteChunk { u32 begin, end, slots; size_t entries; u32 most; };   // most = the blocks of its largest paste
struct PastePlan {
	std::vector<PasteChunk> chunks;
	std::vector<u32> first, last, snapOf;   // per block of the grid; first = ~0: untouched
	std::vector<u32> marked;                // the touched blocks: a plan that is kept clears only these for the next batch
	u32 distinct = 0, snaps = 0;
	size_t maxEntries = 0;
	u32 maxSlots = 0;
};

inline void paste_plan(const Paste* pastes, u32 count, const u32 (*sizes)[3], u32 n, size_t listCap, PasteResult* results, PastePlan& plan)
{
	const u32 nb = n >> 4;
	const size_t blocks = (size_t)nb * nb * nb;
	plan.chunks.clear();
	if (plan.first.size() != blocks) { plan.first.assign(blocks, ~0u); plan.last.assign(blocks, ~0u); }
	else for (u32 id : plan.marked) plan.first[id] = plan.last[id] = ~0u;
	plan.marked.clear(); plan.snapOf.clear();
	plan.distinct = plan.snaps = 0;
	PasteChunk cur = { 0, 0, 0, 0, 0 };
	for (u32 i = 0; i < count; ++i) {
		RecBox box;
		const int hit = paste_box(pastes[i], sizes[pastes[i].stamp], n, &box);
		const u32 touched = hit ? paste_box_block_count(box) : 0u;
		if (results) { results[i].box = box; results[i].touched_blocks = touched; results[i].reserved = 0; }
		if (!touched) continue;
		if (cur.entries && cur.entries + touched > listCap) { cur.end = i; plan.chunks.push_back(cur); cur = PasteChunk{ i, i, 0, 0, 0 }; }
		const u32 chunk = (u32)plan.chunks.size();
		u32 f[3], c[3];
		paste_box_blocks(box, f, c);
		for (u32 z = f[2]; z < f[2] + c[2]; ++z)
		for (u32 y = f[1]; y < f[1] + c[1]; ++y)
		for (u32 x = f[0]; x < f[0] + c[0]; ++x) {
			const size_t id = ((size_t)z * nb + y) * nb + x;
			if (plan.first[id] == ~0u) { plan.first[id] = chunk; ++plan.distinct; plan.marked.push_back((u32)id); }
			if (plan.last[id] != chunk) { plan.last[id] = chunk; ++cur.slots; }
		}
		cur.entries += touched;
		if (touched > cur.most) cur.most = touched;
	}
	cur.end = count;
	plan.chunks.push_back(cur);
	plan.maxEntries = 0; plan.maxSlots = 0;
	for (const PasteChunk& k : plan.chunks) { if (k.entries > plan.maxEntries) plan.maxEntries = k.entries; if (k.slots > plan.maxSlots) plan.maxSlots = k.slots; }
	if (plan.chunks.size() > 1) {
		plan.snapOf.assign(blocks, ~0u);
		for (u32 id : plan.marked) if (plan.first[id] != plan.last[id]) plan.snapOf[id] = plan.snaps++;
	}
}

} // namespace tv
