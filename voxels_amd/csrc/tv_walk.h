// tv_walk.h — the per-tile logic of vx_grid_walk_field (include/voxels_hip.h, "walk fields"): the cost of the cheapest walk
// from every standable voxel of a box of the grid to the nearest goal, and the move to take there.  DESIGN.md §19.
//
// Shared by the device kernels (vx_walk.inl) and the sequential CPU emulation of the tests (tests/walk/walk_host.cpp): every
// function is what ONE lane of a workgroup does in one phase, the caller supplies the lanes (a workgroup, or a loop) and the
// barriers between the phases.  Cells that several lanes touch go through an `Ops` policy: relaxed atomics on the device,
// plain reads and writes in the emulation.  Region and tile bookkeeping are those of tv_island.h.
//
// The field F holds one u32 per voxel of the region, x fastest.  Every value ever stored in it is WALK_UNREACHED or the cost
// of a real walk from that cell to a goal, and a cell's value only ever falls: whatever order the tiles are served in, the
// values stop falling exactly at the least solution of the recurrence in the header.
#pragma once

#include <string.h>

#include "tv_island.h"

namespace tv {

typedef uint16_t u16;

enum : u32 { WALK_UNREACHED = 0xFFFFFFFFu, WALK_MAX_GOALS = 65536u, WALK_MAX_COST = 1u << 30 };
enum { WALK_DIR_UNREACHED = 0xFF, WALK_DIR_GOAL = 0xFE };
enum {
	WALK_MAX_STEP = 4,                         // step_up, step_down
	WALK_LX = 18,                              // a tile with its halo of one voxel in x and y ...
	WALK_LZ = 16 + 2 * WALK_MAX_STEP,          // ... and of max(step_up, step_down) voxels in z
	WALK_CELLS = WALK_LZ * WALK_LX * WALK_LX,  // 7776 words of field
	WALK_COLS = WALK_LX * WALK_LX,             // one word of standable bits per column of the staged tile
	WALK_TILE_PASSES = 64,                     // cap of the relaxation passes of one tile in one sweep
	WALK_SWEEP_BATCH = 8,                      // sweeps the host launches between two looks at the counters
	WALK_SELF = 13                             // bit of the tile itself in a mask over the 3 x 3 x 3 tiles around it
};

struct WalkQuery {       // = vx_walk_query
	u32 lo[3], hi[3];
	u32 whole_grid, clearance, step_up, step_down, cost_axial, cost_diagonal, cost_climb, max_cost, flags, reserved;
};

struct WalkGoal { u32 x, y, z, cost; };   // = vx_walk_goal

struct WalkCounts {      // = vx_walk_counts
	unsigned long long standable, reached;
	u32 goals_used, goals_ignored, max_distance, sweeps;
};

struct WalkParams {
	u32 clearance, up, down, halo;   // halo = max(up, down): the z halo of a staged tile
	u32 axial, diagonal, climb, maxCost;
};

struct WalkOpsPlain : IslOpsPlain {
	static TV_HD void store(u32* p, u32 v) { *p = v; }
};

// The checks of the header, in its order; nullptr when the query is fine.  lo / hi receive the box.
inline const char* walk_check(u32 n, bool wholeGridOwned, const WalkQuery* q, const void* goals, u32 goalCount, const void* counts,
                              const void* field, u32 lo[3], u32 hi[3], WalkParams* P)
{
	if (!q || !counts) return "null query or counts";
	if (!wholeGridOwned) return "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)";
	if (q->flags) return "flags must be 0";
	if (q->clearance < 1u || q->clearance > 32u) return "clearance outside 1..32";
	if (q->step_up > (u32)WALK_MAX_STEP || q->step_down > (u32)WALK_MAX_STEP) return "step_up or step_down above 4";
	if (q->cost_axial < 1u || q->cost_axial > 65535u) return "cost_axial outside 1..65535";
	if (q->cost_diagonal > 65535u || q->cost_climb > 65535u) return "cost_diagonal or cost_climb above 65535";
	if (q->max_cost > (u32)WALK_MAX_COST) return "max_cost above 2^30";
	if (goalCount > (u32)WALK_MAX_GOALS) return "more than VX_WALK_MAX_GOALS goals";
	if (goalCount && !goals) return "null goal array";
	if (field && ((uintptr_t)field & 15u)) return "d_field is not 16-byte aligned";
	unsigned long long V = 1;
	for (int k = 0; k < 3; ++k) {
		lo[k] = q->whole_grid ? 0u : q->lo[k];
		hi[k] = q->whole_grid ? n : q->hi[k];
		if (!(lo[k] < hi[k] && hi[k] <= n)) return "the box needs lo < hi <= n on every axis";
		V *= hi[k] - lo[k];
	}
	if (V > (1ull << 28)) return "the box holds more than 2^28 voxels";
	P->clearance = q->clearance; P->up = q->step_up; P->down = q->step_down; P->halo = q->step_up > q->step_down ? q->step_up : q->step_down;
	P->axial = q->cost_axial; P->diagonal = q->cost_diagonal; P->climb = q->cost_climb; P->maxCost = q->max_cost;
	return nullptr;
}

TV_HD bool walk_in_region(const IslRegion& r, int x, int y, int z)
{
	return x >= (int)r.lo[0] && x < (int)(r.lo[0] + r.ext[0]) && y >= (int)r.lo[1] && y < (int)(r.lo[1] + r.ext[1]) && z >= (int)r.lo[2] && z < (int)(r.lo[2] + r.ext[2]);
}

// tile index of the block that holds voxel (x, y, z) of the region
TV_HD u32 walk_tile_of(const IslRegion& r, u32 x, u32 y, u32 z) { return (((z >> 4) - r.tb0[2]) * r.tn[1] + ((y >> 4) - r.tb0[1])) * r.tn[0] + ((x >> 4) - r.tb0[0]); }

// The standable volume: per tile 256 words of 16 bits, word (y & 15) + 16 (z & 15), bit x & 15; bits outside the region are 0.
TV_HD u32 walk_stand_bit(const IslRegion& r, const u16* stand, u32 x, u32 y, u32 z)
{
	return ((u32)stand[(size_t)walk_tile_of(r, x, y, z) * 256u + (y & 15u) + 16u * (z & 15u)] >> (x & 15u)) & 1u;
}

// horizontal offsets of the move codes 0..7: (+1,0) (-1,0) (0,+1) (0,-1) (+1,+1) (-1,+1) (+1,-1) (-1,-1)
TV_HD int walk_dx(int o) { return o < 2 ? (o == 0 ? 1 : -1) : o < 4 ? 0 : ((o & 1) ? -1 : 1); }
TV_HD int walk_dy(int o) { return o < 2 ? 0 : o < 4 ? (o == 2 ? 1 : -1) : (o < 6 ? 1 : -1); }

// ---- phase "stand": lane t owns row t = (y = t & 15, z = t >> 4) of the block ----

// bit x set <=> sample x of the 16-sample row (16-byte aligned) is solid
TV_HD u32 walk_solid_bits(const i8* row)
{
	u32 w[4];
	memcpy(w, __builtin_assume_aligned(row, 16), 16);
	u32 m = 0;
	for (int k = 0; k < 4; ++k) m |= (((w[k] >> 7) & 1u) | ((w[k] >> 14) & 2u) | ((w[k] >> 21) & 4u) | ((w[k] >> 28) & 8u)) << (4 * k);
	return m;
}

// the standable cells of the row, clipped to the region: solid below, air over `clearance` samples from the cell up; the
// column is read from the grid, whatever the box
TV_HD u32 walk_stand_row(const i8* dist, u32 n, const IslTile& T, u32 t, u32 clearance)
{
	const u32 y = t & 15u, z = t >> 4;
	if (!isl_row_inside(T, y, z)) return 0u;
	const u32 gy = T.org[1] + y, gz = T.org[2] + z;
	if (gz == 0u) return 0u;
	const i8* at = dist + ((size_t)gz * n + gy) * n + T.org[0];
	const size_t plane = (size_t)n * n;
	u32 m = walk_solid_bits(at - plane) & isl_clip_bits(T);
	for (u32 k = 0; k < clearance && m; ++k) if (gz + k < n) m &= ~walk_solid_bits(at + k * plane);
	return m;
}

// every voxel of the tile's clip starts unreached
TV_HD void walk_field_init(const IslRegion& r, const IslTile& T, u32 t, u32 lanes, u32* F)
{
	for (u32 li = t; li < 4096u; li += lanes) {
		const u32 x = T.org[0] + (li & 15u);
		if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8)) F[isl_local_to_region(r, T, li)] = (u32)WALK_UNREACHED;
	}
}

// The tiles, as bits of the 3 x 3 x 3 around the tile of block-local cell (x, y, z), that hold a cell with a move onto that
// cell: a cell one column away, up to step_up below or step_down above.
TV_HD u32 walk_reach_mask(const WalkParams& P, int x, int y, int z)
{
	const int sx = x == 0 ? -1 : x == 15 ? 1 : 0, sy = y == 0 ? -1 : y == 15 ? 1 : 0, sz = z < (int)P.up ? -1 : z + (int)P.down > 15 ? 1 : 0;
	u32 mask = 0u;
	for (int c = 1; c < 8; ++c) {
		const int ax = (c & 1) ? sx : 0, ay = (c & 2) ? sy : 0, az = (c & 4) ? sz : 0;
		if (ax || ay || az) mask |= 1u << ((az + 1) * 9 + (ay + 1) * 3 + (ax + 1));
	}
	return mask;
}

// the k-th tile (k < 27) of the 3 x 3 x 3 around `tile`, WALK_UNREACHED when it lies outside the region or holds no standable cell
TV_HD u32 walk_tile_around(const IslRegion& r, u32 tile, u32 k, const u32* tileStand)
{
	const int b[3] = { (int)(tile % r.tn[0]) + (int)(k % 3u) - 1, (int)((tile / r.tn[0]) % r.tn[1]) + (int)((k / 3u) % 3u) - 1, (int)(tile / (r.tn[0] * r.tn[1])) + (int)(k / 9u) - 1 };
	for (int a = 0; a < 3; ++a) if (b[a] < 0 || b[a] >= (int)r.tn[a]) return (u32)WALK_UNREACHED;
	const u32 nt = ((u32)b[2] * r.tn[1] + (u32)b[1]) * r.tn[0] + (u32)b[0];
	return tileStand[nt] ? nt : (u32)WALK_UNREACHED;
}

// ---- phase "seed": one goal ----
// A used goal lowers its cell like a relaxation does, so it flags what a relaxation would flag: its own tile and every tile
// that holds a cell with a move onto the goal cell (a goal on a tile border may be the only way into the tile next door).
template <class O> TV_HD void walk_seed(const IslRegion& r, const WalkParams& P, const u16* stand, const u32* tileStand, const WalkGoal& g, u32* F, u32* active, WalkCounts* counts)
{
	const bool inside = g.x < r.n && g.y < r.n && g.z < r.n && walk_in_region(r, (int)g.x, (int)g.y, (int)g.z);
	if (!inside || g.cost > P.maxCost || !walk_stand_bit(r, stand, g.x, g.y, g.z)) { O::aadd(&counts->goals_ignored, 1u); return; }
	O::amin(F + isl_index(r, g.x, g.y, g.z), g.cost);
	const u32 tile = walk_tile_of(r, g.x, g.y, g.z);
	const u32 mask = walk_reach_mask(P, (int)(g.x & 15u), (int)(g.y & 15u), (int)(g.z & 15u)) | (1u << WALK_SELF);
	for (u32 k = 0; k < 27u; ++k) {
		if (!((mask >> k) & 1u)) continue;
		const u32 nt = walk_tile_around(r, tile, k, tileStand);
		if (nt != (u32)WALK_UNREACHED) O::aor(active + nt, 1u);
	}
	O::aadd(&counts->goals_used, 1u);
}

// ---- the staged tile: sF[WALK_CELLS] and sCol[WALK_COLS], cell (x, y, z) of the block, x and y in -1..16, z in -halo..15+halo ----

TV_HD u32 walk_cell(const WalkParams& P, int x, int y, int z) { return (u32)((z + (int)P.halo) * WALK_LX + (y + 1)) * WALK_LX + (u32)(x + 1); }
TV_HD u32 walk_col(int x, int y) { return (u32)(y + 1) * WALK_LX + (u32)(x + 1); }

TV_HD void walk_stage_clear(u32 t, u32 lanes, u32* sCol)
{
	for (u32 i = t; i < (u32)WALK_COLS; i += lanes) sCol[i] = 0u;
}

// field values (other tiles' cells may be falling meanwhile: any value read is the cost of a real walk) and standable bits
template <class O> TV_HD void walk_stage(const IslRegion& r, const IslTile& T, const WalkParams& P, u32 t, u32 lanes, const u32* F, const u16* stand, u32* sF, u32* sCol)
{
	const u32 depth = 16u + 2u * P.halo, cells = depth * (u32)WALK_COLS;
	for (u32 i = t; i < cells; i += lanes) {
		const u32 lz = i / (u32)WALK_COLS, c = i % (u32)WALK_COLS;
		const int x = (int)(T.org[0] + c % (u32)WALK_LX) - 1, y = (int)(T.org[1] + c / (u32)WALK_LX) - 1, z = (int)(T.org[2] + lz) - (int)P.halo;
		u32 f = (u32)WALK_UNREACHED;
		if (walk_in_region(r, x, y, z) && walk_stand_bit(r, stand, (u32)x, (u32)y, (u32)z)) {
			f = O::load(F + isl_index(r, (u32)x, (u32)y, (u32)z));
			O::aor(sCol + c, 1u << lz);
		}
		sF[i] = f;
	}
}

// The cheapest move out of cell (x, y, z) of the staged tile: the least w + F(c') over the moves c -> c' whose sum does not
// exceed max_cost, and among those the least move code; WALK_UNREACHED / WALK_DIR_GOAL when there is none.  Sums stay below
// 2^30 + 5 * 65535: no wrap.
template <class O> TV_HD u32 walk_best(const WalkParams& P, const u32* sF, const u32* sCol, int x, int y, int z, u32* code)
{
	const u32 lz = (u32)(z + (int)P.halo);
	const u32 range = ((2u << (lz + P.up)) - 1u) & ~((1u << (lz - P.down)) - 1u); // bits lz - down .. lz + up (lz + up <= 23)
	u32 best = (u32)WALK_UNREACHED, bestCode = (u32)WALK_DIR_GOAL;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
	for (int o = 0; o < 8; ++o) {
		const int dx = walk_dx(o), dy = walk_dy(o);
		if (o >= 4 && !P.diagonal) continue;
		u32 m = sCol[walk_col(x + dx, y + dy)] & range;
		if (o >= 4 && (!(sCol[walk_col(x + dx, y)] & range) || !(sCol[walk_col(x, y + dy)] & range))) m = 0u; // no cutting of corners
		const u32 flat = o >= 4 ? P.diagonal : P.axial;
		for (u32 k = 0; k <= P.up + P.down && m; ++k) {
			const u32 tz = (u32)__builtin_ctz(m);
			m &= m - 1u;
			const u32 f = O::load(sF + (tz * (u32)WALK_LX + (u32)(y + dy + 1)) * (u32)WALK_LX + (u32)(x + dx + 1));
			if (f == (u32)WALK_UNREACHED) continue;
			const int dz = (int)tz - (int)lz;
			const u32 cand = f + flat + (u32)(dz < 0 ? -dz : dz) * P.climb, c = (u32)o | ((u32)(dz + 4) << 3);
			if (cand > P.maxCost) continue;
			if (cand < best || (cand == best && c < bestCode)) { best = cand; bestCode = c; }
		}
	}
	*code = bestCode;
	return best;
}

// ---- phase "relax": lane t owns column (x = t & 15, y = t >> 4) of the block ----

// one pass over the column; true when a cell fell
template <class O> TV_HD bool walk_relax_column(const WalkParams& P, u32 t, u32* sF, const u32* sCol)
{
	const int x = (int)(t & 15u), y = (int)(t >> 4);
	u32 own = (sCol[walk_col(x, y)] >> P.halo) & 0xFFFFu;
	bool fell = false;
	for (u32 k = 0; k < 16u && own; ++k) {
		const int z = __builtin_ctz(own);
		own &= own - 1u;
		u32 code;
		const u32 best = walk_best<O>(P, sF, sCol, x, y, z, &code), at = walk_cell(P, x, y, z);
		if (best < O::load(sF + at)) { O::store(sF + at, best); fell = true; }
	}
	return fell;
}

// The column's cells that fell go back to the field (the tile is the only writer of its cells).  Returns the tiles, as bits of
// the 3 x 3 x 3 around this one, that hold a cell with a move onto one that fell: a cell one column away, up to step_up below
// or step_down above.
template <class O> TV_HD u32 walk_store_column(const IslRegion& r, const IslTile& T, const WalkParams& P, u32 t, const u32* sF, const u32* sCol, u32* F)
{
	const int x = (int)(t & 15u), y = (int)(t >> 4);
	u32 own = (sCol[walk_col(x, y)] >> P.halo) & 0xFFFFu, mask = 0u;
	for (u32 k = 0; k < 16u && own; ++k) {
		const int z = __builtin_ctz(own);
		own &= own - 1u;
		const u32 v = sF[walk_cell(P, x, y, z)], i = isl_index(r, T.org[0] + (u32)x, T.org[1] + (u32)y, T.org[2] + (u32)z);
		if (v >= F[i]) continue;
		O::store(F + i, v);
		mask |= walk_reach_mask(P, x, y, z);
	}
	return mask;
}

// lane k < 27: the k-th tile around this one is flagged for the next sweep when the mask names it, it exists and it holds
// standable cells; the counter counts the tiles newly flagged
template <class O> TV_HD void walk_flag_tile(const IslRegion& r, u32 tile, u32 k, u32 mask, const u32* tileStand, u32* next, u32* counter)
{
	if (k >= 27u || !((mask >> k) & 1u)) return;
	const u32 nt = walk_tile_around(r, tile, k, tileStand);
	if (nt != (u32)WALK_UNREACHED && O::aor(next + nt, 1u) == 0u) O::aadd(counter, 1u);
}

// ---- phase "finish": lane t owns column t of the block: reached cells, the largest distance, the direction bytes ----
template <class O> TV_HD void walk_finish_column(const IslRegion& r, const IslTile& T, const WalkParams& P, u32 t, const u32* sF, const u32* sCol, u8* dirs, u32* reached, u32* maxDist)
{
	const int x = (int)(t & 15u), y = (int)(t >> 4);
	const u32 gx = T.org[0] + (u32)x, gy = T.org[1] + (u32)y;
	if (gx < T.c0[0] || gx >= T.c1[0] || gy < T.c0[1] || gy >= T.c1[1]) return;
	u32 count = 0, far = 0;
	for (u32 z = T.c0[2] - T.org[2]; z < T.c1[2] - T.org[2]; ++z) {
		const u32 f = sF[walk_cell(P, x, y, (int)z)];
		u32 code = (u32)WALK_DIR_UNREACHED;
		if (f != (u32)WALK_UNREACHED) {
			++count;
			far = f > far ? f : far;
			if (dirs && walk_best<O>(P, sF, sCol, x, y, (int)z, &code) != f) code = (u32)WALK_DIR_GOAL;
		}
		if (dirs) dirs[isl_index(r, gx, gy, T.org[2] + z)] = (u8)code;
	}
	if (count) { O::aadd(reached, count); O::amax(maxDist, far); }
}

// a tile without standable cells: nothing is reached
TV_HD void walk_finish_dead(const IslRegion& r, const IslTile& T, u32 t, u32 lanes, u8* dirs)
{
	for (u32 li = t; li < 4096u; li += lanes) {
		const u32 x = T.org[0] + (li & 15u);
		if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8)) dirs[isl_local_to_region(r, T, li)] = (u8)WALK_DIR_UNREACHED;
	}
}

} // namespace tv
