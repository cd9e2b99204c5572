// vx_walk.inl — vx_grid_walk_field (include/voxels_hip.h, "walk fields"): walking distances to the nearest goal and flow
// directions over a box of the resident grid; included by vx_hip.hip after vx_smooth.inl (HIP only).  DESIGN.md §19.  The
// per-lane logic is tv_walk.h, shared with the CPU emulation of the tests.
//
//   k_walk_stand   one workgroup per tile (a 16^3 block clipped to the box), one lane per x-row: the standable cells from the
//                  grid's columns, one bit per voxel; the tile's part of the field becomes UNREACHED; standable cells counted
//   k_walk_seed    one lane per goal: checked against the standable volume, its cost applied by an integer minimum on the
//                  field cell, its tile and the tiles that can reach the cell flagged, used and ignored goals counted
//   -- the host reads the counts (the cap of the sweep loop is the number of standable cells) --
//   k_walk_relax   one sweep: one workgroup per tile; a tile that is not flagged returns at once, a flagged one stages its field
//                  and standable bits with their halo into LDS, relaxes there until a pass changes nothing (or the pass cap), stores
//                  its own cells that fell and flags, for the NEXT sweep, the tiles around it that can reach one of them
//   -- the host launches sweeps in batches and reads, per batch, how many tiles each sweep flagged; zero ends the loop --
//   k_walk_finish  one workgroup per tile: reached cells, the largest distance, the direction bytes.
// No workgroup waits for another; every loop is bounded by a constant or by a launch parameter.
#include "tv_walk.h"

namespace {

struct WalkOpsDev : IslOpsDev {
#if defined(__HIP_DEVICE_COMPILE__)
	static TV_HD void store(u32* p, u32 v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
	static TV_HD void store(u32* p, u32 v) { *p = v; }
#endif
};

struct WalkState {
	void* volume = nullptr;   // the field when the caller gives none
	size_t volumeCap = 0;
	void* perTile = nullptr;  // standable bits (512 bytes), standable count and the two sweep flags (12 bytes) per tile
	size_t perTileCap = 0;
	void* goals = nullptr;
	size_t goalsCap = 0;
	void* small = nullptr;    // WalkCounts, then the counters of one batch of sweeps

	void release(vx_ctx* c)
	{
		c->be.free(volume); c->be.free(perTile); c->be.free(goals); c->be.free(small);
	}
};

enum { WALK_SMALL_BYTES = 128, WALK_AT_COUNTERS = 64 };

__global__ __launch_bounds__(WG) void k_walk_stand(GridView g, IslRegion r, WalkParams P, u16* stand, u32* tileStand, u32* F, WalkCounts* counts)
{
	__shared__ u32 sCount;
	const u32 t = threadIdx.x;
	const IslTile T = isl_tile(r, blockIdx.x);
	if (t == 0) sCount = 0;
	__syncthreads();
	const u32 mask = walk_stand_row(g.dist, r.n, T, t, P.clearance);
	stand[(size_t)blockIdx.x * 256u + t] = (u16)mask;
	if (mask) atomicAdd(&sCount, (u32)__builtin_popcount(mask));
	walk_field_init(r, T, t, WG, F);
	__syncthreads();
	if (t == 0) {
		tileStand[blockIdx.x] = sCount;
		if (sCount) WalkOpsDev::aadd64(&counts->standable, sCount);
	}
}

__global__ __launch_bounds__(WG) void k_walk_seed(IslRegion r, WalkParams P, const u16* stand, const u32* tileStand, const WalkGoal* goals, u32 count, u32* F, u32* active, WalkCounts* counts)
{
	const u32 k = blockIdx.x * WG + threadIdx.x;
	if (k < count) walk_seed<WalkOpsDev>(r, P, stand, tileStand, goals[k], F, active, counts);
}

__global__ __launch_bounds__(WG) void k_walk_relax(IslRegion r, WalkParams P, const u16* stand, const u32* tileStand, u32* F, u32* active, u32* next, u32* counter)
{
	__shared__ u32 sF[WALK_CELLS];
	__shared__ u32 sCol[WALK_COLS];
	__shared__ u32 sAround;
	const u32 t = threadIdx.x, tile = blockIdx.x;
	if (!active[tile]) return; // (uniform; the flag is cleared behind the barriers below)
	const IslTile T = isl_tile(r, tile);
	walk_stage_clear(t, WG, sCol);
	if (t == 0) sAround = 0;
	__syncthreads();
	walk_stage<WalkOpsDev>(r, T, P, t, WG, F, stand, sF, sCol);
	__syncthreads();
	int fell = 1;
	for (u32 pass = 0; pass < (u32)WALK_TILE_PASSES && fell; ++pass)
		fell = __syncthreads_or(walk_relax_column<WalkOpsDev>(P, t, sF, sCol) ? 1 : 0);
	u32 around = walk_store_column<WalkOpsDev>(r, T, P, t, sF, sCol, F);
	if (fell) around |= 1u << WALK_SELF; // the cap ended the passes: this tile goes on in the next sweep
	if (around) atomicOr(&sAround, around);
	__syncthreads();
	walk_flag_tile<WalkOpsDev>(r, tile, t, sAround, tileStand, next, counter);
	if (t == 0) active[tile] = 0;
}

__global__ __launch_bounds__(WG) void k_walk_finish(IslRegion r, WalkParams P, const u16* stand, const u32* tileStand, const u32* F, u8* dirs, WalkCounts* counts)
{
	__shared__ u32 sF[WALK_CELLS];
	__shared__ u32 sCol[WALK_COLS];
	__shared__ u32 sReached, sFar;
	const u32 t = threadIdx.x, tile = blockIdx.x;
	const IslTile T = isl_tile(r, tile);
	if (!tileStand[tile]) { // (uniform)
		if (dirs) walk_finish_dead(r, T, t, WG, dirs);
		return;
	}
	walk_stage_clear(t, WG, sCol);
	if (t == 0) { sReached = 0; sFar = 0; }
	__syncthreads();
	walk_stage<WalkOpsDev>(r, T, P, t, WG, F, stand, sF, sCol);
	__syncthreads();
	walk_finish_column<WalkOpsDev>(r, T, P, t, sF, sCol, dirs, &sReached, &sFar);
	__syncthreads();
	if (t == 0 && sReached) {
		WalkOpsDev::aadd64(&counts->reached, sReached);
		WalkOpsDev::amax(&counts->max_distance, sFar);
	}
}

} // namespace

extern "C" {

static_assert(sizeof(vx_walk_query) == 64 && sizeof(vx_walk_goal) == 16 && sizeof(vx_walk_counts) == 32, "vx_walk_query / vx_walk_goal / vx_walk_counts layout");
static_assert(sizeof(WalkQuery) == sizeof(vx_walk_query) && sizeof(WalkGoal) == sizeof(vx_walk_goal) && sizeof(WalkCounts) == sizeof(vx_walk_counts), "tv_walk.h records");
static_assert(VX_WALK_UNREACHED == tv::WALK_UNREACHED && VX_WALK_MAX_GOALS == tv::WALK_MAX_GOALS, "walk constants");

int vx_grid_walk_field(vx_ctx* c, const vx_walk_query* query, const vx_walk_goal* goals, uint32_t goal_count,
                       uint32_t* d_field, uint8_t* d_dirs, vx_walk_counts* counts)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_walk_field: ";
	if (!c) return VX_ERR_INVALID;
	if (counts) memset(counts, 0, sizeof(*counts));
	const bool whole = c->ownsGrid && c->n && c->zBegin == 0 && c->zEnd == c->n && c->yBegin == 0 && c->yEnd == c->n;
	u32 lo[3], hi[3];
	WalkParams P;
	if (const char* bad = walk_check(c->n, whole, (const WalkQuery*)query, goals, goal_count, counts, d_field, lo, hi, &P)) return fail(c, VX_ERR_INVALID, what + bad);

	WalkState* s = module_state<WalkState>(c, MOD_WALK);
	const IslRegion r = isl_region(c->n, lo, hi);
	const u32 tiles = isl_tiles(r);
	const size_t V = (size_t)r.ext[0] * r.ext[1] * r.ext[2];
	auto noMemory = [&]() { return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error()); };
	if (!s->small && !(s->small = c->be.alloc(WALK_SMALL_BYTES))) return noMemory();
	if (!d_field && !dev_grow(c, s->volume, s->volumeCap, V * 4)) return noMemory();
	const size_t atStand = 0, atCount = (size_t)tiles * 512, atFlags = atCount + (size_t)tiles * 4;
	if (!dev_grow(c, s->perTile, s->perTileCap, atFlags + (size_t)tiles * 8)) return noMemory();
	if (goal_count && !dev_grow(c, s->goals, s->goalsCap, (size_t)goal_count * sizeof(WalkGoal))) return noMemory();

	u32* F = d_field ? d_field : (u32*)s->volume;
	u16* stand = (u16*)((char*)s->perTile + atStand);
	u32* tileStand = (u32*)((char*)s->perTile + atCount);
	u32* flag[2] = { (u32*)((char*)s->perTile + atFlags), (u32*)((char*)s->perTile + atFlags) + tiles };
	WalkCounts* dCounts = (WalkCounts*)s->small;
	u32* dCounters = (u32*)((char*)s->small + WALK_AT_COUNTERS);
	hipStream_t st = c->be.stream;
	auto deviceFailed = [&]() { return fail(c, VX_ERR_DEVICE, what + "device query failed: " + c->be.error()); };

	bool ok = c->be.fill(s->small, 0, WALK_SMALL_BYTES) && c->be.fill(flag[0], 0, (size_t)tiles * 8);
	if (ok && goal_count) ok = c->be.h2d(s->goals, goals, (size_t)goal_count * sizeof(WalkGoal));
	if (!ok) return deviceFailed();
	hipLaunchKernelGGL(k_walk_stand, dim3(tiles), dim3(WG), 0, st, resident_view(c), r, P, stand, tileStand, F, dCounts);
	if (goal_count) hipLaunchKernelGGL(k_walk_seed, dim3((goal_count + WG - 1) / WG), dim3(WG), 0, st, r, P, (const u16*)stand, (const u32*)tileStand, (const WalkGoal*)s->goals, goal_count, F, flag[0], dCounts);
	ok = c->be.check(hipGetLastError(), "k_walk launch");
	WalkCounts hc;
	memset(&hc, 0, sizeof(hc));
	ok = ok && c->be.d2h(&hc, dCounts, sizeof(hc)); // (waits: the number of standable cells caps the sweep loop)
	if (!ok) return deviceFailed();

	// The sweep loop.  A sweep that lowers no cell flags nobody, and after sweep k every cell whose cheapest walk has at most
	// k moves holds its final value: standable + 2 sweeps are more than correct code can need.
	const unsigned long long cap = hc.standable + 2;
	unsigned long long sweeps = 0;
	bool live = hc.goals_used != 0;
	while (live) {
		if (sweeps >= cap) return fail(c, VX_ERR_DEVICE, what + "walk field did not converge");
		const u32 batch = (u32)std::min<unsigned long long>(WALK_SWEEP_BATCH, cap - sweeps);
		u32 flagged[WALK_SWEEP_BATCH];
		ok = c->be.fill(dCounters, 0, sizeof(flagged));
		for (u32 k = 0; k < batch; ++k, ++sweeps)
			hipLaunchKernelGGL(k_walk_relax, dim3(tiles), dim3(WG), 0, st, r, P, (const u16*)stand, (const u32*)tileStand, F, flag[sweeps & 1], flag[(sweeps + 1) & 1], dCounters + k);
		ok = ok && c->be.check(hipGetLastError(), "k_walk_relax launch");
		ok = ok && c->be.d2h(flagged, dCounters, sizeof(flagged));
		if (!ok) return deviceFailed();
		live = flagged[batch - 1] != 0;
	}
	hipLaunchKernelGGL(k_walk_finish, dim3(tiles), dim3(WG), 0, st, r, P, (const u16*)stand, (const u32*)tileStand, (const u32*)F, d_dirs, dCounts);
	ok = c->be.check(hipGetLastError(), "k_walk_finish launch");
	ok = ok && c->be.d2h(&hc, dCounts, sizeof(hc));
	if (!ok) return deviceFailed();
	hc.sweeps = (u32)std::min<unsigned long long>(sweeps, 0xFFFFFFFFull);
	memcpy(counts, &hc, sizeof(hc));
	return VX_OK;
}

} // extern "C"
