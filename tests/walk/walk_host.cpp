// walk_host.cpp — host side of the tests of vx_grid_walk_field (tests only; built by voxels_amd/build.py build_walk_host()).
//
// Two independent things behind one C interface:
//   wh_oracle   the definition of include/voxels_hip.h ("walk fields") written out plainly: standability by the definition,
//               Dijkstra with a binary heap from the used goals over the reversed moves, directions by the definition, counts.
//               It shares nothing with voxels_amd/csrc/tv_walk.h.
//   wh_emulate  the tile pipeline of tv_walk.h - stand, seed, the sweep loop of relax, finish - with the lanes of a workgroup
//               as loops and the phases in the order vx_walk.inl launches them: the algorithm of the device path, testable
//               where there is no GPU.
// Both: dist is n^3 int8, x fastest, Z up; field (V uint32) and dirs (V bytes) may be NULL; the return value is what
// vx_grid_walk_field returns.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_walk.h"

namespace {

struct Box { int lo[3], hi[3], ext[3]; size_t V; };

bool oracle_check(uint32_t n, const vx_walk_query* q, const vx_walk_goal* goals, uint32_t goalCount, const vx_walk_counts* counts, const uint32_t* field, Box* b)
{
	if (!q || !counts) return false;
	if (q->flags != 0) return false;
	if (q->clearance < 1 || q->clearance > 32 || q->step_up > 4 || q->step_down > 4) return false;
	if (q->cost_axial < 1 || q->cost_axial > 65535 || q->cost_diagonal > 65535 || q->cost_climb > 65535) return false;
	if (q->max_cost > (1u << 30)) return false;
	if (goalCount > VX_WALK_MAX_GOALS || (goalCount && !goals)) return false;
	if (field && ((uintptr_t)field % 16) != 0) return false;
	b->V = 1;
	for (int k = 0; k < 3; ++k) {
		const uint32_t lo = q->whole_grid ? 0 : q->lo[k], hi = q->whole_grid ? n : q->hi[k];
		if (!(lo < hi && hi <= n)) return false;
		b->lo[k] = (int)lo; b->hi[k] = (int)hi; b->ext[k] = (int)(hi - lo);
		b->V *= hi - lo;
	}
	return b->V <= ((size_t)1 << 28);
}

struct Oracle {
	int n;
	const int8_t* dist;
	const vx_walk_query* q;
	Box b;
	std::vector<uint8_t> stand;

	bool solid(int x, int y, int z) const { return z >= 0 && z < n && dist[((size_t)z * n + y) * n + x] < 0; }
	bool air(int x, int y, int z) const { return z >= n || (z >= 0 && dist[((size_t)z * n + y) * n + x] >= 0); }
	bool inside(int x, int y, int z) const { return x >= b.lo[0] && x < b.hi[0] && y >= b.lo[1] && y < b.hi[1] && z >= b.lo[2] && z < b.hi[2]; }
	size_t index(int x, int y, int z) const { return ((size_t)(z - b.lo[2]) * b.ext[1] + (y - b.lo[1])) * b.ext[0] + (x - b.lo[0]); }
	bool standable(int x, int y, int z) const { return inside(x, y, z) && stand[index(x, y, z)]; }
	bool by_definition(int x, int y, int z) const
	{
		if (z < 1 || !solid(x, y, z - 1)) return false;
		for (int k = 0; k < (int)q->clearance; ++k) if (!air(x, y, z + k)) return false;
		return true;
	}
	// does column (x, y) hold a standable in-region cell within the step range of height z
	bool column_has(int x, int y, int z) const
	{
		for (int dz = -(int)q->step_down; dz <= (int)q->step_up; ++dz) if (standable(x, y, z + dz)) return true;
		return false;
	}
	// the move (offset o, dz) out of (x, y, z): does it exist, and its weight
	bool move(int x, int y, int z, int o, int dz, uint32_t* w) const
	{
		static const int DX[8] = { 1, -1, 0, 0, 1, -1, 1, -1 }, DY[8] = { 0, 0, 1, -1, 1, 1, -1, -1 };
		if (!standable(x + DX[o], y + DY[o], z + dz)) return false;
		if (o >= 4) {
			if (q->cost_diagonal == 0) return false;
			if (!column_has(x + DX[o], y, z) || !column_has(x, y + DY[o], z)) return false;
		}
		*w = (o < 4 ? q->cost_axial : q->cost_diagonal) + (uint32_t)(dz < 0 ? -dz : dz) * q->cost_climb;
		return true;
	}
};

} // namespace

extern "C" {

int wh_oracle(uint32_t n, const int8_t* dist, const vx_walk_query* q, const vx_walk_goal* goals, uint32_t goalCount,
              uint32_t* field, uint8_t* dirs, vx_walk_counts* counts)
{
	static const int DX[8] = { 1, -1, 0, 0, 1, -1, 1, -1 }, DY[8] = { 0, 0, 1, -1, 1, 1, -1, -1 };
	if (counts) memset(counts, 0, sizeof(*counts));
	Oracle o;
	if (!oracle_check(n, q, goals, goalCount, counts, field, &o.b)) return VX_ERR_INVALID;
	o.n = (int)n; o.dist = dist; o.q = q;
	const Box& b = o.b;
	o.stand.assign(b.V, 0);
	for (int z = b.lo[2]; z < b.hi[2]; ++z) for (int y = b.lo[1]; y < b.hi[1]; ++y) for (int x = b.lo[0]; x < b.hi[0]; ++x)
		if (o.by_definition(x, y, z)) { o.stand[o.index(x, y, z)] = 1; ++counts->standable; }
	std::vector<uint32_t> F(b.V, VX_WALK_UNREACHED);
	typedef std::pair<uint32_t, uint32_t> Item; // (cost, region index)
	std::priority_queue<Item, std::vector<Item>, std::greater<Item> > heap;
	for (uint32_t k = 0; k < goalCount; ++k) {
		const vx_walk_goal& g = goals[k];
		const bool used = g.x < n && g.y < n && g.z < n && o.standable((int)g.x, (int)g.y, (int)g.z) && g.cost <= q->max_cost;
		if (!used) { ++counts->goals_ignored; continue; }
		++counts->goals_used;
		const size_t i = o.index((int)g.x, (int)g.y, (int)g.z);
		if (g.cost < F[i]) { F[i] = g.cost; heap.push(Item(g.cost, (uint32_t)i)); }
	}
	while (!heap.empty()) {
		const Item top = heap.top();
		heap.pop();
		if (top.first != F[top.second]) continue;
		const int x = b.lo[0] + (int)(top.second % b.ext[0]), y = b.lo[1] + (int)((top.second / b.ext[0]) % b.ext[1]), z = b.lo[2] + (int)(top.second / ((size_t)b.ext[0] * b.ext[1]));
		// every cell c with a move c -> (x, y, z)
		for (int k = 0; k < 8; ++k) for (int dz = -(int)q->step_down; dz <= (int)q->step_up; ++dz) {
			const int cx = x - DX[k], cy = y - DY[k], cz = z - dz;
			uint32_t w;
			if (!o.standable(cx, cy, cz) || !o.move(cx, cy, cz, k, dz, &w)) continue;
			const uint64_t cand = (uint64_t)top.first + w;
			const size_t i = o.index(cx, cy, cz);
			if (cand <= q->max_cost && cand < F[i]) { F[i] = (uint32_t)cand; heap.push(Item((uint32_t)cand, (uint32_t)i)); }
		}
	}
	for (int z = b.lo[2]; z < b.hi[2]; ++z) for (int y = b.lo[1]; y < b.hi[1]; ++y) for (int x = b.lo[0]; x < b.hi[0]; ++x) {
		const size_t i = o.index(x, y, z);
		uint8_t d = 0xFF;
		if (F[i] != VX_WALK_UNREACHED) {
			++counts->reached;
			counts->max_distance = std::max(counts->max_distance, F[i]);
			d = 0xFE;
			for (int dz = -(int)q->step_down; dz <= (int)q->step_up && d == 0xFE; ++dz) for (int k = 0; k < 8 && d == 0xFE; ++k) {
				uint32_t w;
				if (!o.move(x, y, z, k, dz, &w)) continue;
				const uint32_t f = F[o.index(x + DX[k], y + DY[k], z + dz)];
				if (f != VX_WALK_UNREACHED && (uint64_t)f + w == F[i]) d = (uint8_t)(k | ((dz + 4) << 3));
			}
		}
		if (dirs) dirs[i] = d;
	}
	if (field) memcpy(field, F.data(), b.V * 4);
	return VX_OK;
}

int wh_emulate(uint32_t n, const int8_t* dist, const vx_walk_query* q, const vx_walk_goal* goals, uint32_t goalCount,
               uint32_t* field, uint8_t* dirs, vx_walk_counts* counts)
{
	using namespace tv;
	typedef WalkOpsPlain O;
	if (counts) memset(counts, 0, sizeof(*counts));
	u32 lo[3], hi[3];
	WalkParams P;
	if (walk_check(n, true, (const WalkQuery*)q, goals, goalCount, counts, field, lo, hi, &P)) return VX_ERR_INVALID;
	const IslRegion r = isl_region(n, lo, hi);
	const u32 tiles = isl_tiles(r);
	std::vector<u32> own;
	if (!field) { own.resize((size_t)r.ext[0] * r.ext[1] * r.ext[2]); field = own.data(); }
	u32* F = field;
	std::vector<u16> stand((size_t)tiles * 256);
	std::vector<u32> tileStand(tiles), flagA(tiles, 0), flagB(tiles, 0);
	u32* flag[2] = { flagA.data(), flagB.data() };
	WalkCounts hc;
	memset(&hc, 0, sizeof(hc));

	// k_walk_stand
	for (u32 tile = 0; tile < tiles; ++tile) {
		const IslTile T = isl_tile(r, tile);
		u32 count = 0;
		for (u32 t = 0; t < 256; ++t) {
			const u32 mask = walk_stand_row(dist, n, T, t, P.clearance);
			stand[(size_t)tile * 256 + t] = (u16)mask;
			count += (u32)__builtin_popcount(mask);
			walk_field_init(r, T, t, 256, F);
		}
		tileStand[tile] = count;
		hc.standable += count;
	}
	// k_walk_seed
	for (u32 k = 0; k < goalCount; ++k) walk_seed<O>(r, P, stand.data(), tileStand.data(), *(const WalkGoal*)&goals[k], F, flag[0], &hc);
	// the sweep loop of k_walk_relax
	std::vector<u32> sF(WALK_CELLS), sCol(WALK_COLS);
	const unsigned long long cap = hc.standable + 2;
	unsigned long long sweeps = 0;
	bool live = hc.goals_used != 0;
	while (live) {
		if (sweeps >= cap) return VX_ERR_DEVICE;
		const u32 batch = (u32)std::min<unsigned long long>(WALK_SWEEP_BATCH, cap - sweeps);
		u32 flagged[WALK_SWEEP_BATCH] = { 0 };
		for (u32 k = 0; k < batch; ++k, ++sweeps) {
			u32* active = flag[sweeps & 1];
			u32* next = flag[(sweeps + 1) & 1];
			for (u32 tile = 0; tile < tiles; ++tile) {
				if (!active[tile]) continue;
				const IslTile T = isl_tile(r, tile);
				for (u32 t = 0; t < 256; ++t) walk_stage_clear(t, 256, sCol.data());
				for (u32 t = 0; t < 256; ++t) walk_stage<O>(r, T, P, t, 256, F, stand.data(), sF.data(), sCol.data());
				bool fell = true;
				for (u32 pass = 0; pass < (u32)WALK_TILE_PASSES && fell; ++pass) {
					fell = false;
					for (u32 t = 0; t < 256; ++t) fell = walk_relax_column<O>(P, t, sF.data(), sCol.data()) || fell;
				}
				u32 around = fell ? 1u << WALK_SELF : 0u;
				for (u32 t = 0; t < 256; ++t) around |= walk_store_column<O>(r, T, P, t, sF.data(), sCol.data(), F);
				for (u32 t = 0; t < 256; ++t) walk_flag_tile<O>(r, tile, t, around, tileStand.data(), next, &flagged[k]);
				active[tile] = 0;
			}
		}
		live = flagged[batch - 1] != 0;
	}
	// k_walk_finish
	for (u32 tile = 0; tile < tiles; ++tile) {
		const IslTile T = isl_tile(r, tile);
		if (!tileStand[tile]) {
			if (dirs) for (u32 t = 0; t < 256; ++t) walk_finish_dead(r, T, t, 256, dirs);
			continue;
		}
		for (u32 t = 0; t < 256; ++t) walk_stage_clear(t, 256, sCol.data());
		for (u32 t = 0; t < 256; ++t) walk_stage<O>(r, T, P, t, 256, F, stand.data(), sF.data(), sCol.data());
		u32 reached = 0, far = 0;
		for (u32 t = 0; t < 256; ++t) walk_finish_column<O>(r, T, P, t, sF.data(), sCol.data(), dirs, &reached, &far);
		hc.reached += reached;
		hc.max_distance = std::max(hc.max_distance, far);
	}
	hc.sweeps = (u32)std::min<unsigned long long>(sweeps, 0xFFFFFFFFull);
	memcpy(counts, &hc, sizeof(hc));
	return VX_OK;
}

// sizes of the three records as the C compiler lays out the header's structs
uint32_t wh_sizes(uint32_t which) { return which == 0 ? (uint32_t)sizeof(vx_walk_query) : which == 1 ? (uint32_t)sizeof(vx_walk_goal) : (uint32_t)sizeof(vx_walk_counts); }

// offsets of their fields, in declaration order; UINT32_MAX past the last
uint32_t wh_offset(uint32_t which, uint32_t field)
{
	static const size_t query[] = { offsetof(vx_walk_query, lo), offsetof(vx_walk_query, hi), offsetof(vx_walk_query, whole_grid), offsetof(vx_walk_query, clearance),
	                                offsetof(vx_walk_query, step_up), offsetof(vx_walk_query, step_down), offsetof(vx_walk_query, cost_axial), offsetof(vx_walk_query, cost_diagonal),
	                                offsetof(vx_walk_query, cost_climb), offsetof(vx_walk_query, max_cost), offsetof(vx_walk_query, flags), offsetof(vx_walk_query, reserved) };
	static const size_t goal[] = { offsetof(vx_walk_goal, x), offsetof(vx_walk_goal, y), offsetof(vx_walk_goal, z), offsetof(vx_walk_goal, cost) };
	static const size_t counts[] = { offsetof(vx_walk_counts, standable), offsetof(vx_walk_counts, reached), offsetof(vx_walk_counts, goals_used), offsetof(vx_walk_counts, goals_ignored),
	                                 offsetof(vx_walk_counts, max_distance), offsetof(vx_walk_counts, sweeps) };
	if (which == 0 && field < sizeof(query) / sizeof(query[0])) return (uint32_t)query[field];
	if (which == 1 && field < sizeof(goal) / sizeof(goal[0])) return (uint32_t)goal[field];
	if (which == 2 && field < sizeof(counts) / sizeof(counts[0])) return (uint32_t)counts[field];
	return UINT32_MAX;
}

} // extern "C"
