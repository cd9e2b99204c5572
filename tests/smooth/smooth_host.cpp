// smooth_host.cpp — host side of the tests of vx_grid_smooth (tests only; built by voxels_amd/build.py build_smooth_host()).
//
// voxels_amd/csrc/tv_smooth.h compiled for the host (-ffp-contract=off: the float32 operations of the kernels) behind one C
// interface:
//   sh_plain    a sequential loop over the dense array: smooth_kernel_sum over an edge-clamped accessor, smooth_weight,
//               smooth_value, a copy of the grid per iteration
//   sh_tiles    the tile pipeline of vx_smooth.inl - stage, eval, commit, results - with the lanes of a workgroup as loops and the
//               launches in their order: tile clipping, halo staging and the clamps, testable where there is no GPU
//   sh_weight   smooth_weight over arrays
// Both edits: dist (n^3 int8, x fastest, Z up) is rewritten in place; results has room for count records; the return value is
// what vx_grid_smooth returns (validation included, everything but the context).
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_smooth.h"

namespace {

bool valid(uint32_t n, const vx_smooth* ops, uint32_t count)
{
	if (count && !ops) return false;
	if (count > VX_SMOOTH_MAX_COUNT) return false;
	for (uint32_t i = 0; i < count; ++i) {
		const vx_smooth& o = ops[i];
		for (int k = 0; k < 3; ++k) if (!(o.lo[k] < o.hi[k] && o.hi[k] <= n)) return false;
		for (int k = 0; k < 3; ++k) if (!std::isfinite(o.center[k])) return false;
		if (!std::isfinite(o.radius) || !std::isfinite(o.strength) || o.radius < 0.f || o.strength < 0.f || o.strength > 1.f) return false;
		if (o.iterations > VX_SMOOTH_MAX_ITERATIONS) return false;
	}
	return true;
}

void hand_back(uint32_t n, const std::vector<tv::SmoothSlot>& slots, vx_smooth_result* results, float umin[3], float umax[3], uint64_t* changed)
{
	tv::SmoothSlot all;
	memset(&all, 0, sizeof(all));
	for (size_t i = 0; i < slots.size(); ++i) {
		const tv::SmoothResult r = tv::smooth_result(n, slots[i]);
		if (results) memcpy(&results[i], &r, sizeof(r));
		if (!slots[i].changed) continue;
		for (int k = 0; k < 3; ++k) { all.notMin[k] = std::max(all.notMin[k], slots[i].notMin[k]); all.max[k] = std::max(all.max[k], slots[i].max[k]); }
		all.changed += slots[i].changed;
	}
	const tv::SmoothResult u = tv::smooth_result(n, all);
	for (int k = 0; k < 3; ++k) { if (umin) umin[k] = u.out_min[k]; if (umax) umax[k] = u.out_max[k]; }
	if (changed) *changed = u.changed;
}

} // namespace

extern "C" {

int sh_plain(uint32_t n, int8_t* dist, const vx_smooth* ops, uint32_t count, vx_smooth_result* results, float umin[3], float umax[3], uint64_t* changed)
{
	using namespace tv;
	if (!valid(n, ops, count)) return VX_ERR_INVALID;
	std::vector<SmoothSlot> slots(count);
	if (count) memset(slots.data(), 0, count * sizeof(SmoothSlot));
	const size_t V = (size_t)n * n * n;
	for (uint32_t i = 0; i < count; ++i) {
		const vx_smooth& o = ops[i];
		if (!o.iterations || o.strength == 0.f) continue;
		const std::vector<int8_t> first(dist, dist + V);
		for (uint32_t it = 0; it < o.iterations; ++it) {
			const std::vector<int8_t> before(dist, dist + V);
			for (uint32_t z = o.lo[2]; z < o.hi[2]; ++z)
			for (uint32_t y = o.lo[1]; y < o.hi[1]; ++y)
			for (uint32_t x = o.lo[0]; x < o.hi[0]; ++x) {
				auto at = [&](int dx, int dy, int dz) {
					const int64_t cx = std::min<int64_t>(std::max<int64_t>((int64_t)x + dx, 0), n - 1), cy = std::min<int64_t>(std::max<int64_t>((int64_t)y + dy, 0), n - 1);
					const int64_t cz = std::min<int64_t>(std::max<int64_t>((int64_t)z + dz, 0), n - 1);
					return before[((size_t)cz * n + cy) * n + cx];
				};
				const int S = smooth_kernel_sum(at);
				dist[((size_t)z * n + y) * n + x] = smooth_value(at(0, 0, 0), S, smooth_weight(x, y, z, o.center, o.radius, o.strength));
			}
		}
		SmoothSlot& s = slots[i];
		for (uint32_t z = o.lo[2]; z < o.hi[2]; ++z)
		for (uint32_t y = o.lo[1]; y < o.hi[1]; ++y)
		for (uint32_t x = o.lo[0]; x < o.hi[0]; ++x) {
			if (dist[((size_t)z * n + y) * n + x] == first[((size_t)z * n + y) * n + x]) continue;
			const uint32_t p[3] = { x, y, z };
			for (int k = 0; k < 3; ++k) { s.notMin[k] = std::max(s.notMin[k], ~p[k]); s.max[k] = std::max(s.max[k], p[k]); }
			++s.changed;
		}
	}
	hand_back(n, slots, results, umin, umax, changed);
	return VX_OK;
}

int sh_tiles(uint32_t n, int8_t* dist, const vx_smooth* ops, uint32_t count, vx_smooth_result* results, float umin[3], float umax[3], uint64_t* changed)
{
	using namespace tv;
	if (!valid(n, ops, count)) return VX_ERR_INVALID;
	std::vector<SmoothSlot> slots(count);
	if (count) memset(slots.data(), 0, count * sizeof(SmoothSlot));
	// (uint64 elements: the 16-byte rows of the byte volumes are aligned)
	std::vector<uint64_t> volume, original;
	std::vector<u32> staged(SMOOTH_STAGE_WORDS);
	for (uint32_t i = 0; i < count; ++i) {
		const vx_smooth& o = ops[i];
		if (!o.iterations || o.strength == 0.f) continue;
		const SmoothRegion r = smooth_region(n, o.lo, o.hi);
		const u32 tiles = smooth_tiles(r);
		volume.assign((size_t)tiles * 512 + 2, 0);
		original.assign((size_t)tiles * 512 + 2, 0);
		i8* vol = (i8*)(((uintptr_t)volume.data() + 15) & ~(uintptr_t)15);
		i8* org = (i8*)(((uintptr_t)original.data() + 15) & ~(uintptr_t)15);
		for (uint32_t it = 0; it < o.iterations; ++it) {
			const u32 mode = o.iterations == 1 ? (u32)SMOOTH_COMPARE_GRID : it == 0 ? (u32)SMOOTH_SAVE_ORIGINAL : it + 1 == o.iterations ? (u32)SMOOTH_COMPARE_ORIGINAL : 0u;
			// k_smooth_eval
			for (u32 tile = 0; tile < tiles; ++tile) {
				const SmoothTile T = smooth_tile(r, tile);
				for (u32 row = 0; row < (u32)SMOOTH_STAGE_ROWS; ++row) smooth_stage_row(dist, n, T, row, staged.data());
				for (u32 t = 0; t < 256; ++t) {
					if (!smooth_row_inside(T, t & 15u, t >> 4)) continue;
					u32 out[4];
					smooth_eval_row(staged.data(), T, t, o.center, o.radius, o.strength, out);
					memcpy(vol + (size_t)tile * 4096 + t * 16, out, 16);
				}
			}
			// k_smooth_commit
			for (u32 tile = 0; tile < tiles; ++tile) {
				const SmoothTile T = smooth_tile(r, tile);
				for (u32 t = 0; t < 256; ++t) {
					const size_t at = (size_t)tile * 4096 + t * 16;
					smooth_slot_add(slots[i], T, t, smooth_commit_row(dist, n, T, t, vol + at, org + at, mode));
				}
			}
		}
	}
	hand_back(n, slots, results, umin, umax, changed);
	return VX_OK;
}

void sh_weight(uint32_t count, const uint32_t* v /* 3 per sample */, const float* center /* 3 per sample */, const float* radius, const float* strength, float* out)
{
	for (uint32_t i = 0; i < count; ++i) out[i] = tv::smooth_weight(v[3 * i], v[3 * i + 1], v[3 * i + 2], center + 3 * i, radius[i], strength[i]);
}

int8_t sh_value(int d, int S, float w) { return tv::smooth_value(d, S, w); }

uint32_t sh_sizes(uint32_t which) { return which == 0 ? (uint32_t)sizeof(vx_smooth) : (uint32_t)sizeof(vx_smooth_result); }

} // extern "C"
