// island_host.cpp — host side of the tests of vx_grid_islands (tests only; built by voxels_amd/build.py build_island_host()).
//
// Two independent things behind one C interface:
//   ih_oracle   a plain breadth-first flood fill over the dense region.  It shares nothing with voxels_amd/csrc/tv_island.h:
//               labels, records, counts, the removal, the BF_Empty rule and the dirty box are all written out again here.
//   ih_emulate  the tile pipeline of tv_island.h - local, merge, flatten, roots, stats, mark, remove - with the lanes of a
//               workgroup as loops and the phases in the order vx_island.inl launches them: the algorithm of the device
//               path, testable where there is no GPU.
// Both: dist (n^3 int8, x fastest, Z up) and flags (BF_Empty per block) are rewritten in place by a removal; labels has room
// for the region's voxels; the return value is what vx_grid_islands returns.
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <unordered_set>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_island.h"

namespace {

bool resolve_box(uint32_t n, const vx_island_query* q, const vx_island_counts* counts, const vx_island* recs, uint32_t capacity, uint32_t lo[3], uint32_t hi[3])
{
	if (!q || !counts || (capacity && !recs)) return false;
	if ((q->flags & ~3u) || q->anchor_faces > 0x3Fu) return false;
	if ((q->flags & VX_ISLANDS_REMOVE) && (q->air_value < 1 || q->air_value > 127)) return false;
	uint64_t V = 1;
	for (int k = 0; k < 3; ++k) {
		lo[k] = q->whole_grid ? 0 : q->lo[k];
		hi[k] = q->whole_grid ? n : q->hi[k];
		if (!(lo[k] < hi[k] && hi[k] <= n)) return false;
		V *= hi[k] - lo[k];
	}
	return V <= (1ull << 30);
}

// BF_Empty as the grid file codec decides it: the block's 4096 samples in x, y, z order cut into stretches of one value, a
// stretch of length l being ceil(l / 255) runs; empty <=> no more than 2048 runs and every sample strictly of the first one's sign
uint8_t oracle_block_empty(const int8_t* dist, uint32_t n, uint32_t bx, uint32_t by, uint32_t bz)
{
	std::vector<int8_t> s;
	s.reserve(4096);
	for (uint32_t z = 0; z < 16; ++z) for (uint32_t y = 0; y < 16; ++y) for (uint32_t x = 0; x < 16; ++x)
		s.push_back(dist[((size_t)(bz * 16 + z) * n + by * 16 + y) * n + bx * 16 + x]);
	size_t runs = 0;
	for (size_t i = 0; i < s.size();) {
		size_t j = i;
		while (j < s.size() && s[j] == s[i]) ++j;
		runs += (j - i + 254) / 255;
		i = j;
	}
	for (int8_t v : s) if ((int)v * (int)s[0] <= 0) return 0;
	return runs <= 2048 ? 1 : 0;
}

} // namespace

extern "C" {

int ih_oracle(uint32_t n, int8_t* dist, uint8_t* flags, const vx_island_query* q, vx_island* recs, uint32_t capacity,
              vx_island_counts* counts, uint32_t* labels, float outMin[3], float outMax[3])
{
	for (int k = 0; k < 3; ++k) outMin[k] = outMax[k] = 0.f;
	uint32_t lo[3], hi[3];
	if (!resolve_box(n, q, counts, recs, capacity, lo, hi)) return VX_ERR_INVALID;
	memset(counts, 0, sizeof(*counts));
	const uint32_t ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
	const size_t V = (size_t)ex * ey * ez;
	auto sample = [&](uint32_t x, uint32_t y, uint32_t z) -> int8_t& { return dist[((size_t)(lo[2] + z) * n + lo[1] + y) * n + lo[0] + x]; };
	std::fill(labels, labels + V, UINT32_MAX);
	std::vector<vx_island> all;
	std::vector<uint32_t> queue;
	for (size_t start = 0; start < V; ++start) {
		const uint32_t sx = (uint32_t)(start % ex), sy = (uint32_t)((start / ex) % ey), sz = (uint32_t)(start / ((size_t)ex * ey));
		if (labels[start] != UINT32_MAX || sample(sx, sy, sz) >= 0) continue;
		vx_island e;
		memset(&e, 0, sizeof(e));
		e.label = (uint32_t)start;
		for (int k = 0; k < 3; ++k) { e.min[k] = UINT32_MAX; e.max[k] = 0; }
		queue.clear();
		queue.push_back((uint32_t)start);
		labels[start] = (uint32_t)start;
		for (size_t head = 0; head < queue.size(); ++head) {
			const uint32_t i = queue[head];
			const uint32_t p[3] = { i % ex, (i / ex) % ey, i / (ex * ey) };
			const uint32_t ext[3] = { ex, ey, ez };
			++e.voxels;
			for (int k = 0; k < 3; ++k) {
				e.min[k] = std::min(e.min[k], lo[k] + p[k]);
				e.max[k] = std::max(e.max[k], lo[k] + p[k]);
				if (p[k] == 0) e.faces |= 1u << (2 * k);
				if (p[k] == ext[k] - 1) e.faces |= 2u << (2 * k);
				for (int d = -1; d <= 1; d += 2) {
					if ((d < 0 && p[k] == 0) || (d > 0 && p[k] == ext[k] - 1)) continue;
					uint32_t nbr[3] = { p[0], p[1], p[2] };
					nbr[k] += d;
					const uint32_t j = (nbr[2] * ey + nbr[1]) * ex + nbr[0];
					if (labels[j] == UINT32_MAX && sample(nbr[0], nbr[1], nbr[2]) < 0) { labels[j] = (uint32_t)start; queue.push_back(j); }
				}
			}
		}
		all.push_back(e);
	}
	std::unordered_set<uint32_t> gone;
	std::vector<vx_island> listed;
	uint32_t rmin[3] = { UINT32_MAX, UINT32_MAX, UINT32_MAX }, rmax[3] = { 0, 0, 0 };
	for (const vx_island& e : all) {
		++counts->components;
		counts->solid_voxels += e.voxels;
		const bool detached = (e.faces & q->anchor_faces) == 0;
		if (detached) {
			++counts->detached;
			counts->detached_voxels += e.voxels;
			if ((q->flags & VX_ISLANDS_REMOVE) && (q->max_voxels == 0 || e.voxels <= q->max_voxels)) {
				++counts->removed;
				counts->removed_voxels += e.voxels;
				gone.insert(e.label);
				for (int k = 0; k < 3; ++k) { rmin[k] = std::min(rmin[k], e.min[k]); rmax[k] = std::max(rmax[k], e.max[k]); }
			}
		}
		if (detached || !(q->flags & VX_ISLANDS_DETACHED_ONLY)) listed.push_back(e);
	}
	counts->listed = (uint32_t)listed.size();
	for (size_t i = 0; i < listed.size() && i < capacity; ++i) recs[i] = listed[i];
	if (!gone.empty()) {
		const uint32_t nb = n / 16;
		std::vector<uint8_t> hit((size_t)nb * nb * nb, 0);
		for (size_t i = 0; i < V; ++i) {
			if (labels[i] == UINT32_MAX || !gone.count(labels[i])) continue;
			const uint32_t x = (uint32_t)(i % ex), y = (uint32_t)((i / ex) % ey), z = (uint32_t)(i / ((size_t)ex * ey));
			sample(x, y, z) = (int8_t)q->air_value;
			hit[(((lo[2] + z) / 16) * nb + (lo[1] + y) / 16) * nb + (lo[0] + x) / 16] = 1;
		}
		for (uint32_t b = 0; b < nb * nb * nb; ++b) if (hit[b]) { ++counts->touched_blocks; flags[b] = oracle_block_empty(dist, n, b % nb, (b / nb) % nb, b / (nb * nb)); }
		// output order: x, then the internal z, then the internal y
		const int order[3] = { 0, 2, 1 };
		for (int k = 0; k < 3; ++k) { outMin[k] = (float)std::min(rmin[order[k]], n); outMax[k] = (float)std::min(rmax[order[k]] + 1, n); }
	}
	return counts->listed > capacity ? VX_ERR_OVERFLOW : VX_OK;
}

int ih_emulate(uint32_t n, int8_t* dist, uint8_t* flags, const vx_island_query* q, vx_island* recs, uint32_t capacity,
               vx_island_counts* counts, uint32_t* labels, float outMin[3], float outMax[3])
{
	using namespace tv;
	typedef IslOpsPlain O;
	for (int k = 0; k < 3; ++k) outMin[k] = outMax[k] = 0.f;
	uint32_t lo[3], hi[3];
	if (!resolve_box(n, q, counts, recs, capacity, lo, hi)) return VX_ERR_INVALID;
	memset(counts, 0, sizeof(*counts));
	const IslRegion r = isl_region(n, lo, hi);
	const u32 tiles = isl_tiles(r), rows = isl_rows(r);
	u32* L = labels;

	// k_isl_local
	std::vector<u32> parent(4096), masks(256);
	for (u32 tile = 0; tile < tiles; ++tile) {
		const IslTile T = isl_tile(r, tile);
		if (flags[T.block]) {
			const u32 label = dist[((size_t)T.org[2] * n + T.org[1]) * n + T.org[0]] < 0 ? isl_tile_first(r, T) : (u32)ISL_AIR;
			for (u32 li = 0; li < 4096; ++li) {
				const u32 x = T.org[0] + (li & 15u);
				if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8)) L[isl_local_to_region(r, T, li)] = label;
			}
			continue;
		}
		for (u32 t = 0; t < 256; ++t) {
			u32 mask = 0;
			if (isl_row_inside(T, t & 15u, t >> 4)) mask = isl_solid_bits(dist + ((size_t)(T.org[2] + (t >> 4)) * n + T.org[1] + (t & 15u)) * n + T.org[0]) & isl_clip_bits(T);
			masks[t] = mask;
			isl_local_init(t, mask, parent.data());
		}
		for (u32 t = 0; t < 256; ++t) isl_local_link<O>(t, masks.data(), parent.data());
		for (u32 t = 0; t < 256; ++t) isl_local_flatten<O>(t, masks[t], parent.data());
		for (u32 li = 0; li < 4096; ++li) {
			const u32 x = T.org[0] + (li & 15u);
			if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8))
				L[isl_local_to_region(r, T, li)] = parent[li] == (u32)ISL_AIR ? (u32)ISL_AIR : isl_local_to_region(r, T, parent[li]);
		}
	}
	// k_isl_merge
	for (u32 tile = 0; tile < tiles; ++tile) { const IslTile T = isl_tile(r, tile); for (u32 t = 0; t < 256; ++t) isl_merge_lane<O>(r, T, t, L); }
	// k_isl_flatten, k_isl_scan
	std::vector<u32> rowOff(rows + 1, 0);
	for (u32 row = 0; row < rows; ++row) for (u32 x = 0; x < r.ext[0]; ++x) rowOff[row] += isl_flatten_voxel<O>(L, row * r.ext[0] + x) ? 1u : 0u;
	u32 comps = 0;
	for (u32 row = 0; row < rows; ++row) { const u32 c = rowOff[row]; rowOff[row] = comps; comps += c; }
	// k_isl_roots
	std::vector<u32> roots(comps);
	std::vector<IslRecord> rec(comps);
	for (u32 row = 0; row < rows; ++row) {
		u32 at = rowOff[row];
		for (u32 x = 0; x < r.ext[0]; ++x) { const u32 i = row * r.ext[0] + x; if (L[i] == i) { roots[at] = i; rec[at] = isl_empty_record(i); ++at; } }
	}
	IslCounts hc;
	memset(&hc, 0, sizeof(hc));
	u32 dirty[6] = { 0, 0, 0, 0, 0, 0 };
	std::vector<IslRecord> out;
	if (comps) {
		// k_isl_stats
		std::vector<u32> key(ISL_HASH_SLOTS), cnt(ISL_HASH_SLOTS), xy(ISL_HASH_SLOTS), zf(ISL_HASH_SLOTS);
		for (u32 tile = 0; tile < tiles; ++tile) {
			const IslTile T = isl_tile(r, tile);
			if (flags[T.block]) {
				const u32 label = L[isl_tile_first(r, T)];
				if (label != (u32)ISL_AIR) isl_stats_uniform<O>(r, T, label, roots.data(), comps, rec.data());
				continue;
			}
			for (u32 s = 0; s < (u32)ISL_HASH_SLOTS; ++s) { key[s] = (u32)ISL_AIR; cnt[s] = xy[s] = zf[s] = 0; }
			for (u32 t = 0; t < 256; ++t) isl_stats_row<O>(r, T, t, L, key.data(), cnt.data(), xy.data(), zf.data());
			for (u32 s = 0; s < (u32)ISL_HASH_SLOTS; ++s) isl_stats_flush<O>(T, s, key.data(), cnt.data(), xy.data(), zf.data(), roots.data(), comps, rec.data());
		}
		// k_isl_mark, k_isl_scan, k_isl_compact
		std::vector<u8> marks(comps);
		for (u32 k = 0; k < comps; ++k) marks[k] = (u8)isl_mark<O>(rec[k], q->flags, q->anchor_faces, q->max_voxels, &hc, dirty);
		for (u32 k = 0; k < comps; ++k) if (marks[k] & ISL_MARK_LISTED) out.push_back(rec[k]);
		// k_isl_remove, then the flags of the blocks it collected
		if ((q->flags & VX_ISLANDS_REMOVE) && hc.removed) {
			std::vector<u32> touched;
			for (u32 tile = 0; tile < tiles; ++tile) {
				const IslTile T = isl_tile(r, tile);
				if (!isl_tile_in_dirty(T, dirty)) continue;
				bool any = false;
				for (u32 t = 0; t < 256; ++t) {
					i8* row = dist + ((size_t)(T.org[2] + (t >> 4)) * n + T.org[1] + (t & 15u)) * n + T.org[0];
					any = isl_remove_row(r, T, t, L, roots.data(), comps, marks.data(), (i8)q->air_value, row) || any;
				}
				if (any) touched.push_back(T.block);
			}
			hc.touched_blocks = (u32)touched.size();
			for (u32 b : touched) flags[b] = isl_block_empty(dist, n, b);
		}
	}
	memcpy(counts, &hc, sizeof(hc));
	for (size_t i = 0; i < out.size() && i < capacity; ++i) memcpy(&recs[i], &out[i], sizeof(vx_island));
	isl_dirty_box(n, hc.removed, dirty, outMin, outMax);
	return hc.listed > capacity ? VX_ERR_OVERFLOW : VX_OK;
}

uint32_t ih_sizes(uint32_t which) { return which == 0 ? (uint32_t)sizeof(vx_island_query) : which == 1 ? (uint32_t)sizeof(vx_island) : (uint32_t)sizeof(vx_island_counts); }

} // extern "C"
