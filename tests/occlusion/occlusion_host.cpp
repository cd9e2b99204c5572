// occlusion_host.cpp — host side of the tests of vx_occlusion (tests only; built by voxels_amd/build.py
// build_measure_host() into the measurements' host library, whose rows and sign summaries the staging shares).
//
// voxels_amd/csrc/tv_occlusion.h compiled for the host behind one C interface, with two paths through a bake:
//   path 0   a plain loop: vertex after vertex, every sample read from the dense grid
//   path 1   the pipeline of vx_occlusion.inl for one block - the row masks of its neighbourhood first (the lanes as a loop over
//            rows), then the vertices with their probes, a sample inside the staged region as a bit test, one outside read from
//            the grid.  `reach` is the region's reach (the kernel's is steps + 2; a smaller one forces the reads from the grid);
//            `skip` = 1 lets the per-block sign summaries (formed here from the grid, by the rule of the mirrors: 1 = no sample
//            < 0, 2 = every sample < 0) stand in for distance rows at level 0, as the kernel does.  *outside receives the
//            samples that were read from the grid.
//   oh_quantise, oh_dir   the quantisation and the direction table alone
//   oh_check    the entry checks            oh_layout / oh_limit   the header's structs and constants as this compiler sees them
// A grid is dist (n^3 bytes, x fastest, Z up); vertices are vx_vertex records.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_occlusion.h"

using namespace tv;

namespace {

static_assert(sizeof(OcclParams) == sizeof(vx_occlusion_params) && sizeof(OcclCounts) == sizeof(vx_occlusion_counts) && sizeof(vx_vertex) == 48, "tv_occlusion.h records");

u32 block_summary(u32 n, const u8* dist, u32 id)
{
	bool neg = false, pos = false;
	for (u32 row = 0; row < 256; ++row) {
		const i8* p = (const i8*)dist + rec_grid_row(n, id, row);
		for (u32 x = 0; x < 16; ++x) { if (p[x] < 0) neg = true; else pos = true; }
	}
	return neg && pos ? 0u : neg ? 2u : 1u;
}

// what the device does with atomics
void merge(OcclSlot& s, const u32 v[9])
{
	s.notDarkest = s.notDarkest > v[0] ? s.notDarkest : v[0];
	s.vertices += v[6]; s.sum += v[7]; s.open += v[8];
}

} // namespace

extern "C" {

int oh_check(uint32_t whole_grid, uint32_t have_surface, uint32_t levels_run, uint32_t level, const vx_occlusion_params* p, uint32_t has_array,
             uint64_t capacity, uint64_t n_verts)
{
	static const char some = 0;
	return occl_check(whole_grid != 0, have_surface != 0, levels_run, level, (const OcclParams*)p, has_array ? &some : nullptr, capacity, n_verts) ? VX_ERR_INVALID : VX_OK;
}

// one block's bake: `count` vertices -> out[count]; b = the block's coordinate at the level (path 1)
int oh_bake(uint32_t path, uint32_t n, const uint8_t* dist, uint32_t level, uint32_t steps, const vx_vertex* verts, uint32_t count, const uint32_t b[3],
            uint32_t reach, uint32_t skip, uint8_t* out, vx_occlusion_counts* counts, uint64_t* outside)
{
	if (steps < 1u || steps > OCCL_MAX_STEPS || (path && reach > OCCL_MAX_STEPS + 2u)) return VX_ERR_INVALID;
	const u32 lim = occl_limit(n, level);
	OcclSlot slot;
	memset(&slot, 0, sizeof(slot));
	u32 v[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	u64 reads = 0;
	std::vector<u64> masks;
	std::vector<u16> sign;
	OcclRegion R = occl_region(0, 0, 0, 0);
	if (path) {
		if (skip && level == 0u) {
			const u32 nb = n >> 4;
			sign.resize((size_t)nb * nb * nb);
			for (u32 id = 0; id < nb * nb * nb; ++id) sign[id] = (u16)block_summary(n, dist, id);
		}
		R = occl_region(b[0], b[1], b[2], reach);
		masks.resize((size_t)R.edge * R.edge);
		for (u32 row = 0; row < R.edge * R.edge; ++row) masks[row] = occl_row_mask(dist, n, level, sign.empty() ? nullptr : sign.data(), R, row);   // a lane as a row
	}
	for (u32 i = 0; i < count; ++i) {                                  // a lane as a vertex
		float pos[3], nrm[3];
		occl_vertex_read(verts + i, pos, nrm);
		OcclVertex q;
		u32 byte = 255u;
		if (occl_quantise(pos, nrm, level, q)) {
			if (!path) byte = occl_byte(q, steps, lim, [&](int cx, int cy, int cz) { return occl_grid_solid(dist, n, level, cx, cy, cz); });
			else byte = occl_byte(q, steps, lim, [&](int cx, int cy, int cz) {
				u32 row, bit;
				if (occl_region_holds(R, cx, cy, cz, row, bit)) return ((masks[row] >> bit) & 1ull) != 0ull;
				++reads;
				return occl_grid_solid(dist, n, level, cx, cy, cz);
			});
			occl_vertex_counts(byte, v);
		}
		out[i] = (u8)byte;
	}
	merge(slot, v);
	slot.visited = 1;
	if (counts) {
		const OcclCounts r = occl_finish(slot, 1u);
		memcpy(counts, &r, sizeof(r));
	}
	if (outside) *outside = reads;
	return VX_OK;
}

// -> 1 = baked, with P and N in out[6]; 0 = not baked
uint32_t oh_quantise(const float pos[3], const float nrm[3], uint32_t level, int32_t out[6])
{
	OcclVertex v;
	memset(&v, 0, sizeof(v));
	const bool ok = occl_quantise(pos, nrm, level, v);
	const int32_t r[6] = { v.px, v.py, v.pz, v.nx, v.ny, v.nz };
	memcpy(out, r, sizeof(r));
	return ok ? 1u : 0u;
}

void oh_dir(uint32_t k, int32_t out[3])
{
	int x, y, z;
	occl_dir(k, x, y, z);
	out[0] = x; out[1] = y; out[2] = z;
}

// which: 0 = sizes of vx_occlusion_params, vx_occlusion_counts, vx_vertex; 1 = offsets inside vx_occlusion_params; 2 = inside
// vx_occlusion_counts; 3 = pos, nrm inside vx_vertex
uint32_t oh_layout(uint32_t which, uint32_t* out)
{
	if (which == 0) { const uint32_t v[] = { sizeof(vx_occlusion_params), sizeof(vx_occlusion_counts), sizeof(vx_vertex) }; memcpy(out, v, sizeof(v)); return 3; }
	if (which == 1) {
		const uint32_t v[] = { offsetof(vx_occlusion_params, steps), offsetof(vx_occlusion_params, flags), offsetof(vx_occlusion_params, box_min),
		                       offsetof(vx_occlusion_params, box_max), offsetof(vx_occlusion_params, reserved) };
		memcpy(out, v, sizeof(v)); return 5;
	}
	if (which == 2) {
		const uint32_t v[] = { offsetof(vx_occlusion_counts, vertices), offsetof(vx_occlusion_counts, sum), offsetof(vx_occlusion_counts, entries),
		                       offsetof(vx_occlusion_counts, visited_entries), offsetof(vx_occlusion_counts, darkest), offsetof(vx_occlusion_counts, open) };
		memcpy(out, v, sizeof(v)); return 6;
	}
	const uint32_t v[] = { offsetof(vx_vertex, pos), offsetof(vx_vertex, nrm) };
	memcpy(out, v, sizeof(v)); return 2;
}

// 0 = VX_OCCLUSION_MAX_STEPS, 1 = VX_OCCLUSION_TRANSITIONS, 2 = the directions, 3 = the largest staged edge
uint32_t oh_limit(uint32_t which)
{
	const uint32_t v[] = { VX_OCCLUSION_MAX_STEPS, VX_OCCLUSION_TRANSITIONS, OCCL_DIRS, OCCL_MAX_EDGE };
	return which < 4 ? v[which] : 0;
}

} // extern "C"
