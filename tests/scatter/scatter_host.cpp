// Host side of the tests of vx_scatter (include/voxels_hip.h, "scattering"): the arithmetic of voxels_amd/csrc/tv_scatter.h in a
// plain loop over a level's block table and meshes, the algorithm of the kernels without their lanes - tests only
// (tests/test_scatter.py, tests/test_abi_scatter.py).  Built with -ffp-contract=off: the same float32 operations as the device.
#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_scatter.h"

using namespace tv;

static_assert(sizeof(ScatterRules) == sizeof(vx_scatter_params), "ScatterRules mirrors vx_scatter_params");

extern "C" {

uint32_t sc_sizes(uint32_t k)
{
	const uint32_t s[6] = { sizeof(vx_scatter_params), sizeof(vx_scatter_point), sizeof(vx_scatter_range), sizeof(vx_scatter_counts),
	                        sizeof(vx_vertex), sizeof(vx_listed_block) };
	return k < 6 ? s[k] : 0;
}

// vx_scatter on host arrays: `verts` and `idx` are the pools the table's offsets point into.  Returns 0, or -3 when
// points > capacity (everything the header promises is written first).
int sc_scatter(uint32_t level, const vx_scatter_params* prm, const vx_listed_block* table, uint32_t nEntries, const vx_vertex* verts,
               const uint32_t* idx, uint32_t capacity, vx_scatter_point* points, vx_scatter_range* ranges, vx_scatter_counts* counts)
{
	ScatterRules r;
	memcpy(&r, prm, sizeof(r));
	vx_scatter_counts c;
	memset(&c, 0, sizeof(c));
	c.entries = nEntries;
	// first pass: counts only (is the total within 32 bits?); second pass: ranges and points
	for (int pass = 0; pass < 2; ++pass) {
		if (pass == 1 && c.points > 0xFFFFFFFFull) break;
		uint64_t at = 0;
		for (uint32_t e = 0; e < nEntries; ++e) {
			const vx_listed_block& b = table[e];
			uint64_t kept = 0;
			if (scatter_box_meets(r, b.min_corner, b.max_corner)) {
				if (pass == 0) ++c.visited_entries;
				const vx_vertex* v = verts + b.v_off;
				const uint32_t* ix = idx + b.i_off;
				const u32 hb = scatter_block_hash(r.seed, level, b.coord_id);
				for (u32 t = 0; t < b.i_count / 3u; ++t) {
					const ScatterVertex a = scatter_vertex(&v[ix[3 * t]], true, true), b1 = scatter_vertex(&v[ix[3 * t + 1]], true, true);
					const ScatterVertex c1 = scatter_vertex(&v[ix[3 * t + 2]], true, true);
					if (!scatter_mask_passes(r, a.tex0, a.tex1)) continue;
					const u32 ht = scatter_tri_hash(hb, t), n = scatter_count(a.p, b1.p, c1.p, r.density, ht);
					if (pass == 0) { ++c.triangles; c.candidates += n; }
					for (u32 k = 0; k < n; ++k) {
						const ScatterSample s = scatter_sample(a, b1, c1, ht, k);
						if (!scatter_keeps(r, s)) continue;
						if (pass == 1 && at + kept < capacity) {
							vx_scatter_point& o = points[at + kept];
							o.pos[0] = s.pos.x; o.pos[1] = s.pos.y; o.pos[2] = s.pos.z; o.rand = s.rand;
							o.nrm[0] = s.nrm.x; o.nrm[1] = s.nrm.y; o.nrm[2] = s.nrm.z; o.entry = e;
							o.block_id = b.id; o.tri = t; o.tex[0] = a.tex0; o.tex[1] = a.tex1;
						}
						++kept;
					}
				}
			}
			if (pass == 0) c.points += kept;
			else if (ranges) { ranges[e].first = (uint32_t)at; ranges[e].count = (uint32_t)kept; }
			at += kept;
		}
	}
	*counts = c;
	return c.points > capacity ? -3 : 0;
}

} // extern "C"
