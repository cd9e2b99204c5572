// geomkeep_host.cpp — host side of tests/test_geometry_keep_host.py (tests only; built by voxels_amd/build.py
// build_measure_host() into the measurements' host library).
//
// The CPU emulation of tests/emu (the product's host orchestration over sequential phases; a complete C ABI, vx_*) with one
// addition behind the regular pass of every full run: every table-driven regular block of every level is walked once more with
// the serial forms (f0_block_serial, f1_block_serial) into pools of its own, and for every vertex the texture-only form
// (f0_vertex_tex, f1_vertex_tex: voxels_amd/csrc/tv_fast0.h, tv_fast1.h) is run on the block's state and its 8 bytes are compared
// with bytes 40..47 of the vertex the full form stored.  gkh_counts() = per level what the last attempt of a full run compared
// (a run that outgrows its pools is attempted again, and every attempt compares everything); gkh_reset() clears it:
//   [0] vertices compared   [1] of them different   [2] took the "both end voxels have the cell's material" branch of the rv.mat
//   rule   [3] took the other   [4] used a table row that is not valid   [5] blocks of the level that the serial forms declined
//   (a zero sample, a chain that ended on a voxel, more cells than the first capacity class: none of their vertices is compared)
//   [6] blocks walked   [7] texture-only forms of a level >= 1 that did not return "strictly inside its edge"
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../voxels_amd/csrc/tv_block.h"
#include "../../voxels_amd/csrc/tv_fast0.h"
#include "../../voxels_amd/csrc/tv_fast1.h"
#include "../../voxels_amd/csrc/vx_terrain_math.h"

#define VX_BACKEND_NAME "emu:cpu (tests only, texture-only vertex forms compared)"

namespace {
using namespace tv;

template <typename T>
u32 exclusive_scan(T* a, u32 n)
{
	u32 run = 0;
	for (u32 i = 0; i < n; ++i) { const u32 v = a[i]; a[i] = (T)run; run += v; }
	return run;
}
}

#define Backend EmuBackend
#include "../emu/emu_backend.inl"
#undef Backend

namespace {

enum { GK_FIGURES = 8 };
uint64_t g_counts[MAX_LEVELS][GK_FIGURES];

struct TexCapture {
	u32* out;
	void operator()(u32 t0, u32 t1) const { out[0] = t0; out[1] = t1; }
};

void tally(u32 level, const u32 got[2], const PolyVertex& full, bool sameBranch, unsigned long long row)
{
	uint64_t* n = g_counts[level];
	++n[0];
	if (memcmp(got, full.tex, 8) != 0) ++n[1];
	++n[sameBranch ? 2 : 3];
	if (((row >> 48) & 0xFFu) == 0) ++n[4];
}

// which branch of f1_vertex's rv.mat rule a vertex takes: the chain walk and the three material reads, restated
bool f1_same_branch(const Fast1State<640>& st, const F0Tables& T, const F1HostSampler& smp, const u16* blockCache, u32 desc, int level, int ox, int oy, int oz)
{
	const u32 c = desc & 0xFFFu;
	const F0Edge e = T.edge[desc >> 12];
	const int cx = (int)(c & 15u), cy = (int)((c >> 4) & 15u), cz = (int)(c >> 8), mult = 1 << level;
	const i8* s0 = st.samp + (cz * F1_SPLANE + cy * F1_SROW + cx) + (e.z & 0xFFFFu);
	int p0 = s0[0];
	const u32 v0 = (e.y >> 20) & 7u, axis = (e.y >> 23) & 3u;
	int q[3] = { ox + (cx + (int)(v0 & 1u)) * mult, oy + (cy + (int)((v0 >> 1) & 1u)) * mult, oz + (cz + (int)(v0 >> 2)) * mult };
	for (int len = mult; len > 1; len >>= 1) {
		int m[3] = { q[0], q[1], q[2] };
		m[axis] += len >> 1;
		const int midV = dist_at(*smp.g, m[0], m[1], m[2]);
		if (p0 * midV > 0) { q[axis] = m[axis]; p0 = midV; }
	}
	int q1[3] = { q[0], q[1], q[2] };
	q1[axis] += 1;
	const u32 M0 = mat_at(*smp.g, q[0], q[1], q[2]) & 0xFFu, M1 = mat_at(*smp.g, q1[0], q1[1], q1[2]) & 0xFFu;
	return M0 == M1 && M0 == (u32)(blockCache[c] & 0xFFu);
}

struct Backend : EmuBackend {
	template <typename P>
	void run_regular(const P& p, u32 levels)
	{
		EmuBackend::run_regular(p, levels);
		if (!p.G.dirty) compare_texture_forms(p, levels);
	}

	template <typename P>
	void compare_texture_forms(const P& p, u32 levels)
	{
		memset(g_counts, 0, sizeof(g_counts));
		std::vector<unsigned long long> vrow(256, 0);
		for (u32 code = 0; code < 256; ++code) memcpy(&vrow[code], p.tables + TAB_REG_VERT + code * 6, 6);
		const F0Tables FT = f0_tables_from_image(p.tables, vrow.data());
		Fast0State<640>* f0 = new Fast0State<640>;
		Fast1State<640>* f1 = new Fast1State<640>;
		// pools, records and statistics of this walk's own: the run's stay what the regular pass made them
		std::vector<PolyVertex> verts(65536);
		std::vector<u32> idx(3 * 65536);
		u32 cursors[16], stats[64];
		Pools PS = p.P;
		PS.verts = verts.data(); PS.idx = idx.data(); PS.cursors = cursors; PS.vertCap = 65536; PS.idxCap = 3 * 65536;
		const F1HostSampler smp{ &p.G.grid };
		for (u32 level = 0; level < levels && level < (u32)PYRAMID_LEVELS; ++level) {
			LevelDesc L = p.levels[level];
			const u32 slots = item_count(p, level);
			std::vector<BlockRecord> recs(slots ? slots : 1u);
			L.records = recs.data();
			for (u32 slot = 0; slot < slots; ++slot) {
				const u32 ntc = L.ntCount[slot];
				if (ntc == 0 || (level == 0 && L.skip[slot])) continue;
				if (ntc > 640u) { ++g_counts[level][5]; continue; }
				u32 bx, by, bz;
				block_coords(L.slotCoord[slot], L.cnt, bx, by, bz);
				memset(cursors, 0, sizeof(cursors));
				memset(stats, 0, sizeof(stats));
				const int mult = (int)L.mult, ox = (int)bx * 16 * mult, oy = (int)by * 16 * mult, oz = (int)bz * 16 * mult;
				const bool ok = level == 0 ? f0_block_serial(*f0, FT, p.G, L, PS, slot, bx, by, bz, stats)
				                           : f1_block_serial(*f1, FT, p.G, L, PS, level, slot, bx, by, bz, stats);
				if (!ok || cursors[CUR_OVF]) { ++g_counts[level][5]; continue; }
				++g_counts[level][6];
				const u32 vOff = recs[slot].vOff, vTotal = recs[slot].vCount;
				const u16* blockCache = level ? L.cache + (size_t)slot * BLOCK_CELLS : nullptr;
				for (u32 cv = 0; cv < vTotal; cv += (u32)F0_VDESC) {
					const u32 vEnd = vTotal - cv < (u32)F0_VDESC ? vTotal - cv : (u32)F0_VDESC;
					u32 got[2];
					if (level == 0) {
						const u32 nt = f0->wordPrefix[128];
						for (u32 k = 0; k < nt; ++k) f0_describe(*f0, FT, k, f0->cellC[k], cv, 0u, false);
						for (u32 j = 0; j < vEnd; ++j) {
							const u32 desc = f0->vdesc[j], c = desc & 0xFFFu;
							const int mo = (int)((c >> 8) * F0_MPLANE + ((c >> 4) & 15u) * F0_MROW + (c & 15u));
							const u32 cellId = f0->matId[mo];
							const unsigned long long row = lut_row(p.G.lut, cellId);
							f0_vertex_tex(*f0, FT, desc, row, TexCapture{ got });
							const F0Edge e = FT.edge[desc >> 12];
							const int m0 = mo + (int)(e.y & 0x3FFu), m1 = m0 + (int)((e.y >> 10) & 0x3FFu);
							tally(level, got, verts[vOff + cv + j], f0->matId[m0] == f0->matId[m1] && f0->matId[m0] == cellId, row);
						}
					} else {
						static_assert((int)F1_VDESC == (int)F0_VDESC, "one chunk size");
						const u32 nt = f1->wordPrefix[128];
						for (u32 k = 0; k < nt; ++k) f0_describe(*f1, FT, k, f1->cellC[k], cv, 0u, false);
						for (u32 j = 0; j < vEnd; ++j) {
							const u32 desc = f1->vdesc[j];
							const unsigned long long row = lut_row(p.G.lut, f1->cacheId[desc & 0xFFFu]);
							if (!f1_vertex_tex(*f1, FT, smp, blockCache, desc, (int)level, ox, oy, oz, row, TexCapture{ got })) ++g_counts[level][7];
							tally(level, got, verts[vOff + cv + j], f1_same_branch(*f1, FT, smp, blockCache, desc, (int)level, ox, oy, oz), row);
						}
					}
				}
			}
		}
		delete f0;
		delete f1;
	}
};

}

#include "../../voxels_amd/csrc/vx_host.inl"

extern "C" {

void gkh_reset(void) { memset(g_counts, 0, sizeof(g_counts)); }
uint32_t gkh_levels(void) { return (uint32_t)MAX_LEVELS; }
// out[gkh_levels()][8]
void gkh_counts(uint64_t* out) { memcpy(out, g_counts, sizeof(g_counts)); }

} // extern "C"
