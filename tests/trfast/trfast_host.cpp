// trfast_host.cpp — host side of tests/test_trfast_tables.py (tests only; built by voxels_amd/build.py build_trfast_host()).
//
// The CPU emulation of tests/emu (the product's host orchestration over sequential phases) with a transition pass whose
// body is selectable: trfh_set_mode(0) runs the general phases of tv_block.h for every block, trfh_set_mode(1) runs
// trf_block_serial (voxels_amd/csrc/tv_fastt.h) and, where that declines a block, the general phases on the planes it staged
// - what tr_block does on the GPU.  trfh_counts() = blocks by body since the last trfh_set_mode.  The library is a complete
// C ABI (vx_*), so a test compares whole runs: vertices, indices, records with their per-face ranges.
//
// trfh_check_tables() is the exhaustive check of the derived case rows: every case code 1..510 as the cell at (row, col) in
// {0, 1}^2 of a face (the four values of the reuse mask), every same-material combination of its two reuse directions, the
// surrounding samples non-zero with pseudo-random signs (the neighbours share the cell's samples as on a real plane), on a
// face of either winding: the general phases and the table-driven functions must give the same created masks, stored slot
// ordinals, bases and index lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../voxels_amd/csrc/tv_block.h"
#include "../../voxels_amd/csrc/tv_fast0.h"
#include "../../voxels_amd/csrc/tv_fast1.h"
#include "../../voxels_amd/csrc/tv_fastt.h"
#include "../../voxels_amd/csrc/vx_terrain_math.h"

#define VX_BACKEND_NAME "emu:cpu (tests only, transition body selectable)"

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

int g_mode = 1;
u32 g_counts[2] = { 0, 0 };

// the general phases of one block behind tr_phase_load (tests/emu/emu_backend.inl run_transition)
template <typename SMP>
void general_phases(TrState& st, const Tables& T, const Globals& G, const LevelDesc& L, const Pools& P, const RegBlockCtx& b, const SMP& smp, const u16* preMat)
{
	tr_phase_classify(st, 0, 1);
	for (int f0 = 0; f0 < 6;) {
		const int f1 = tr_batch_end(st, f0);
		tr_phase_batch_bits(st, f0, f1, 0, 1);
		st.wordPrefix[48] = (u16)exclusive_scan(st.wordPrefix, 48);
		st.vTotal = st.iTotal = st.vOff = st.iOff = 0;
		if (st.wordPrefix[48]) {
			tr_phase_cells_of(st, 0, 1);
			tr_phase_list(st, T, L, b, 0, 1, preMat);
			tr_phase_count(st, T, 0, 1);
			st.vTotal = exclusive_scan(st.vbase, st.wordPrefix[48]);
			st.iTotal = exclusive_scan(st.ibase, st.wordPrefix[48]);
			st.vOff = TV_ATOMIC_ADD(&P.cursors[CUR_V], st.vTotal);
			st.iOff = TV_ATOMIC_ADD(&P.cursors[CUR_I], st.iTotal);
			if (P.verts) for (u32 chunk = 0; chunk == 0 || chunk < st.vTotal; chunk += VDESC_CAP) {
				tr_phase_describe(st, chunk, 0, 1);
				tr_phase_emit_vertices(st, T, G, smp, P, b, chunk, 0, 1);
			}
			for (u32 chunk = 0; chunk < st.iTotal; chunk += TR_INDEX_CHUNK) {
				tr_phase_stage_indices(st, T, chunk, 0, 1);
				tr_phase_flush_indices(st, T, P, chunk, 0, 1);
			}
		}
		if (L.records) tr_phase_record(st, L, b, P, f0, f1, 0);
		f0 = f1;
	}
}

struct Backend : EmuBackend {
	template <typename P>
	void run_transition(const P& p, u32 levels)
	{
		if (g_mode == 0) { EmuBackend::run_transition(p, levels); return; }
		const Tables T = tables_from_image(p.tables);
		const TrfRow* rows = (const TrfRow*)(p.tables + TAB_FT_CASE);
		TrState* st = new TrState;
		for (u32 level = 1; level < levels; ++level) {
			const LevelDesc& L = p.levels[level];
			if (!L.hasTransitions) continue;
			for (u32 it = 0; it < item_count(p, level); ++it) {
				RegBlockCtx b;
				b.level = level; b.slot = item_slot(p, level, it); b.mult = L.mult;
				block_coords(L.slotCoord[b.slot], L.cnt, b.bx, b.by, b.bz);
				if (trf_block_serial(*st, T, rows, p.G, L, p.P, b)) { ++g_counts[0]; continue; }
				++g_counts[1];
				general_phases(*st, T, p.G, L, p.P, b, F1HostSampler{ &p.G.grid }, nullptr);
			}
		}
		delete st;
	}
};

}

#include "../../voxels_amd/csrc/vx_host.inl"

namespace {

struct NoSampler { // (the table check emits no vertices)
	typedef size_t Off;
	Off tx(int) const { return 0; } Off ty(int) const { return 0; } Off tz(int) const { return 0; }
	int dist(Off) const { return 1; } u32 mat(Off, int, int, int) const { return 0; }
};

u32 rng_next(u32& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

}

extern "C" {

void trfh_set_mode(int mode) { g_mode = mode; g_counts[0] = g_counts[1] = 0; }
void trfh_counts(uint32_t out[2]) { out[0] = g_counts[0]; out[1] = g_counts[1]; }

// returns the number of configurations checked; *mismatches = those that differ (the first few are described on stderr)
uint32_t trfh_check_tables(uint32_t fills, uint32_t* mismatches)
{
	std::vector<u8> img;
	build_table_image(img);
	const Tables T = tables_from_image(img.data());
	const TrfRow* rows = (const TrfRow*)(img.data() + TAB_FT_CASE);
	TrState* a = new TrState;
	TrState* g = new TrState;
	std::vector<u32> idxA(TR_CAP * 36), idxG(TR_CAP * 36);
	u32 cursorsA[8] = { 0 }, cursorsG[8] = { 0 };
	Globals G; memset(&G, 0, sizeof(G));
	LevelDesc L; memset(&L, 0, sizeof(L));
	RegBlockCtx b; memset(&b, 0, sizeof(b));
	u32 checked = 0, bad = 0, seed = 12345u;
	for (u32 code = 1; code < 511; ++code)
	for (u32 pos = 0; pos < 4; ++pos)
	for (u32 same = 0; same < 4; ++same)
	for (u32 face = 0; face < 2; ++face)
	for (u32 fill = 0; fill < fills; ++fill) {
		const int row = (int)(pos >> 1), col = (int)(pos & 1u);
		memset(g, 0, sizeof(TrState));
		g->faceOn = 1u << face;
		i8* pl = g->plane[face];
		for (int v = 0; v < 33; ++v) for (int u = 0; u < 33; ++u) pl[v * TR_PROW + u] = 7;
		for (int v = 0; v < 7; ++v) for (int u = 0; u < 7; ++u) pl[v * TR_PROW + u] = (i8)((rng_next(seed) & 1u) ? -(int)(1 + (rng_next(seed) % 127u)) : (int)(1 + (rng_next(seed) % 127u)));
		// the cell's own nine samples from its case code (tr_case_code's weights)
		static const u32 weight[9] = { 1, 2, 4, 0x80, 0x100, 8, 0x40, 0x20, 0x10 };
		for (int j = 0; j < 3; ++j) for (int i = 0; i < 3; ++i) {
			i8& s = pl[(row * 2 + j) * TR_PROW + col * 2 + i];
			const int mag = s < 0 ? -(int)s : (int)s;
			s = (i8)((code & weight[j * 3 + i]) ? -mag : mag);
		}
		for (u32 c = 0; c < (u32)TR_CELLS; ++c) g->faceMat[c] = 3;
		const u32 cell = (face << 8) | ((u32)row << 4) | (u32)col;
		g->faceMat[cell] = 1 | (9u << 8);
		if (col) g->faceMat[cell - 1] = (u16)(((same & 1u) ? 1u : 2u) | (5u << 8));
		if (row) g->faceMat[cell - 16] = (u16)(((same & 2u) ? 1u : 2u) | (6u << 8));
		memcpy(a, g, sizeof(TrState));
		// general phases (no vertices: P.verts = nullptr)
		Pools PG; memset(&PG, 0, sizeof(PG));
		PG.idx = idxG.data(); PG.cursors = cursorsG; PG.vertCap = ~0u; PG.idxCap = ~0u; cursorsG[CUR_V] = cursorsG[CUR_I] = 0;
		general_phases(*g, T, G, L, PG, b, NoSampler(), g->faceMat);
		// table-driven functions
		tr_phase_classify(*a, 0, 1);
		bool ok = trf_list_serial(*a) && !trf_planes_have_zero(*a);
		const u32 nt = a->wordPrefix[48];
		u32 run = 0;
		for (u32 k = 0; ok && k < nt; ++k) {
			const u32 c = a->cellOf[k];
			const u32 cnt = trf_cell(*a, rows, k, a->faceMat[c], a->faceMat[c - ((c & 15u) ? 1u : 0u)], a->faceMat[c - ((c & 0xF0u) ? 16u : 0u)]);
			a->vbase[k] = (u16)(run & 0xFFFFu); a->ibase[k] = (u16)(run >> 16);
			run += cnt;
		}
		a->vTotal = run & 0xFFFFu; a->iTotal = run >> 16;
		ok = ok && nt == g->wordPrefix[48] && a->vTotal == g->vTotal && a->iTotal == g->iTotal;
		for (u32 k = 0; ok && k < nt; ++k) {
			ok = a->cellOf[k] == g->cellOf[k] && a->newMask[k] == g->newMask[k] && a->vbase[k] == g->vbase[k] && a->ibase[k] == g->ibase[k]
			  && (a->cellBits[k] & 0x1FFu) == (g->cellBits[k] & 0x1FFu) && (g->cellBits[k] >> 9) == 0u && g->valid[k] == T.trOwn(g->cellBits[k] & 0x1FFu);
			// every slot the general pass stores is one of the six, with the same ordinal
			for (u32 s = 0; ok && s < 10; ++s) if ((g->valid[k] >> s) & 1u)
				ok = (s >= 3 && s != 7) && ((u32)(g->ords[k] >> (4 * s)) & 15u) == (((u32)a->ords[k] >> (4 * trf_slot_nibble(s))) & 15u);
		}
		const u32 tTotal = a->iTotal / 3u;
		for (u32 chunk = 0; ok && chunk * TRF_TDESC < tTotal; ++chunk) {
			for (u32 k = 0; k < nt; ++k) trf_describe(*a, T, k, ~0u - VDESC_CAP, chunk * TRF_TDESC); // (triangles only)
			const u32 tEnd = tTotal - chunk * TRF_TDESC < (u32)TRF_TDESC ? tTotal - chunk * TRF_TDESC : (u32)TRF_TDESC;
			for (u32 t = 0; t < tEnd; ++t) trf_triangle(*a, T, t, idxA.data() + (chunk * TRF_TDESC + t) * 3u);
		}
		ok = ok && memcmp(idxA.data(), idxG.data(), a->iTotal * 4u) == 0;
		++checked;
		if (!ok && bad++ < 5) fprintf(stderr, "[trfast] mismatch: case %u at (row %d, col %d), same-material bits %u, face %u, fill %u\n", code, row, col, same, face, fill);
	}
	delete a; delete g;
	*mismatches = bad;
	return checked;
}

} // extern "C"
