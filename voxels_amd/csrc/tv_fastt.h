// tv_fastt.h — the transition cells of a block whose staged boundary planes hold no exact zero, table-driven.
// (The transition part of PolygonizeBlock, src/TransVoxelImpl.cpp, restricted to the inputs where none of its end-point
// rules can fire; the counterpart of tv_fast0.h for the regular cells.)
//
// In a transition cell none of whose 9 plane samples is zero
//   * every table vertex lies strictly inside its edge: no corner vertex, no trCorner look-up, t = "inside";
//   * the vertex words of the table carry the directions 1, 2 (reuse from column - 1 / row - 1 of the same face),
//     4 (always created, never stored) and 8 (created and stored);
//   * the owner of a direction-1 / direction-2 vertex is that neighbour cell, and it is non-trivial: it holds both end
//     points of the shared edge, hence its sign change - and it stores the vertex in the slot the word names (its own
//     word for that edge has direction 8 and the same slot).  So "a non-trivial cell earlier in the row" (mask2 bit 0) holds
//     whenever a direction-1 vertex exists in a column > 0, and reuse is decided by (case, mask2, "that neighbour has my
//     low-resolution material") alone.
// Per case that is one 8-byte row: the vertices reused from either direction as masks, the counts, the class, and the list
// positions of the vertices stored in the six slots a neighbour can ask for.  tests/test_trfast_tables.py checks the rows
// against tr_resolve() and the general index logic for every case, mask and material combination.
//
// The per-lane functions are __host__ __device__: trf_block (vx_fastt.inl) runs them on the GPU, trf_block_serial() below
// on the CPU.  A block with a zero on a staged plane, or with more non-trivial transition cells than one batch holds, goes
// through the general phases of tv_block.h; results are identical either way.
#pragma once

#include "tv_fast1.h"

namespace tv {

enum : u32 {
	TAB_FT_CASE = TAB_F0_BYTES,            // 512 x 2 dwords, see trf_build_tables (appended to the image of tv_fast0.h)
	TAB_FT_BYTES = TAB_F0_BYTES + 512 * 8
};
enum { TRF_TDESC = TR_CAP };               // triangles described per chunk (TrState::valid holds the descriptors: the table-driven body
                                           // needs no slot masks); vertices: VDESC_CAP per chunk, in TrState::vdesc

// x: reused from direction 1 (12) | vertices << 12 | reused from direction 2 << 16 | triangles << 28
// y: list positions of the vertices stored in the slots 3, 4, 5, 6, 8, 9 (4 bits each, 15: none) | class << 24
struct alignas(8) TrfRow { u32 x, y; };

// the slots a neighbour can ask for are 3..6 and 8, 9 (the direction-1 and direction-2 words of the table): nibble 0..5
TV_HD u32 trf_slot_nibble(u32 slot) { return slot - 3u - (slot >= 8u ? 1u : 0u); }

// Host side: fills the TAB_FT_CASE part of the table image from Lengyel's transition tables (trClass[512], trCell[56][40],
// trVert[512][12] words (dir << 12 | slot << 8 | v0 << 4 | v1)).
inline void trf_build_tables(u8* img, const unsigned char* trClass, const unsigned char* trCell, const unsigned short* trVert)
{
	for (u32 code = 0; code < 512; ++code) {
		const u32 cls = trClass[code], geom = trCell[(cls & 0x7Fu) * 40], nv = geom >> 4, ntri = geom & 15u;
		u32 r1 = 0, r2 = 0, own = 0xFFFFFFu;
		for (u32 vi = 0; vi < nv; ++vi) {
			const u32 w = trVert[code * 12 + vi], dir = w >> 12, slot = (w >> 8) & 15u;
			if (dir == 1u) r1 |= 1u << vi;
			else if (dir == 2u) r2 |= 1u << vi;
			else if (dir == 8u) { const u32 j = trf_slot_nibble(slot) * 4u; own = (own & ~(15u << j)) | (vi << j); }
		}
		const TrfRow row = { r1 | (nv << 12) | (r2 << 16) | (ntri << 28), own | (cls << 24) };
		memcpy(img + TAB_FT_CASE + code * 8, &row, 8);
	}
}

// what the case row, the reuse mask and the materials of the two neighbours decide about a cell
struct TrfCell {
	u32 newMask;   // table vertices the cell creates
	u32 ords;      // ordinal, among the created ones, of the vertex stored in each of the six slots (4 bits each)
	u32 counts;    // created vertices | indices << 16
};

//   mask2: bit 0 = a non-trivial transition cell exists earlier in this row, bit 1 = row > 0 (tr_mask2)
//   same:  bit 0 = the cell at column - 1 has this cell's low-resolution material id, bit 1 = the cell at row - 1 has
TV_HD TrfCell trf_resolve(const TrfRow& row, u32 mask2, u32 same)
{
	const u32 allow = mask2 & same;
	const u32 reused = ((0u - (allow & 1u)) & row.x) | ((0u - ((allow >> 1) & 1u)) & (row.x >> 16));
	const u32 nv = (row.x >> 12) & 15u;
	TrfCell r;
	r.newMask = ((1u << nv) - 1u) & ~reused;
	r.ords = 0;
#pragma unroll
	for (u32 j = 0; j < 6; ++j) {
		const u32 pos = (row.y >> (4u * j)) & 15u;
		r.ords |= (u32)TV_POPC(r.newMask & ((1u << pos) - 1u)) << (4u * j);
	}
	r.counts = (u32)TV_POPC(r.newMask) | ((row.x >> 28) * 3u << 16);
	return r;
}

// case code of cell (f, row, col) from the staged plane: two reads per sample row (the samples 2 col, 2 col + 1 as one aligned
// half-word)
TV_HD u32 trf_case_code(const TrState& st, int f, int row, int col)
{
	const i8* p = st.plane[f] + (row * 2) * TR_PROW + col * 2;
	u32 s[3];
#pragma unroll
	for (int j = 0; j < 3; ++j) {
		const u32 lo = *(const u16*)(p + j * TR_PROW), hi = (u32)(u8)p[j * TR_PROW + 2];
		s[j] = ((lo >> 7) & 1u) | ((lo >> 14) & 2u) | ((hi >> 5) & 4u); // signs of the row's three samples
	}
	// weights 1,2,4,0x80,0x100,8,0x40,0x20,0x10 for samples 0..8 (tr_case_code)
	return s[0] | ((s[1] & 1u) << 7) | ((s[1] & 2u) << 7) | ((s[1] & 4u) << 1) | ((s[2] & 1u) << 6) | ((s[2] & 2u) << 4) | ((s[2] & 4u) << 2);
}

// tr_mask2 on the bitmap of all faces (the table-driven body handles a block as one batch)
TV_HD u32 trf_mask2(const TrState& st, u32 c)
{
	const u32 r = c >> 4, col = c & 15u;
	const u32 rowBits = (st.ntAll[r >> 1] >> ((r & 1u) * 16u)) & 0xFFFFu;
	return ((rowBits & ((1u << col) - 1u)) ? 1u : 0u) | ((r & 15u) ? 2u : 0u);
}

// index into a block's material cache of the low-resolution cell behind transition cell c, and the steps to the cells behind
// the transition cells at column - 1 / row - 1 of the same face
TV_HD u32 trf_low_index(u32 c, u32& stepCol, u32& stepRow)
{
	const FaceGeom fg = face_geom((int)(c >> 8));
	int local[3];
	tr_low_local(fg, (int)((c >> 4) & 15u), (int)(c & 15u), local);
	stepCol = 1u << (4 * fg.ua); stepRow = 1u << (4 * fg.va);
	return (u32)((local[2] << 8) | (local[1] << 4) | local[0]);
}

// ---- one compact cell: case, reuse resolution, counts (returns created vertices | indices << 16) ------------------------
// mat, matCol, matRow: the material entries of the low-resolution cells behind this cell and behind the cells at column - 1 and
// row - 1 (any value where there is no such cell: mask2 rules it out)
TV_HD u32 trf_cell(TrState& st, const TrfRow* rows, u32 k, u32 mat, u32 matCol, u32 matRow)
{
	const u32 c = st.cellOf[k];
	const u32 code = trf_case_code(st, (int)(c >> 8), (int)((c >> 4) & 15u), (int)(c & 15u));
	const TrfRow row = rows[code];
	const u32 same = (((matCol ^ mat) & 0xFFu) == 0u ? 1u : 0u) | (((matRow ^ mat) & 0xFFu) == 0u ? 2u : 0u);
	const TrfCell r = trf_resolve(row, trf_mask2(st, c), same);
	st.cellMat[k] = (u16)mat;
	st.cellBits[k] = code | ((row.y >> 24) << 9); // case | class (bit 7: winding) << 9; no sample is zero: the bits above 8 are not a zero mask here
	st.newMask[k] = (u16)r.newMask;
	st.ords[k] = r.ords;
	return r.counts;
}

// descriptors of cell k's new vertices and triangles that fall into the given chunks (vbase / ibase scanned)
// tris == false (uniform; a run that keeps the index pool, MainPlan::layout 2): no triangle descriptor is written (f0_describe)
TV_HD void trf_describe(TrState& st, const Tables& T, u32 k, u32 chunkV, u32 chunkT, const bool tris = true)
{
	u32 m = st.newMask[k];
	u32 j = st.vbase[k];
	if (m && j < chunkV + (u32)VDESC_CAP && j + 12 > chunkV) {
		while (m) {
			const u32 vi = (u32)F0_CTZ(m);
			m &= m - 1;
			if (j >= chunkV && j < chunkV + (u32)VDESC_CAP) st.vdesc[j - chunkV] = (u16)(k | (vi << 11));
			++j;
		}
	}
	if (!tris) return;
	const u32 ntri = (u32)T.trCell((st.cellBits[k] >> 9) & 0x7Fu)[0] & 15u;
	u32 t = (u32)st.ibase[k] / 3u; // (index counts are multiples of three, and so are their prefix sums)
	if (t < chunkT + (u32)TRF_TDESC && t + 12 > chunkT) {
		for (u32 tr = 0; tr < ntri; ++tr, ++t)
			if (t >= chunkT && t < chunkT + (u32)TRF_TDESC) st.valid[t - chunkT] = (u16)(k | (tr << 9));
	}
}

// ---- one lane = one new vertex: tr_emit_vertex of tv_block.h with "no sample is zero" ------------------------------------
template <typename SMP>
TV_HD void trf_vertex(const TrState& st, const Tables& T, const Globals& G, const SMP& smp, const RegBlockCtx& b, u32 desc, PolyVertex* out)
{
	const u32 k = desc & 0x7FFu;
	tr_emit_vertex(st, T, G, smp, b, k, desc >> 11, st.cellBits[k] & 0x1FFu, 0u, out);
}

// ---- one lane = one triangle of the chunk: its three indices, relative to the face's first vertex -----------------------
// Winding flipped per class and face as in tr_phase_flush_indices.  A created vertex is the cell's vertex base plus its rank
// among the cell's created vertices; a reused one the owner's base plus the stored ordinal of the slot.  Both forms are
// evaluated and one is picked (f0_triangle): direction and slot come straight from the vertex word - strictly inside its
// edge, nothing else can change them - and for a created vertex the "owner" is taken to be the cell itself, so every read
// stays inside the staged state.
TV_HD void trf_triangle(const TrState& st, const Tables& T, u32 t, u32 out[3])
{
	const u32 d = st.valid[t];
	const u32 k = d & 0x1FFu, tr = d >> 9;
	const u32 c = st.cellOf[k], f = c >> 8;
	const u32 bits = st.cellBits[k], code = bits & 0x1FFu, cls = bits >> 9;
	const u8* cd = T.trCell(cls & 0x7Fu) + 1u + tr * 3u;
	const bool flip = ((cls >> 7) ^ (f & 1u)) != 0; // reverseWinding = {0,1,0,1,0,1}
	const u32 faceVBase = st.vbase[st.wordPrefix[f * 8]]; // the face's first cell exists: cell k is in it
	const u32 nm = st.newMask[k], own = (u32)st.vbase[k] - faceVBase;
#pragma unroll
	for (u32 e = 0; e < 3; ++e) {
		const u32 vi = cd[(flip && e) ? 3u - e : e];
		const u32 created = own + (u32)TV_POPC(nm & ((1u << vi) - 1u));
		const u32 w = T.trVert(code, vi), dir = w >> 12, slot = (w >> 8) & 15u;
		const bool isNew = ((nm >> vi) & 1u) != 0;
		const u32 c2 = isNew ? c : c - ((dir & 1u) + ((dir & 2u) << 3)); // (a reused vertex has its neighbour: mask2)
		const u32 k2 = bit_rank(st.ntAll, st.wordPrefix, c2);
		const u32 reused = (u32)st.vbase[k2] - faceVBase + (((u32)st.ords[k2] >> (4u * trf_slot_nibble(slot))) & 15u);
		out[e] = isNew ? created : reused;
	}
}

// the bitmap of all faces as the one batch: per-word popcount prefix and the compact list; false: more cells than a batch holds
TV_HD bool trf_list_serial(TrState& st)
{
	u32 nt = 0;
	for (int w = 0; w < 48; ++w) nt += (u32)TV_POPC(st.ntAll[w]);
	if (nt > (u32)TR_CAP) return false;
	nt = 0;
	for (int w = 0; w < 48; ++w) { st.ntBits[w] = st.ntAll[w]; st.wordPrefix[w] = (u16)nt; nt += (u32)TV_POPC(st.ntAll[w]); }
	st.wordPrefix[48] = (u16)nt;
	if (nt) tr_phase_cells_of(st, 0, 1);
	return true;
}

// a staged face that is on holds an exact zero
TV_HD bool trf_planes_have_zero(const TrState& st)
{
	for (int f = 0; f < 6; ++f) {
		if (!((st.faceOn >> f) & 1u)) continue;
		for (int v = 0; v < 33; ++v) for (int u = 0; u < 33; ++u) if (st.plane[f][v * TR_PROW + u] == 0) return true;
	}
	return false;
}

#if !defined(__HIPCC__)
// ---- CPU form of one block (tests/trfast): the same per-lane functions, serial scans -----------------------------------------
// b: level, slot, mult and block coordinates set.  false: the block belongs to the general phases (which the caller runs on
// the planes staged here); nothing was written then.
inline bool trf_block_serial(TrState& st, const Tables& T, const TrfRow* rows, const Globals& G, const LevelDesc& L, const Pools& P, const RegBlockCtx& b)
{
	tr_phase_load(st, G, L, b, 0, 1);
	if (trf_planes_have_zero(st)) return false;
	tr_phase_classify(st, 0, 1);
	if (!trf_list_serial(st)) return false;
	const u32 nt = st.wordPrefix[48];
	st.vTotal = st.iTotal = st.vOff = st.iOff = 0;
	if (nt) {
		const u16* cache = L.cache + (size_t)b.slot * BLOCK_CELLS;
		u32 run = 0;
		for (u32 k = 0; k < nt; ++k) {
			const u32 c = st.cellOf[k];
			u32 stepCol, stepRow;
			const u32 idx = trf_low_index(c, stepCol, stepRow);
			const u32 cnt = trf_cell(st, rows, k, cache[idx], cache[idx - ((c & 15u) ? stepCol : 0u)], cache[idx - ((c & 0xF0u) ? stepRow : 0u)]);
			st.vbase[k] = (u16)(run & 0xFFFFu); st.ibase[k] = (u16)(run >> 16);
			run += cnt;
		}
		st.vTotal = run & 0xFFFFu; st.iTotal = run >> 16;
		st.vOff = TV_ATOMIC_ADD(&P.cursors[CUR_V], st.vTotal);
		st.iOff = TV_ATOMIC_ADD(&P.cursors[CUR_I], st.iTotal);
		const bool room = st.vOff + st.vTotal <= P.vertCap && st.iOff + st.iTotal <= P.idxCap;
		const u32 tTotal = st.iTotal / 3u;
		for (u32 chunk = 0; room && (chunk * VDESC_CAP < st.vTotal || chunk * TRF_TDESC < tTotal); ++chunk) {
			const u32 cv = chunk * VDESC_CAP, ct = chunk * TRF_TDESC;
			for (u32 k = 0; k < nt; ++k) trf_describe(st, T, k, cv, ct);
			const u32 vEnd = cv < st.vTotal ? (st.vTotal - cv < (u32)VDESC_CAP ? st.vTotal - cv : (u32)VDESC_CAP) : 0u;
			const u32 tEnd = ct < tTotal ? (tTotal - ct < (u32)TRF_TDESC ? tTotal - ct : (u32)TRF_TDESC) : 0u;
			for (u32 j = 0; j < vEnd; ++j) trf_vertex(st, T, G, F1HostSampler{ &G.grid }, b, st.vdesc[j], P.verts + st.vOff + cv + j);
			for (u32 t = 0; t < tEnd; ++t) trf_triangle(st, T, t, P.idx + st.iOff + (ct + t) * 3u);
		}
	}
	tr_phase_record(st, L, b, P, 0, 6, 0);
	return true;
}
#endif

} // namespace tv
