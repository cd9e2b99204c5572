// vx_fastt.inl — trf_block: the table-driven body of one block's transition cells (tv_fastt.h has the per-lane logic), written
// for gfx950.  Included by vx_hip.hip in front of tr_block, which stages the planes, the sign summaries and the quiet faces
// for both bodies, notes while it deposits the rows whether a face that is on holds an exact zero (TrState::zero), classifies
// the cells and then calls this.  k_main<false>, k_main<true> and the stand-alone k_transition all come through here.
//
// Eligible is a block without such a zero whose non-trivial transition cells fit one batch (TR_CAP); any other block returns
// false before anything is written and tr_block runs the general phases in place, on the planes already staged.
// Phases behind the classification (a barrier between each two):
//   bitmap prefix per wave (DPP scan, no exchange) + compact list
//   | cells: wave-contiguous ranges, case row -> created mask, slot ordinals, counts; DPP scan, one total per wave
//   | bases + the one reservation + descriptors of vertices and triangles together
//   | one loop: a lane emits a vertex (tr_emit_vertex) and a triangle (trf_triangle).
// The case rows are read from the table image in device memory (4 KB, one 8-byte load per non-trivial cell beside the loads of
// its materials): the LDS table area keeps the general tables, which the vertices, the triangles and the fallback need.
namespace {

template <bool WIDE, bool GATED>
__device__ __forceinline__ bool trf_block(const ExecParamsDev& p, const RegBlockCtx& b, TrState& st, const Tables& T, u32* waveTot,
                                          const BrickSamplerT<typename std::conditional<WIDE, size_t, u32>::type>& smp, const int tid, bool& matReady, const bool preMat)
{
	// GATED, in a run that keeps the mesh layout (MainPlan::layout, main_layout_kept): the ranges come from the slot's record, the
	// totals are checked against it, and no record is stored (see f0_walk)
	const u32 lane = (u32)tid & 63u, wave = (u32)tid >> 6;
	const LevelDesc& L = p.levels[b.level];

	// ---- popcount prefix of the bitmap (every wave computes all of it: no exchange), compact cell list -------------------
	const u32 word = lane < 48u ? st.ntAll[lane] : 0u;
	const u32 wordCnt = (u32)__popc(word);
	const u32 incl = wave_inclusive_scan_dpp(wordCnt);
	const u32 nt = r0_uniform((u32)__shfl((int)incl, 63, 64));
	if (r0_uniform(st.zero) != 0u || nt > (u32)TR_CAP) return false;
	if (nt == 0u) {
		if (tid == 0 && !(GATED && main_layout_kept())) tr_write_empty_record(L, b.slot);
		return true;
	}
	{
		const u32 excl = incl - wordCnt;
		if (wave == 0u) {
			if (lane < 48u) st.wordPrefix[lane] = (u16)excl;
			if (lane == 48u) st.wordPrefix[48] = (u16)nt;
		}
		// one lane per (face, cell row) half-word of the bitmap: lane tid takes half (tid & 1) of word tid >> 1
		const int src = (tid >> 1) & 63;
		const u32 wSel = (u32)__shfl((int)word, src, 64);
		u32 kk = (u32)__shfl((int)excl, src, 64);
		if (tid < 96) {
			u32 bits = wSel & 0xFFFFu;
			if (tid & 1) { kk += (u32)__popc(bits); bits = wSel >> 16; }
			while (bits) {
				const u32 col = (u32)__builtin_ctz(bits);
				bits &= bits - 1;
				st.cellOf[kk++] = (u16)(((u32)tid << 4) | col);
			}
		}
	}
	if (GATED && !matReady) {
		// the block's material cache (the cells behind the faces) comes from another workgroup of this launch
		if (tid == 0) (void)wait_done(L.matDone + b.slot, p.G.epoch, p.G.giveUp);
		acquire_and_meet(tid < 64);
		matReady = true;
	} else
		__syncthreads();

	// ---- cells: wave w owns the compact cells [w * Q, w * Q + Q), Q a multiple of 64; local scan per wave ------------------
	const u32 Q = ((nt + WG - 1) / WG) * 64u;
	const u32 kBeg = r0_uniform(min(wave * Q, nt)), kEnd = r0_uniform(min(wave * Q + Q, nt));
	{
		const TrfRow* rows = (const TrfRow*)(p.tables + TAB_FT_CASE);
		const u16* cache = L.cache + (size_t)b.slot * BLOCK_CELLS;
		u32 carry = 0;
		for (u32 k0 = kBeg; k0 < kEnd; k0 += 64u) {
			const u32 k = k0 + lane;
			u32 cnt = 0;
			if (k < kEnd) {
				const u32 c = st.cellOf[k];
				u32 mat, matCol, matRow;
				if (preMat) { // (uniform) the entries behind all transition cells were staged with the planes
					mat = st.faceMat[c]; matCol = st.faceMat[c - ((c & 15u) ? 1u : 0u)]; matRow = st.faceMat[c - ((c & 0xF0u) ? 16u : 0u)];
				} else {
					u32 stepCol, stepRow;
					const u32 idx = trf_low_index(c, stepCol, stepRow);
					mat = TV_LOAD_THROUGH(&cache[idx]);
					matCol = TV_LOAD_THROUGH(&cache[idx - ((c & 15u) ? stepCol : 0u)]);
					matRow = TV_LOAD_THROUGH(&cache[idx - ((c & 0xF0u) ? stepRow : 0u)]);
				}
				cnt = trf_cell(st, rows, k, mat, matCol, matRow);
#if defined(VX_CASE_DUMP)
				L.trCaseDump[(size_t)b.slot * TR_CELLS + c] = (u16)(st.cellBits[k] & 0x1FFu);
#endif
			}
			const u32 in = wave_inclusive_scan_dpp(cnt);
			if (k < kEnd) { const u32 base = carry + in - cnt; st.vbase[k] = (u16)base; st.ibase[k] = (u16)(base >> 16); }
			carry += (u32)__shfl((int)in, 63, 64);
		}
		if (lane == 0u) waveTot[wave] = carry;
	}
	__syncthreads();

	// ---- bases, the reservation (requested here, first looked at behind the descriptors), descriptors ----------------------
	{
		u32 waveBase = 0, tot = 0;
#pragma unroll
		for (u32 w = 0; w < (u32)(WG / 64); ++w) {
			const u32 s = waveTot[w];
			if (w < wave) waveBase += s;
			tot += s;
		}
		if (tid == WG - 1) {
			st.vTotal = tot & 0xFFFFu; st.iTotal = tot >> 16;
			if (GATED && main_layout_kept()) layout_ranges_faces(p, L.records[b.slot], 0, 6, tot & 0xFFFFu, tot >> 16, st.vOff, st.iOff);
			else reserve_both(p.P.cursors, tot & 0xFFFFu, tot >> 16, st.vOff, st.iOff);
		}
		const bool tris = !(GATED && main_indices_kept()); // (the index pool is kept: no triangle descriptors, see f0_walk)
		for (u32 k0 = kBeg; k0 < kEnd; k0 += 64u) {
			const u32 k = k0 + lane;
			if (k < kEnd) {
				st.vbase[k] = (u16)((u32)st.vbase[k] + (waveBase & 0xFFFFu));
				st.ibase[k] = (u16)((u32)st.ibase[k] + (waveBase >> 16));
				trf_describe(st, T, k, 0u, 0u, tris);
			}
		}
	}
	__syncthreads();

	// ---- one lane = one vertex and one triangle ----------------------------------------------------------------------------
	// (the index pool is kept, MainPlan::layout 2, read where it decides: no chunk for the triangles' sake, none described, tEnd 0)
	const u32 vTotal = r0_uniform(st.vTotal), iTotal = r0_uniform(st.iTotal), tTotal = iTotal / 3u;
	const u32 vOff = r0_uniform(st.vOff), iOff = r0_uniform(st.iOff);
	if (vOff + vTotal <= p.P.vertCap && iOff + iTotal <= p.P.idxCap) {
		for (u32 chunk = 0; chunk == 0 || chunk * VDESC_CAP < vTotal || (chunk * TRF_TDESC < tTotal && !(GATED && main_indices_kept())); ++chunk) {
			const u32 cv = chunk * VDESC_CAP, ct = chunk * TRF_TDESC;
			if (chunk) {
				__syncthreads();
				for (u32 k = (u32)tid; k < nt; k += WG) trf_describe(st, T, k, cv, ct, !(GATED && main_indices_kept()));
				__syncthreads();
			}
			const u32 vEnd = cv < vTotal ? min(vTotal - cv, (u32)VDESC_CAP) : 0u;
			const u32 tEnd = (ct < tTotal && !(GATED && main_indices_kept())) ? min(tTotal - ct, (u32)TRF_TDESC) : 0u;
			PolyVertex* vOut = p.P.verts + vOff + cv;
			u32* iOut = p.P.idx + iOff + ct * 3u;
			for (u32 base = 0; base < vEnd || base < tEnd; base += WG) {
				const u32 j = base + (u32)tid;
				if (j < vEnd) trf_vertex(st, T, p.G, smp, b, st.vdesc[j], vOut + j);
				if (j < tEnd) {
					u32 ids[3];
					trf_triangle(st, T, j, ids);
					u32* o3 = iOut + j * 3u;
					TV_STREAM_STORE(&o3[0], ids[0]); TV_STREAM_STORE(&o3[1], ids[1]); TV_STREAM_STORE(&o3[2], ids[2]);
				}
			}
		}
	}
	if (!(GATED && main_layout_kept())) tr_phase_record(st, L, b, p.P, 0, 6, tid); // (layout kept: the record is the run before's)
	return true;
}

} // namespace
