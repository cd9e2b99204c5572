// vx_measure.inl — the measurements (include/voxels_hip.h, "measurements"): vx_grid_measure, the solid volume, bounds and
// material tallies of a batch of voxel boxes of the resident grid, and vx_record_measure, what an edit did, read off the undo
// record captured around it; included by vx_hip.hip after vx_stamp.inl (HIP only).  DESIGN.md §23.  The per-row and per-block
// logic is tv_measure.h, shared with the host build of the tests.
//
// The work item is a (box, block) pair.  The host knows the boxes, so the boxes and the running sums of their block counts go up
// in one copy each and nothing is binned on the device.  Pairs are launched in chunks (a range of pair numbers per launch):
//   k_measure_pairs   one workgroup per MEASURE_GROUP consecutive pairs of the launch, one pair after the other: finds the box
//                     of its first pair by binary search in the sums; a lane per 16-byte row of the block - sign mask, clip,
//                     popcount, bounds; the materials of the solid voxels into a 256-bin histogram in LDS, a run of equal bytes
//                     as one atomic.  Per box the workgroup meets: counts and bounds reduced per wave and per workgroup, then
//                     one 64-bit add and at most six 32-bit maxima, and one 64-bit add per non-empty bin
//   k_measure_finish  one wave per box: the non-empty bins counted, the result record written
//   k_rec_measure     one workgroup per 8 consecutive held blocks of a record: the record's rows beside the grid's, two
//                     histograms, one set of atomics per workgroup
// Every atomic is an integer sum or maximum, so the results do not depend on an order, a chunk size or a schedule.  Both calls
// only read the grid and the record; they wait once, at their end, for the copies back.
#include "tv_measure.h"

namespace {

struct MeasureState {
	void* buf = nullptr;       // everything sized by the call
	size_t bufCap = 0;
	u64 chunk = MEASURE_CHUNK_PAIRS;
	bool shortcuts = true;     // the sign summaries may stand in for the distance rows (vx_debug_measure_shortcuts)

	void release(vx_ctx* c)
	{
		c->be.free(buf);
	}
};

// The sign summaries (MirrorState::blockSign, field 0: 1 = every sample of the block is >= 0, 2 = every sample is < 0) describe
// the dense fields while the mirrors are current: every device edit brings them up to date over the blocks it touched
// (rebrick_blocks), and whatever writes the dense fields another way marks the mirrors stale.  Stale or absent: no shortcut.
const u16* grid_block_signs(const vx_ctx* c)
{
	if (c->bricksStale || !c->dBlockSign || c->brickN != c->n) return nullptr;
	return (const u16*)c->dBlockSign;
}

// ... for the measurements (the height maps read them under the same conditions, vx_height.inl)
const u16* measure_signs(const vx_ctx* c, const MeasureState* s)
{
#if defined(VX_MEASURE_NO_SKIP)
	(void)c; (void)s;
	return nullptr;
#else
	return s->shortcuts ? grid_block_signs(c) : nullptr;
#endif
}

// v[0..2] ~min, v[3..5] max, v[6..6 + SUMS) sums, per lane -> v[0] of lane t < 6 + SUMS is entry t over the workgroup; sRed
// holds the waves' partial results behind the barrier in here (the caller adds up the sums it needs on every lane)
template <int SUMS> __device__ __forceinline__ void measure_reduce(u32 (&v)[6 + SUMS], u32 (*sRed)[6 + SUMS], u32 t)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
		for (int k = 0; k < 6; ++k) v[k] = max(v[k], (u32)__shfl_xor((int)v[k], d));
#pragma unroll
		for (int k = 6; k < 6 + SUMS; ++k) v[k] += (u32)__shfl_xor((int)v[k], d);
	}
	if ((t & 63u) == 0) {
#pragma unroll
		for (int k = 0; k < 6 + SUMS; ++k) sRed[t >> 6][k] = v[k];
	}
	__syncthreads();
	if (t < 6 + SUMS) {
		u32 a = sRed[0][t];
#pragma unroll
		for (u32 w = 1; w < WG / 64; ++w) a = t < 6 ? max(a, sRed[w][t]) : a + sRed[w][t];
		v[0] = a;
	}
}

// The pairs [base + blockIdx.x * MEASURE_GROUP, + MEASURE_GROUP) of the batch, cut at `end` (the end of the launch's chunk): the
// workgroup walks them in order and keeps count, bounds and histogram on chip while they belong to one box - what it has
// gathered goes out once per box it meets, not once per pair (a whole-grid box at 1024^3 is 262 144 pairs that all add to the
// same few words).  sign = nullptr: no shortcuts.
__global__ __launch_bounds__(WG) void k_measure_pairs(RecGrid g, const RecBox* boxes, const u64* prefix, u32 count, u64 base, u64 end, const u16* sign,
                                                       MeasureSlot* slots, u64* tallies)
{
	__shared__ u32 sHist[256];
	__shared__ u32 sRed[WG / 64][7];
	const u32 t = threadIdx.x, nb = g.n >> 4;
	u64 pair = base + (u64)blockIdx.x * MEASURE_GROUP;
	const u64 last = pair + MEASURE_GROUP < end ? pair + MEASURE_GROUP : end;
	sHist[t] = 0;
	__syncthreads();
	u32 bi = measure_pair_box(prefix, count, pair);          // (everything that steers the loops is uniform)
	while (pair < last) {
		const RecBox box = boxes[bi];
		const u64 first = prefix[bi], boxEnd = prefix[bi + 1u] < last ? prefix[bi + 1u] : last;
		u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 };
		for (; pair < boxEnd; ++pair) {
			const u32 id = measure_pair_block(box, nb, (u32)(pair - first));
			const u32 summary = sign ? ((u32)sign[id] & 3u) : 0u;
			if (summary == 1u) continue;                      // no sample of the block is negative
			const bool allSolid = summary == 2u && measure_block_inside(box, nb, id);
			const size_t rowAt = rec_grid_row(g.n, id, t);
			u32 mask = allSolid ? 0xFFFFu : measure_clip_mask(box, nb, id, t);
			if (mask && !allSolid) mask &= measure_sign_mask(rec_load16(g.dist + rowAt));
			rec_row_bounds(g.n, id, t, mask, v);
			if (mask) measure_row_materials(rec_load16(g.mat + rowAt), mask, [&](u32 m, u32 voxels) { atomicAdd(&sHist[m], voxels); });
		}
		measure_reduce<1>(v, sRed, t);   // (its barrier also orders the histogram)
		if (t < 7) {
			const u32 a = v[0], solid = sRed[0][6] + sRed[1][6] + sRed[2][6] + sRed[3][6];
			if (solid) {
				if (t < 3) atomicMax(&slots[bi].notMin[t], a);
				else if (t < 6) atomicMax(&slots[bi].max[t - 3], a);
				else atomicAdd(&slots[bi].solid, (u64)a);
			}
		}
		const u32 h = sHist[t];
		if (h) atomicAdd(&tallies[(size_t)bi * 256u + t], (u64)h);
		sHist[t] = 0;
		__syncthreads();                 // the histogram and the waves' partial results are free for the next box
		++bi;
	}
}

// one wave per box
__global__ __launch_bounds__(WG) void k_measure_finish(const RecBox* boxes, u32 count, const MeasureSlot* slots, const u64* tallies, MeasureResult* results)
{
	const u32 lane = threadIdx.x & 63u, bi = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (bi >= count) return; // (a whole wave)
	u32 bins = 0;
#pragma unroll
	for (u32 k = 0; k < 4; ++k) bins += tallies[(size_t)bi * 256u + k * 64u + lane] ? 1u : 0u;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) bins += (u32)__shfl_xor((int)bins, d);
	if (lane == 0) results[bi] = measure_finish(boxes[bi], slots[bi], bins);
}

// One workgroup per REC_GROUP consecutive held blocks, one after the other, a lane per row; everything is kept on chip and goes
// out once per workgroup.  tallies[0..255] removed by the record's material, [256..511] added by the grid's.
__global__ __launch_bounds__(WG) void k_rec_measure(RecGrid g, RecView r, DeltaSlot* slot, u64* tallies)
{
	__shared__ u32 sHist[2][256];
	__shared__ u32 sRed[WG / 64][9];
	__shared__ u32 sBlocks;
	const u32 t = threadIdx.x;
	sHist[0][t] = 0; sHist[1][t] = 0;
	if (t == 0) sBlocks = 0;
	__syncthreads();
	u32 v[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 }; // [6] removed, [7] added, [8] repainted
	const u32 begin = blockIdx.x * REC_GROUP, end = begin + REC_GROUP < r.blocks ? begin + REC_GROUP : r.blocks;
	for (u32 entry = begin; entry < end; ++entry) {            // (uniform)
		const u32 id = r.ids[entry];
		const size_t at = rec_grid_row(g.n, id, t), in = rec_row(entry, t);
		const u32 was = measure_sign_mask(rec_load16(r.dist + in)), is = measure_sign_mask(rec_load16(g.dist + at));
		bool any = false;
		if (was | is) {
			const RecRow rm = rec_load16(r.mat + in), gm = rec_load16(g.mat + at);
			const DeltaRow d = measure_delta_row(was, is, rm, gm);
			rec_row_bounds(g.n, id, t, d.removed | d.added, v);   // (its count of the moved voxels lands in v[6]: overwritten below)
			any = (d.removed | d.added | d.repainted) != 0u;
			v[7] += (u32)__builtin_popcount(d.added); v[8] += (u32)__builtin_popcount(d.repainted);
			measure_row_materials(rm, d.removed, [&](u32 m, u32 voxels) { atomicAdd(&sHist[0][m], voxels); });
			measure_row_materials(gm, d.added, [&](u32 m, u32 voxels) { atomicAdd(&sHist[1][m], voxels); });
		}
		if (__syncthreads_or(any ? 1 : 0) && t == 0) ++sBlocks;
	}
	v[6] -= v[7];                                               // moved = removed + added
	measure_reduce<3>(v, sRed, t);
	if (t < 9) {
		const u32 a = v[0];
		u32 moved = 0;
#pragma unroll
		for (u32 w = 0; w < WG / 64; ++w) moved += sRed[w][6] + sRed[w][7];
		if (moved) {
			if (t < 3) atomicMax(&slot->notMin[t], a);
			else if (t < 6) atomicMax(&slot->max[t - 3], a);
		}
		if (t == 6 && a) atomicAdd(&slot->removed, (u64)a);
		if (t == 7 && a) atomicAdd(&slot->added, (u64)a);
		if (t == 8 && a) atomicAdd(&slot->repainted, (u64)a);
		if (t == 0 && sBlocks) atomicAdd(&slot->blocks, sBlocks);
	}
	const u32 h0 = sHist[0][t], h1 = sHist[1][t];
	if (h0) atomicAdd(&tallies[t], (u64)h0);
	if (h1) atomicAdd(&tallies[256u + t], (u64)h1);
}

} // namespace

extern "C" {

static_assert(sizeof(vx_measure) == 48 && sizeof(vx_record_delta) == 64, "vx_measure / vx_record_delta layout");
static_assert(sizeof(MeasureResult) == sizeof(vx_measure) && sizeof(RecordDelta) == sizeof(vx_record_delta) && sizeof(MeasureSlot) == 32 && sizeof(DeltaSlot) == 56, "tv_measure.h records");
static_assert(VX_MEASURE_MAX_BOXES == tv::MEASURE_MAX_BOXES, "measurement limits");

// test hooks: the pairs per launch of this context's measurements (0 = the default), and whether the sign summaries may stand in
// for distance rows (the default); nothing of a result depends on either
int vx_debug_measure_chunk(vx_ctx* c, uint32_t pairs)
{
	if (!c) return VX_ERR_INVALID;
	module_state<MeasureState>(c, MOD_MEASURE)->chunk = pairs ? std::min<u64>(pairs, 1u << 30) : (u64)MEASURE_CHUNK_PAIRS; // (a launch's workgroup count has a limit of its own)
	return VX_OK;
}

int vx_debug_measure_shortcuts(vx_ctx* c, uint32_t enable)
{
	if (!c) return VX_ERR_INVALID;
	module_state<MeasureState>(c, MOD_MEASURE)->shortcuts = enable != 0;
	return VX_OK;
}

int vx_grid_measure(vx_ctx* c, const vx_box* boxes, uint32_t count, vx_measure* results, uint64_t* outTallies)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_measure: ";
	if (!c) return VX_ERR_INVALID;
	if (!undo_whole_grid(c)) return fail(c, VX_ERR_INVALID, what + "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (const char* bad = measure_check(c->n, (const RecBox*)boxes, count, results)) return fail(c, VX_ERR_INVALID, what + bad);
	if (!count) return VX_OK;

	MeasureState* s = module_state<MeasureState>(c, MOD_MEASURE);
	std::vector<u64> prefix((size_t)count + 1u);
	prefix[0] = 0;
	for (u32 i = 0; i < count; ++i) prefix[i + 1u] = prefix[i] + measure_box_pairs(((const RecBox*)boxes)[i]);
	const u64 pairs = prefix[count];

	// one buffer: boxes | sums | slots, tallies (zeroed together) | results
	auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t atBoxes = 0, atPrefix = pad((size_t)count * sizeof(RecBox)), atSlots = atPrefix + pad(((size_t)count + 1u) * 8u);
	const size_t atTallies = atSlots + pad((size_t)count * sizeof(MeasureSlot)), atResults = atTallies + (size_t)count * 2048u;
	const size_t need = atResults + (size_t)count * sizeof(MeasureResult);
	if (!dev_grow(c, s->buf, s->bufCap, need)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	char* base = (char*)s->buf;
	const RecBox* dBoxes = (const RecBox*)(base + atBoxes);
	const u64* dPrefix = (const u64*)(base + atPrefix);
	MeasureSlot* dSlots = (MeasureSlot*)(base + atSlots);
	u64* dTallies = (u64*)(base + atTallies);
	MeasureResult* dResults = (MeasureResult*)(base + atResults);
	bool ok = c->be.h2d_async(base + atBoxes, boxes, (size_t)count * sizeof(RecBox)) && c->be.h2d_async(base + atPrefix, prefix.data(), ((size_t)count + 1u) * 8u)
	       && c->be.fill(base + atSlots, 0, atResults - atSlots);
	const u16* sign = measure_signs(c, s);
	for (u64 at = 0; at < pairs && ok; at += s->chunk) {
		const u64 end = std::min<u64>(at + s->chunk, pairs);
		const u32 wgs = (u32)((end - at + MEASURE_GROUP - 1u) / MEASURE_GROUP);
		hipLaunchKernelGGL(k_measure_pairs, dim3(wgs), dim3(WG), 0, c->be.stream, undo_grid(c), dBoxes, dPrefix, count, at, end, sign, dSlots, dTallies);
		ok = c->be.check(hipGetLastError(), "k_measure_pairs launch");
	}
	if (ok) {
		hipLaunchKernelGGL(k_measure_finish, dim3((count + WG / 64 - 1) / (WG / 64)), dim3(WG), 0, c->be.stream, dBoxes, count, (const MeasureSlot*)dSlots, (const u64*)dTallies, dResults);
		ok = c->be.check(hipGetLastError(), "k_measure_finish launch");
	}
	ok = ok && c->be.d2h_async(results, dResults, (size_t)count * sizeof(MeasureResult));
	if (outTallies) ok = ok && c->be.d2h_async(outTallies, dTallies, (size_t)count * 2048u);
	if (!ok) { c->be.sync(); return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	if (!c->be.sync_ok()) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); // (the call's one wait)
	return VX_OK;
}

int vx_record_measure(vx_ctx* c, const vx_record* r, vx_record_delta* delta, uint64_t* removed, uint64_t* added)
{
	VX_ENTER(c);
	const std::string what = "vx_record_measure: ";
	if (delta) memset(delta, 0, sizeof(*delta));
	if (!c) return VX_ERR_INVALID;
	if (!delta) return fail(c, VX_ERR_INVALID, what + "null delta");
	if (const char* bad = undo_check(c, r)) return fail(c, VX_ERR_INVALID, what + bad);
	if (removed) memset(removed, 0, 2048);
	if (added) memset(added, 0, 2048);
	if (!r->blocks) return VX_OK;

	MeasureState* s = module_state<MeasureState>(c, MOD_MEASURE);
	const size_t atTallies = 256, bytes = atTallies + 4096u;   // the slot | removed, added
	if (!dev_grow(c, s->buf, s->bufCap, bytes)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	char* base = (char*)s->buf;
	bool ok = c->be.fill(base, 0, bytes);
	if (ok) {
		hipLaunchKernelGGL(k_rec_measure, dim3(rec_groups(r->blocks)), dim3(WG), 0, c->be.stream, undo_grid(c), rec_view(r->mem, r->blocks), (DeltaSlot*)base, (u64*)(base + atTallies));
		ok = c->be.check(hipGetLastError(), "k_rec_measure launch");
	}
	DeltaSlot slot;
	memset(&slot, 0, sizeof(slot));
	ok = ok && c->be.d2h_async(&slot, base, sizeof(slot));
	if (removed) ok = ok && c->be.d2h_async(removed, base + atTallies, 2048);
	if (added) ok = ok && c->be.d2h_async(added, base + atTallies + 2048, 2048);
	if (!ok) { c->be.sync(); return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	if (!c->be.sync_ok()) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); // (the call's one wait)
	const RecordDelta res = measure_delta_finish(slot);
	memcpy(delta, &res, sizeof(res));
	return VX_OK;
}

} // extern "C"
