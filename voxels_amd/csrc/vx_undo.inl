// vx_undo.inl — the undo records (include/voxels_hip.h, "undo records"): capture, trim and swap of whole 16^3 blocks of the
// resident grid; included by vx_hip.hip after vx_host.inl (HIP only).  DESIGN.md §20.  The per-lane logic and the tiling of the
// copy passes are tv_undo.h, shared with the host build of the tests.
//
//   k_rec_mark     one workgroup row per box, lanes over the x-runs of the blocks the box intersects: one bit per grid block,
//                  one atomicOr per bitmap word a run reaches
//   k_rec_scan     one workgroup: the set bits below every word of a bitmap and their total (popcounts, wave scan)
//   -- the host reads the total: it sizes the allocation --
//   k_rec_list     one lane per word: the ascending list of the set bits (nothing depends on which atomic was served first)
//   k_rec_capture  the dense fields and the flag bytes of the listed blocks into the record
//   k_rec_diff     one bit per entry: does it differ from the grid (a ballot over the lanes' row compares) - the bitmap that
//                  k_rec_scan and k_rec_list turn into the list of the entries a trim keeps
//   k_rec_pack     the kept entries into the new allocation, in order
//   k_rec_swap     the exchange; the differing voxels' bounds and count, the changed blocks and flags, reduced per wave and per
//                  workgroup, then one set of integer atomics per workgroup
// All copy passes: one workgroup per group of 8 consecutive entries, 16-byte loads and stores (tv_undo.h).
#include "tv_undo.h"

struct vx_record {
	vx_ctx* owner = nullptr;
	u32 n = 0, blocks = 0, swaps = 0;
	void* mem = nullptr;            // tv::rec_view(mem, blocks)
	size_t bytes = 0;
	bool boundsKnown = false;       // min / max below describe the held blocks (found by vx_record_info_get from the ids)
	u32 min[3] = { 0, 0, 0 }, max[3] = { 0, 0, 0 };
};

namespace {

struct UndoState {
	std::vector<vx_record*> records;
	void* bits = nullptr;      // a bitmap (grid blocks of a capture | entries of a trim), then its prefix sums
	size_t bitsCap = 0;
	void* list = nullptr;      // the boxes of a capture | the kept entries of a trim
	size_t listCap = 0;
	void* slot = nullptr;      // RecSwapSlot
	std::vector<void*> retired; // allocations a trim replaced while its copy out of them was still queued (undo_release)

	void release(vx_ctx* c)
	{
		for (vx_record* r : records) { c->be.free(r->mem); delete r; }
		for (void* p : retired) c->be.free(p);
		c->be.free(bits); c->be.free(list); c->be.free(slot);
	}
};

// behind a wait for the stream: what a trim retired is no longer read
void undo_release(vx_ctx* c, UndoState* s)
{
	for (void* p : s->retired) c->be.free(p);
	s->retired.clear();
}

// (these two are also used by vx_stamp.inl and vx_measure.inl)
bool undo_whole_grid(const vx_ctx* c) { return c->ownsGrid && c->n && c->zBegin == 0 && c->zEnd == c->n && c->yBegin == 0 && c->yEnd == c->n; }

RecGrid undo_grid(const vx_ctx* c)
{
	RecGrid g;
	g.dist = (u8*)c->dDist; g.mat = (u8*)c->dMat; g.blend = (u8*)c->dBlend; g.flags = (u8*)c->dFlags;
	g.n = c->n;
	return g;
}

// nullptr = the record may be used with the context's grid as it is now
const char* undo_check(const vx_ctx* c, const vx_record* r)
{
	if (!r) return "null record";
	if (r->owner != c) return "the record belongs to another context";
	if (!undo_whole_grid(c)) return "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)";
	if (r->n != c->n) return "the record was captured from a grid of another size";
	return nullptr;
}

__global__ __launch_bounds__(WG) void k_rec_mark(const RecBox* boxes, u32 nb, u32* bits)
{
	const RecBox b = boxes[blockIdx.x];
	const u32 runs = rec_box_runs(b), length = rec_box_run_length(b);
	for (u32 q = blockIdx.y * WG + threadIdx.x; q < runs; q += gridDim.y * WG)
		rec_mark_run(rec_box_run(b, nb, q), length, [bits](u32 word, u32 mask) { atomicOr(&bits[word], mask); });
}

// prefix[w] = the set bits of the words below w; prefix[words] = all of them.  One workgroup.
__global__ __launch_bounds__(WG) void k_rec_scan(const u32* bits, u32 words, u32* prefix)
{
	__shared__ u32 sWave[WG / 64];
	const u32 t = threadIdx.x;
	u32 carry = 0; // (uniform)
	for (u32 base = 0; base < words; base += WG) {
		const u32 w = base + t;
		const u32 cnt = w < words ? (u32)__builtin_popcount(bits[w]) : 0u;
		const u32 incl = wave_inclusive_scan(cnt);
		if ((t & 63u) == 63u) sWave[t >> 6] = incl;
		__syncthreads();
		u32 before = 0, total = 0;
#pragma unroll
		for (u32 k = 0; k < WG / 64; ++k) { const u32 s = sWave[k]; before += k < (t >> 6) ? s : 0u; total += s; }
		if (w < words) prefix[w] = carry + before + incl - cnt;
		carry += total;
		__syncthreads(); // the wave totals are rewritten by the next round
	}
	if (t == 0) prefix[words] = carry;
}

__global__ __launch_bounds__(WG) void k_rec_list(const u32* bits, const u32* prefix, u32 words, u32* out)
{
	const u32 w = blockIdx.x * WG + threadIdx.x;
	if (w < words) rec_list_word(bits[w], w, prefix[w], out);
}

__global__ __launch_bounds__(WG) void k_rec_capture(RecGrid g, RecView r)
{
	const u32 t = threadIdx.x, entry = blockIdx.x * REC_GROUP + rec_lane_entry(t);
	if (entry >= r.blocks) return;
	const u32 id = r.ids[entry];
#pragma unroll 2
	for (u32 step = 0; step < REC_STEPS; ++step) rec_capture_row(g, r, entry, id, rec_lane_row(t, step));
	if (t < REC_GROUP) r.flags[entry] = g.flags[id];
}

// bit e of the 8 low bits: does one of the lanes of entry e (lane & 7 == e) of this wave say yes
__device__ __forceinline__ u32 rec_entry_ballot(bool yes)
{
	unsigned long long m = __ballot(yes);
	m |= m >> 32; m |= m >> 16; m |= m >> 8;
	return (u32)(m & 0xFFu);
}

// keep8[group]: bit e set where entry group * 8 + e differs from the grid - read as u32 words it is the bitmap of the entries
__global__ __launch_bounds__(WG) void k_rec_diff(RecGrid g, RecView r, u8* keep8)
{
	__shared__ u32 sAny;
	const u32 t = threadIdx.x, entry = blockIdx.x * REC_GROUP + rec_lane_entry(t);
	if (t == 0) sAny = 0;
	__syncthreads();
	bool differs = false;
	if (entry < r.blocks) {
		const u32 id = r.ids[entry];
#pragma unroll 2
		for (u32 step = 0; step < REC_STEPS; ++step) differs = rec_differs_row(g, r, entry, id, rec_lane_row(t, step)) || differs;
		if (t < REC_GROUP) differs = differs || g.flags[id] != r.flags[entry];
	}
	const u32 any = rec_entry_ballot(differs);
	if ((t & 63u) == 0 && any) atomicOr(&sAny, any);
	__syncthreads();
	if (t == 0) keep8[blockIdx.x] = (u8)sAny;
}

__global__ __launch_bounds__(WG) void k_rec_pack(RecView src, RecView dst, const u32* kept)
{
	const u32 t = threadIdx.x, to = blockIdx.x * REC_GROUP + rec_lane_entry(t);
	if (to >= dst.blocks) return;
	const u32 from = kept[to];
#pragma unroll 2
	for (u32 step = 0; step < REC_STEPS; ++step) rec_pack_row(src, dst, from, to, rec_lane_row(t, step));
	if (t < REC_GROUP) rec_pack_entry(src, dst, from, to);
}

__global__ __launch_bounds__(WG) void k_rec_swap(RecGrid g, RecView r, RecSwapSlot* slot)
{
	__shared__ u32 sRed[WG / 64][7];
	__shared__ u32 sAny;
	const u32 t = threadIdx.x, entry = blockIdx.x * REC_GROUP + rec_lane_entry(t);
	const bool held = entry < r.blocks;
	if (t == 0) sAny = 0;
	__syncthreads();
	// [0..2] ~min, [3..5] max, [6] count: zeros where nothing differed, all combined by max / sum
	u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 };
	const u32 id = held ? r.ids[entry] : 0u;
	if (held) {
#pragma unroll 2
		for (u32 step = 0; step < REC_STEPS; ++step) {
			const u32 row = rec_lane_row(t, step);
			rec_row_bounds(g.n, id, row, rec_swap_row(g, r, entry, id, row), v);
		}
	}
	const u32 any = rec_entry_ballot(v[6] != 0u);
	if ((t & 63u) == 0 && any) atomicOr(&sAny, any);
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
		for (int k = 0; k < 6; ++k) v[k] = max(v[k], (u32)__shfl_xor((int)v[k], d));
		v[6] += (u32)__shfl_xor((int)v[6], d);
	}
	if ((t & 63u) == 0) {
#pragma unroll
		for (int k = 0; k < 7; ++k) sRed[t >> 6][k] = v[k];
	}
	__syncthreads();
	if (t < 64) { // (the first wave, whole: the ballots below count over its lanes)
		const bool flagDiffers = t < REC_GROUP && held && rec_swap_flag(g, r, entry, id);
		const bool blockChanged = t < REC_GROUP && held && (((sAny >> t) & 1u) || flagDiffers);
		const u32 nFlags = (u32)__popcll(__ballot(flagDiffers)), nBlocks = (u32)__popcll(__ballot(blockChanged));
		if (t == 0 && nBlocks) atomicAdd(&slot->blocks, nBlocks);
		if (t == 0 && nFlags) atomicAdd(&slot->flagChanges, nFlags);
		if (t < 7) {
			u32 a = sRed[0][t], count = sRed[0][6];
#pragma unroll
			for (u32 w = 1; w < WG / 64; ++w) { a = t < 6 ? max(a, sRed[w][t]) : a + sRed[w][t]; count += sRed[w][6]; }
			if (count) {
				if (t < 3) atomicMax(&slot->notMin[t], a);
				else if (t < 6) atomicMax(&slot->max[t - 3], a);
				else atomicAdd(&slot->changed, (unsigned long long)a);
			}
		}
	}
}

u32 rec_groups(u32 blocks) { return (blocks + REC_GROUP - 1u) / REC_GROUP; }

// a bitmap of `bitCount` bits at s->bits, zeroed, with room for its prefix sums behind it
bool undo_bitmap(vx_ctx* c, UndoState* s, size_t bitCount, u32*& bits, u32*& prefix, u32& words)
{
	words = (u32)((bitCount + 31u) / 32u);
	if (!dev_grow(c, s->bits, s->bitsCap, ((size_t)words * 2u + 1u) * 4u)) return false;
	bits = (u32*)s->bits; prefix = bits + words;
	return c->be.fill(bits, 0, (size_t)words * 4u);
}

} // namespace

extern "C" {

static_assert(sizeof(vx_box) == 24 && sizeof(vx_record_info) == 48 && sizeof(vx_swap_result) == 48, "vx_box / vx_record_info / vx_swap_result layout");
static_assert(sizeof(RecBox) == sizeof(vx_box) && sizeof(RecSwapResult) == sizeof(vx_swap_result) && sizeof(RecSwapSlot) == 40, "tv_undo.h records");
static_assert(VX_RECORD_MAX_BLOCKS == tv::REC_MAX_BLOCKS && VX_RECORD_MAX_BOXES == tv::REC_MAX_BOXES && WG == (int)tv::REC_LANES, "undo record limits");

int vx_grid_capture(vx_ctx* c, const vx_box* boxes, uint32_t count, vx_record** out)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_capture: ";
	if (out) *out = nullptr;
	if (!c) return VX_ERR_INVALID;
	if (!out) return fail(c, VX_ERR_INVALID, what + "null out pointer");
	if (!undo_whole_grid(c)) return fail(c, VX_ERR_INVALID, what + "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (const char* bad = rec_check_boxes(c->n, (const RecBox*)boxes, count)) return fail(c, VX_ERR_INVALID, what + bad);

	UndoState* s = module_state<UndoState>(c, MOD_UNDO);
	vx_record* r = new vx_record();
	r->owner = c; r->n = c->n;
	auto keep = [&]() { s->records.push_back(r); *out = r; return VX_OK; };
	if (!count) return keep();

	const u32 nb = c->n / 16;
	hipStream_t st = c->be.stream;
	auto noMemory = [&]() { delete r; return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error()); };
	auto deviceFailed = [&]() { c->be.free(r->mem); delete r; return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); };
	u32 *bits, *prefix, words;
	if (!dev_grow(c, s->list, s->listCap, (size_t)count * sizeof(RecBox)) || !undo_bitmap(c, s, (size_t)nb * nb * nb, bits, prefix, words)) return noMemory();
	if (!c->be.h2d(s->list, boxes, (size_t)count * sizeof(RecBox))) return deviceFailed();
	u32 most = 0;
	for (u32 i = 0; i < count; ++i) most = std::max(most, rec_box_runs(((const RecBox*)boxes)[i]));
	const u32 chunks = std::min<u32>((most + WG - 1) / WG, 64u); // (lanes over the runs of the largest box)
	hipLaunchKernelGGL(k_rec_mark, dim3(count, chunks), dim3(WG), 0, st, (const RecBox*)s->list, nb, bits);
	hipLaunchKernelGGL(k_rec_scan, dim3(1), dim3(WG), 0, st, (const u32*)bits, words, prefix);
	u32 blocks = 0;
	if (!c->be.check(hipGetLastError(), "k_rec_mark launch") || !c->be.d2h(&blocks, prefix + words, 4)) return deviceFailed(); // (waits: the count sizes the allocation)
	undo_release(c, s);
	if (blocks > VX_RECORD_MAX_BLOCKS) { delete r; return fail(c, VX_ERR_INVALID, what + "more than VX_RECORD_MAX_BLOCKS distinct blocks"); }

	r->bytes = rec_bytes(blocks);
	r->mem = c->be.alloc(r->bytes);
	if (!r->mem) return noMemory();
	r->blocks = blocks;
	const RecView v = rec_view(r->mem, blocks);
	hipLaunchKernelGGL(k_rec_list, dim3((words + WG - 1) / WG), dim3(WG), 0, st, (const u32*)bits, (const u32*)prefix, words, v.ids);
	hipLaunchKernelGGL(k_rec_capture, dim3(rec_groups(blocks)), dim3(WG), 0, st, undo_grid(c), v);
	if (!c->be.check(hipGetLastError(), "k_rec_capture launch")) return deviceFailed();
	return keep();
}

int vx_record_trim(vx_ctx* c, vx_record* r, uint32_t* dropped)
{
	VX_ENTER(c);
	const std::string what = "vx_record_trim: ";
	if (dropped) *dropped = 0;
	if (!c) return VX_ERR_INVALID;
	if (const char* bad = undo_check(c, r)) return fail(c, VX_ERR_INVALID, what + bad);
	if (!r->blocks) return VX_OK;

	UndoState* s = module_state<UndoState>(c, MOD_UNDO);
	hipStream_t st = c->be.stream;
	const u32 groups = rec_groups(r->blocks);
	u32 *bits, *prefix, words;
	// (one bit per entry, written a byte per group: the bitmap has a byte for every group)
	if (!undo_bitmap(c, s, (size_t)groups * 8u, bits, prefix, words) || !dev_grow(c, s->list, s->listCap, (size_t)r->blocks * 4u))
		return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	auto deviceFailed = [&]() { return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); };
	const RecView old = rec_view(r->mem, r->blocks);
	hipLaunchKernelGGL(k_rec_diff, dim3(groups), dim3(WG), 0, st, undo_grid(c), old, (u8*)bits);
	hipLaunchKernelGGL(k_rec_scan, dim3(1), dim3(WG), 0, st, (const u32*)bits, words, prefix);
	u32 kept = 0;
	if (!c->be.check(hipGetLastError(), "k_rec_diff launch") || !c->be.d2h(&kept, prefix + words, 4)) return deviceFailed(); // (waits: the count sizes the new allocation)
	undo_release(c, s);
	if (kept == r->blocks) return VX_OK;

	void* mem = nullptr;
	if (kept) {
		mem = c->be.alloc(rec_bytes(kept));
		if (!mem) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
		hipLaunchKernelGGL(k_rec_list, dim3((words + WG - 1) / WG), dim3(WG), 0, st, (const u32*)bits, (const u32*)prefix, words, (u32*)s->list);
		hipLaunchKernelGGL(k_rec_pack, dim3(rec_groups(kept)), dim3(WG), 0, st, old, rec_view(mem, kept), (const u32*)s->list);
		if (!c->be.check(hipGetLastError(), "k_rec_pack launch")) { s->retired.push_back(mem); return deviceFailed(); }
		s->retired.push_back(r->mem); // (the copy out of it is queued: released behind the next wait of an undo call, or with the context)
	} else {
		c->be.free(r->mem);
	}
	if (dropped) *dropped = r->blocks - kept;
	r->mem = mem; r->blocks = kept; r->bytes = kept ? rec_bytes(kept) : 0;
	r->boundsKnown = false;
	return VX_OK;
}

int vx_record_swap(vx_ctx* c, vx_record* r, vx_swap_result* result)
{
	VX_ENTER(c);
	const std::string what = "vx_record_swap: ";
	if (result) memset(result, 0, sizeof(*result));
	if (!c) return VX_ERR_INVALID;
	if (const char* bad = undo_check(c, r)) return fail(c, VX_ERR_INVALID, what + bad);
	if (!r->blocks) { ++r->swaps; return VX_OK; }

	UndoState* s = module_state<UndoState>(c, MOD_UNDO);
	if (!s->slot && !(s->slot = c->be.alloc(sizeof(RecSwapSlot)))) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	const RecView v = rec_view(r->mem, r->blocks);
	bool ok = c->be.fill(s->slot, 0, sizeof(RecSwapSlot));
	if (ok) {
		hipLaunchKernelGGL(k_rec_swap, dim3(rec_groups(r->blocks)), dim3(WG), 0, c->be.stream, undo_grid(c), v, (RecSwapSlot*)s->slot);
		ok = c->be.check(hipGetLastError(), "k_rec_swap launch");
	}
	// The mirrors follow as after any edit, queued before the call's one wait.  What rebrick_blocks marks on the host - the
	// material store invalid, the cell map stale - holds only where a byte or a flag changed: the wait's result says so, and
	// a swap that exchanged equal bytes (the mirrors were rewritten with what they held) puts both marks back.
	const bool storeValid = c->matStoreValid, mapStale = c->cellMapStale;
	if (ok) rebrick_blocks(c, v.ids, r->blocks);
	RecSwapSlot slot;
	memset(&slot, 0, sizeof(slot));
	ok = ok && c->be.d2h(&slot, s->slot, sizeof(slot));
	if (!ok) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error());
	undo_release(c, s);
	if (!slot.blocks) { c->matStoreValid = storeValid; c->cellMapStale = mapStale; }
	++r->swaps;
	const RecSwapResult res = rec_swap_result(c->n, slot);
	if (result) memcpy(result, &res, sizeof(res));
	return VX_OK;
}

int vx_record_info_get(vx_ctx* c, const vx_record* cr, vx_record_info* info)
{
	VX_ENTER(c);
	const std::string what = "vx_record_info_get: ";
	if (info) memset(info, 0, sizeof(*info));
	if (!c) return VX_ERR_INVALID;
	if (!cr || !info) return fail(c, VX_ERR_INVALID, what + "null argument");
	if (cr->owner != c) return fail(c, VX_ERR_INVALID, what + "the record belongs to another context");
	vx_record* r = const_cast<vx_record*>(cr);
	if (r->blocks && !r->boundsKnown) {
		std::vector<u32> ids(r->blocks);
		if (!c->be.d2h(ids.data(), rec_view(r->mem, r->blocks).ids, (size_t)r->blocks * 4u)) return fail(c, VX_ERR_DEVICE, what + "copy failed: " + c->be.error());
		const u32 nb = r->n / 16;
		for (int k = 0; k < 3; ++k) { r->min[k] = nb; r->max[k] = 0; }
		for (u32 id : ids) {
			const u32 b[3] = { id % nb, (id / nb) % nb, id / (nb * nb) };
			for (int k = 0; k < 3; ++k) { r->min[k] = std::min(r->min[k], b[k]); r->max[k] = std::max(r->max[k], b[k]); }
		}
		r->boundsKnown = true;
	}
	info->n = r->n; info->blocks = r->blocks; info->bytes = r->bytes; info->swaps = r->swaps;
	for (int k = 0; k < 3; ++k) { info->min[k] = r->blocks ? r->min[k] : 0; info->max[k] = r->blocks ? r->max[k] : 0; }
	return VX_OK;
}

int vx_record_block_ids(vx_ctx* c, const vx_record* r, uint32_t* ids, uint32_t capacity)
{
	VX_ENTER(c);
	const std::string what = "vx_record_block_ids: ";
	if (!c) return VX_ERR_INVALID;
	if (!r) return fail(c, VX_ERR_INVALID, what + "null record");
	if (r->owner != c) return fail(c, VX_ERR_INVALID, what + "the record belongs to another context");
	if (capacity < r->blocks || (r->blocks && !ids)) return fail(c, VX_ERR_INVALID, what + "the array is smaller than the record's block count");
	if (!r->blocks) return VX_OK;
	return c->be.d2h(ids, rec_view(r->mem, r->blocks).ids, (size_t)r->blocks * 4u) ? VX_OK : fail(c, VX_ERR_DEVICE, what + "copy failed: " + c->be.error());
}

int vx_record_read_block(vx_ctx* c, const vx_record* r, uint32_t index, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* empty_flag)
{
	VX_ENTER(c);
	const std::string what = "vx_record_read_block: ";
	if (!c) return VX_ERR_INVALID;
	if (!r) return fail(c, VX_ERR_INVALID, what + "null record");
	if (r->owner != c) return fail(c, VX_ERR_INVALID, what + "the record belongs to another context");
	if (index >= r->blocks) return fail(c, VX_ERR_INVALID, what + "index out of range");
	const RecView v = rec_view(r->mem, r->blocks);
	const size_t at = rec_row(index, 0);
	bool ok = true;
	if (dist) ok = ok && c->be.d2h_async(dist, v.dist + at, 4096);
	if (mat) ok = ok && c->be.d2h_async(mat, v.mat + at, 4096);
	if (blend) ok = ok && c->be.d2h_async(blend, v.blend + at, 4096);
	if (empty_flag) ok = ok && c->be.d2h_async(empty_flag, v.flags + index, 1);
	ok = ok && c->be.sync_ok();
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, what + "copy failed: " + c->be.error());
}

void vx_record_free(vx_ctx* c, vx_record* r)
{
	VX_ENTER(c);
	if (!c || !r || r->owner != c || !module_peek<UndoState>(c, MOD_UNDO)) return;
	UndoState* s = module_peek<UndoState>(c, MOD_UNDO);
	auto it = std::find(s->records.begin(), s->records.end(), r);
	if (it == s->records.end()) return;
	s->records.erase(it);
	c->be.sync(); // (a capture or a swap of the record may still be queued)
	c->be.free(r->mem);
	delete r;
}

int vx_brush_box(const vx_brush* brush, uint32_t n, vx_box* out)
{
	if (out) memset(out, 0, sizeof(*out));
	if (!brush || !out || !n || n % 16u || n > (u32)VX_MAX_GRID) return VX_ERR_INVALID;
	return rec_brush_box(brush->position, brush->extents, n, (RecBox*)out);
}

} // extern "C"
