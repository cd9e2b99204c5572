// undo_host.cpp — host side of the tests of the undo records (tests only; built by voxels_amd/build.py build_undo_host()).
//
// voxels_amd/csrc/tv_undo.h compiled for the host behind one C interface: the pipeline of vx_undo.inl - mark, scan, list,
// capture, diff, pack, swap - with the lanes of a workgroup as loops and the launches in their order, so the tiling of the copy
// passes, the bitmaps and the reductions are testable where there is no GPU.
//   uh_capture   boxes -> a record (caller's arrays, `capacity` blocks of room); returns the block count, or what
//                vx_grid_capture returns for bad arguments (everything but the context)
//   uh_trim      a record against the grid -> the kept count; the record's arrays are packed in place
//   uh_swap      grid and record exchanged in place; the result record
//   uh_check     the entry check of vx_grid_capture alone
//   uh_brush_box vx_brush_box
//   uh_layout    sizes and offsets of the header's structs as this compiler lays them out
// A grid is dist / mat / blend (n^3 bytes each, x fastest, Z up) and flags ((n / 16)^3 bytes); a record is ids, then dist / mat /
// blend of 4096 bytes per block (rows z-major, as vx_grid_read_block), then one flag byte per block.
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_undo.h"

using namespace tv;

namespace {

// k_rec_scan
void scan(const std::vector<u32>& bits, std::vector<u32>& prefix)
{
	prefix.assign(bits.size() + 1, 0);
	for (size_t w = 0; w < bits.size(); ++w) prefix[w + 1] = prefix[w] + (u32)__builtin_popcount(bits[w]);
}

// the record as one allocation of tv_undo.h's layout (uint64 elements: the rows are 16-byte aligned after the round-up)
struct Mem {
	std::vector<uint64_t> store;
	RecView view;
	explicit Mem(u32 blocks) : store(rec_bytes(blocks) / 8 + 4, 0) { view = rec_view((void*)(((uintptr_t)store.data() + 15) & ~(uintptr_t)15), blocks); }
};

void load(Mem& m, const u32* ids, const u8* dist, const u8* mat, const u8* blend, const u8* flags)
{
	const u32 b = m.view.blocks;
	if (!b) return;
	memcpy(m.view.ids, ids, (size_t)b * 4); memcpy(m.view.dist, dist, (size_t)b * 4096); memcpy(m.view.mat, mat, (size_t)b * 4096);
	memcpy(m.view.blend, blend, (size_t)b * 4096); memcpy(m.view.flags, flags, b);
}

void store(const Mem& m, u32* ids, u8* dist, u8* mat, u8* blend, u8* flags)
{
	const u32 b = m.view.blocks;
	if (!b) return;
	memcpy(ids, m.view.ids, (size_t)b * 4); memcpy(dist, m.view.dist, (size_t)b * 4096); memcpy(mat, m.view.mat, (size_t)b * 4096);
	memcpy(blend, m.view.blend, (size_t)b * 4096); memcpy(flags, m.view.flags, b);
}

RecGrid grid(uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* flags)
{
	RecGrid g;
	g.dist = (u8*)dist; g.mat = mat; g.blend = blend; g.flags = flags; g.n = n;
	return g;
}

u32 groups_of(u32 blocks) { return (blocks + REC_GROUP - 1u) / REC_GROUP; }

} // namespace

extern "C" {

int uh_check(uint32_t n, const vx_box* boxes, uint32_t count) { return rec_check_boxes(n, (const RecBox*)boxes, count) ? VX_ERR_INVALID : VX_OK; }

int uh_capture(uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* flags, const vx_box* boxes, uint32_t count,
               uint32_t capacity, uint32_t* ids, uint8_t* rdist, uint8_t* rmat, uint8_t* rblend, uint8_t* rflags)
{
	if (rec_check_boxes(n, (const RecBox*)boxes, count)) return VX_ERR_INVALID;
	const u32 nb = n / 16;
	const RecGrid g = grid(n, dist, mat, blend, flags);
	std::vector<u32> bits(((size_t)nb * nb * nb + 31) / 32, 0), prefix;
	// k_rec_mark
	for (u32 i = 0; i < count; ++i) {
		const RecBox b = ((const RecBox*)boxes)[i];
		for (u32 q = 0; q < rec_box_runs(b); ++q) rec_mark_run(rec_box_run(b, nb, q), rec_box_run_length(b), [&](u32 word, u32 mask) { bits[word] |= mask; });
	}
	scan(bits, prefix);
	const u32 blocks = prefix.back();
	if (blocks > VX_RECORD_MAX_BLOCKS || blocks > capacity) return VX_ERR_INVALID;
	Mem m(blocks);
	// k_rec_list
	for (u32 w = 0; w < (u32)bits.size(); ++w) rec_list_word(bits[w], w, prefix[w], m.view.ids);
	// k_rec_capture
	for (u32 group = 0; group < groups_of(blocks); ++group)
	for (u32 t = 0; t < REC_LANES; ++t) {
		const u32 entry = group * REC_GROUP + rec_lane_entry(t);
		if (entry >= blocks) continue;
		const u32 id = m.view.ids[entry];
		for (u32 step = 0; step < REC_STEPS; ++step) rec_capture_row(g, m.view, entry, id, rec_lane_row(t, step));
		if (t < REC_GROUP) m.view.flags[entry] = g.flags[id];
	}
	store(m, ids, rdist, rmat, rblend, rflags);
	return (int)blocks;
}

int uh_trim(uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* flags, uint32_t blocks, uint32_t* ids, uint8_t* rdist,
            uint8_t* rmat, uint8_t* rblend, uint8_t* rflags)
{
	const RecGrid g = grid(n, dist, mat, blend, flags);
	Mem old(blocks);
	load(old, ids, rdist, rmat, rblend, rflags);
	const u32 groups = groups_of(blocks);
	std::vector<u32> bits(((size_t)groups * 8 + 31) / 32, 0), prefix;
	// k_rec_diff: a byte per group
	for (u32 group = 0; group < groups; ++group) {
		u32 any = 0;
		for (u32 t = 0; t < REC_LANES; ++t) {
			const u32 entry = group * REC_GROUP + rec_lane_entry(t);
			if (entry >= blocks) continue;
			const u32 id = old.view.ids[entry];
			bool differs = false;
			for (u32 step = 0; step < REC_STEPS; ++step) differs = rec_differs_row(g, old.view, entry, id, rec_lane_row(t, step)) || differs;
			if (t < REC_GROUP) differs = differs || g.flags[id] != old.view.flags[entry];
			if (differs) any |= 1u << rec_lane_entry(t);
		}
		((u8*)bits.data())[group] = (u8)any;
	}
	scan(bits, prefix);
	const u32 kept = prefix.back();
	if (kept == blocks) return (int)kept;
	std::vector<u32> list(kept + 1);
	// k_rec_list
	for (u32 w = 0; w < (u32)bits.size(); ++w) rec_list_word(bits[w], w, prefix[w], list.data());
	Mem fresh(kept);
	// k_rec_pack
	for (u32 group = 0; group < groups_of(kept); ++group)
	for (u32 t = 0; t < REC_LANES; ++t) {
		const u32 to = group * REC_GROUP + rec_lane_entry(t);
		if (to >= kept) continue;
		const u32 from = list[to];
		for (u32 step = 0; step < REC_STEPS; ++step) rec_pack_row(old.view, fresh.view, from, to, rec_lane_row(t, step));
		if (t < REC_GROUP) rec_pack_entry(old.view, fresh.view, from, to);
	}
	store(fresh, ids, rdist, rmat, rblend, rflags);
	return (int)kept;
}

int uh_swap(uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* flags, uint32_t blocks, uint32_t* ids, uint8_t* rdist,
            uint8_t* rmat, uint8_t* rblend, uint8_t* rflags, vx_swap_result* result)
{
	const RecGrid g = grid(n, dist, mat, blend, flags);
	Mem m(blocks);
	load(m, ids, rdist, rmat, rblend, rflags);
	RecSwapSlot slot;
	memset(&slot, 0, sizeof(slot));
	// k_rec_swap
	for (u32 group = 0; group < groups_of(blocks); ++group) {
		u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 }, any = 0;
		for (u32 t = 0; t < REC_LANES; ++t) {
			const u32 entry = group * REC_GROUP + rec_lane_entry(t);
			if (entry >= blocks) continue;
			const u32 id = m.view.ids[entry], before = v[6];
			for (u32 step = 0; step < REC_STEPS; ++step) {
				const u32 row = rec_lane_row(t, step);
				rec_row_bounds(n, id, row, rec_swap_row(g, m.view, entry, id, row), v);
			}
			if (v[6] != before) any |= 1u << rec_lane_entry(t);
		}
		for (u32 t = 0; t < REC_GROUP; ++t) {
			const u32 entry = group * REC_GROUP + t;
			if (entry >= blocks) continue;
			const bool flagDiffers = rec_swap_flag(g, m.view, entry, m.view.ids[entry]);
			if (flagDiffers) ++slot.flagChanges;
			if (((any >> t) & 1u) || flagDiffers) ++slot.blocks;
		}
		if (v[6]) {
			for (int k = 0; k < 3; ++k) { if (v[k] > slot.notMin[k]) slot.notMin[k] = v[k]; if (v[3 + k] > slot.max[k]) slot.max[k] = v[3 + k]; }
			slot.changed += v[6];
		}
	}
	store(m, ids, rdist, rmat, rblend, rflags);
	const RecSwapResult r = rec_swap_result(n, slot);
	static_assert(sizeof(RecSwapResult) == sizeof(vx_swap_result), "tv_undo.h records");
	if (result) memcpy(result, &r, sizeof(r));
	return VX_OK;
}

int uh_brush_box(const vx_brush* brush, uint32_t n, vx_box* out) { return rec_brush_box(brush->position, brush->extents, n, (RecBox*)out); }

// which: 0 = sizes of vx_box, vx_record_info, vx_swap_result, vx_brush; 1 = offsets inside vx_record_info; 2 = inside vx_swap_result
uint32_t uh_layout(uint32_t which, uint32_t* out)
{
	if (which == 0) { const uint32_t v[] = { sizeof(vx_box), sizeof(vx_record_info), sizeof(vx_swap_result), sizeof(vx_brush), offsetof(vx_box, hi) }; memcpy(out, v, sizeof(v)); return 5; }
	if (which == 1) {
		const uint32_t v[] = { offsetof(vx_record_info, n), offsetof(vx_record_info, blocks), offsetof(vx_record_info, bytes), offsetof(vx_record_info, min),
		                       offsetof(vx_record_info, max), offsetof(vx_record_info, swaps), offsetof(vx_record_info, reserved) };
		memcpy(out, v, sizeof(v)); return 7;
	}
	const uint32_t v[] = { offsetof(vx_swap_result, out_min), offsetof(vx_swap_result, out_max), offsetof(vx_swap_result, changed_voxels),
	                       offsetof(vx_swap_result, changed_blocks), offsetof(vx_swap_result, flag_changes), offsetof(vx_swap_result, reserved) };
	memcpy(out, v, sizeof(v)); return 6;
}

uint32_t uh_limit(uint32_t which) { return which == 0 ? VX_RECORD_MAX_BLOCKS : VX_RECORD_MAX_BOXES; }

} // extern "C"
