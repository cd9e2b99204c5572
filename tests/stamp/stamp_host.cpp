// stamp_host.cpp — host side of the tests of the stamps (tests only; built by voxels_amd/build.py build_stamp_host()).
//
// voxels_amd/csrc/tv_stamp.h compiled for the host behind one C interface, with two paths through a paste batch:
//   path 0   a plain sequential loop: paste after paste, voxel after voxel of its clipped box, then the flags of the blocks that
//            a paste other than PAINT touched, and the counts from a copy of the grid taken before
//   path 1   the pipeline of vx_stamp.inl - plan, count, offsets, fill, sort, per-block apply from a tile, flags, comparison,
//            snapshots of the blocks that several chunks touch - with the lanes of a workgroup as loops and the launches in their
//            order.  `list_cap` is the capacity of the (paste, block) lists, so that chunking happens at small sizes, and `seed`
//            permutes the order in which the binning's counters are served (slots and list positions are only places).
//   sh_check*    the entry checks          sh_paste_box   vx_paste_box's arithmetic
//   sh_layout    sizes and offsets of the header's structs as this compiler lays them out; sh_limit the limits
// A grid is dist / mat / blend (n^3 bytes each, x fastest, Z up) and flags ((n / 16)^3 bytes); stamp i is bases[i]: three fields of
// sizes[i] voxels each, one after the other (sizes[i][0] == 0: a null entry, bases[i] unused).
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_stamp.h"

using namespace tv;

namespace {

typedef const u32 (*Sizes)[3];

struct Lcg {
	uint64_t s;
	u32 next(u32 bound) { s = s * 6364136223846793005ull + 1442695040888963407ull; return (u32)((s >> 33) % bound); }
};

void plain(u32 n, u8* dist, u8* mat, u8* blend, u8* flags, const u8* const* bases, Sizes sizes, const Paste* pastes, u32 count,
           PasteResult* results, PasteCounts* counts)
{
	const u32 nb = n / 16;
	const size_t V = (size_t)n * n * n;
	const std::vector<u8> d0(dist, dist + V), m0(mat, mat + V), b0(blend, blend + V);
	std::vector<u8> touched((size_t)nb * nb * nb, 0); // 1 = touched, 2 = by a paste other than PAINT
	for (u32 i = 0; i < count; ++i) {
		const Paste& p = pastes[i];
		const u32* size = sizes[p.stamp];
		RecBox box;
		const int hit = paste_box(p, size, n, &box);
		if (results) { results[i].box = box; results[i].touched_blocks = hit ? paste_box_block_count(box) : 0u; results[i].reserved = 0; }
		if (!hit) continue;
		const PasteMap map = paste_map(p.orient, size[0], size[1]);
		const size_t voxels = stamp_voxels(size);
		for (u32 z = box.lo[2]; z < box.hi[2]; ++z)
		for (u32 y = box.lo[1]; y < box.hi[1]; ++y)
		for (u32 x = box.lo[0]; x < box.hi[0]; ++x) {
			const i32 u = (i32)((i64)x - p.origin[0]), v = (i32)((i64)y - p.origin[1]), k = (i32)((i64)z - p.origin[2]);
			const size_t from = ((size_t)k * size[1] + (u32)paste_map_j(map, u, v)) * size[0] + (u32)paste_map_i(map, u, v);
			const size_t at = ((size_t)z * n + y) * n + x;
			i8 d = (i8)dist[at];
			paste_combine(p.mode, (i8)bases[p.stamp][from], bases[p.stamp][voxels + from], bases[p.stamp][2 * voxels + from], d, mat[at], blend[at]);
			dist[at] = (u8)d;
			u8& tb = touched[((size_t)(z >> 4) * nb + (y >> 4)) * nb + (x >> 4)];
			tb |= paste_mode_writes_distance(p.mode) ? 3 : 1;
		}
	}
	RecSwapSlot slot;
	memset(&slot, 0, sizeof(slot));
	u32 distinct = 0;
	for (u32 id = 0; id < (u32)touched.size(); ++id) {
		if (!touched[id]) continue;
		++distinct;
		const u32 bx = id % nb, by = (id / nb) % nb, bz = id / (nb * nb);
		i8 blockDist[4096];
		u32 differing = 0;
		for (u32 li = 0; li < 4096; ++li) {
			const u32 x = bx * 16 + (li & 15), y = by * 16 + ((li >> 4) & 15), z = bz * 16 + (li >> 8);
			const size_t at = ((size_t)z * n + y) * n + x;
			blockDist[li] = (i8)dist[at];
			if (dist[at] == d0[at] && mat[at] == m0[at] && blend[at] == b0[at]) continue;
			++differing;
			const u32 c[3] = { x, y, z };
			for (int k = 0; k < 3; ++k) { slot.notMin[k] = std::max(slot.notMin[k], ~c[k]); slot.max[k] = std::max(slot.max[k], c[k]); }
		}
		slot.changed += differing;
		bool flagDiffers = false;
		if (touched[id] & 2) { const u8 f = paste_block_empty(blockDist); flagDiffers = f != flags[id]; flags[id] = f; }
		if (flagDiffers) ++slot.flagChanges;
		if (differing || flagDiffers) ++slot.blocks;
	}
	if (counts) *counts = paste_counts(n, slot, distinct);
}

void pipeline(u32 n, u8* dist, u8* mat, u8* blend, u8* flags, const u8* const* bases, Sizes sizes, const Paste* pastes, u32 count,
              size_t listCap, uint64_t seed, PasteResult* results, PasteCounts* counts)
{
	const u32 nb = n / 16;
	RecGrid g;
	g.dist = dist; g.mat = mat; g.blend = blend; g.flags = flags; g.n = n;
	PastePlan plan;
	paste_plan(pastes, count, sizes, n, listCap, results, plan);
	RecSwapSlot slot;
	memset(&slot, 0, sizeof(slot));
	if (counts) *counts = paste_counts(n, slot, 0);
	if (!plan.distinct) return;
	const bool several = plan.chunks.size() > 1;
	std::vector<u32> cnt((size_t)nb * nb * nb, 0), slotOf(cnt.size(), 0);
	std::vector<u8> snaps((size_t)plan.snaps * 12289u);
	Lcg rng = { seed };
	for (u32 chunk = 0; chunk < (u32)plan.chunks.size(); ++chunk) {
		const PasteChunk& ch = plan.chunks[chunk];
		if (!ch.slots) continue;
		// the order in which the "waves" of the binning passes are served
		std::vector<u32> order;
		for (u32 i = ch.begin; i < ch.end; ++i) order.push_back(i);
		if (seed) for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rng.next((u32)i)]);
		std::vector<u32> ids(ch.slots), offset(ch.slots), cursor(ch.slots), list(ch.entries);
		u32 slots = 0, entries = 0;
		auto blocks_of = [&](u32 i, const auto& each) {
			RecBox box;
			if (!paste_box(pastes[i], sizes[pastes[i].stamp], n, &box)) return;
			u32 f[3], c[3];
			paste_box_blocks(box, f, c);
			for (u32 q = 0; q < c[0] * c[1] * c[2]; ++q) each(((f[2] + q / (c[0] * c[1])) * nb + f[1] + (q / c[0]) % c[1]) * nb + f[0] + q % c[0]);
		};
		// k_paste_count
		for (u32 i : order) blocks_of(i, [&](u32 id) { if (cnt[id]++ == 0) { ids[slots] = id; slotOf[id] = slots++; } });
		// k_brush_offsets
		for (u32 s = 0; s < slots; ++s) { offset[s] = cursor[s] = entries; entries += cnt[ids[s]]; }
		// k_paste_fill
		for (u32 i : order) blocks_of(i, [&](u32 id) { list[cursor[slotOf[id]]++] = i; });
		// k_paste_apply
		for (u32 s = 0; s < slots; ++s) {
			const u32 id = ids[s], L = cnt[id];
			const u32 bc[3] = { id % nb, (id / nb) % nb, id / (nb * nb) };
			std::sort(list.begin() + offset[s], list.begin() + offset[s] + L);
			alignas(16) u8 sDist[4096], sMat[4096], sBlend[4096], sTile[3][4096];
			RecRow d0[256], m0[256], b0[256];
			bool anyCarve = false;
			for (u32 k = 0; k < L; ++k) anyCarve = anyCarve || paste_mode_writes_distance(pastes[list[offset[s] + k]].mode);
			for (u32 t = 0; t < 256; ++t) {
				const size_t rowAt = rec_grid_row(n, id, t);
				d0[t] = rec_load16(g.dist + rowAt); m0[t] = rec_load16(g.mat + rowAt); b0[t] = rec_load16(g.blend + rowAt);
				rec_store16(sDist + t * 16, d0[t]); rec_store16(sMat + t * 16, m0[t]); rec_store16(sBlend + t * 16, b0[t]);
			}
			u8 flag0 = g.flags[id];
			for (u32 k = 0; k < L; ++k) {
				const Paste& ps = pastes[list[offset[s] + k]];
				const u32* size = sizes[ps.stamp];
				PasteSection sec;
				if (!paste_section(ps, size, bc, sec)) continue;
				const size_t voxels = stamp_voxels(size);
				const bool mats = paste_mode_reads_materials(ps.mode);
				memset(sTile, 0xA5, sizeof(sTile)); // (what a tile held before is never read)
				for (u32 q = 0; q < paste_tile_count(sec); ++q) {
					u32 at;
					const size_t from = paste_tile_source(sec, size, q, at);
					sTile[0][at] = bases[ps.stamp][from];
					if (mats) { sTile[1][at] = bases[ps.stamp][voxels + from]; sTile[2][at] = bases[ps.stamp][2 * voxels + from]; }
				}
				for (u32 v = 0; v < paste_voxel_count(sec); ++v) {
					u32 li;
					const u32 at = paste_tile_index(sec, v, li);
					i8 d = (i8)sDist[li];
					paste_combine(ps.mode, (i8)sTile[0][at], mats ? sTile[1][at] : (u8)0, mats ? sTile[2][at] : (u8)0, d, sMat[li], sBlend[li]);
					sDist[li] = (u8)d;
				}
			}
			cnt[id] = 0;
			for (u32 t = 0; t < 256; ++t) {
				const size_t rowAt = rec_grid_row(n, id, t);
				rec_store16(g.dist + rowAt, rec_load16(sDist + t * 16)); rec_store16(g.mat + rowAt, rec_load16(sMat + t * 16)); rec_store16(g.blend + rowAt, rec_load16(sBlend + t * 16));
			}
			u8 flag1 = flag0;
			if (anyCarve) g.flags[id] = flag1 = paste_block_empty((const i8*)sDist);
			bool compare = true;
			if (several && plan.first[id] != plan.last[id]) {
				u8* snap = snaps.data() + (size_t)plan.snapOf[id] * 12289u;
				if (chunk == plan.first[id]) {
					for (u32 t = 0; t < 256; ++t) { memcpy(snap + t * 16, d0[t].w, 16); memcpy(snap + 4096 + t * 16, m0[t].w, 16); memcpy(snap + 8192 + t * 16, b0[t].w, 16); }
					snap[12288] = flag0;
				} else if (chunk == plan.last[id]) {
					for (u32 t = 0; t < 256; ++t) { memcpy(d0[t].w, snap + t * 16, 16); memcpy(m0[t].w, snap + 4096 + t * 16, 16); memcpy(b0[t].w, snap + 8192 + t * 16, 16); }
					flag0 = snap[12288];
				}
				compare = chunk == plan.last[id];
			}
			if (!compare) continue;
			u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 };
			for (u32 t = 0; t < 256; ++t)
				rec_row_bounds(n, id, t, rec_row_diff(d0[t], rec_load16(sDist + t * 16)) | rec_row_diff(m0[t], rec_load16(sMat + t * 16)) | rec_row_diff(b0[t], rec_load16(sBlend + t * 16)), v);
			if (v[6]) {
				for (int k = 0; k < 3; ++k) { slot.notMin[k] = std::max(slot.notMin[k], v[k]); slot.max[k] = std::max(slot.max[k], v[3 + k]); }
				slot.changed += v[6];
			}
			if (v[6] || flag0 != flag1) ++slot.blocks;
			if (flag0 != flag1) ++slot.flagChanges;
		}
	}
	if (counts) *counts = paste_counts(n, slot, plan.distinct);
}

} // namespace

extern "C" {

int sh_check(const vx_paste* pastes, uint32_t count, const uint32_t* sizes, uint32_t n_stamps)
{
	return paste_check((const Paste*)pastes, count, (Sizes)sizes, n_stamps) ? VX_ERR_INVALID : VX_OK;
}
int sh_check_size(const uint32_t* size) { return stamp_check_size(size) ? VX_ERR_INVALID : VX_OK; }
int sh_check_box(uint32_t n, const vx_box* box) { return stamp_check_box(n, (const RecBox*)box) ? VX_ERR_INVALID : VX_OK; }

// what vx_grid_paste returns for bad arguments (everything but the context and the owners of the stamps), else VX_OK with the
// batch applied; nothing is changed where it refuses
int sh_paste(uint32_t path, uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, uint8_t* flags, const uint8_t* const* bases,
             const uint32_t* sizes, uint32_t n_stamps, const vx_paste* pastes, uint32_t count, uint32_t list_cap, uint64_t seed,
             vx_paste_result* results, vx_paste_counts* counts)
{
	static_assert(sizeof(Paste) == sizeof(vx_paste) && sizeof(PasteResult) == sizeof(vx_paste_result) && sizeof(PasteCounts) == sizeof(vx_paste_counts), "tv_stamp.h records");
	if (counts) memset(counts, 0, sizeof(*counts));
	if (paste_check((const Paste*)pastes, count, (Sizes)sizes, n_stamps)) return VX_ERR_INVALID;
	for (u32 i = 0; i < n_stamps; ++i) if (sizes[i * 3] && stamp_check_size(sizes + i * 3)) return VX_ERR_INVALID;
	if (!count) return VX_OK;
	if (path == 0) plain(n, (u8*)dist, mat, blend, flags, bases, (Sizes)sizes, (const Paste*)pastes, count, (PasteResult*)results, (PasteCounts*)counts);
	else pipeline(n, (u8*)dist, mat, blend, flags, bases, (Sizes)sizes, (const Paste*)pastes, count, list_cap ? list_cap : (size_t)1 << 22, seed, (PasteResult*)results, (PasteCounts*)counts);
	return VX_OK;
}

int sh_paste_box(const vx_paste* paste, const uint32_t* size, uint32_t n, vx_box* out) { return paste_box(*(const Paste*)paste, size, n, (RecBox*)out); }

// which: 0 = sizes of vx_stamp_info, vx_paste, vx_paste_result, vx_paste_counts; 1 = offsets inside vx_stamp_info; 2 = inside vx_paste;
// 3 = inside vx_paste_result; 4 = inside vx_paste_counts
uint32_t sh_layout(uint32_t which, uint32_t* out)
{
	if (which == 0) { const uint32_t v[] = { sizeof(vx_stamp_info), sizeof(vx_paste), sizeof(vx_paste_result), sizeof(vx_paste_counts) }; memcpy(out, v, sizeof(v)); return 4; }
	if (which == 1) { const uint32_t v[] = { offsetof(vx_stamp_info, size), offsetof(vx_stamp_info, reserved), offsetof(vx_stamp_info, voxels), offsetof(vx_stamp_info, bytes) }; memcpy(out, v, sizeof(v)); return 4; }
	if (which == 2) {
		const uint32_t v[] = { offsetof(vx_paste, origin), offsetof(vx_paste, stamp), offsetof(vx_paste, orient), offsetof(vx_paste, mode), offsetof(vx_paste, reserved) };
		memcpy(out, v, sizeof(v)); return 5;
	}
	if (which == 3) { const uint32_t v[] = { offsetof(vx_paste_result, box), offsetof(vx_paste_result, touched_blocks), offsetof(vx_paste_result, reserved) }; memcpy(out, v, sizeof(v)); return 3; }
	const uint32_t v[] = { offsetof(vx_paste_counts, out_min), offsetof(vx_paste_counts, out_max), offsetof(vx_paste_counts, changed_voxels), offsetof(vx_paste_counts, changed_blocks),
	                       offsetof(vx_paste_counts, flag_changes), offsetof(vx_paste_counts, touched_blocks), offsetof(vx_paste_counts, reserved) };
	memcpy(out, v, sizeof(v)); return 7;
}

// 0 = VX_STAMP_MAX_EDGE, 1 = VX_STAMP_MAX_VOXELS, 2 = VX_PASTE_MAX_COUNT, 3 = VX_PASTE_MAX_STAMPS, 4..7 = the modes
uint32_t sh_limit(uint32_t which)
{
	const uint32_t v[] = { VX_STAMP_MAX_EDGE, VX_STAMP_MAX_VOXELS, VX_PASTE_MAX_COUNT, VX_PASTE_MAX_STAMPS, VX_PASTE_REPLACE, VX_PASTE_UNION, VX_PASTE_SUBTRACT, VX_PASTE_PAINT };
	return which < 8 ? v[which] : 0;
}

} // extern "C"
