// measure_host.cpp — host side of the tests of the measurements (tests only; built by voxels_amd/build.py build_measure_host()).
//
// voxels_amd/csrc/tv_measure.h compiled for the host behind one C interface, with two paths through a batch of boxes:
//   path 0   a plain triple loop: box after box, voxel after voxel
//   path 1   the pipeline of vx_measure.inl - the running sums of the boxes' block counts, pairs launched in chunks of `chunk`, a
//            workgroup per MEASURE_GROUP consecutive pairs of a launch: the binary search for the box of its first pair, per box it
//            meets a partial (a 256-bin u32 histogram, count and bounds) from the 256 rows of each block, the partial merged into
//            the box's 64-bit slot and tallies, and the finish pass - with the lanes of a workgroup as loops and the launches in
//            their order.  `skip` = 1 lets the per-block sign summaries (formed here from the grid, by the rule of
//            the mirrors: 1 = no sample < 0, 2 = every sample < 0) stand in for distance rows, as the kernel does.
//   mh_record    vx_record_measure the same two ways        mh_merge   the 64-bit merge of 32-bit partial counts alone
//   mh_layout    sizes and offsets of the header's structs as this compiler lays them out; mh_limit the limits
// A grid is dist / mat (n^3 bytes each, x fastest, Z up); a record is ids (ascending block ids) and per entry 4096 bytes of each
// field, rows z-major (the layout of vx_record_read_block).
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_measure.h"

using namespace tv;

namespace {

static_assert(sizeof(MeasureResult) == sizeof(vx_measure) && sizeof(RecordDelta) == sizeof(vx_record_delta) && sizeof(RecBox) == sizeof(vx_box), "tv_measure.h records");

// what the device does with atomics: a 32-bit partial into a 64-bit total, maxima into maxima
void merge_count(u64& total, u32 part) { total += part; }
void merge_bounds(u32 notMin[3], u32 mx[3], const u32 v[6])
{
	for (int k = 0; k < 3; ++k) { notMin[k] = std::max(notMin[k], v[k]); mx[k] = std::max(mx[k], v[3 + k]); }
}

void plain_measure(u32 n, const i8* dist, const u8* mat, const RecBox* boxes, u32 count, MeasureResult* results, u64* tallies)
{
	for (u32 i = 0; i < count; ++i) {
		const RecBox& b = boxes[i];
		MeasureSlot s;
		memset(&s, 0, sizeof(s));
		u64 bins[256] = { 0 };
		for (u32 z = b.lo[2]; z < b.hi[2]; ++z)
			for (u32 y = b.lo[1]; y < b.hi[1]; ++y)
				for (u32 x = b.lo[0]; x < b.hi[0]; ++x) {
					const size_t at = ((size_t)z * n + y) * n + x;
					if (dist[at] >= 0) continue;
					const u32 c[3] = { x, y, z };
					for (int k = 0; k < 3; ++k) { s.notMin[k] = std::max(s.notMin[k], ~c[k]); s.max[k] = std::max(s.max[k], c[k]); }
					++s.solid;
					++bins[mat[at]];
				}
		u32 materials = 0;
		for (u32 m = 0; m < 256; ++m) materials += bins[m] ? 1u : 0u;
		results[i] = measure_finish(b, s, materials);
		if (tallies) memcpy(tallies + (size_t)i * 256u, bins, sizeof(bins));
	}
}

u32 block_summary(u32 n, const i8* dist, u32 id)
{
	bool neg = false, pos = false;
	for (u32 row = 0; row < 256; ++row) {
		const i8* p = dist + rec_grid_row(n, id, row);
		for (u32 x = 0; x < 16; ++x) { if (p[x] < 0) neg = true; else pos = true; }
	}
	return neg && pos ? 0u : neg ? 2u : 1u;
}

void pipeline_measure(u32 n, const i8* dist, const u8* mat, const RecBox* boxes, u32 count, u64 chunk, u32 skip, MeasureResult* results, u64* outTallies)
{
	const u32 nb = n >> 4;
	std::vector<u64> prefix((size_t)count + 1u, 0);
	for (u32 i = 0; i < count; ++i) prefix[i + 1u] = prefix[i] + measure_box_pairs(boxes[i]);
	std::vector<MeasureSlot> slots(count);
	memset(slots.data(), 0, slots.size() * sizeof(MeasureSlot));
	std::vector<u64> tallies((size_t)count * 256u, 0);
	for (u64 base = 0; base < prefix[count]; base += chunk) {                 // a launch
		const u64 end = std::min<u64>(base + chunk, prefix[count]);
		for (u64 wg = 0; wg < (end - base + MEASURE_GROUP - 1u) / MEASURE_GROUP; ++wg) {   // k_measure_pairs: a workgroup
			u64 pair = base + wg * MEASURE_GROUP;
			const u64 last = std::min<u64>(pair + MEASURE_GROUP, end);
			u32 bi = measure_pair_box(prefix.data(), count, pair);
			while (pair < last) {                                             // a box the workgroup meets
				const RecBox& box = boxes[bi];
				const u64 first = prefix[bi], boxEnd = std::min<u64>(prefix[bi + 1u], last);
				u32 hist[256] = { 0 }, v[7] = { 0, 0, 0, 0, 0, 0, 0 };
				for (; pair < boxEnd; ++pair) {
					const u32 id = measure_pair_block(box, nb, (u32)(pair - first));
					const u32 summary = skip ? block_summary(n, dist, id) : 0u;
					if (summary == 1u) continue;
					const bool allSolid = summary == 2u && measure_block_inside(box, nb, id);
					for (u32 t = 0; t < 256; ++t) {                           // a lane
						const size_t rowAt = rec_grid_row(n, id, t);
						u32 mask = allSolid ? 0xFFFFu : measure_clip_mask(box, nb, id, t);
						if (mask && !allSolid) mask &= measure_sign_mask(rec_load16((const u8*)dist + rowAt));
						rec_row_bounds(n, id, t, mask, v);
						if (mask) measure_row_materials(rec_load16(mat + rowAt), mask, [&](u32 m, u32 voxels) { hist[m] += voxels; });
					}
				}
				if (v[6]) { merge_bounds(slots[bi].notMin, slots[bi].max, v); merge_count(slots[bi].solid, v[6]); }
				for (u32 m = 0; m < 256; ++m) if (hist[m]) merge_count(tallies[(size_t)bi * 256u + m], hist[m]);
				++bi;
			}
		}
	}
	for (u32 bi = 0; bi < count; ++bi) {                                      // k_measure_finish
		u32 bins = 0;
		for (u32 m = 0; m < 256; ++m) bins += tallies[(size_t)bi * 256u + m] ? 1u : 0u;
		results[bi] = measure_finish(boxes[bi], slots[bi], bins);
	}
	if (outTallies) memcpy(outTallies, tallies.data(), tallies.size() * 8u);
}

void plain_record(u32 n, const i8* dist, const u8* mat, u32 blocks, const u32* ids, const i8* rdist, const u8* rmat, RecordDelta* delta, u64* removed, u64* added)
{
	const u32 nb = n >> 4;
	DeltaSlot s;
	memset(&s, 0, sizeof(s));
	for (u32 e = 0; e < blocks; ++e) {
		const u32 id = ids[e], org[3] = { (id % nb) * 16u, ((id / nb) % nb) * 16u, (id / (nb * nb)) * 16u };
		bool any = false;
		for (u32 v = 0; v < 4096; ++v) {
			const u32 c[3] = { org[0] + (v & 15u), org[1] + ((v >> 4) & 15u), org[2] + (v >> 8) };
			const size_t at = ((size_t)c[2] * n + c[1]) * n + c[0];
			const bool was = rdist[(size_t)e * 4096u + v] < 0, is = dist[at] < 0;
			const u8 wm = rmat[(size_t)e * 4096u + v], im = mat[at];
			if (was && is) { if (wm != im) { ++s.repainted; any = true; } continue; }
			if (was == is) continue;
			any = true;
			if (was) { ++s.removed; if (removed) ++removed[wm]; } else { ++s.added; if (added) ++added[im]; }
			for (int k = 0; k < 3; ++k) { s.notMin[k] = std::max(s.notMin[k], ~c[k]); s.max[k] = std::max(s.max[k], c[k]); }
		}
		s.blocks += any ? 1u : 0u;
	}
	*delta = measure_delta_finish(s);
}

void pipeline_record(u32 n, const i8* dist, const u8* mat, u32 blocks, const u32* ids, const i8* rdist, const u8* rmat, RecordDelta* delta, u64* removed, u64* added)
{
	DeltaSlot s;
	memset(&s, 0, sizeof(s));
	u64 tallies[512] = { 0 };
	for (u32 wg = 0; wg < (blocks + REC_GROUP - 1u) / REC_GROUP; ++wg) {      // k_rec_measure: a workgroup
		u32 hist[2][256] = { { 0 }, { 0 } }, b[7] = { 0, 0, 0, 0, 0, 0, 0 }, sums[3] = { 0, 0, 0 }, changed = 0;
		for (u32 entry = wg * REC_GROUP; entry < std::min(wg * REC_GROUP + REC_GROUP, blocks); ++entry) {
			const u32 id = ids[entry];
			const u32 before = sums[0] + sums[1] + sums[2];
			for (u32 t = 0; t < 256; ++t) {
				const size_t at = rec_grid_row(n, id, t), in = rec_row(entry, t);
				const u32 was = measure_sign_mask(rec_load16((const u8*)rdist + in)), is = measure_sign_mask(rec_load16((const u8*)dist + at));
				if (!(was | is)) continue;
				const RecRow rm = rec_load16(rmat + in), gm = rec_load16(mat + at);
				const DeltaRow d = measure_delta_row(was, is, rm, gm);
				u32 moved[7] = { 0, 0, 0, 0, 0, 0, 0 };
				rec_row_bounds(n, id, t, d.removed | d.added, moved);
				for (int k = 0; k < 6; ++k) b[k] = std::max(b[k], moved[k]);
				sums[0] += (u32)__builtin_popcount(d.removed); sums[1] += (u32)__builtin_popcount(d.added); sums[2] += (u32)__builtin_popcount(d.repainted);
				measure_row_materials(rm, d.removed, [&](u32 m, u32 voxels) { hist[0][m] += voxels; });
				measure_row_materials(gm, d.added, [&](u32 m, u32 voxels) { hist[1][m] += voxels; });
			}
			if (sums[0] + sums[1] + sums[2] != before) ++changed;
		}
		if (sums[0] + sums[1]) merge_bounds(s.notMin, s.max, b);
		merge_count(s.removed, sums[0]); merge_count(s.added, sums[1]); merge_count(s.repainted, sums[2]);
		s.blocks += changed;
		for (u32 m = 0; m < 256; ++m) { merge_count(tallies[m], hist[0][m]); merge_count(tallies[256u + m], hist[1][m]); }
	}
	*delta = measure_delta_finish(s);
	if (removed) memcpy(removed, tallies, 2048);
	if (added) memcpy(added, tallies + 256, 2048);
}

} // namespace

extern "C" {

int mh_check(uint32_t n, const vx_box* boxes, uint32_t count, const void* results)
{
	return measure_check(n, (const RecBox*)boxes, count, results) ? VX_ERR_INVALID : VX_OK;
}

// what vx_grid_measure returns for bad arguments (everything but the context), else VX_OK with the answers written
int mh_measure(uint32_t path, uint32_t n, const int8_t* dist, const uint8_t* mat, const vx_box* boxes, uint32_t count, uint64_t chunk, uint32_t skip,
               vx_measure* results, uint64_t* tallies)
{
	if (measure_check(n, (const RecBox*)boxes, count, results)) return VX_ERR_INVALID;
	if (!count) return VX_OK;
	if (path == 0) plain_measure(n, dist, mat, (const RecBox*)boxes, count, (MeasureResult*)results, (u64*)tallies);
	else pipeline_measure(n, dist, mat, (const RecBox*)boxes, count, chunk ? chunk : (u64)MEASURE_CHUNK_PAIRS, skip, (MeasureResult*)results, (u64*)tallies);
	return VX_OK;
}

// what vx_record_measure returns for bad arguments (everything but the owners): has_record = 0 stands for a null record, rec_n for
// the edge of the grid it was captured from
int mh_record(uint32_t path, uint32_t n, const int8_t* dist, const uint8_t* mat, uint32_t has_record, uint32_t rec_n, uint32_t blocks, const uint32_t* ids,
              const int8_t* rdist, const uint8_t* rmat, vx_record_delta* delta, uint64_t* removed, uint64_t* added)
{
	if (delta) memset(delta, 0, sizeof(*delta));
	if (!delta || !has_record || rec_n != n) return VX_ERR_INVALID;
	if (removed) memset(removed, 0, 2048);
	if (added) memset(added, 0, 2048);
	if (!blocks) return VX_OK;
	if (path == 0) plain_record(n, dist, mat, blocks, ids, rdist, rmat, (RecordDelta*)delta, (u64*)removed, (u64*)added);
	else pipeline_record(n, dist, mat, blocks, ids, rdist, rmat, (RecordDelta*)delta, (u64*)removed, (u64*)added);
	return VX_OK;
}

// the merge of `count` 32-bit partial counts into one 64-bit total, as the pipeline does it
uint64_t mh_merge(const uint32_t* parts, uint64_t count)
{
	u64 total = 0;
	for (u64 i = 0; i < count; ++i) merge_count(total, parts[i]);
	return total;
}

// which: 0 = sizes of vx_measure, vx_record_delta, vx_box; 1 = offsets inside vx_measure; 2 = inside vx_record_delta
uint32_t mh_layout(uint32_t which, uint32_t* out)
{
	if (which == 0) { const uint32_t v[] = { sizeof(vx_measure), sizeof(vx_record_delta), sizeof(vx_box) }; memcpy(out, v, sizeof(v)); return 3; }
	if (which == 1) {
		const uint32_t v[] = { offsetof(vx_measure, voxels), offsetof(vx_measure, solid_voxels), offsetof(vx_measure, min), offsetof(vx_measure, max), offsetof(vx_measure, materials), offsetof(vx_measure, reserved) };
		memcpy(out, v, sizeof(v)); return 6;
	}
	const uint32_t v[] = { offsetof(vx_record_delta, removed_voxels), offsetof(vx_record_delta, added_voxels), offsetof(vx_record_delta, repainted_voxels), offsetof(vx_record_delta, min),
	                       offsetof(vx_record_delta, max), offsetof(vx_record_delta, blocks), offsetof(vx_record_delta, reserved) };
	memcpy(out, v, sizeof(v)); return 7;
}

// 0 = VX_MEASURE_MAX_BOXES, 1 = the default pairs per launch
uint32_t mh_limit(uint32_t which)
{
	const uint32_t v[] = { VX_MEASURE_MAX_BOXES, MEASURE_CHUNK_PAIRS };
	return which < 2 ? v[which] : 0;
}

} // extern "C"
