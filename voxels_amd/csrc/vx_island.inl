// vx_island.inl — vx_grid_islands (include/voxels_hip.h, "detached solid pieces"): the connected components of the solid
// voxels of a box of the resident grid, and the removal of the detached ones; included by vx_hip.hip after vx_brush.inl (HIP
// only).  DESIGN.md §16.  The per-lane logic is tv_island.h, shared with the CPU emulation of the tests.
//
//   k_isl_local    one workgroup per tile (a 16^3 block clipped to the box): union-find over the runs of solid voxels of the
//                  tile's rows in LDS, provisional labels (the region index of the tile-local root) into the label volume
//   k_isl_merge    one workgroup per tile, one lane per voxel pair across the tile's three lower faces: lock-free unions on the
//                  label volume; a root is only ever re-pointed to a smaller index, so the final root is the least index
//   k_isl_flatten  one wave per x-row of the box: every solid voxel's label becomes its root; roots per row counted
//   k_isl_scan     one workgroup: exclusive sums (of the roots per row; later of the listed records)
//   -- the host reads the number of components and sizes the records --
//   k_isl_roots    one wave per x-row: the roots in index order (= label order) and an empty record for each
//   k_isl_stats    one workgroup per tile: (voxels, box, faces) per distinct label of the tile in an LDS table, then one set
//                  of integer atomics per (tile, label) into the record found by binary search
//   k_isl_mark     one lane per record: detached / listed / to be removed, the counts, the box of what is removed
//   k_isl_compact  the listed records, in label order, into the output
//   k_isl_remove   (VX_ISLANDS_REMOVE) one workgroup per tile inside that box: the voxels of the marked records become air;
//                  the ids of the blocks that changed are collected
//   -- the host reads the counts --
//   k_edit_flags + rebrick_blocks over the collected blocks.
#include "tv_island.h"

namespace {

struct IslOpsDev {
#if defined(__HIP_DEVICE_COMPILE__)
	static TV_HD u32 load(const u32* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	static TV_HD u32 amin(u32* p, u32 v) { return atomicMin(p, v); }
	static TV_HD u32 amax(u32* p, u32 v) { return atomicMax(p, v); }
	static TV_HD u32 aadd(u32* p, u32 v) { return atomicAdd(p, v); }
	static TV_HD u32 aor(u32* p, u32 v) { return atomicOr(p, v); }
	static TV_HD u32 cas(u32* p, u32 expect, u32 v) { return atomicCAS(p, expect, v); }
	static TV_HD void aadd64(unsigned long long* p, unsigned long long v) { atomicAdd(p, v); }
#else
	static TV_HD u32 load(const u32* p) { return IslOpsPlain::load(p); }
	static TV_HD u32 amin(u32* p, u32 v) { return IslOpsPlain::amin(p, v); }
	static TV_HD u32 amax(u32* p, u32 v) { return IslOpsPlain::amax(p, v); }
	static TV_HD u32 aadd(u32* p, u32 v) { return IslOpsPlain::aadd(p, v); }
	static TV_HD u32 aor(u32* p, u32 v) { return IslOpsPlain::aor(p, v); }
	static TV_HD u32 cas(u32* p, u32 expect, u32 v) { return IslOpsPlain::cas(p, expect, v); }
	static TV_HD void aadd64(unsigned long long* p, unsigned long long v) { IslOpsPlain::aadd64(p, v); }
#endif
};

struct IslState {
	void* volume = nullptr;   // the label volume when the caller gives none
	size_t volumeCap = 0;
	void* rows = nullptr;     // per x-row of the box: roots (then their exclusive sums); [rows] = the total
	size_t rowsCap = 0;
	void* perRecord = nullptr; // roots, records, marks, list offsets, output
	size_t perRecordCap = 0;
	void* touched = nullptr;  // ids of the blocks a removal rewrote (one per tile at most)
	size_t touchedCap = 0;
	void* small = nullptr;    // IslCounts, the dirty box, the list total

	void release(vx_ctx* c)
	{
		c->be.free(volume); c->be.free(rows); c->be.free(perRecord); c->be.free(touched); c->be.free(small);
	}
};

enum { ISL_SMALL_BYTES = 256, ISL_AT_DIRTY = 64, ISL_AT_LISTED = 96 };

__global__ __launch_bounds__(WG) void k_isl_local(GridView g, const u8* flags, IslRegion r, u32* L)
{
	__shared__ u32 sParent[4096];
	__shared__ u32 sMask[WG];
	const u32 t = threadIdx.x;
	const IslTile T = isl_tile(r, blockIdx.x);
	const u32 n = r.n, y = t & 15u, z = t >> 4;
	if (flags[T.block]) { // all solid or all air: one sample tells
		const u32 label = g.dist[((size_t)T.org[2] * n + T.org[1]) * n + T.org[0]] < 0 ? isl_tile_first(r, T) : (u32)ISL_AIR;
		for (u32 li = t; li < 4096u; li += WG) {
			const u32 x = T.org[0] + (li & 15u);
			if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8)) L[isl_local_to_region(r, T, li)] = label;
		}
		return;
	}
	u32 mask = 0;
	if (isl_row_inside(T, y, z)) {
		const uint4 raw = *(const uint4*)(g.dist + ((size_t)(T.org[2] + z) * n + T.org[1] + y) * n + T.org[0]);
		i8 v[16];
		memcpy(v, &raw, 16);
		mask = isl_solid_bits(v) & isl_clip_bits(T);
	}
	sMask[t] = mask;
	isl_local_init(t, mask, sParent);
	__syncthreads();
	isl_local_link<IslOpsDev>(t, sMask, sParent);
	__syncthreads();
	isl_local_flatten<IslOpsDev>(t, mask, sParent);
	__syncthreads();
	for (u32 li = t; li < 4096u; li += WG) {
		const u32 x = T.org[0] + (li & 15u);
		if (x >= T.c0[0] && x < T.c1[0] && isl_row_inside(T, (li >> 4) & 15u, li >> 8)) {
			const u32 root = sParent[li];
			L[isl_local_to_region(r, T, li)] = root == (u32)ISL_AIR ? (u32)ISL_AIR : isl_local_to_region(r, T, root);
		}
	}
}

__global__ __launch_bounds__(WG) void k_isl_merge(IslRegion r, u32* L)
{
	isl_merge_lane<IslOpsDev>(r, isl_tile(r, blockIdx.x), threadIdx.x, L);
}

__global__ __launch_bounds__(WG) void k_isl_flatten(IslRegion r, u32* L, u32* rowCount)
{
	const u32 lane = threadIdx.x & 63u, row = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (row >= isl_rows(r)) return;
	const u32 base = row * r.ext[0];
	u32 roots = 0;
	for (u32 x0 = 0; x0 < r.ext[0]; x0 += 64) {
		const u32 x = x0 + lane;
		const bool isRoot = x < r.ext[0] && isl_flatten_voxel<IslOpsDev>(L, base + x);
		roots += (u32)__builtin_popcountll(__ballot(isRoot));
	}
	if (lane == 0) rowCount[row] = roots;
}

// a[0 .. count) -> its exclusive sums, in place; *total = the sum.  One workgroup.
__global__ __launch_bounds__(WG) void k_isl_scan(u32* a, u32 count, u32* total)
{
	__shared__ u32 waveSum[WG / 64];
	const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6;
	u32 carry = 0;
	for (u32 base = 0; base < count; base += WG * 16u) {
		const u32 i0 = base + t * 16u;
		u32 v[16], s = 0;
#pragma unroll
		for (u32 j = 0; j < 16; ++j) { v[j] = i0 + j < count ? a[i0 + j] : 0u; s += v[j]; }
		u32 incl = s;
#pragma unroll
		for (u32 d = 1; d < 64; d <<= 1) { const u32 o = __shfl_up(incl, d); if (lane >= d) incl += o; }
		if (lane == 63) waveSum[w] = incl;
		__syncthreads();
		u32 run = carry + incl - s, all = 0;
#pragma unroll
		for (u32 k = 0; k < WG / 64; ++k) { if (k < w) run += waveSum[k]; all += waveSum[k]; }
#pragma unroll
		for (u32 j = 0; j < 16; ++j) { if (i0 + j < count) a[i0 + j] = run; run += v[j]; }
		carry += all;
		__syncthreads();
	}
	if (t == 0) *total = carry;
}

__global__ __launch_bounds__(WG) void k_isl_roots(IslRegion r, const u32* L, const u32* rowOff, u32* roots, IslRecord* recs, u32 count)
{
	const u32 lane = threadIdx.x & 63u, row = blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (row >= isl_rows(r)) return;
	const u32 base = row * r.ext[0];
	u32 at = rowOff[row];
	for (u32 x0 = 0; x0 < r.ext[0]; x0 += 64) {
		const u32 x = x0 + lane;
		const bool isRoot = x < r.ext[0] && L[base + x] == base + x;
		const unsigned long long m = __ballot(isRoot);
		const u32 mine = at + (u32)__builtin_popcountll(m & ((1ull << lane) - 1ull));
		if (isRoot && mine < count) { roots[mine] = base + x; recs[mine] = isl_empty_record(base + x); }
		at += (u32)__builtin_popcountll(m);
	}
}

__global__ __launch_bounds__(WG) void k_isl_stats(const u8* flags, IslRegion r, const u32* L, const u32* roots, u32 count, IslRecord* recs)
{
	__shared__ u32 sKey[ISL_HASH_SLOTS], sCnt[ISL_HASH_SLOTS], sXy[ISL_HASH_SLOTS], sZf[ISL_HASH_SLOTS];
	const u32 t = threadIdx.x;
	const IslTile T = isl_tile(r, blockIdx.x);
	if (flags[T.block]) {
		if (t == 0) { const u32 label = L[isl_tile_first(r, T)]; if (label != (u32)ISL_AIR) isl_stats_uniform<IslOpsDev>(r, T, label, roots, count, recs); }
		return;
	}
	for (u32 s = t; s < (u32)ISL_HASH_SLOTS; s += WG) { sKey[s] = (u32)ISL_AIR; sCnt[s] = 0; sXy[s] = 0; sZf[s] = 0; }
	__syncthreads();
	isl_stats_row<IslOpsDev>(r, T, t, L, sKey, sCnt, sXy, sZf);
	__syncthreads();
	for (u32 s = t; s < (u32)ISL_HASH_SLOTS; s += WG) isl_stats_flush<IslOpsDev>(T, s, sKey, sCnt, sXy, sZf, roots, count, recs);
}

__global__ __launch_bounds__(WG) void k_isl_mark(const IslRecord* recs, u32 count, u32 flags, u32 anchorFaces, unsigned long long maxVoxels,
                                                 u8* marks, u32* listFlag, IslCounts* counts, u32* dirty)
{
	const u32 k = blockIdx.x * WG + threadIdx.x;
	if (k >= count) return;
	const u32 m = isl_mark<IslOpsDev>(recs[k], flags, anchorFaces, maxVoxels, counts, dirty);
	marks[k] = (u8)m;
	listFlag[k] = (m & (u32)ISL_MARK_LISTED) ? 1u : 0u;
}

__global__ __launch_bounds__(WG) void k_isl_compact(const IslRecord* recs, u32 count, const u8* marks, const u32* listOff, IslRecord* out, u32 capacity)
{
	const u32 k = blockIdx.x * WG + threadIdx.x;
	if (k >= count || !(marks[k] & (u32)ISL_MARK_LISTED) || listOff[k] >= capacity) return;
	out[listOff[k]] = recs[k];
}

__global__ __launch_bounds__(WG) void k_isl_remove(GridView g, IslRegion r, const u32* L, const u32* roots, u32 count, const u8* marks, const u32* dirty,
                                                   int air, u32* touched, u32 touchedCap, IslCounts* counts)
{
	const u32 t = threadIdx.x;
	const IslTile T = isl_tile(r, blockIdx.x);
	if (!counts->removed || !isl_tile_in_dirty(T, dirty)) return; // (uniform)
	const u32 n = r.n, y = t & 15u, z = t >> 4;
	i8* at = const_cast<i8*>(g.dist) + ((size_t)(T.org[2] + z) * n + T.org[1] + y) * n + T.org[0];
	bool changed = false;
	if (isl_row_inside(T, y, z)) {
		uint4 raw = *(const uint4*)at;
		i8 v[16];
		memcpy(v, &raw, 16);
		changed = isl_remove_row(r, T, t, L, roots, count, marks, (i8)air, v);
		if (changed) { memcpy(&raw, v, 16); *(uint4*)at = raw; }
	}
	const int any = __syncthreads_or(changed ? 1 : 0);
	if (t == 0 && any) { const u32 slot = atomicAdd(&counts->touched_blocks, 1u); if (slot < touchedCap) touched[slot] = T.block; }
}

} // namespace

extern "C" {

static_assert(sizeof(vx_island_query) == 48 && sizeof(vx_island) == 40 && sizeof(vx_island_counts) == 48, "vx_island_query / vx_island / vx_island_counts layout");
static_assert(sizeof(IslRecord) == sizeof(vx_island) && sizeof(IslCounts) == sizeof(vx_island_counts), "tv_island.h records");
static_assert(VX_ISLANDS_DETACHED_ONLY == tv::ISL_DETACHED_ONLY && VX_ISLANDS_REMOVE == tv::ISL_REMOVE, "island flags");

int vx_grid_islands(vx_ctx* c, const vx_island_query* q, vx_island* islands, uint32_t capacity, vx_island_counts* counts,
                    uint32_t* d_labels, float out_min[3], float out_max[3])
{
	VX_ENTER(c);
	const char* what = "vx_grid_islands";
	if (out_min) out_min[0] = out_min[1] = out_min[2] = 0.f;
	if (out_max) out_max[0] = out_max[1] = out_max[2] = 0.f;
	if (!c) return VX_ERR_INVALID;
	if (!q || !counts) return fail(c, VX_ERR_INVALID, std::string(what) + ": null query or counts");
	memset(counts, 0, sizeof(*counts));
	if (!c->ownsGrid || !c->n || (c->zBegin != 0 || c->zEnd != c->n || c->yBegin != 0 || c->yEnd != c->n)) return fail(c, VX_ERR_INVALID, std::string(what) + ": needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (q->flags & ~(VX_ISLANDS_DETACHED_ONLY | VX_ISLANDS_REMOVE)) return fail(c, VX_ERR_INVALID, std::string(what) + ": unknown flag bits");
	if (q->anchor_faces > 0x3Fu) return fail(c, VX_ERR_INVALID, std::string(what) + ": anchor_faces above 0x3F");
	const bool remove = (q->flags & VX_ISLANDS_REMOVE) != 0;
	if (remove && (q->air_value < 1 || q->air_value > 127)) return fail(c, VX_ERR_INVALID, std::string(what) + ": air_value outside 1..127");
	if (capacity && !islands) return fail(c, VX_ERR_INVALID, std::string(what) + ": null record array");
	if (d_labels && ((uintptr_t)d_labels & 15u)) return fail(c, VX_ERR_INVALID, std::string(what) + ": d_labels is not 16-byte aligned");
	u32 lo[3] = { 0, 0, 0 }, hi[3] = { c->n, c->n, c->n };
	if (!q->whole_grid) for (int k = 0; k < 3; ++k) { lo[k] = q->lo[k]; hi[k] = q->hi[k]; }
	unsigned long long V = 1;
	for (int k = 0; k < 3; ++k) {
		if (!(lo[k] < hi[k] && hi[k] <= c->n)) return fail(c, VX_ERR_INVALID, std::string(what) + ": the box needs lo < hi <= n on every axis");
		V *= hi[k] - lo[k];
	}
	if (V > (1ull << 30)) return fail(c, VX_ERR_INVALID, std::string(what) + ": the box holds more than 2^30 voxels");

	IslState* s = module_state<IslState>(c, MOD_ISLAND);
	const IslRegion r = isl_region(c->n, lo, hi);
	const u32 tiles = isl_tiles(r), rows = isl_rows(r);
	auto noMemory = [&]() { return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error()); };
	if (!s->small && !(s->small = c->be.alloc(ISL_SMALL_BYTES))) return noMemory();
	if (!d_labels && !dev_grow(c, s->volume, s->volumeCap, (size_t)V * 4)) return noMemory();
	if (!dev_grow(c, s->rows, s->rowsCap, ((size_t)rows + 1) * 4)) return noMemory();
	if (remove && !dev_grow(c, s->touched, s->touchedCap, (size_t)tiles * 4)) return noMemory();

	u32* L = d_labels ? d_labels : (u32*)s->volume;
	u32* rowOff = (u32*)s->rows;
	IslCounts* dCounts = (IslCounts*)s->small;
	u32* dDirty = (u32*)((char*)s->small + ISL_AT_DIRTY);
	u32* dListed = (u32*)((char*)s->small + ISL_AT_LISTED);
	const GridView g = resident_view(c);
	const u8* flags = (const u8*)c->dFlags;
	hipStream_t st = c->be.stream;
	const u32 rowGroups = (rows + WG / 64 - 1) / (WG / 64);
	auto deviceFailed = [&]() { return fail(c, VX_ERR_DEVICE, std::string(what) + ": device query failed: " + c->be.error()); };

	bool ok = c->be.fill(s->small, 0, ISL_SMALL_BYTES);
	hipLaunchKernelGGL(k_isl_local, dim3(tiles), dim3(WG), 0, st, g, flags, r, L);
	hipLaunchKernelGGL(k_isl_merge, dim3(tiles), dim3(WG), 0, st, r, L);
	hipLaunchKernelGGL(k_isl_flatten, dim3(rowGroups), dim3(WG), 0, st, r, L, rowOff);
	hipLaunchKernelGGL(k_isl_scan, dim3(1), dim3(WG), 0, st, rowOff, rows, rowOff + rows);
	ok = ok && c->be.check(hipGetLastError(), "k_isl launch");
	u32 comps = 0;
	ok = ok && c->be.d2h(&comps, rowOff + rows, 4); // (waits: the records are sized by the number of components)
	if (!ok) return deviceFailed();

	IslCounts hc;
	memset(&hc, 0, sizeof(hc));
	u32 hDirty[6] = { 0, 0, 0, 0, 0, 0 };
	if (comps) {
		const u32 outCap = std::min(capacity, comps);
		auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
		const size_t atRoots = 0, atRecs = pad((size_t)comps * 4), atMarks = atRecs + pad((size_t)comps * sizeof(IslRecord));
		const size_t atList = atMarks + pad(comps), atOut = atList + pad((size_t)comps * 4), need = atOut + pad((size_t)outCap * sizeof(IslRecord));
		if (!dev_grow(c, s->perRecord, s->perRecordCap, need)) return noMemory();
		char* base = (char*)s->perRecord;
		u32* roots = (u32*)(base + atRoots);
		IslRecord* recs = (IslRecord*)(base + atRecs);
		u8* marks = (u8*)(base + atMarks);
		u32* listOff = (u32*)(base + atList);
		IslRecord* out = (IslRecord*)(base + atOut);
		const u32 recGroups = (comps + WG - 1) / WG;
		hipLaunchKernelGGL(k_isl_roots, dim3(rowGroups), dim3(WG), 0, st, r, (const u32*)L, (const u32*)rowOff, roots, recs, comps);
		hipLaunchKernelGGL(k_isl_stats, dim3(tiles), dim3(WG), 0, st, flags, r, (const u32*)L, (const u32*)roots, comps, recs);
		hipLaunchKernelGGL(k_isl_mark, dim3(recGroups), dim3(WG), 0, st, (const IslRecord*)recs, comps, q->flags, q->anchor_faces, (unsigned long long)q->max_voxels, marks, listOff, dCounts, dDirty);
		hipLaunchKernelGGL(k_isl_scan, dim3(1), dim3(WG), 0, st, listOff, comps, dListed);
		if (outCap) hipLaunchKernelGGL(k_isl_compact, dim3(recGroups), dim3(WG), 0, st, (const IslRecord*)recs, comps, (const u8*)marks, (const u32*)listOff, out, outCap);
		if (remove) hipLaunchKernelGGL(k_isl_remove, dim3(tiles), dim3(WG), 0, st, g, r, (const u32*)L, (const u32*)roots, comps, (const u8*)marks, (const u32*)dDirty, (int)q->air_value, (u32*)s->touched, tiles, dCounts);
		ok = c->be.check(hipGetLastError(), "k_isl launch");
		ok = ok && c->be.d2h_async(&hc, dCounts, sizeof(hc)) && c->be.d2h_async(hDirty, dDirty, sizeof(hDirty));
		if (ok && outCap) ok = c->be.d2h_async(islands, out, (size_t)outCap * sizeof(IslRecord)); // (listed <= components: the tail beyond `listed` is not meaningful)
		ok = ok && c->be.sync_ok();
		if (!ok) return deviceFailed();
		if (hc.touched_blocks) { // the flags and the mirrors follow, as after an edit
			hipLaunchKernelGGL(k_edit_flags, dim3(hc.touched_blocks), dim3(WG), 0, st, g, (u8*)c->dFlags, (const u32*)s->touched, hc.touched_blocks);
			ok = c->be.check(hipGetLastError(), "k_edit_flags launch");
			if (ok) rebrick_blocks(c, (const u32*)s->touched, hc.touched_blocks);
			ok = c->be.sync_ok() && ok;
			if (!ok) return deviceFailed();
		}
	}
	memcpy(counts, &hc, sizeof(hc));
	float mn[3], mx[3];
	isl_dirty_box(c->n, hc.removed, hDirty, mn, mx);
	for (int k = 0; k < 3; ++k) { if (out_min) out_min[k] = mn[k]; if (out_max) out_max[k] = mx[k]; }
	if (hc.listed > capacity) return fail(c, VX_ERR_OVERFLOW, std::string(what) + ": " + std::to_string(hc.listed) + " records listed, room for " + std::to_string(capacity));
	return VX_OK;
}

} // extern "C"
