// tv_island.h — the per-tile logic of vx_grid_islands (include/voxels_hip.h, "detached solid pieces"): connected components
// of the solid voxels of a box of the grid, 6-connectivity.  DESIGN.md §16.
//
// Shared by the device kernels (vx_island.inl) and the sequential CPU emulation of the tests (tests/island/island_host.cpp):
// every function is what ONE lane of a workgroup does in one phase, the caller supplies the lanes (a workgroup, or a loop) and
// the barriers between the phases.  Cells that several lanes update go through an `Ops` policy: relaxed atomics on the
// device, plain reads and writes in the emulation.
//
// The label volume L holds one u32 per voxel of the region, x fastest: ISL_AIR for air, otherwise the region-local index of
// another voxel of the same component that is not larger than the voxel's own - a parent pointer.  A root (L[i] == i) is only
// ever re-pointed to a smaller index, so when all unions are done every component has exactly one root and it is the
// component's least index: the label.  Nothing of that depends on the order in which the unions were served.
#pragma once

#include <stdint.h>
#include <stddef.h>

#if !defined(TV_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TV_HD __host__ __device__ __forceinline__
#else
#include <math.h>
#define TV_HD inline
#endif
#endif

namespace tv {

typedef uint8_t u8;
typedef uint32_t u32;
typedef int8_t i8;

enum : u32 { ISL_AIR = 0xFFFFFFFFu, ISL_HASH_SLOTS = 3072u };
enum { ISL_DETACHED_ONLY = 1, ISL_REMOVE = 2, ISL_MARK_DETACHED = 1, ISL_MARK_LISTED = 2, ISL_MARK_REMOVE = 4 };

struct IslRegion {
	u32 n;               // grid edge
	u32 lo[3], ext[3];   // the box [lo, lo + ext) in grid coordinates (x, y, z internal axes)
	u32 tb0[3], tn[3];   // first block and number of blocks (tiles) per axis
};

struct IslTile {
	u32 block;           // id of the grid block: (bz * nb + by) * nb + bx
	u32 org[3];          // the block's first voxel
	u32 c0[3], c1[3];    // the block clipped to the region, grid coordinates, [c0, c1)
};

struct IslRecord {       // = vx_island
	u32 label, faces;
	unsigned long long voxels;
	u32 min[3], max[3];
};

struct IslCounts {       // = vx_island_counts
	unsigned long long solid_voxels, detached_voxels, removed_voxels;
	u32 components, detached, listed, removed, touched_blocks, reserved;
};

struct IslOpsPlain {
	static TV_HD u32 load(const u32* p) { return *p; }
	static TV_HD u32 amin(u32* p, u32 v) { const u32 o = *p; if (v < o) *p = v; return o; }
	static TV_HD u32 amax(u32* p, u32 v) { const u32 o = *p; if (v > o) *p = v; return o; }
	static TV_HD u32 aadd(u32* p, u32 v) { const u32 o = *p; *p = o + v; return o; }
	static TV_HD u32 aor(u32* p, u32 v) { const u32 o = *p; *p = o | v; return o; }
	static TV_HD u32 cas(u32* p, u32 expect, u32 v) { const u32 o = *p; if (o == expect) *p = v; return o; }
	static TV_HD void aadd64(unsigned long long* p, unsigned long long v) { *p += v; }
};

TV_HD IslRegion isl_region(u32 n, const u32 lo[3], const u32 hi[3])
{
	IslRegion r;
	r.n = n;
	for (int k = 0; k < 3; ++k) {
		r.lo[k] = lo[k]; r.ext[k] = hi[k] - lo[k];
		r.tb0[k] = lo[k] >> 4; r.tn[k] = ((hi[k] + 15u) >> 4) - r.tb0[k];
	}
	return r;
}

TV_HD u32 isl_tiles(const IslRegion& r) { return r.tn[0] * r.tn[1] * r.tn[2]; }
TV_HD u32 isl_rows(const IslRegion& r) { return r.ext[1] * r.ext[2]; }
// region-local linear index of grid voxel (x, y, z)
TV_HD u32 isl_index(const IslRegion& r, u32 x, u32 y, u32 z) { return ((z - r.lo[2]) * r.ext[1] + (y - r.lo[1])) * r.ext[0] + (x - r.lo[0]); }

TV_HD IslTile isl_tile(const IslRegion& r, u32 tile)
{
	IslTile T;
	const u32 b[3] = { r.tb0[0] + tile % r.tn[0], r.tb0[1] + (tile / r.tn[0]) % r.tn[1], r.tb0[2] + tile / (r.tn[0] * r.tn[1]) };
	const u32 nb = r.n >> 4;
	T.block = (b[2] * nb + b[1]) * nb + b[0];
	for (int k = 0; k < 3; ++k) {
		T.org[k] = b[k] * 16u;
		T.c0[k] = T.org[k] > r.lo[k] ? T.org[k] : r.lo[k];
		const u32 end = T.org[k] + 16u, hi = r.lo[k] + r.ext[k];
		T.c1[k] = end < hi ? end : hi;
	}
	return T;
}

// the tile's least region index: its clipped corner
TV_HD u32 isl_tile_first(const IslRegion& r, const IslTile& T) { return isl_index(r, T.c0[0], T.c0[1], T.c0[2]); }
// block-local voxel li = (z * 16 + y) * 16 + x -> region index (the voxel must lie inside the clip)
TV_HD u32 isl_local_to_region(const IslRegion& r, const IslTile& T, u32 li) { return isl_index(r, T.org[0] + (li & 15u), T.org[1] + ((li >> 4) & 15u), T.org[2] + (li >> 8)); }
// is row (y, z) of the block (block-local) inside the clip
TV_HD bool isl_row_inside(const IslTile& T, u32 y, u32 z) { return T.org[1] + y >= T.c0[1] && T.org[1] + y < T.c1[1] && T.org[2] + z >= T.c0[2] && T.org[2] + z < T.c1[2]; }
// the bits of the block-local x positions inside the clip
TV_HD u32 isl_clip_bits(const IslTile& T) { const u32 a = T.c0[0] - T.org[0], b = T.c1[0] - T.org[0]; return ((1u << b) - 1u) & ~((1u << a) - 1u); }

// bit x set <=> sample x of the 16-sample row is solid (< 0: the sign bit reg_case_code reads)
TV_HD u32 isl_solid_bits(const i8* row)
{
	u32 m = 0;
	for (u32 x = 0; x < 16; ++x) m |= (u32)((u8)row[x] >> 7) << x;
	return m;
}

// first position of the run of set bits of `mask` that contains bit x
TV_HD u32 isl_run_head(u32 mask, u32 x)
{
	const u32 zerosBelow = ~mask & ((1u << x) - 1u);
	return zerosBelow ? 32u - (u32)__builtin_clz(zerosBelow) : 0u;
}

template <class O> TV_HD u32 isl_find(const u32* P, u32 i)
{
	for (;;) { const u32 p = O::load(P + i); if (p == i) return i; i = p; }
}

// The larger root goes under the smaller: a minimum on the root's own cell.  When the cell turned out not to be a root any
// more (someone else re-pointed it to `old`), it now holds min(old, b) and the union goes on from (old, b): whichever of the
// two the cell lost is linked again from its root.
template <class O> TV_HD void isl_union(u32* P, u32 a, u32 b)
{
	for (;;) {
		a = isl_find<O>(P, a); b = isl_find<O>(P, b);
		if (a == b) return;
		if (a < b) { const u32 s = a; a = b; b = s; }
		const u32 old = O::amin(P + a, b);
		if (old == a) return;
		a = old;
	}
}

// ---- phase "local": lane t owns row t = (y = t & 15, z = t >> 4) of the block; parent[4096] and masks[256] are the tile's ----

// every solid voxel of the row points at the head of its run
TV_HD void isl_local_init(u32 t, u32 mask, u32* parent)
{
	for (u32 x = 0; x < 16; ++x) parent[t * 16u + x] = (mask >> x) & 1u ? t * 16u + isl_run_head(mask, x) : (u32)ISL_AIR;
}

template <class O> TV_HD void isl_local_link_rows(u32 t, u32 other, const u32* masks, u32* parent)
{
	const u32 mine = masks[t], theirs = masks[other], both = mine & theirs;
	u32 starts = both & ~(both << 1); // one union per pair of overlapping runs: where their overlap begins
	while (starts) {
		const u32 x = (u32)__builtin_ctz(starts);
		starts &= starts - 1u;
		isl_union<O>(parent, t * 16u + isl_run_head(mine, x), other * 16u + isl_run_head(theirs, x));
	}
}

template <class O> TV_HD void isl_local_link(u32 t, const u32* masks, u32* parent)
{
	if (!masks[t]) return;
	if (t & 15u) isl_local_link_rows<O>(t, t - 1u, masks, parent);
	if (t >> 4) isl_local_link_rows<O>(t, t - 16u, masks, parent);
}

// every solid voxel of the row points at its root (other lanes may still be walking through these cells: a cell only ever
// moves to an ancestor)
template <class O> TV_HD void isl_local_flatten(u32 t, u32 mask, u32* parent)
{
	for (u32 x = 0; x < 16; ++x) if ((mask >> x) & 1u) { const u32 root = isl_find<O>(parent, t * 16u + x); parent[t * 16u + x] = root; }
}

// ---- phase "merge": lane t of the tile's workgroup takes one voxel pair of each of the tile's three lower faces ----

template <class O> TV_HD void isl_merge_pair(u32* L, u32 a, u32 b, bool hasPrev)
{
	const u32 la = O::load(L + a), lb = O::load(L + b);
	if (la == (u32)ISL_AIR || lb == (u32)ISL_AIR) return;
	// facing runs along x: the pair before this one already joined the same two provisional trees
	if (hasPrev && O::load(L + a - 1) != (u32)ISL_AIR && O::load(L + b - 1) != (u32)ISL_AIR) return;
	isl_union<O>(L, a, b);
}

template <class O> TV_HD void isl_merge_lane(const IslRegion& r, const IslTile& T, u32 t, u32* L)
{
	const u32 u = t & 15u, v = t >> 4;
	// -z face: (x = u, y = v) against the plane below; -y face: (x = u, z = v); -x face: (y = u, z = v)
	if (T.c0[2] > r.lo[2]) {
		const u32 x = T.org[0] + u, y = T.org[1] + v;
		if (x >= T.c0[0] && x < T.c1[0] && y >= T.c0[1] && y < T.c1[1]) { const u32 a = isl_index(r, x, y, T.c0[2]); isl_merge_pair<O>(L, a, a - r.ext[0] * r.ext[1], x > T.c0[0]); }
	}
	if (T.c0[1] > r.lo[1]) {
		const u32 x = T.org[0] + u, z = T.org[2] + v;
		if (x >= T.c0[0] && x < T.c1[0] && z >= T.c0[2] && z < T.c1[2]) { const u32 a = isl_index(r, x, T.c0[1], z); isl_merge_pair<O>(L, a, a - r.ext[0], x > T.c0[0]); }
	}
	if (T.c0[0] > r.lo[0]) {
		const u32 y = T.org[1] + u, z = T.org[2] + v;
		if (y >= T.c0[1] && y < T.c1[1] && z >= T.c0[2] && z < T.c1[2]) { const u32 a = isl_index(r, T.c0[0], y, z); isl_merge_pair<O>(L, a, a - 1u, false); }
	}
}

// ---- phase "flatten": one voxel; true when it is a root ----
template <class O> TV_HD bool isl_flatten_voxel(u32* L, u32 i)
{
	const u32 l = O::load(L + i);
	if (l == (u32)ISL_AIR) return false;
	const u32 root = isl_find<O>(L, i);
	if (root != l) L[i] = root;
	return root == i;
}

TV_HD IslRecord isl_empty_record(u32 label)
{
	IslRecord e;
	e.label = label; e.faces = 0; e.voxels = 0;
	for (int k = 0; k < 3; ++k) { e.min[k] = 0xFFFFFFFFu; e.max[k] = 0; }
	return e;
}

// position of `label` in the ascending root list (it is there: every final label is a root)
TV_HD u32 isl_search(const u32* roots, u32 count, u32 label)
{
	u32 lo = 0, hi = count;
	while (lo + 1u < hi) { const u32 mid = (lo + hi) >> 1; if (roots[mid] <= label) lo = mid; else hi = mid; }
	return lo;
}

// ---- phase "stats": per tile a table (label -> voxels, occupied x / y / z positions of the block, faces) filled by the
// lanes, then one record update per occupied slot ----

TV_HD u32 isl_faces_of(const IslRegion& r, u32 x0, u32 x1, u32 y, u32 z) // voxels x0 .. x1 of row (y, z), grid coordinates
{
	u32 f = 0;
	if (x0 == r.lo[0]) f |= 1u;
	if (x1 == r.lo[0] + r.ext[0] - 1u) f |= 2u;
	if (y == r.lo[1]) f |= 4u;
	if (y == r.lo[1] + r.ext[1] - 1u) f |= 8u;
	if (z == r.lo[2]) f |= 16u;
	if (z == r.lo[2] + r.ext[2] - 1u) f |= 32u;
	return f;
}

template <class O> TV_HD void isl_table_add(u32* key, u32* cnt, u32* xy, u32* zf, u32 label, u32 count, u32 xbits, u32 y, u32 z, u32 faces)
{
	u32 h = ((label * 2654435761u) >> 12) % (u32)ISL_HASH_SLOTS;
	for (;;) {
		const u32 k = O::cas(key + h, (u32)ISL_AIR, label);
		if (k == (u32)ISL_AIR || k == label) break;
		h = h + 1u == (u32)ISL_HASH_SLOTS ? 0u : h + 1u; // (a tile has at most 2048 components: the table never fills)
	}
	O::aadd(cnt + h, count);
	O::aor(xy + h, xbits | (1u << (16u + y)));
	O::aor(zf + h, (1u << z) | (faces << 16));
}

// lane t: the runs of equal labels of row t into the table
template <class O> TV_HD void isl_stats_row(const IslRegion& r, const IslTile& T, u32 t, const u32* L, u32* key, u32* cnt, u32* xy, u32* zf)
{
	const u32 y = t & 15u, z = t >> 4;
	if (!isl_row_inside(T, y, z)) return;
	const u32 gy = T.org[1] + y, gz = T.org[2] + z, base = isl_index(r, T.c0[0], gy, gz);
	u32 cur = (u32)ISL_AIR, bits = 0;
	const u32 x0 = T.c0[0] - T.org[0], x1 = T.c1[0] - T.org[0];
	for (u32 x = x0; x <= x1; ++x) {
		const u32 l = x < x1 ? L[base + (x - x0)] : (u32)ISL_AIR;
		if (l == cur && bits) { bits |= 1u << x; continue; }
		if (bits) {
			const u32 first = (u32)__builtin_ctz(bits), last = 31u - (u32)__builtin_clz(bits);
			isl_table_add<O>(key, cnt, xy, zf, cur, (u32)__builtin_popcount(bits), bits, y, z, isl_faces_of(r, T.org[0] + first, T.org[0] + last, gy, gz));
		}
		cur = l;
		bits = l != (u32)ISL_AIR ? 1u << x : 0u;
	}
}

template <class O> TV_HD void isl_record_add(IslRecord* rec, unsigned long long voxels, const u32 mn[3], const u32 mx[3], u32 faces)
{
	O::aadd64(&rec->voxels, voxels);
	for (int k = 0; k < 3; ++k) { O::amin(&rec->min[k], mn[k]); O::amax(&rec->max[k], mx[k]); }
	if (faces) O::aor(&rec->faces, faces);
}

template <class O> TV_HD void isl_stats_flush(const IslTile& T, u32 slot, const u32* key, const u32* cnt, const u32* xy, const u32* zf, const u32* roots, u32 count, IslRecord* recs)
{
	if (key[slot] == (u32)ISL_AIR) return;
	const u32 xb = xy[slot] & 0xFFFFu, yb = xy[slot] >> 16, zb = zf[slot] & 0xFFFFu;
	const u32 mn[3] = { T.org[0] + (u32)__builtin_ctz(xb), T.org[1] + (u32)__builtin_ctz(yb), T.org[2] + (u32)__builtin_ctz(zb) };
	const u32 mx[3] = { T.org[0] + 31u - (u32)__builtin_clz(xb), T.org[1] + 31u - (u32)__builtin_clz(yb), T.org[2] + 31u - (u32)__builtin_clz(zb) };
	isl_record_add<O>(recs + isl_search(roots, count, key[slot]), cnt[slot], mn, mx, zf[slot] >> 16);
}

// a tile whose block is BF_Empty and solid: one component, the whole clip
template <class O> TV_HD void isl_stats_uniform(const IslRegion& r, const IslTile& T, u32 label, const u32* roots, u32 count, IslRecord* recs)
{
	const u32 mx[3] = { T.c1[0] - 1u, T.c1[1] - 1u, T.c1[2] - 1u };
	const u32 faces = (isl_faces_of(r, T.c0[0], mx[0], T.c0[1], T.c0[2]) & 0x15u) | (isl_faces_of(r, T.c0[0], mx[0], mx[1], mx[2]) & 0x2Au);
	isl_record_add<O>(recs + isl_search(roots, count, label), (unsigned long long)(T.c1[0] - T.c0[0]) * (T.c1[1] - T.c0[1]) * (T.c1[2] - T.c0[2]), T.c0, mx, faces);
}

// ---- phase "mark": one record -> ISL_MARK_* bits, the counts, the box of what is removed (dirty[0..2] = ~min, [3..5] = max,
// all zero before: maxima only) ----
template <class O> TV_HD u32 isl_mark(const IslRecord& e, u32 flags, u32 anchorFaces, unsigned long long maxVoxels, IslCounts* counts, u32* dirty)
{
	u32 m = 0;
	O::aadd(&counts->components, 1u);
	O::aadd64(&counts->solid_voxels, e.voxels);
	if ((e.faces & anchorFaces) == 0) {
		m |= (u32)ISL_MARK_DETACHED;
		O::aadd(&counts->detached, 1u);
		O::aadd64(&counts->detached_voxels, e.voxels);
		if ((flags & (u32)ISL_REMOVE) && (maxVoxels == 0 || e.voxels <= maxVoxels)) {
			m |= (u32)ISL_MARK_REMOVE;
			O::aadd(&counts->removed, 1u);
			O::aadd64(&counts->removed_voxels, e.voxels);
			for (int k = 0; k < 3; ++k) { O::amax(dirty + k, ~e.min[k]); O::amax(dirty + 3 + k, e.max[k]); }
		}
	}
	if (!(flags & (u32)ISL_DETACHED_ONLY) || (m & (u32)ISL_MARK_DETACHED)) { m |= (u32)ISL_MARK_LISTED; O::aadd(&counts->listed, 1u); }
	return m;
}

// ---- phase "remove": lane t rewrites the voxels of row t that belong to a marked record; row = the block's 16 samples ----
TV_HD bool isl_tile_in_dirty(const IslTile& T, const u32* dirty)
{
	for (int k = 0; k < 3; ++k) if (T.c1[k] <= ~dirty[k] || T.c0[k] > dirty[3 + k]) return false;
	return true;
}

TV_HD bool isl_remove_row(const IslRegion& r, const IslTile& T, u32 t, const u32* L, const u32* roots, u32 count, const u8* marks, i8 air, i8* row)
{
	const u32 y = t & 15u, z = t >> 4;
	if (!isl_row_inside(T, y, z)) return false;
	const u32 base = isl_index(r, T.c0[0], T.org[1] + y, T.org[2] + z), x0 = T.c0[0] - T.org[0], x1 = T.c1[0] - T.org[0];
	u32 cur = (u32)ISL_AIR;
	bool gone = false, changed = false;
	for (u32 x = x0; x < x1; ++x) {
		const u32 l = L[base + (x - x0)];
		if (l == (u32)ISL_AIR) continue;
		if (l != cur) { cur = l; gone = (marks[isl_search(roots, count, l)] & (u32)ISL_MARK_REMOVE) != 0; }
		if (gone) { row[x] = air; changed = true; }
	}
	return changed;
}

// BF_Empty by the codec's rule (edit_block_empty of tv_block.h) on a dense whole grid
TV_HD u8 isl_block_empty(const i8* dist, u32 n, u32 block)
{
	const u32 nb = n >> 4, bx = block % nb, by = (block / nb) % nb, bz = block / (nb * nb);
	const i8* base = dist + ((size_t)(bz * 16u) * n + by * 16u) * n + bx * 16u;
	const i8 first = base[0];
	i8 last = first;
	u32 counter = 0, size = 1;
	bool empty = true;
	for (u32 z = 0; z < 16; ++z)
	for (u32 y = 0; y < 16; ++y) {
		const i8* row = base + ((size_t)z * n + y) * n;
		for (u32 x = 0; x < 16; ++x) {
			const i8 cur = row[x];
			if (last == cur && counter < 0xFF) { ++counter; continue; }
			size += 2; counter = 1; last = cur;
			if ((int)first * (int)last <= 0) empty = false;
			if (size > 4096) return 0;
		}
	}
	return empty ? 1 : 0;
}

// the box handed back after a removal: output order (x, z, y), [a, b + 1] clamped to [0, n]; zeros when nothing was removed
TV_HD void isl_dirty_box(u32 n, u32 removed, const u32* dirty, float outMin[3], float outMax[3])
{
	const int order[3] = { 0, 2, 1 };
	for (int k = 0; k < 3; ++k) {
		const u32 a = ~dirty[order[k]], b = dirty[3 + order[k]] + 1u;
		outMin[k] = removed ? (float)(a < n ? a : n) : 0.f;
		outMax[k] = removed ? (float)(b < n ? b : n) : 0.f;
	}
}

} // namespace tv
