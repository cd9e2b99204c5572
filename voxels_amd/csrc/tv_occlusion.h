// tv_occlusion.h — the arithmetic of vx_occlusion (include/voxels_hip.h, "ambient occlusion", where the rule stands in full).
// DESIGN.md §25.
//
// This header is the one place where the rule is written down, shared by the device kernel (vx_occlusion.inl) and the host build
// of the tests (tests/occlusion/occlusion_host.cpp).  Everything behind the quantisation is int32 arithmetic; the two float32
// expressions of the quantisation are one rounding per written operation (compile with -ffp-contract=off).
//
//   occl_check                       what the entry points refuse
//   occl_dir, OCCL_DIR_TABLE         the 98 step vectors, a literal table
//   occl_quantise                    a vertex -> P (24.8 fixed point, voxels of the level) and N (-127..127), or "not baked"
//   occl_region, occl_row_mask       the staged neighbourhood of a block: one 64-bit sign mask per (y, z) row of lattice points
//   occl_grid_solid                  one lattice point read from the dense field
//   occl_byte                        the probes of one vertex -> its byte; the caller says how a lattice point is looked up
//   occl_vertex_counts, occl_finish  the counts: sums and maxima only (the least byte is kept as the greatest complement)
#pragma once

#include "tv_measure.h"

namespace tv {

typedef uint16_t u16;

enum : u32 { OCCL_MAX_STEPS = 12, OCCL_TRANSITIONS = 1, OCCL_DIRS = 98 };
enum : u32 { OCCL_MAX_EDGE = 16 + 2 * (OCCL_MAX_STEPS + 2) + 1, OCCL_MAX_ROWS = OCCL_MAX_EDGE * OCCL_MAX_EDGE };   // 45 lattice points per axis, 2025 rows

struct OcclParams {          // = vx_occlusion_params
	u32 steps, flags;
	float boxMin[3], boxMax[3];
	u32 reserved[4];
};

struct OcclCounts {          // = vx_occlusion_counts
	u64 vertices, sum;
	u32 entries, visited_entries, darkest, open;
};

// per call, accumulated with integer sums and one maximum: all zero = nothing baked yet
struct OcclSlot {            // 32 bytes
	u64 vertices, sum;
	u32 visited;
	u32 notDarkest;          // greatest 255 - byte
	u32 open, pad;
};

// ---- the entry check ------------------------------------------------------------------------------------------------------------

TV_HD bool occl_nan(float f) { return f != f; }

// what vx_occlusion refuses before anything is launched, given what the context knows; nullptr = fine
TV_HD const char* occl_check(bool wholeGrid, bool haveSurface, u32 levelsRun, u32 level, const OcclParams* p, const void* array, u64 capacity, u64 nVerts)
{
	if (!wholeGrid) return "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)";
	if (!haveSurface) return "no surface (run vx_polygonize first)";
	if (level >= levelsRun) return "no such level";
	if (!p) return "null parameters";
	if (p->steps < 1u || p->steps > OCCL_MAX_STEPS) return "steps must be 1..VX_OCCLUSION_MAX_STEPS";
	if (p->flags & ~(u32)OCCL_TRANSITIONS) return "unknown flag bits";
	if (p->reserved[0] | p->reserved[1] | p->reserved[2] | p->reserved[3]) return "reserved words must be zero";
	for (int a = 0; a < 3; ++a) if (occl_nan(p->boxMin[a]) || occl_nan(p->boxMax[a])) return "NaN box";
	for (int a = 0; a < 3; ++a) if (p->boxMin[a] > p->boxMax[a]) return "box_min > box_max";
	if (!array) return "null array";
	if (capacity < nVerts) return "capacity below the pool's n_verts";
	return nullptr;
}

// an entry is visited by the rule of vx_scatter: its table box meets the filter box
TV_HD bool occl_box_meets(const OcclParams& p, const float minc[3], const float maxc[3])
{
	return minc[0] <= p.boxMax[0] && maxc[0] >= p.boxMin[0] && minc[1] <= p.boxMax[1] && maxc[1] >= p.boxMin[1]
	    && minc[2] <= p.boxMax[2] && maxc[2] >= p.boxMin[2];
}

// ---- directions -----------------------------------------------------------------------------------------------------------------

// The integer vectors d with max(|dx|, |dy|, |dz|) == 2 in ascending order of ((dz + 2) * 5 + (dy + 2)) * 5 + (dx + 2), each as
// S = floor(256 * d / |d| + 0.5) per axis; a row is packed into one word, 10 bits per axis, biased by 512.
#define OCCL_D(x, y, z) ((u32)((x) + 512) | ((u32)((y) + 512) << 10) | ((u32)((z) + 512) << 20))
#define OCCL_DIR_TABLE(D) \
	D(-148,-148,-148), D( -85,-171,-171), D(   0,-181,-181), D(  85,-171,-171), D( 148,-148,-148), D(-171, -85,-171), D(-105,-105,-209), \
	D(   0,-114,-229), D( 105,-105,-209), D( 171, -85,-171), D(-181,   0,-181), D(-114,   0,-229), D(   0,   0,-256), D( 114,   0,-229), \
	D( 181,   0,-181), D(-171,  85,-171), D(-105, 105,-209), D(   0, 114,-229), D( 105, 105,-209), D( 171,  85,-171), D(-148, 148,-148), \
	D( -85, 171,-171), D(   0, 181,-181), D(  85, 171,-171), D( 148, 148,-148), D(-171,-171, -85), D(-105,-209,-105), D(   0,-229,-114), \
	D( 105,-209,-105), D( 171,-171, -85), D(-209,-105,-105), D( 209,-105,-105), D(-229,   0,-114), D( 229,   0,-114), D(-209, 105,-105), \
	D( 209, 105,-105), D(-171, 171, -85), D(-105, 209,-105), D(   0, 229,-114), D( 105, 209,-105), D( 171, 171, -85), D(-181,-181,   0), \
	D(-114,-229,   0), D(   0,-256,   0), D( 114,-229,   0), D( 181,-181,   0), D(-229,-114,   0), D( 229,-114,   0), D(-256,   0,   0), \
	D( 256,   0,   0), D(-229, 114,   0), D( 229, 114,   0), D(-181, 181,   0), D(-114, 229,   0), D(   0, 256,   0), D( 114, 229,   0), \
	D( 181, 181,   0), D(-171,-171,  85), D(-105,-209, 105), D(   0,-229, 114), D( 105,-209, 105), D( 171,-171,  85), D(-209,-105, 105), \
	D( 209,-105, 105), D(-229,   0, 114), D( 229,   0, 114), D(-209, 105, 105), D( 209, 105, 105), D(-171, 171,  85), D(-105, 209, 105), \
	D(   0, 229, 114), D( 105, 209, 105), D( 171, 171,  85), D(-148,-148, 148), D( -85,-171, 171), D(   0,-181, 181), D(  85,-171, 171), \
	D( 148,-148, 148), D(-171, -85, 171), D(-105,-105, 209), D(   0,-114, 229), D( 105,-105, 209), D( 171, -85, 171), D(-181,   0, 181), \
	D(-114,   0, 229), D(   0,   0, 256), D( 114,   0, 229), D( 181,   0, 181), D(-171,  85, 171), D(-105, 105, 209), D(   0, 114, 229), \
	D( 105, 105, 209), D( 171,  85, 171), D(-148, 148, 148), D( -85, 171, 171), D(   0, 181, 181), D(  85, 171, 171), D( 148, 148, 148)

// The table is read with an index every lane of a wave shares: on the device it lives in constant memory, where such a read is
// one scalar load, and no lane keeps it in registers of its own.
static const u32 OCCL_DIR_HOST[OCCL_DIRS] = { OCCL_DIR_TABLE(OCCL_D) };
#if defined(__HIPCC__)
static __constant__ u32 OCCL_DIR_DEVICE[OCCL_DIRS] = { OCCL_DIR_TABLE(OCCL_D) };
#endif

TV_HD void occl_dir(u32 k, int& sx, int& sy, int& sz)
{
#if defined(__HIP_DEVICE_COMPILE__)
	const u32 w = OCCL_DIR_DEVICE[k];
#else
	const u32 w = OCCL_DIR_HOST[k];
#endif
	sx = (int)(w & 1023u) - 512; sy = (int)((w >> 10) & 1023u) - 512; sz = (int)((w >> 20) & 1023u) - 512;
}

// ---- quantisation ---------------------------------------------------------------------------------------------------------------

TV_HD bool occl_finite(float f) { u32 w; memcpy(&w, &f, 4); return (w & 0x7F800000u) != 0x7F800000u; }

TV_HD int occl_normal(float m)
{
	if (!occl_finite(m)) return 0;
	float f = floorf(m * 127.0f + 0.5f);   // (may be an infinity: clamped before it becomes an integer)
	f = f < -127.0f ? -127.0f : f;
	f = f > 127.0f ? 127.0f : f;
	return (int)f;
}

struct OcclVertex { int px, py, pz, nx, ny, nz; };   // grid axes

// pos, nrm: the vertex's, mesh axes (Y up).  false: the vertex is not baked.
TV_HD bool occl_quantise(const float pos[3], const float nrm[3], u32 level, OcclVertex& v)
{
	const float gx = pos[0], gy = pos[2], gz = pos[1];
	if (!(occl_finite(gx) && occl_finite(gy) && occl_finite(gz))) return false;
	if (fabsf(gx) > 4096.0f || fabsf(gy) > 4096.0f || fabsf(gz) > 4096.0f) return false;
	const float scale = 256.0f / (float)(1u << level);
	v.px = (int)floorf(gx * scale + 0.5f); v.py = (int)floorf(gy * scale + 0.5f); v.pz = (int)floorf(gz * scale + 0.5f);
	v.nx = occl_normal(nrm[0]); v.ny = occl_normal(nrm[2]); v.nz = occl_normal(nrm[1]);
	return true;
}

// position and normal out of the 48 bytes of a vx_vertex (pos at 0, nrm at 28)
TV_HD void occl_vertex_read(const void* vertex, float pos[3], float nrm[3])
{
	memcpy(pos, vertex, 12);
	memcpy(nrm, (const char*)vertex + 28, 12);
}

// ---- the grid -------------------------------------------------------------------------------------------------------------------

// lattice points per axis of the level: c is outside the grid where (u32)c >= this (c < 0, or c * s >= n)
TV_HD u32 occl_limit(u32 n, u32 level) { return (n + (1u << level) - 1u) >> level; }

// lattice point c of the level, inside the grid, read from the dense distance field
TV_HD bool occl_grid_solid(const u8* dist, u32 n, u32 level, int cx, int cy, int cz)
{
	return (i8)dist[(((size_t)cz << level) * n + ((size_t)cy << level)) * n + ((size_t)cx << level)] < 0;
}

// The staged neighbourhood of the block at lattice origin 16 * b: `edge` lattice points per axis from 16 * b - reach; the
// kernel's reach is steps + 2, the tests also shrink it.
struct OcclRegion { int x0, y0, z0; u32 edge; };

TV_HD OcclRegion occl_region(u32 bx, u32 by, u32 bz, u32 reach)
{
	OcclRegion r;
	r.x0 = (int)(16u * bx) - (int)reach; r.y0 = (int)(16u * by) - (int)reach; r.z0 = (int)(16u * bz) - (int)reach;
	r.edge = 16u + 2u * reach + 1u;
	return r;
}

// Row `row` (y fastest) of the region: bit i = lattice point (x0 + i, cy, cz) is solid; points outside the grid are air.  At
// level 0 the row is contiguous bytes, read as the 16-byte rows of the level-0 blocks it crosses (n is a multiple of 16), and a
// block whose sign summary (sign: per level-0 block, or null) says one sign is not read; above, a strided read.
TV_HD u64 occl_row_mask(const u8* dist, u32 n, u32 level, const u16* sign, const OcclRegion& r, u32 row)
{
	const int cy = r.y0 + (int)(row % r.edge), cz = r.z0 + (int)(row / r.edge);
	const u32 lim = occl_limit(n, level);
	if ((u32)cy >= lim || (u32)cz >= lim) return 0ull;
	const size_t rowAt = (((size_t)cz << level) * n + ((size_t)cy << level)) * n;
	u64 m = 0ull;
	if (level == 0u) {
		const u32 nb = n >> 4;
		const int end = r.x0 + (int)r.edge;
		for (int xa = r.x0 & ~15; xa < end; xa += 16) {
			if ((u32)xa >= n) continue;
			const u32 summary = sign ? (u32)sign[(((u32)cz >> 4) * nb + ((u32)cy >> 4)) * nb + ((u32)xa >> 4)] & 3u : 0u;
			const u64 bits = summary == 1u ? 0ull : summary == 2u ? 0xFFFFull : (u64)measure_sign_mask(rec_load16(dist + rowAt + (u32)xa));
			const int sh = xa - r.x0;        // -15 .. edge - 1
			m |= sh >= 0 ? bits << sh : bits >> -sh;
		}
		if (r.edge < 64u) m &= (1ull << r.edge) - 1ull;
	} else {
		for (u32 i = 0; i < r.edge; ++i) {
			const int cx = r.x0 + (int)i;
			if ((u32)cx < lim && (i8)dist[rowAt + ((size_t)cx << level)] < 0) m |= 1ull << i;
		}
	}
	return m;
}

// is lattice point c one of the region's, and then which bit of which row
TV_HD bool occl_region_holds(const OcclRegion& r, int cx, int cy, int cz, u32& row, u32& bit)
{
	const u32 lx = (u32)(cx - r.x0), ly = (u32)(cy - r.y0), lz = (u32)(cz - r.z0);
	row = lz * r.edge + ly; bit = lx;
	return lx < r.edge && ly < r.edge && lz < r.edge;
}

// ---- the probes -----------------------------------------------------------------------------------------------------------------

// The byte of one vertex.  solid(cx, cy, cz): is this lattice point INSIDE the grid solid - out of staged masks, or out of the
// grid itself; lim = occl_limit.
template <class Solid> TV_HD u32 occl_byte(const OcclVertex& v, u32 steps, u32 lim, const Solid& solid)
{
	const int ox = v.px + 2 * v.nx, oy = v.py + 2 * v.ny, oz = v.pz + 2 * v.nz;
	u32 tot = 0, occ = 0;
	for (u32 k = 0; k < OCCL_DIRS; ++k) {
		int sx, sy, sz;
		occl_dir(k, sx, sy, sz);
		const int w = (v.nx * sx + v.ny * sy + v.nz * sz) >> 8;
		if (w <= 0) continue;
		tot += (u32)w;
		int qx = ox, qy = oy, qz = oz;
		for (u32 j = 1; j <= steps; ++j) {
			qx += sx; qy += sy; qz += sz;
			const int cx = (qx + 128) >> 8, cy = (qy + 128) >> 8, cz = (qz + 128) >> 8;
			if ((u32)cx >= lim || (u32)cy >= lim || (u32)cz >= lim) break;   // out of the grid: unoccluded
			if (solid(cx, cy, cz)) { occ += (u32)w * (steps + 1u - j); break; }
		}
	}
	tot *= steps;
	return tot ? 255u - (255u * occ) / tot : 255u;
}

// ---- counts ---------------------------------------------------------------------------------------------------------------------

// What one baked vertex adds to the slot, in the layout of measure_reduce: v[0] the maximum of 255 - byte, v[1..5] unused, then
// the sums v[6] vertices, v[7] bytes, v[8] open ones.  `add` accumulates a lane's vertices.
TV_HD void occl_vertex_counts(u32 byte, u32 v[9])
{
	const u32 dark = 255u - byte;
	v[0] = v[0] > dark ? v[0] : dark;
	v[6] += 1u; v[7] += byte; v[8] += byte == 255u ? 1u : 0u;
}

TV_HD OcclCounts occl_finish(const OcclSlot& s, u32 entries)
{
	OcclCounts r;
	r.vertices = s.vertices; r.sum = s.sum;
	r.entries = entries; r.visited_entries = s.visited;
	r.darkest = 255u - s.notDarkest;
	r.open = s.open;
	return r;
}

} // namespace tv
