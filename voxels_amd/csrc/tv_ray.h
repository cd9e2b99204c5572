// tv_ray.h — the box arithmetic and the ray-triangle test of the ray casts (vx_ray.inl), host and device.
//
// A level's index (vx_ray.inl, k_ray_index) sorts the triangles of every listed block into the 4 x 4 x 4 sub-bricks of the
// block (a sub-brick = 4^3 cells); k_raycast walks the level's block grid and then the sub-bricks of a meshed block with the
// same DDA (Amanatides and Woo 1987).  Both take block origins, sub-brick boxes and bucket numbers from here, so that what the
// build puts into a bucket is what the traversal finds there.
//
// Mesh space (vx_vertex.pos) is Y-up; the block coordinates of the tables are internal (Z-up): block (bx, by, bz) of level L
// covers mesh x in [bx S, (bx+1) S], mesh y in [bz S, ...], mesh z in [by S, ...] with S = 16 * 2^L.
#pragma once

#include "tv_core.h"

namespace tv {

enum : u32 { RAY_SUB = 4, RAY_BUCKETS = 64, RAY_NONE = 0xFFFFFFFFu };

TV_HD float ray_inf() { return __builtin_huge_valf(); }

// internal coordinate id (bz * cnt + by) * cnt + bx of the block at mesh-space cell (mx, my, mz) of the level's block grid
TV_HD u32 ray_coord_id(const int m[3], u32 cnt) { return ((u32)m[1] * cnt + (u32)m[2]) * cnt + (u32)m[0]; }

// mesh-space origin of the block with internal coordinate id `coord`
TV_HD void ray_block_origin(u32 coord, u32 cnt, float size, float out[3])
{
	const u32 bx = coord % cnt, by = (coord / cnt) % cnt, bz = coord / (cnt * cnt);
	out[0] = (float)bx * size; out[1] = (float)bz * size; out[2] = (float)by * size;
}

// sub-brick of a point of a block (clamped: points on the block's far faces belong to the last sub-brick)
TV_HD int ray_sub_of(float p, float origin, float subSize)
{
	const float f = floorf((p - origin) / subSize);
	return f < 0.f ? 0 : (f > (float)(RAY_SUB - 1) ? (int)RAY_SUB - 1 : (int)f);
}

TV_HD u32 ray_bucket(const int s[3]) { return ((u32)s[2] * RAY_SUB + (u32)s[1]) * RAY_SUB + (u32)s[0]; }

// the segment [t0, t1] of the ray o + t d inside the closed box [0, extent]^3; false if empty.  inv[a] = 1 / d[a] (0 where
// d[a] = 0: that axis is tested on the origin alone)
TV_HD bool ray_clip_cube(const float o[3], const float d[3], const float inv[3], float extent, float& t0, float& t1)
{
	for (int a = 0; a < 3; ++a) {
		if (d[a] == 0.f) {
			if (!(o[a] >= 0.f && o[a] <= extent)) return false;
			continue;
		}
		float ta = (0.f - o[a]) * inv[a], tb = (extent - o[a]) * inv[a];
		if (ta > tb) { const float x = ta; ta = tb; tb = x; }
		t0 = ta > t0 ? ta : t0;
		t1 = tb < t1 ? tb : t1;
	}
	return t0 <= t1;
}

// 3-D DDA over a grid of count^3 cubes of edge `size` starting at `origin`: cell = the cube that holds the point at t,
// next[a] = the t where the ray leaves it across axis a (exact boundary positions, no accumulated increments)
struct RayDda {
	int cell[3];
	int step[3];
	float next[3];
	int axis; // the axis the last advance crossed (-1 before the first)

	TV_HD void boundary(int a, const float o[3], const float inv[3], const float origin[3], float size)
	{
		next[a] = step[a] == 0 ? ray_inf() : (origin[a] + (float)(cell[a] + (step[a] > 0 ? 1 : 0)) * size - o[a]) * inv[a];
	}
	TV_HD void init(const float o[3], const float d[3], const float inv[3], float t, const float origin[3], float size, int count)
	{
		for (int a = 0; a < 3; ++a) {
			const float p = o[a] + t * d[a];
			const float f = floorf((p - origin[a]) / size);
			cell[a] = f < 0.f ? 0 : (f > (float)(count - 1) ? count - 1 : (int)f);
			step[a] = d[a] > 0.f ? 1 : (d[a] < 0.f ? -1 : 0);
			boundary(a, o, inv, origin, size);
		}
		axis = -1;
	}
	TV_HD float exit_t() const
	{
		const float m = next[0] < next[1] ? next[0] : next[1];
		return m < next[2] ? m : next[2];
	}
	// to the neighbour across the nearest boundary; false when that leaves the grid
	TV_HD bool advance(const float o[3], const float inv[3], const float origin[3], float size, int count)
	{
		const int a = next[0] <= next[1] ? (next[0] <= next[2] ? 0 : 2) : (next[1] <= next[2] ? 1 : 2);
		cell[a] += step[a];
		axis = a;
		if (cell[a] < 0 || cell[a] >= count) return false;
		boundary(a, o, inv, origin, size);
		return true;
	}
};

// Which neighbours of a sub-brick the segment [tIn, tOut] of the ray passes within eps of: near[a] = -1 / +1 when the
// segment's coordinate along axis a comes within eps of the box's lower / upper face without crossing it there (the faces
// it enters and leaves by, entryAxis and exitAxis, lead to boxes the DDA visits anyway), 0 otherwise.  A ray that passes
// along an edge or a corner of the sub-brick grid may find the triangle the watertight test hits there in a box it never
// enters (the test decides within rounding of the exact geometry); those boxes are searched too.
TV_HD bool ray_near_faces(const float o[3], const float d[3], float tIn, float tOut, const float lo[3], float size, const int step[3],
                          int entryAxis, int exitAxis, float eps, int near[3])
{
	bool any = false;
	for (int a = 0; a < 3; ++a) {
		const float pa = o[a] + tIn * d[a], pb = o[a] + tOut * d[a];
		const float mn = pa < pb ? pa : pb, mx = pa < pb ? pb : pa;
		const bool crossLo = (a == entryAxis && step[a] > 0) || (a == exitAxis && step[a] < 0);
		const bool crossHi = (a == entryAxis && step[a] < 0) || (a == exitAxis && step[a] > 0);
		near[a] = (!crossLo && mn - lo[a] < eps) ? -1 : ((!crossHi && lo[a] + size - mx < eps) ? 1 : 0);
		any = any || near[a] != 0;
	}
	return any;
}

// Watertight ray-triangle intersection (Woop, Benthin, Wald, "Watertight Ray/Triangle Intersection", JCGT 2(1), 2013), both
// faces.  The edge functions of a shared edge are computed from the same two projected vertices in both triangles, with
// the factors of each product in the same order, so that they are exact negatives of each other (this needs
// -ffp-contract=off, which the library is built with); a zero is recomputed in double precision.
struct RayShear {
	int kx, ky, kz;
	float sx, sy, sz;
};

TV_HD RayShear ray_shear(const float d[3])
{
	RayShear r;
	const float ax = fabsf(d[0]), ay = fabsf(d[1]), az = fabsf(d[2]);
	r.kz = ax > ay ? (ax > az ? 0 : 2) : (ay > az ? 1 : 2);
	r.kx = r.kz == 2 ? 0 : r.kz + 1;
	r.ky = r.kx == 2 ? 0 : r.kx + 1;
	if (d[r.kz] < 0.f) { const int k = r.kx; r.kx = r.ky; r.ky = k; } // keeps the winding (both faces count either way)
	r.sx = d[r.kx] / d[r.kz];
	r.sy = d[r.ky] / d[r.kz];
	r.sz = 1.f / d[r.kz];
	return r;
}

// hit: t (units of |d|), u, v = weights of the triangle's 2nd and 3rd vertex
TV_HD bool ray_triangle(const RayShear& r, const float o[3], const float A[3], const float B[3], const float C[3], float& t, float& u, float& v)
{
	const float az = A[r.kz] - o[r.kz], bz = B[r.kz] - o[r.kz], cz = C[r.kz] - o[r.kz];
	const float ax = (A[r.kx] - o[r.kx]) - r.sx * az, ay = (A[r.ky] - o[r.ky]) - r.sy * az;
	const float bx = (B[r.kx] - o[r.kx]) - r.sx * bz, by = (B[r.ky] - o[r.ky]) - r.sy * bz;
	const float cx = (C[r.kx] - o[r.kx]) - r.sx * cz, cy = (C[r.ky] - o[r.ky]) - r.sy * cz;
	float U = cx * by - cy * bx;
	float V = ax * cy - ay * cx;
	float W = bx * ay - by * ax;
	if (U == 0.f || V == 0.f || W == 0.f) {
		U = (float)((double)cx * (double)by - (double)cy * (double)bx);
		V = (float)((double)ax * (double)cy - (double)ay * (double)cx);
		W = (float)((double)bx * (double)ay - (double)by * (double)ax);
	}
	if ((U < 0.f || V < 0.f || W < 0.f) && (U > 0.f || V > 0.f || W > 0.f)) return false;
	const float det = U + V + W;
	if (det == 0.f) return false;
	const float T = U * (r.sz * az) + V * (r.sz * bz) + W * (r.sz * cz);
	t = T / det;
	u = V / det;
	v = W / det;
	return true;
}

} // namespace tv
