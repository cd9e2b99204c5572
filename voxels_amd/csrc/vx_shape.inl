// vx_shape.inl — sphere casts and closest-point queries against the regular meshes of one LOD level (include/voxels_hip.h,
// "sphere casts and closest points"); included by vx_hip.hip after vx_ray.inl, whose per-level index they read (HIP only).
//
// Both rely on the index's invariant (vx_ray.inl): every triangle lies inside the closed box of its bucket's sub-brick,
// within +-1/256 (`straddling` = 0).  So a triangle within r of a point lies in a bucket whose box is within r + 1/256 of it.
//   k_spherecast     one lane per cast: a DDA over the level's sub-brick grid, dilated by r + 1/256, along the centre line;
//                    for each cell the buckets within r + 1/256 of it are tested (the whole cube around the first cell, then
//                    only the slab that a step brings in: every triangle is tested over the whole t window, so a bucket
//                    already tested need not be tested again).  The walk ends after the cell whose exit is >= the best t.
//   k_closest_point  one lane per query: blocks in growing Chebyshev rings around the query, then the buckets of a meshed
//                    block, each pruned by its box distance minus 1/256 against min(best, max_dist).
// DESIGN.md §14 gives the argument.  Sphere-triangle arithmetic: tv_shape.h.
#include "tv_shape.h"

namespace {

struct ShapeParams {
	const float4* in;     // vx_sphere_cast (three float4) / vx_point_query (one)
	float4* out;          // vx_sphere_hit (four float4) / vx_point_hit (three)
	u32 n;
	const u32* map;
	const u16* starts;
	const u16* perm;
	const ListedBlock* table;
	const PolyVertex* verts;
	const u32* idx;
	u32 cnt;              // blocks per axis of the level
	float size;           // block edge in voxels
};

// the key: least t (or dist), then the nearer start contact, then the smallest (entry, tri)
struct ShapeBest {
	float t, dist;
	u32 e, tri;
	bool start;
};

__device__ __forceinline__ bool shape_before(float t, float dist, u32 e, u32 tri, const ShapeBest& b)
{
	return t < b.t || (t == b.t && (dist < b.dist || (dist == b.dist && (e < b.e || (e == b.e && tri < b.tri)))));
}

__device__ __forceinline__ SV shape_vertex(const PolyVertex* v, u32 i)
{
	const float4 q = *(const float4*)&v[i];
	return sv(q.x, q.y, q.z);
}

struct SphereCast {
	SV o, d;
	float r, tLo, tHi;
};

// the triangles of the bucket of world sub-brick s (mesh-space axes, may lie outside the level) against the cast
__device__ __forceinline__ void sphere_test_bucket(const ShapeParams& p, const SphereCast& c, int sx, int sy, int sz, ShapeBest& best)
{
	const int cs = (int)(p.cnt * RAY_SUB);
	if (sx < 0 || sy < 0 || sz < 0 || sx >= cs || sy >= cs || sz >= cs) return;
	const int blk[3] = { sx / (int)RAY_SUB, sy / (int)RAY_SUB, sz / (int)RAY_SUB };
	const u32 e = p.map[ray_coord_id(blk, p.cnt)];
	if (e == RAY_NONE) return;
	const int s[3] = { sx % (int)RAY_SUB, sy % (int)RAY_SUB, sz % (int)RAY_SUB };
	const u32 bucket = ray_bucket(s);
	const u16* starts = p.starts + (size_t)e * (RAY_BUCKETS + 1);
	const u32 k0 = starts[bucket], k1 = starts[bucket + 1];
	if (k0 == k1) return;
	const ListedBlock& b = p.table[e];
	const PolyVertex* v = p.verts + b.rec.vOff;
	const u32* ix = p.idx + b.rec.iOff;
	const u16* perm = p.perm + b.rec.iOff / 3;
	for (u32 k = k0; k < k1; ++k) {
		const u32 tri = perm[k];
		const SV A = shape_vertex(v, ix[3 * tri]), B = shape_vertex(v, ix[3 * tri + 1]), C = shape_vertex(v, ix[3 * tri + 2]);
		float t, dist;
		bool start;
		if (!shape_sphere_triangle(c.o, c.d, c.r, c.tLo, c.tHi, A, B, C, t, dist, start)) continue;
		if (shape_before(t, dist, e, tri, best)) { best.t = t; best.dist = dist; best.e = e; best.tri = tri; best.start = start; }
	}
}

// the buckets (x0..x1, y0..y1, z0..z1) of world sub-bricks, clipped to the level
__device__ __forceinline__ void sphere_test_range(const ShapeParams& p, const SphereCast& c, int x0, int x1, int y0, int y1, int z0, int z1, ShapeBest& best)
{
	const int cs = (int)(p.cnt * RAY_SUB);
	x0 = max(x0, 0); y0 = max(y0, 0); z0 = max(z0, 0);
	x1 = min(x1, cs - 1); y1 = min(y1, cs - 1); z1 = min(z1, cs - 1);
	for (int z = z0; z <= z1; ++z)
		for (int y = y0; y <= y1; ++y)
			for (int x = x0; x <= x1; ++x) sphere_test_bucket(p, c, x, y, z, best);
}

__global__ __launch_bounds__(WG) void k_spherecast(ShapeParams p)
{
	const u32 i = blockIdx.x * WG + threadIdx.x;
	if (i >= p.n) return;
	const float4 c0 = p.in[3 * i], c1 = p.in[3 * i + 1], c2 = p.in[3 * i + 2];
	SphereCast c;
	c.o = sv(c0.x, c0.y, c0.z);
	c.d = sv(c1.x, c1.y, c1.z);
	c.r = c2.x;
	c.tLo = c0.w;
	c.tHi = c1.w;
	ShapeBest best = { ray_inf(), ray_inf(), RAY_NONE, RAY_NONE, false };
	const bool valid = !(c.o.x != c.o.x || c.o.y != c.o.y || c.o.z != c.o.z || c.d.x != c.d.x || c.d.y != c.d.y || c.d.z != c.d.z)
	                   && c.r > 0.f && c.r < ray_inf() && c.tLo <= c.tHi;
	if (valid) {
		const int cs = (int)(p.cnt * RAY_SUB);
		const float sub = p.size / (float)RAY_SUB, extent = (float)p.cnt * p.size;
		// reach: a triangle within r of the centre lies in a bucket within m of the centre's cell (+ rounding of the DDA)
		const float m = c.r + (1.f / 256.f) + extent * 1e-6f;
		const float kf = floorf(m / sub) + 1.f;
		const int k = kf >= (float)cs ? cs : (int)kf;
		// the centre line clipped to the level dilated by m, walked over a grid of sub-bricks dilated by k (shifted by +m)
		const float o[3] = { c.o.x + m, c.o.y + m, c.o.z + m }, d[3] = { c.d.x, c.d.y, c.d.z };
		const float inv[3] = { d[0] != 0.f ? 1.f / d[0] : 0.f, d[1] != 0.f ? 1.f / d[1] : 0.f, d[2] != 0.f ? 1.f / d[2] : 0.f };
		const float org[3] = { m - (float)k * sub, m - (float)k * sub, m - (float)k * sub };
		float t0 = c.tLo, t1 = c.tHi;
		if (ray_clip_cube(o, d, inv, extent + 2.f * m, t0, t1)) {
			RayDda dda;
			dda.init(o, d, inv, t0, org, sub, cs + 2 * k);
			// the cube of world sub-bricks (DDA cell - k) +- k around the first cell; a reach of the whole level is one cube
			const bool whole = k == cs;
			int lo[3], hi[3];
			for (int a = 0; a < 3; ++a) { lo[a] = whole ? 0 : dda.cell[a] - 2 * k; hi[a] = whole ? cs - 1 : dda.cell[a]; }
			for (;;) {
				sphere_test_range(p, c, lo[0], hi[0], lo[1], hi[1], lo[2], hi[2], best);
				const float tExit = fminf(dda.exit_t(), t1);
				if (whole || best.t <= tExit || tExit >= t1 || !dda.advance(o, inv, org, sub, cs + 2 * k)) break;
				// the slab that the step across dda.axis brings into the cube
				for (int a = 0; a < 3; ++a) {
					const int w = dda.cell[a] - k + (a == dda.axis ? dda.step[a] * k : 0);
					lo[a] = a == dda.axis ? w : dda.cell[a] - 2 * k;
					hi[a] = a == dda.axis ? w : dda.cell[a];
				}
			}
		}
	}
	float4 h0 = make_float4(ray_inf(), 0.f, 0.f, 0.f), h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2, h3;
	if (best.e != RAY_NONE) {
		const ListedBlock& b = p.table[best.e];
		const PolyVertex* v = p.verts + b.rec.vOff;
		const u32* ix = p.idx + b.rec.iOff + 3 * best.tri;
		const SV A = shape_vertex(v, ix[0]), B = shape_vertex(v, ix[1]), C = shape_vertex(v, ix[2]);
		const bool moving = c.d.x != 0.f || c.d.y != 0.f || c.d.z != 0.f;
		const SV p0 = sv_sub(c.o, A);
		const SV pr = moving ? sv_add(p0, sv_mul(c.d, best.t)) : p0;      // the centre relative to A
		float vv, ww;
		const SV qr = shape_closest_rel(pr, sv_sub(B, A), sv_sub(C, A), vv, ww);
		const SV g = sv_sub(pr, qr);
		const float len = sqrtf(sv_dot(g, g));
		SV nrm;
		if (len > 0.f) {
			nrm = sv_mul(g, 1.f / len);
		} else {
			const SV e1 = sv_sub(B, A), e2 = sv_sub(C, A);
			const double ex = e1.x, ey = e1.y, ez = e1.z, fx = e2.x, fy = e2.y, fz = e2.z;
			const double nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
			const double l = sqrt(nx * nx + ny * ny + nz * nz);
			const double s = l > 0.0 ? 1.0 / l : 0.0;
			nrm = sv((float)(nx * s), (float)(ny * s), (float)(nz * s));
		}
		const SV ctr = moving ? sv_add(c.o, sv_mul(c.d, best.t)) : c.o;
		const SV con = sv_add(A, qr);
		h0 = make_float4(best.t, ctr.x, ctr.y, ctr.z);
		h1 = make_float4(con.x, con.y, con.z, nrm.x);
		h2 = make_float4(nrm.y, nrm.z, best.start ? c.r - best.dist : 0.f, __uint_as_float(best.e));
		h3 = make_float4(__uint_as_float(b.id), __uint_as_float(best.tri), __uint_as_float(best.start ? 1u : 0u), 0.f);
	} else {
		h2 = make_float4(0.f, 0.f, 0.f, __uint_as_float(RAY_NONE));
		h3 = make_float4(__uint_as_float(RAY_NONE), __uint_as_float(RAY_NONE), 0.f, 0.f);
	}
	p.out[4 * i] = h0;
	p.out[4 * i + 1] = h1;
	p.out[4 * i + 2] = h2;
	p.out[4 * i + 3] = h3;
}

// distance from x to the interval [lo, hi] along one axis
__device__ __forceinline__ float shape_gap(float x, float lo, float hi)
{
	return x < lo ? lo - x : (x > hi ? x - hi : 0.f);
}

__device__ __forceinline__ float shape_box_dist(SV q, float x0, float y0, float z0, float edge)
{
	const float gx = shape_gap(q.x, x0, x0 + edge), gy = shape_gap(q.y, y0, y0 + edge), gz = shape_gap(q.z, z0, z0 + edge);
	return sqrtf(gx * gx + gy * gy + gz * gz);
}

// the buckets of table entry e (block at mesh-space cell bx, by, bz) against the query
__device__ __forceinline__ void point_test_block(const ShapeParams& p, SV q, float maxd, u32 e, int bx, int by, int bz, ShapeBest& best)
{
	const ListedBlock& b = p.table[e];
	const PolyVertex* v = p.verts + b.rec.vOff;
	const u32* ix = p.idx + b.rec.iOff;
	const u16* perm = p.perm + b.rec.iOff / 3;
	const u16* starts = p.starts + (size_t)e * (RAY_BUCKETS + 1);
	const float sub = p.size / (float)RAY_SUB, margin = 1.f / 256.f;
	u32 k0 = starts[0];
	for (u32 bucket = 0; bucket < RAY_BUCKETS; ++bucket) {
		const u32 k1 = starts[bucket + 1];
		const u32 kb = k0;
		k0 = k1;
		if (kb == k1) continue;
		const u32 sx = bucket % RAY_SUB, sy = (bucket / RAY_SUB) % RAY_SUB, sz = bucket / (RAY_SUB * RAY_SUB);
		const float bound = fminf(best.dist, maxd);
		if (shape_box_dist(q, (float)bx * p.size + (float)sx * sub, (float)by * p.size + (float)sy * sub, (float)bz * p.size + (float)sz * sub, sub) - margin > bound)
			continue;
		for (u32 k = kb; k < k1; ++k) {
			const u32 tri = perm[k];
			const SV A = shape_vertex(v, ix[3 * tri]), B = shape_vertex(v, ix[3 * tri + 1]), C = shape_vertex(v, ix[3 * tri + 2]);
			const SV pr = sv_sub(q, A);
			float vv, ww;
			const SV g = sv_sub(pr, shape_closest_rel(pr, sv_sub(B, A), sv_sub(C, A), vv, ww));
			const float dist = sqrtf(sv_dot(g, g));
			if (dist <= maxd && shape_before(dist, dist, e, tri, best)) { best.t = dist; best.dist = dist; best.e = e; best.tri = tri; }
		}
	}
}

__global__ __launch_bounds__(WG) void k_closest_point(ShapeParams p)
{
	const u32 i = blockIdx.x * WG + threadIdx.x;
	if (i >= p.n) return;
	const float4 in = p.in[i];
	const SV q = sv(in.x, in.y, in.z);
	const float maxd = in.w;
	// best.t = best.dist = the distance (start, the second key, is not used)
	ShapeBest best = { ray_inf(), ray_inf(), RAY_NONE, RAY_NONE, false };
	const bool valid = !(q.x != q.x || q.y != q.y || q.z != q.z) && maxd >= 0.f;
	if (valid) {
		const int cnt = (int)p.cnt;
		const float margin = 1.f / 256.f;
		const float qa[3] = { q.x, q.y, q.z };
		int h[3];
		for (int a = 0; a < 3; ++a) {
			const float f = floorf(qa[a] / p.size);
			h[a] = f < 0.f ? 0 : (f > (float)(cnt - 1) ? cnt - 1 : (int)f);
		}
		for (int R = 0;; ++R) {
			const float bound = fminf(best.dist, maxd);
			if (R > 0) {
				// the ring's blocks each lie on one of its six faces: the least distance to a face column that exists
				float lb = ray_inf();
				for (int a = 0; a < 3; ++a) {
					const int j0 = h[a] - R, j1 = h[a] + R;
					if (j0 >= 0) lb = fminf(lb, shape_gap(qa[a], (float)j0 * p.size, (float)(j0 + 1) * p.size));
					if (j1 < cnt) lb = fminf(lb, shape_gap(qa[a], (float)j1 * p.size, (float)(j1 + 1) * p.size));
				}
				if (lb == ray_inf() || lb - margin > bound) break;   // (no block left in this ring or any later one / too far)
			}
			const int z0 = max(h[2] - R, 0), z1 = min(h[2] + R, cnt - 1), y0 = max(h[1] - R, 0), y1 = min(h[1] + R, cnt - 1);
			for (int z = z0; z <= z1; ++z)
				for (int y = y0; y <= y1; ++y) {
					const bool face = z == h[2] - R || z == h[2] + R || y == h[1] - R || y == h[1] + R;
					const int xs = face ? 1 : 2 * R;   // inside the ring's yz square only the two x faces
					for (int x = h[0] - R; x <= h[0] + R; x += (xs > 0 ? xs : 1)) {
						if (x < 0 || x >= cnt) continue;
						if (shape_box_dist(q, (float)x * p.size, (float)y * p.size, (float)z * p.size, p.size) - margin > fminf(best.dist, maxd)) continue;
						const int m[3] = { x, y, z };
						const u32 e = p.map[ray_coord_id(m, p.cnt)];
						if (e != RAY_NONE) point_test_block(p, q, maxd, e, x, y, z, best);
					}
				}
		}
	}
	float4 h0 = make_float4(ray_inf(), 0.f, 0.f, 0.f), h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2;
	if (best.e != RAY_NONE) {
		const ListedBlock& b = p.table[best.e];
		const PolyVertex* v = p.verts + b.rec.vOff;
		const u32* ix = p.idx + b.rec.iOff + 3 * best.tri;
		const SV A = shape_vertex(v, ix[0]), B = shape_vertex(v, ix[1]), C = shape_vertex(v, ix[2]);
		float vv, ww;
		const SV qr = shape_closest_rel(sv_sub(q, A), sv_sub(B, A), sv_sub(C, A), vv, ww);
		const SV pt = sv_add(A, qr);
		const double ex = (double)B.x - A.x, ey = (double)B.y - A.y, ez = (double)B.z - A.z;
		const double fx = (double)C.x - A.x, fy = (double)C.y - A.y, fz = (double)C.z - A.z;
		const double nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
		const double len = sqrt(nx * nx + ny * ny + nz * nz);
		const double s = len > 0.0 ? 1.0 / len : 0.0;
		h0 = make_float4(best.dist, pt.x, pt.y, pt.z);
		h1 = make_float4((float)(nx * s), (float)(ny * s), (float)(nz * s), vv);
		h2 = make_float4(ww, __uint_as_float(best.e), __uint_as_float(b.id), __uint_as_float(best.tri));
	} else {
		h2 = make_float4(0.f, __uint_as_float(RAY_NONE), __uint_as_float(RAY_NONE), __uint_as_float(RAY_NONE));
	}
	p.out[3 * i] = h0;
	p.out[3 * i + 1] = h1;
	p.out[3 * i + 2] = h2;
}

ShapeParams shape_params(vx_ctx* c, uint32_t level, const void* in, uint32_t n, void* out)
{
	const RayState* s = module_peek<RayState>(c, MOD_RAY);
	const RayLevel& l = s->lv[level];
	ShapeParams p;
	p.in = (const float4*)in;
	p.out = (float4*)out;
	p.n = n;
	p.map = l.map;
	p.starts = l.starts;
	p.perm = s->perm;
	p.table = l.table;
	p.verts = (const PolyVertex*)c->dVerts;
	p.idx = (const u32*)c->dIdx;
	p.cnt = c->lv[level].cnt;
	p.size = (float)(16u << level);
	return p;
}

int shape_launch(vx_ctx* c, uint32_t level, bool sphere, const void* dIn, uint32_t n, void* dOut)
{
	const ShapeParams p = shape_params(c, level, dIn, n, dOut);
	if (sphere) hipLaunchKernelGGL(k_spherecast, dim3((n + WG - 1) / WG), dim3(WG), 0, c->be.stream, p);
	else hipLaunchKernelGGL(k_closest_point, dim3((n + WG - 1) / WG), dim3(WG), 0, c->be.stream, p);
	const char* what = sphere ? "vx_spherecast" : "vx_closest_point";
	return c->be.check(hipGetLastError(), sphere ? "k_spherecast launch" : "k_closest_point launch") ? VX_OK : fail(c, VX_ERR_DEVICE, std::string(what) + ": " + c->be.error());
}

int shape_device(vx_ctx* c, uint32_t level, bool sphere, const void* dIn, uint32_t n, void* dOut, const char* what)
{
	int rc = ray_check(c, level, what);
	if (rc != VX_OK) return rc;
	if (n && (!dIn || !dOut)) return fail(c, VX_ERR_INVALID, std::string(what) + ": null array");
	if (((uintptr_t)dIn | (uintptr_t)dOut) & 15u) return fail(c, VX_ERR_INVALID, std::string(what) + ": arrays must be 16-byte aligned");
	if (!n) return VX_OK;
	if ((rc = ray_prepare(c, level)) != VX_OK) return rc;
	return shape_launch(c, level, sphere, dIn, n, dOut);
}

int shape_host(vx_ctx* c, uint32_t level, bool sphere, const void* in, size_t inSize, uint32_t n, void* out, size_t outSize, const char* what)
{
	int rc = ray_check(c, level, what);
	if (rc != VX_OK) return rc;
	if (n && (!in || !out)) return fail(c, VX_ERR_INVALID, std::string(what) + ": null array");
	if (!n) return VX_OK;
	if ((rc = ray_prepare(c, level)) != VX_OK) return rc;
	RayState* s = module_peek<RayState>(c, MOD_RAY);
	const size_t inBytes = (size_t)n * inSize, outBytes = (size_t)n * outSize;
	if (!dev_grow(c, s->io, s->ioCap, inBytes + outBytes)) return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
	void* dIn = s->io;
	void* dOut = (char*)s->io + inBytes;   // (inBytes is a multiple of 16)
	if (!c->be.h2d(dIn, in, inBytes)) return fail(c, VX_ERR_DEVICE, std::string(what) + ": upload failed: " + c->be.error());
	if ((rc = shape_launch(c, level, sphere, dIn, n, dOut)) != VX_OK) return rc;
	if (!c->be.d2h(out, dOut, outBytes)) return fail(c, VX_ERR_DEVICE, std::string(what) + ": download failed: " + c->be.error());
	return VX_OK;
}

} // namespace

extern "C" {

static_assert(sizeof(vx_sphere_cast) == 48 && sizeof(vx_sphere_hit) == 64, "vx_sphere_cast / vx_sphere_hit layout");
static_assert(sizeof(vx_point_query) == 16 && sizeof(vx_point_hit) == 48, "vx_point_query / vx_point_hit layout");

int vx_spherecast_device(vx_ctx* c, uint32_t level, const vx_sphere_cast* d_casts, uint32_t n, vx_sphere_hit* d_hits)
{
	VX_ENTER(c);
	return shape_device(c, level, true, d_casts, n, d_hits, "vx_spherecast_device");
}

int vx_spherecast(vx_ctx* c, uint32_t level, const vx_sphere_cast* casts, uint32_t n, vx_sphere_hit* hits)
{
	VX_ENTER(c);
	return shape_host(c, level, true, casts, sizeof(vx_sphere_cast), n, hits, sizeof(vx_sphere_hit), "vx_spherecast");
}

int vx_closest_point_device(vx_ctx* c, uint32_t level, const vx_point_query* d_q, uint32_t n, vx_point_hit* d_hits)
{
	VX_ENTER(c);
	return shape_device(c, level, false, d_q, n, d_hits, "vx_closest_point_device");
}

int vx_closest_point(vx_ctx* c, uint32_t level, const vx_point_query* q, uint32_t n, vx_point_hit* hits)
{
	VX_ENTER(c);
	return shape_host(c, level, false, q, sizeof(vx_point_query), n, hits, sizeof(vx_point_hit), "vx_closest_point");
}

} // extern "C"
