// tv_shape.h — the sphere-triangle arithmetic of the sphere casts and closest-point queries (vx_shape.inl), host and device,
// float32.  The tests compile this header for the host with g++ -ffp-contract=off (tests/shape/shape_host.cpp) and compare it
// with a float64 oracle, so what runs here is what the kernels run.
//
// Everything is computed relative to the triangle's first vertex A: mesh coordinates reach 2048 and more, where one ulp is
// 2.4e-4 voxels, while the distances that decide a contact are of the order of the radius.  Differences of vertices of one
// triangle are exact (nearby multiples of one ulp), and the swept centre is re-based to the point of its line nearest to A
// before any product is formed.
#pragma once

#include "tv_ray.h"

namespace tv {

struct SV {
	float x, y, z;
};

TV_HD SV sv(float x, float y, float z) { SV r; r.x = x; r.y = y; r.z = z; return r; }
TV_HD SV sv_add(SV a, SV b) { return sv(a.x + b.x, a.y + b.y, a.z + b.z); }
TV_HD SV sv_sub(SV a, SV b) { return sv(a.x - b.x, a.y - b.y, a.z - b.z); }
TV_HD SV sv_mul(SV a, float s) { return sv(a.x * s, a.y * s, a.z * s); }
TV_HD float sv_dot(SV a, SV b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TV_HD SV sv_cross(SV a, SV b) { return sv(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// closest point of the segment [0, e] to p: the parameter in [0, 1]
TV_HD float shape_segment_param(SV p, SV e)
{
	const float ee = sv_dot(e, e);
	if (!(ee > 0.f)) return 0.f;
	const float s = sv_dot(p, e) / ee;
	return s < 0.f ? 0.f : (s > 1.f ? 1.f : s);
}

// Closest point of the triangle (0, ab, ac) to p, all relative to the first vertex (Ericson, Real-Time Collision Detection,
// §5.1.5, ClosestPtPointTriangle): the point, and v, w = the weights of the 2nd and 3rd vertex.  A triangle without area
// (the Voronoi tests all fail) falls back to the nearest of its three edges.
TV_HD SV shape_closest_rel(SV p, SV ab, SV ac, float& v, float& w)
{
	const float d1 = sv_dot(ab, p), d2 = sv_dot(ac, p);
	if (d1 <= 0.f && d2 <= 0.f) { v = 0.f; w = 0.f; return sv(0.f, 0.f, 0.f); }
	const SV bp = sv_sub(p, ab);
	const float d3 = sv_dot(ab, bp), d4 = sv_dot(ac, bp);
	if (d3 >= 0.f && d4 <= d3) { v = 1.f; w = 0.f; return ab; }
	const float vc = d1 * d4 - d3 * d2;
	if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
		const float s = d1 / (d1 - d3);
		v = s; w = 0.f;
		return sv_mul(ab, s);
	}
	const SV cp = sv_sub(p, ac);
	const float d5 = sv_dot(ab, cp), d6 = sv_dot(ac, cp);
	if (d6 >= 0.f && d5 <= d6) { v = 0.f; w = 1.f; return ac; }
	const float vb = d5 * d2 - d1 * d6;
	if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
		const float s = d2 / (d2 - d6);
		v = 0.f; w = s;
		return sv_mul(ac, s);
	}
	const float va = d3 * d6 - d5 * d4;
	if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {
		const float s = (d4 - d3) / ((d4 - d3) + (d5 - d6));
		v = 1.f - s; w = s;
		return sv_add(ab, sv_mul(sv_sub(ac, ab), s));
	}
	const float sum = va + vb + vc;
	if (sum > 0.f) {
		const float den = 1.f / sum;
		v = vb * den; w = vc * den;
		return sv_add(sv_mul(ab, v), sv_mul(ac, w));
	}
	// no area: the nearest of the edges (0, ab), (0, ac), (ab, ac)
	const float s0 = shape_segment_param(p, ab), s1 = shape_segment_param(p, ac), s2 = shape_segment_param(bp, sv_sub(ac, ab));
	const SV q0 = sv_mul(ab, s0), q1 = sv_mul(ac, s1), q2 = sv_add(ab, sv_mul(sv_sub(ac, ab), s2));
	const SV r0 = sv_sub(p, q0), r1 = sv_sub(p, q1), r2 = sv_sub(p, q2);
	const float e0 = sv_dot(r0, r0), e1 = sv_dot(r1, r1), e2 = sv_dot(r2, r2);
	if (e0 <= e1 && e0 <= e2) { v = s0; w = 0.f; return q0; }
	if (e1 <= e2) { v = 0.f; w = s1; return q1; }
	v = 1.f - s2; w = s2;
	return q2;
}

// distance from p to the triangle ABC (absolute coordinates); q = the closest point, v, w its weights of B and C
TV_HD float shape_point_triangle(SV p, SV A, SV B, SV C, SV& q, float& v, float& w)
{
	const SV pr = sv_sub(p, A);
	const SV qr = shape_closest_rel(pr, sv_sub(B, A), sv_sub(C, A), v, w);
	const SV g = sv_sub(pr, qr);
	q = sv_add(A, qr);
	return sqrtf(sv_dot(g, g));
}

// [lo, hi] &= { t : a + b t >= 0 }
TV_HD void shape_half(float a, float b, float& lo, float& hi)
{
	if (b > 0.f) { const float s = -a / b; lo = s > lo ? s : lo; }
	else if (b < 0.f) { const float s = -a / b; hi = s < hi ? s : hi; }
	else if (!(a >= 0.f)) hi = -ray_inf();
}

// [lo, hi] &= { t : qa t^2 + 2 qb t + qc <= 0 } with qa >= 0 (a sphere or an infinite cylinder along a line)
TV_HD void shape_quadratic(float qa, float qb, float qc, float& lo, float& hi)
{
	if (!(qa > 0.f)) {
		if (!(qc <= 0.f)) hi = -ray_inf();
		return;
	}
	const float disc = qb * qb - qa * qc;
	if (!(disc >= 0.f)) { hi = -ray_inf(); return; }
	const float sq = sqrtf(disc);
	const float q = -(qb + (qb < 0.f ? -sq : sq));
	float t1 = 0.f, t2 = 0.f;
	if (q != 0.f) {
		t1 = q / qa;
		t2 = qc / q;
		if (t1 > t2) { const float x = t1; t1 = t2; t2 = x; }
	}
	lo = t1 > lo ? t1 : lo;
	hi = t2 < hi ? t2 : hi;
}

// First t in [tLo, tHi] at which the distance from o + t d to the triangle ABC is <= r (both faces), +INF if none.  The
// triangle inflated by r is the union of seven solids: the slab |dist to the plane| <= r over the triangle, the three
// cylinders of radius r around the edges between their end planes, and the three balls of radius r at the vertices; the set
// of t at which the centre lies in any one of them is an interval, intersected from affine and quadratic conditions in t.
// The first contact is the least start of the seven intervals within the window.
TV_HD float shape_sweep_triangle(SV o, SV d, float r, float tLo, float tHi, SV A, SV B, SV C)
{
	const SV e1 = sv_sub(B, A), e2 = sv_sub(C, A);
	const SV p0 = sv_sub(o, A);
	const float dd = sv_dot(d, d);
	// re-base: y0 = the point of the line nearest to A, relative to A; tau = t - tRef
	const float tRef = dd > 0.f ? -sv_dot(p0, d) / dd : 0.f;
	const SV y0 = sv_add(p0, sv_mul(d, tRef));
	const float wLo = tLo - tRef, wHi = tHi - tRef;
	float best = ray_inf();
	// the slab over the face
	const SV n = sv_cross(e1, e2);
	const float nn = sv_dot(n, n);
	if (nn > 0.f) {
		float lo = wLo, hi = wHi;
		const float rn = r * sqrtf(nn), s0 = sv_dot(n, y0), sd = sv_dot(n, d);
		shape_half(rn - s0, -sd, lo, hi);
		shape_half(rn + s0, sd, lo, hi);
		// the projection of the centre inside the triangle: its three (unnormalised) area coordinates >= 0
		const SV e3 = sv_sub(e2, e1);
		shape_half(sv_dot(n, sv_cross(y0, e2)), sv_dot(n, sv_cross(d, e2)), lo, hi);
		shape_half(sv_dot(n, sv_cross(e1, y0)), sv_dot(n, sv_cross(e1, d)), lo, hi);
		shape_half(sv_dot(n, sv_cross(e3, sv_sub(y0, e1))), sv_dot(n, sv_cross(e3, d)), lo, hi);
		if (lo <= hi && lo < best) best = lo;
	}
	// the three edges (P, P + e): the cylinder around the line, between the planes through P and P + e normal to e
	for (int k = 0; k < 3; ++k) {
		const SV P = k == 0 ? sv(0.f, 0.f, 0.f) : (k == 1 ? e1 : e2);
		const SV e = k == 0 ? e1 : (k == 1 ? sv_sub(e2, e1) : sv_sub(sv(0.f, 0.f, 0.f), e2));
		const float ee = sv_dot(e, e);
		if (!(ee > 0.f)) continue;
		const SV y = sv_sub(y0, P);
		float lo = wLo, hi = wHi;
		const float ye = sv_dot(y, e), de = sv_dot(d, e);
		shape_half(ye, de, lo, hi);
		shape_half(ee - ye, -de, lo, hi);
		const SV w0 = sv_cross(y, e), wd = sv_cross(d, e);
		shape_quadratic(sv_dot(wd, wd), sv_dot(w0, wd), sv_dot(w0, w0) - r * r * ee, lo, hi);
		if (lo <= hi && lo < best) best = lo;
	}
	// the three vertices
	for (int k = 0; k < 3; ++k) {
		const SV y = sv_sub(y0, k == 0 ? sv(0.f, 0.f, 0.f) : (k == 1 ? e1 : e2));
		float lo = wLo, hi = wHi;
		shape_quadratic(dd, sv_dot(y, d), sv_dot(y, y) - r * r, lo, hi);
		if (lo <= hi && lo < best) best = lo;
	}
	if (best == ray_inf()) return best;
	return best <= wLo ? tLo : tRef + best;
}

// One triangle against a sphere cast: false if it is never within r in [tLo, tHi].  A cast that touches it at tLo already
// (tLo finite) gives t = tLo, dist = the distance there, start = true; otherwise t = the first contact and dist = r.
TV_HD bool shape_sphere_triangle(SV o, SV d, float r, float tLo, float tHi, SV A, SV B, SV C, float& t, float& dist, bool& start)
{
	if (tLo > -ray_inf()) {
		const SV p0 = sv_sub(o, A);
		const SV pr = (d.x != 0.f || d.y != 0.f || d.z != 0.f) ? sv_add(p0, sv_mul(d, tLo)) : p0;
		float v, w;
		const SV g = sv_sub(pr, shape_closest_rel(pr, sv_sub(B, A), sv_sub(C, A), v, w));
		const float s = sqrtf(sv_dot(g, g));
		if (s <= r) { t = tLo; dist = s; start = true; return true; }
	}
	t = shape_sweep_triangle(o, d, r, tLo, tHi, A, B, C);
	dist = r;
	start = false;
	return t < ray_inf();
}

} // namespace tv
