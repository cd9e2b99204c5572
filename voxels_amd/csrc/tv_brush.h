// tv_brush.h — the sample functions of the brushes of vx_grid_inject_brushes (include/voxels_hip.h, "edits on the device").
//
// This header is the specification of the arithmetic and the one thing the device kernels (vx_brush.inl) and the host
// oracle of the tests (tests/brush/brush_host.cpp) share.  Everything is float32, one rounding per written operation
// (compile with -ffp-contract=off), dot products associated as (x*x + y*y) + z*z, max / min as the written ternaries.
// p = (x, y, z) is the sample position relative to the brush's `position`, in grid axes (Z up), as Grid::InjectSurface
// hands it to VoxelSurface::GetSurface.
#pragma once

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

enum { BRUSH_BALL = 0, BRUSH_CAPSULE = 1, BRUSH_BOX = 2, BRUSH_MATERIAL = 3, BRUSH_SHAPES = 4 };

TV_HD float brush_max(float a, float b) { return a > b ? a : b; }
TV_HD float brush_min(float a, float b) { return a < b ? a : b; }

// f(p) = |p| - radius: the expression of vx_grid_inject_ball (edit_voxel of tv_block.h)
TV_HD float brush_ball(float x, float y, float z, float radius)
{
	return sqrtf((x * x + y * y) + z * z) - radius;
}

// f(p) = dist(p, segment a..b) - radius; a = b is the ball around a
TV_HD float brush_capsule(float x, float y, float z, const float a[3], const float b[3], float radius)
{
	const float pax = x - a[0], pay = y - a[1], paz = z - a[2];
	const float bax = b[0] - a[0], bay = b[1] - a[1], baz = b[2] - a[2];
	const float bb = (bax * bax + bay * bay) + baz * baz;
	float h = 0.f;
	if (bb != 0.f) {
		h = ((pax * bax + pay * bay) + paz * baz) / bb;
		h = h < 0.f ? 0.f : (h > 1.f ? 1.f : h);
	}
	const float vx = pax - bax * h, vy = pay - bay * h, vz = paz - baz * h;
	return sqrtf((vx * vx + vy * vy) + vz * vz) - radius;
}

// f(p) = rounded box with half sizes a[] and rounding radius `radius`: q = |p| - a,
// f = |max(q, 0)| + min(max(q.x, max(q.y, q.z)), 0) - radius
TV_HD float brush_box(float x, float y, float z, const float a[3], float radius)
{
	const float qx = fabsf(x) - a[0], qy = fabsf(y) - a[1], qz = fabsf(z) - a[2];
	const float mx = brush_max(qx, 0.f), my = brush_max(qy, 0.f), mz = brush_max(qz, 0.f);
	const float outside = sqrtf((mx * mx + my * my) + mz * mz);
	const float inside = brush_min(brush_max(qx, brush_max(qy, qz)), 0.f);
	return (outside + inside) - radius;
}

// the distance brushes by shape (BRUSH_BALL, BRUSH_CAPSULE, BRUSH_BOX)
TV_HD float brush_sample(unsigned shape, float x, float y, float z, const float a[3], const float b[3], float radius)
{
	if (shape == BRUSH_CAPSULE) return brush_capsule(x, y, z, a, b, radius);
	if (shape == BRUSH_BOX) return brush_box(x, y, z, a, radius);
	return brush_ball(x, y, z, radius);
}

} // namespace tv
