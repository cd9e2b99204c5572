// Host build of the sphere-triangle arithmetic of the sphere casts (voxels_amd/csrc/tv_shape.h) for tests/test_shapecast.py:
// g++ -ffp-contract=off, the same float32 operations in the same order as the kernels.  Test infrastructure only.
#include "../../voxels_amd/csrc/tv_shape.h"

using namespace tv;

static SV at(const float* p) { return sv(p[0], p[1], p[2]); }

extern "C" {

// closest points: p[n][3], tri[n][3][3] -> dist[n], q[n][3], vw[n][2]
void shape_closest(long n, const float* p, const float* tri, float* dist, float* q, float* vw)
{
	for (long i = 0; i < n; ++i) {
		const float* t = tri + 9 * i;
		SV c;
		dist[i] = shape_point_triangle(at(p + 3 * i), at(t), at(t + 3), at(t + 6), c, vw[2 * i], vw[2 * i + 1]);
		q[3 * i] = c.x; q[3 * i + 1] = c.y; q[3 * i + 2] = c.z;
	}
}

// sphere casts against one triangle each: o[n][3], d[n][3], r[n], win[n][2] (t_min, t_max), tri[n][3][3]
//   -> t[n] (+INF: no contact), dist[n], start[n]
void shape_sweep(long n, const float* o, const float* d, const float* r, const float* win, const float* tri, float* t, float* dist, int* start)
{
	for (long i = 0; i < n; ++i) {
		const float* v = tri + 9 * i;
		bool s = false;
		if (!shape_sphere_triangle(at(o + 3 * i), at(d + 3 * i), r[i], win[2 * i], win[2 * i + 1], at(v), at(v + 3), at(v + 6), t[i], dist[i], s)) {
			t[i] = __builtin_huge_valf();
			dist[i] = 0.f;
		}
		start[i] = s ? 1 : 0;
	}
}

} // extern "C"
