// tv_lod.h — the node arithmetic of the LOD selection (vx_lod.inl), host and device.
//
// Node (L, c) of level L covers the internal (Z-up) box [c S, (c+1) S]^3, S = 16 * 2^L; its mesh-space (Y-up) box swaps y
// and z, as vx_listed_block.min_corner / max_corner do.  The distance and the plane test are spelled out in the order the
// header states (include/voxels_hip.h, "LOD selection"): the library builds with -ffp-contract=off, so they are bit-exact
// against tests/lod_oracle.py.
#pragma once

#include "tv_core.h"

namespace tv {

// internal axis (x = 0, y = 1, z = 2) and direction of transition face f (BlockPolygons::TransitionFaceId order in mesh
// space: -Y, -Z, -X, +Y, +Z, +X)
TV_HD int lod_face_axis(int f) { return (f % 3) == 0 ? 2 : ((f % 3) == 1 ? 1 : 0); }
TV_HD int lod_face_dir(int f) { return f < 3 ? -1 : 1; }

// blockAdj of a block whose transition faces are `transitions`: a regular vertex with bit b of vertex.sec[3] lies on
// transition face b (the meshes say so: tests/test_gpu_lod.py, test_adjacency_bits_from_the_meshes), so the orders agree
TV_HD u32 lod_adjacency(u32 transitions) { return transitions; }

// mesh-space box of the node with internal block coordinates c at level L
TV_HD void lod_box(const u32 c[3], u32 L, float mn[3], float mx[3])
{
	const float s = (float)(16u << L);
	mn[0] = (float)c[0] * s; mn[1] = (float)c[2] * s; mn[2] = (float)c[1] * s;
	mx[0] = mn[0] + s; mx[1] = mn[1] + s; mx[2] = mn[2] + s;
}

// squared distance of the camera to a box: per axis max(max(min - cam, 0), cam - max), then (dx dx + dy dy) + dz dz
TV_HD float lod_dist2(const float mn[3], const float mx[3], const float cam[3])
{
	float d[3];
	for (int a = 0; a < 3; ++a) {
		const float lo = mn[a] - cam[a], hi = cam[a] - mx[a];
		const float t = lo > 0.f ? lo : 0.f;
		d[a] = t > hi ? t : hi;
	}
	const float xy = d[0] * d[0] + d[1] * d[1];
	return xy + d[2] * d[2];
}

// a box lies wholly outside plane (a, b, c, d) when its corner that maximises a x + b y + c z does
TV_HD bool lod_outside(const float mn[3], const float mx[3], const float pl[4])
{
	const float px = pl[0] >= 0.f ? mx[0] : mn[0], py = pl[1] >= 0.f ? mx[1] : mn[1], pz = pl[2] >= 0.f ? mx[2] : mn[2];
	const float ax = pl[0] * px, by = pl[1] * py, cz = pl[2] * pz;
	const float s = (ax + by) + cz;
	return s + pl[3] < 0.f;
}

} // namespace tv
