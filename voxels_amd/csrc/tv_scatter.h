// tv_scatter.h — the arithmetic of vx_scatter (include/voxels_hip.h, "scattering").  DESIGN.md §18.
//
// This header is the one place where the arithmetic is written down, shared by the device kernels (vx_scatter.inl) and the
// host build of the tests (tests/scatter/scatter_host.cpp).  Everything in float32 is one rounding per written operation
// (compile with -ffp-contract=off); the hash is uint32 arithmetic that wraps.
//
//   scatter_mix / scatter_unit / scatter_*_hash / scatter_draw   the hash: (seed, level, coord_id, t, j) -> 32 bits -> [0, 1)
//   scatter_box_meets                                            is a table entry visited
//   scatter_mask_passes, scatter_count                           does a triangle take part, and with how many candidates
//   scatter_sample, scatter_keeps                                candidate k of a triangle, and the per-point filters
#pragma once

#include <stdint.h>
#include <stddef.h>
#include <string.h>

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

typedef uint32_t u32;

struct ScatterRules {       // = vx_scatter_params
	u32 seed;
	float density;
	float minUp, maxUp;
	float boxMin[3], boxMax[3];
	u32 slot;
	u32 mask[8];
	u32 reserved;
};

struct ScatterV3 { float x, y, z; };

struct ScatterVertex {      // what the scattering reads of a vx_vertex
	ScatterV3 p, n;
	u32 tex0, tex1;         // the 8 tex bytes as two little-endian words
};

struct ScatterSample {
	ScatterV3 pos, nrm;
	float rand;
};

// ---- the hash ---------------------------------------------------------------------------------------------------------------

TV_HD u32 scatter_mix(u32 x)
{
	x ^= x >> 16; x *= 0x7feb352du;
	x ^= x >> 15; x *= 0x846ca68bu;
	x ^= x >> 16;
	return x;
}

// 24 bits into [0, 1): exact
TV_HD float scatter_unit(u32 h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

TV_HD u32 scatter_block_hash(u32 seed, u32 level, u32 coordId) { return scatter_mix(seed ^ scatter_mix(coordId + 0x9E3779B9u * (level + 1u))); }
TV_HD u32 scatter_tri_hash(u32 hb, u32 t) { return scatter_mix(hb + t * 0x85EBCA6Bu); }
TV_HD u32 scatter_draw(u32 ht, u32 j) { return scatter_mix(ht ^ (j * 0xC2B2AE35u)); }

// ---- vertices ---------------------------------------------------------------------------------------------------------------

TV_HD float scatter_float(u32 w) { float f; memcpy(&f, &w, 4); return f; }
TV_HD u32 scatter_word(float f) { u32 w; memcpy(&w, &f, 4); return w; }

// one of the three 16-byte pieces of a 48-byte vertex: pos + sec.x | sec.yzw + nrm.x | nrm.yz + tex
TV_HD void scatter_piece(const void* vertex, u32 piece, u32& a, u32& b, u32& c, u32& d)
{
	u32 w[4];
#if defined(__HIP_DEVICE_COMPILE__)
	memcpy(w, __builtin_assume_aligned((const char*)vertex + 16u * piece, 16), 16); // (the pools are 16-byte aligned: one load)
#else
	memcpy(w, (const char*)vertex + 16u * piece, 16);
#endif
	a = w[0]; b = w[1]; c = w[2]; d = w[3];
}

// position only (the candidate count), or the whole of it (the candidates); `withTex` adds the tex words to the former
TV_HD ScatterVertex scatter_vertex(const void* vertex, bool full, bool withTex)
{
	ScatterVertex v;
	u32 a, b, c, d;
	scatter_piece(vertex, 0, a, b, c, d);
	v.p.x = scatter_float(a); v.p.y = scatter_float(b); v.p.z = scatter_float(c);
	v.n.x = v.n.y = v.n.z = 0.f;
	v.tex0 = v.tex1 = 0;
	if (full) {
		scatter_piece(vertex, 1, a, b, c, d);
		v.n.x = scatter_float(d);
	}
	if (full || withTex) {
		scatter_piece(vertex, 2, a, b, c, d);
		v.n.y = scatter_float(a); v.n.z = scatter_float(b);
		v.tex0 = c; v.tex1 = d;
	}
	return v;
}

// ---- entries and triangles --------------------------------------------------------------------------------------------------

// the table box of an entry meets the filter box
TV_HD bool scatter_box_meets(const ScatterRules& r, const float minc[3], const float maxc[3])
{
	return minc[0] <= r.boxMax[0] && maxc[0] >= r.boxMin[0] && minc[1] <= r.boxMax[1] && maxc[1] >= r.boxMin[1]
	    && minc[2] <= r.boxMax[2] && maxc[2] >= r.boxMin[2];
}

// bit tex[slot] of the mask, tex = the FIRST vertex's bytes (a chain of selects: no indexing by a lane's value)
TV_HD bool scatter_mask_passes(const ScatterRules& r, u32 tex0, u32 tex1)
{
	const u32 s = r.slot & 7u;
	const u32 v = ((s < 4u ? tex0 : tex1) >> ((s & 3u) * 8u)) & 255u, k = v >> 5;
	u32 w = r.mask[0];
	w = k == 1u ? r.mask[1] : w; w = k == 2u ? r.mask[2] : w; w = k == 3u ? r.mask[3] : w; w = k == 4u ? r.mask[4] : w;
	w = k == 5u ? r.mask[5] : w; w = k == 6u ? r.mask[6] : w; w = k == 7u ? r.mask[7] : w;
	return ((w >> (v & 31u)) & 1u) != 0u;
}

// candidates of a triangle with hash ht (the texture mask is the caller's)
TV_HD u32 scatter_count(const ScatterV3& v0, const ScatterV3& v1, const ScatterV3& v2, float density, u32 ht)
{
	const float e1x = v1.x - v0.x, e1y = v1.y - v0.y, e1z = v1.z - v0.z;
	const float e2x = v2.x - v0.x, e2y = v2.y - v0.y, e2z = v2.z - v0.z;
	const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
	const float l2 = (cx * cx + cy * cy) + cz * cz;
	if (!(l2 > 0.f && l2 <= 3.40282347e+38f)) return 0u; // zero, NaN or infinite
	float m = (0.5f * sqrtf(l2)) * density;
	m = m < 65535.0f ? m : 65535.0f;
	const u32 base = (u32)m;
	const float frac = m - (float)base;
	return base + (scatter_unit(scatter_draw(ht, 0u)) < frac ? 1u : 0u);
}

// candidate k of a triangle
TV_HD ScatterSample scatter_sample(const ScatterVertex& a, const ScatterVertex& b, const ScatterVertex& c, u32 ht, u32 k)
{
	ScatterSample s;
	float r1 = scatter_unit(scatter_draw(ht, 3u * k + 1u)), r2 = scatter_unit(scatter_draw(ht, 3u * k + 2u));
	if (r1 + r2 > 1.0f) { r1 = 1.0f - r1; r2 = 1.0f - r2; }
	s.rand = scatter_unit(scatter_draw(ht, 3u * k + 3u));
	s.pos.x = a.p.x + ((b.p.x - a.p.x) * r1 + (c.p.x - a.p.x) * r2);
	s.pos.y = a.p.y + ((b.p.y - a.p.y) * r1 + (c.p.y - a.p.y) * r2);
	s.pos.z = a.p.z + ((b.p.z - a.p.z) * r1 + (c.p.z - a.p.z) * r2);
	const float gx = a.n.x + ((b.n.x - a.n.x) * r1 + (c.n.x - a.n.x) * r2);
	const float gy = a.n.y + ((b.n.y - a.n.y) * r1 + (c.n.y - a.n.y) * r2);
	const float gz = a.n.z + ((b.n.z - a.n.z) * r1 + (c.n.z - a.n.z) * r2);
	const float gl = sqrtf((gx * gx + gy * gy) + gz * gz);
	const bool unit = gl > 0.f;
	s.nrm.x = unit ? gx / gl : 0.f;
	s.nrm.y = unit ? gy / gl : 0.f;
	s.nrm.z = unit ? gz / gl : 0.f;
	return s;
}

// the per-point filters: slope and box
TV_HD bool scatter_keeps(const ScatterRules& r, const ScatterSample& s)
{
	return r.minUp <= s.nrm.y && s.nrm.y <= r.maxUp
	    && r.boxMin[0] <= s.pos.x && s.pos.x <= r.boxMax[0] && r.boxMin[1] <= s.pos.y && s.pos.y <= r.boxMax[1]
	    && r.boxMin[2] <= s.pos.z && s.pos.z <= r.boxMax[2];
}

} // namespace tv
