// tv_overlap.h — the per-lane logic of the overlap queries (include/voxels_hip.h, "overlap queries"), host and device.  DESIGN.md §21.
//
// This header is the one place where the decisions are written down, shared by the device kernels (vx_overlap.inl) and the host
// build of the tests (tests/overlap/overlap_host.cpp).  There is no arithmetic on the result: a match is six float32 comparisons
// of stored positions.  Everything else here is pruning, and pruning is conservative - the result does not depend on it:
//
//   overlap_box_valid                         is the query empty by its own words (NaN, lo > hi)
//   overlap_block_range                       per axis, the blocks that can meet the box: integers from floats clamped IN FLOAT
//   overlap_candidate_cell                    the k-th block of that range in coord_id order (the emission order of blocks)
//   overlap_block_meets, overlap_bucket_meets the dilated-box tests: the very expressions of the index build (ray_tri_bucket)
//   overlap_next_run                          candidate buckets that are neighbours in the permutation, taken as one slice
//   overlap_matches                           the predicate
//   overlap_words, overlap_mark               the per-block bitmap over triangle ordinals: the emission order inside a block
//
// The index's invariant (vx_ray.inl, `straddling` = 0): every vertex p of a triangle in bucket s of a block with origin org has
// org + s*sub - 1/256 <= p <= org + (s+1)*sub + 1/256 on every axis, as floats, these expressions.  A triangle that matches a
// box [lo, hi] has a vertex <= hi and a vertex >= lo on every axis; so its bucket's dilated box has blo <= hi and bhi >= lo, the
// test that keeps a bucket.  A block's dilated box is that of its buckets 0 and 3 per axis.
#pragma once

#include "tv_ray.h"

namespace tv {

enum : u32 { OVERLAP_MAX_TRIS = 16u * 16u * 16u * 5u, OVERLAP_WORDS = OVERLAP_MAX_TRIS / 32u };  // 20 480 regular triangles: 640 words

// lo <= hi on every axis; false for a NaN anywhere
TV_HD bool overlap_box_valid(const float lo[3], const float hi[3])
{
	return lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2];
}

// the closed interval of sub-brick s (0..3) of a block along one axis, dilated by 1/256: ray_tri_bucket's lo and hi
TV_HD float overlap_sub_lo(float org, int s, float sub) { return org + (float)s * sub - (1.f / 256.f); }
TV_HD float overlap_sub_hi(float org, int s, float sub) { return org + (float)(s + 1) * sub + (1.f / 256.f); }

// Blocks c0..c1 of one axis that can pass overlap_block_meets (c1 < c0: none).  The quotients are clamped to [-1, cnt] as
// floats, so that +-INF and huge values never reach the conversion (where host and device differ); one block more on either
// side covers the rounding of lo - 1/256 and hi + 1/256 and the closed ends (a box that starts exactly on a block plane meets
// the block below it).
TV_HD void overlap_block_range(float lo, float hi, float size, u32 cnt, int& c0, int& c1)
{
	const float top = (float)cnt;
	float f0 = floorf((lo - (1.f / 256.f)) / size), f1 = floorf((hi + (1.f / 256.f)) / size);
	f0 = f0 < -1.f ? -1.f : (f0 > top ? top : f0);
	f1 = f1 < -1.f ? -1.f : (f1 > top ? top : f1);
	c0 = (int)f0 - 1;
	c1 = (int)f1 + 1;
	c0 = c0 < 0 ? 0 : c0;
	c1 = c1 > (int)cnt - 1 ? (int)cnt - 1 : c1;
}

// the k-th block of the range c0 + [0, ext) in coord_id order: mesh y outermost, then mesh z, then mesh x (ray_coord_id)
TV_HD void overlap_candidate_cell(u32 k, const int c0[3], const u32 ext[3], int m[3])
{
	m[0] = c0[0] + (int)(k % ext[0]);
	k /= ext[0];
	m[2] = c0[2] + (int)(k % ext[2]);
	m[1] = c0[1] + (int)(k / ext[2]);
}

TV_HD bool overlap_block_meets(const float lo[3], const float hi[3], const float org[3], float sub)
{
	bool meets = true;
	for (int a = 0; a < 3; ++a) meets = meets && overlap_sub_lo(org[a], 0, sub) <= hi[a] && overlap_sub_hi(org[a], (int)RAY_SUB - 1, sub) >= lo[a];
	return meets;
}

// bucket = ray_bucket(s): s[0] = bucket & 3, s[1] = (bucket >> 2) & 3, s[2] = bucket >> 4, mesh axes
TV_HD bool overlap_bucket_meets(const float lo[3], const float hi[3], const float org[3], float sub, u32 bucket)
{
	const int s[3] = { (int)(bucket & 3u), (int)((bucket >> 2) & 3u), (int)(bucket >> 4) };
	bool meets = true;
	for (int a = 0; a < 3; ++a) meets = meets && overlap_sub_lo(org[a], s[a], sub) <= hi[a] && overlap_sub_hi(org[a], s[a], sub) >= lo[a];
	return meets;
}

// The lowest run of set bits of a non-zero mask of buckets: [b0, b1), taken out of the mask.  Buckets b0..b1-1 are one slice
// starts[b0]..starts[b1] of the block's permutation.
TV_HD void overlap_next_run(unsigned long long& mask, u32& b0, u32& b1)
{
	b0 = (u32)__builtin_ctzll(mask);
	const unsigned long long inv = ~(mask >> b0);   // (zeros come in at the top: inv is zero only for b0 = 0 and a full mask)
	b1 = inv ? b0 + (u32)__builtin_ctzll(inv) : 64u;
	mask = b1 < 64u ? mask & (~0ull << b1) : 0ull;
}

// the match of the header: the triangle's bounding box against the closed query box
TV_HD bool overlap_matches(const float lo[3], const float hi[3], const float A[3], const float B[3], const float C[3])
{
	bool m = true;
	for (int a = 0; a < 3; ++a) {
		float mn = A[a] < B[a] ? A[a] : B[a], mx = A[a] > B[a] ? A[a] : B[a];
		mn = C[a] < mn ? C[a] : mn;
		mx = C[a] > mx ? C[a] : mx;
		m = m && mn <= hi[a] && mx >= lo[a];
	}
	return m;
}

// The order inside a block is by triangle ordinal, whatever the order of a bucket's slice of the permutation (k_ray_index
// fills it with atomics): matches are marked in a bitmap over the ordinals and read back ascending.
TV_HD u32 overlap_words(u32 nTri) { return (nTri + 31u) >> 5; }
TV_HD u32 overlap_mark(u32 tri, u32& word) { word = tri >> 5; return 1u << (tri & 31u); }

} // namespace tv
