// tv_smooth.h — the arithmetic and the per-lane logic of vx_grid_smooth (include/voxels_hip.h, "smoothing").  DESIGN.md §17.
//
// This header is the one place where the arithmetic is written down, shared by the device kernels (vx_smooth.inl) and the
// host build of the tests (tests/smooth/smooth_host.cpp).  Everything in float32 is one rounding per written operation
// (compile with -ffp-contract=off); the kernel sum is an exact integer.
//
// The second half is what ONE lane of a workgroup does in one phase of a tile (a 16^3 grid block clipped to the op's box); the
// caller supplies the lanes (a workgroup, or a loop) and the barriers between the phases:
//   smooth_stage_row   one of the 18 x 18 rows of the tile's neighbourhood into the staged tile, edge clamps resolved
//   smooth_eval_row    one x-row of 16 new values from the staged tile
//   smooth_commit_row  one x-row of new values into the grid; which of its voxels differ from the op's original values
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

typedef uint8_t u8;
typedef uint32_t u32;
typedef int8_t i8;

enum { SMOOTH_MAX_ITERATIONS = 64, SMOOTH_MAX_COUNT = 1 << 16 };

// ---- the arithmetic ---------------------------------------------------------------------------------------------------------

// the weight of voxel (vx, vy, vz): `strength` everywhere (radius == 0), or falling off linearly to 0 at `radius` from `center`
TV_HD float smooth_weight(u32 vx, u32 vy, u32 vz, const float center[3], float radius, float strength)
{
	if (radius == 0.f) return strength;
	const float px = (float)vx - center[0], py = (float)vy - center[1], pz = (float)vz - center[2];
	const float r = sqrtf((px * px + py * py) + pz * pz);
	const float q = 1.0f - r / radius;
	return strength * (q > 0.f ? q : 0.f);
}

// the new sample from the old one `d`, the kernel sum `S` (weights sum to 64) and the weight `w`
TV_HD i8 smooth_value(int d, int S, float w)
{
	const float t = (float)S * 0.015625f;
	const float fd = (float)d;
	float f = rintf(fd + w * (t - fd)); // nearest, ties to even
	f = f < -128.f ? -128.f : (f > 127.f ? 127.f : f);
	return (i8)(int)f; // (-0 -> 0)
}

// S = sum of k(dx) k(dy) k(dz) at(dx, dy, dz) over dx, dy, dz in {-1, 0, 1}, k = (1, 2, 1); at() returns the int8 sample
template <class A> TV_HD int smooth_kernel_sum(const A& at)
{
	int S = 0;
	for (int dz = -1; dz <= 1; ++dz)
	for (int dy = -1; dy <= 1; ++dy)
	for (int dx = -1; dx <= 1; ++dx)
		S += (2 - (dx ? 1 : 0)) * (2 - (dy ? 1 : 0)) * (2 - (dz ? 1 : 0)) * (int)at(dx, dy, dz);
	return S;
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------

struct SmoothRegion {
	u32 n;               // grid edge
	u32 lo[3], hi[3];    // the box [lo, hi) in grid coordinates (x, y, z internal axes)
	u32 tb0[3], tn[3];   // first block and number of blocks (tiles) per axis
};

struct SmoothTile {
	u32 block;           // id of the grid block: (bz * nb + by) * nb + bx
	u32 org[3];          // the block's first voxel
	u32 c0[3], c1[3];    // the block clipped to the box, grid coordinates, [c0, c1)
};

// per op, accumulated with integer maxima and one sum: the voxels the op changed
struct SmoothSlot {      // 32 bytes, zero = nothing changed
	u32 notMin[3];       // ~(least changed coordinate) per internal axis
	u32 max[3];          // greatest changed coordinate
	unsigned long long changed;
};

struct SmoothResult {    // = vx_smooth_result
	float out_min[3], out_max[3];
	unsigned long long changed;
};

// staged tile: 18 x 18 rows (z major); byte 3 = the sample at x = org - 1, bytes 4..19 = the block's 16 samples, byte 20 = the
// sample at x = org + 16: 6 words, and a 7th that pads the row to an odd number of words, so that the 32 lanes of a half wave
// (16 values of y, 2 of z) read word k of their rows from 32 different LDS banks
enum { SMOOTH_ROW_WORDS = 7, SMOOTH_STAGE_ROWS = 18 * 18, SMOOTH_STAGE_WORDS = SMOOTH_STAGE_ROWS * SMOOTH_ROW_WORDS };
// commit modes
enum { SMOOTH_SAVE_ORIGINAL = 1, SMOOTH_COMPARE_GRID = 2, SMOOTH_COMPARE_ORIGINAL = 4 };

TV_HD SmoothRegion smooth_region(u32 n, const u32 lo[3], const u32 hi[3])
{
	SmoothRegion r;
	r.n = n;
	for (int k = 0; k < 3; ++k) {
		r.lo[k] = lo[k]; r.hi[k] = hi[k];
		r.tb0[k] = lo[k] >> 4; r.tn[k] = ((hi[k] + 15u) >> 4) - r.tb0[k];
	}
	return r;
}

TV_HD u32 smooth_tiles(const SmoothRegion& r) { return r.tn[0] * r.tn[1] * r.tn[2]; }

TV_HD SmoothTile smooth_tile(const SmoothRegion& r, u32 tile)
{
	SmoothTile T;
	const u32 b[3] = { r.tb0[0] + tile % r.tn[0], r.tb0[1] + (tile / r.tn[0]) % r.tn[1], r.tb0[2] + tile / (r.tn[0] * r.tn[1]) };
	const u32 nb = r.n >> 4;
	T.block = (b[2] * nb + b[1]) * nb + b[0];
	for (int k = 0; k < 3; ++k) {
		T.org[k] = b[k] * 16u;
		T.c0[k] = T.org[k] > r.lo[k] ? T.org[k] : r.lo[k];
		const u32 end = T.org[k] + 16u;
		T.c1[k] = end < r.hi[k] ? end : r.hi[k];
	}
	return T;
}

// is row (y, z) of the block (block-local) inside the clip
TV_HD bool smooth_row_inside(const SmoothTile& T, u32 y, u32 z) { return T.org[1] + y >= T.c0[1] && T.org[1] + y < T.c1[1] && T.org[2] + z >= T.c0[2] && T.org[2] + z < T.c1[2]; }
// the bits of the block-local x positions inside the clip
TV_HD u32 smooth_clip_bits(const SmoothTile& T) { const u32 a = T.c0[0] - T.org[0], b = T.c1[0] - T.org[0]; return ((1u << b) - 1u) & ~((1u << a) - 1u); }
// grid coordinate c + l - 1 clamped to [0, n - 1]
TV_HD u32 smooth_clamped(u32 org, u32 l, u32 n) { const u32 c = org + l; return c == 0 ? 0u : (c - 1u > n - 1u ? n - 1u : c - 1u); }

// 16 samples of a block's x-row: 16-byte aligned in the grid (n is a multiple of 16) and in the byte volumes
TV_HD void smooth_load16(const i8* p, u32 w[4]) { memcpy(w, __builtin_assume_aligned(p, 16), 16); }
TV_HD void smooth_store16(i8* p, const u32 w[4]) { memcpy(__builtin_assume_aligned(p, 16), w, 16); }
TV_HD int smooth_byte(const u32* w, u32 at) { return (int)(i8)(u8)(w[at >> 2] >> ((at & 3u) * 8u)); }

// row = lz * 18 + ly of the tile's neighbourhood (ly, lz in 0..17 stand for org - 1 .. org + 16) into the staged tile
TV_HD void smooth_stage_row(const i8* dist, u32 n, const SmoothTile& T, u32 row, u32* staged)
{
	const u32 y = smooth_clamped(T.org[1], row % 18u, n), z = smooth_clamped(T.org[2], row / 18u, n);
	const i8* p = dist + ((size_t)z * n + y) * n + T.org[0];
	u32 w[4];
	smooth_load16(p, w);
	const i8 left = T.org[0] ? p[-1] : p[0], right = T.org[0] + 16u < n ? p[16] : p[15];
	u32* s = staged + row * (u32)SMOOTH_ROW_WORDS;
	s[0] = (u32)(u8)left << 24;
	s[1] = w[0]; s[2] = w[1]; s[3] = w[2]; s[4] = w[3];
	s[5] = (u32)(u8)right;
}

// lane t = (y = t & 15, z = t >> 4): the 16 new values of its x-row, all of them (the commit clips).  The kernel sum
// separably: C[j] = sum over the 3 x 3 rows around (y, z) of k(dy) k(dz) sample(x = j - 1), then S[x] = C[x] + 2 C[x+1] + C[x+2]
// - the integers of smooth_kernel_sum in another order.
TV_HD void smooth_eval_row(const u32* staged, const SmoothTile& T, u32 t, const float center[3], float radius, float strength, u32 out[4])
{
	const u32 y = t & 15u, z = t >> 4;
	int C[18], d[16];
	for (int j = 0; j < 18; ++j) C[j] = 0;
	for (u32 dz = 0; dz < 3; ++dz)
	for (u32 dy = 0; dy < 3; ++dy) {
		const u32* s = staged + ((z + dz) * 18u + (y + dy)) * (u32)SMOOTH_ROW_WORDS;
		u32 w[6];
		for (int k = 0; k < 6; ++k) w[k] = s[k];
		const int weight = (dy == 1 ? 2 : 1) * (dz == 1 ? 2 : 1);
		for (u32 j = 0; j < 18; ++j) C[j] += weight * smooth_byte(w, 3u + j);
		if (dy == 1 && dz == 1) for (u32 x = 0; x < 16; ++x) d[x] = smooth_byte(w, 4u + x);
	}
	out[0] = out[1] = out[2] = out[3] = 0;
	for (u32 x = 0; x < 16; ++x) {
		const int S = C[x] + 2 * C[x + 1] + C[x + 2];
		const float w = smooth_weight(T.org[0] + x, T.org[1] + y, T.org[2] + z, center, radius, strength);
		out[x >> 2] |= (u32)(u8)smooth_value(d[x], S, w) << ((x & 3u) * 8u);
	}
}

// lane t: its x-row of new values (`fresh`, 16 bytes) into the grid, inside the clip only.  SMOOTH_SAVE_ORIGINAL keeps the
// grid's row in `original` first (the first of several iterations); the return value has bit x set where the new value
// differs from the grid's (SMOOTH_COMPARE_GRID: an op of one iteration) or from `original` (SMOOTH_COMPARE_ORIGINAL: the
// last of several).
TV_HD u32 smooth_commit_row(i8* dist, u32 n, const SmoothTile& T, u32 t, const i8* fresh, i8* original, u32 mode)
{
	const u32 y = t & 15u, z = t >> 4;
	if (!smooth_row_inside(T, y, z)) return 0;
	i8* p = dist + ((size_t)(T.org[2] + z) * n + T.org[1] + y) * n + T.org[0];
	u32 g[4], f[4], o[4], merged[4];
	smooth_load16(p, g);
	smooth_load16(fresh, f);
	if (mode & SMOOTH_SAVE_ORIGINAL) smooth_store16(original, g);
	if (mode & SMOOTH_COMPARE_ORIGINAL) smooth_load16(original, o);
	else for (int k = 0; k < 4; ++k) o[k] = g[k];
	const u32 clip = smooth_clip_bits(T);
	u32 changed = 0;
	for (u32 k = 0; k < 4; ++k) {
		u32 keep = 0;
		for (u32 b = 0; b < 4; ++b) if (!((clip >> (k * 4u + b)) & 1u)) keep |= 0xFFu << (b * 8u);
		merged[k] = (g[k] & keep) | (f[k] & ~keep);
		const u32 diff = (merged[k] ^ o[k]) & ~keep;
		for (u32 b = 0; b < 4; ++b) if ((diff >> (b * 8u)) & 0xFFu) changed |= 1u << (k * 4u + b);
	}
	smooth_store16(p, merged);
	return (mode & (SMOOTH_COMPARE_GRID | SMOOTH_COMPARE_ORIGINAL)) ? changed : 0u;
}

// one row's changed bits into a slot, without atomics (the host; the kernels reduce per workgroup first)
TV_HD void smooth_slot_add(SmoothSlot& s, const SmoothTile& T, u32 t, u32 changed)
{
	if (!changed) return;
	const u32 a[3] = { T.org[0] + (u32)__builtin_ctz(changed), T.org[1] + (t & 15u), T.org[2] + (t >> 4) };
	const u32 b[3] = { T.org[0] + 31u - (u32)__builtin_clz(changed), a[1], a[2] };
	for (int k = 0; k < 3; ++k) {
		if (~a[k] > s.notMin[k]) s.notMin[k] = ~a[k];
		if (b[k] > s.max[k]) s.max[k] = b[k];
	}
	s.changed += (unsigned long long)__builtin_popcount(changed);
}

// a slot as the result record: output order (x, z, y); changed voxels a..b inclusive -> [a, b + 1] clamped to [0, n]
TV_HD SmoothResult smooth_result(u32 n, const SmoothSlot& s)
{
	SmoothResult r;
	const int order[3] = { 0, 2, 1 };
	for (int k = 0; k < 3; ++k) {
		const u32 a = ~s.notMin[order[k]], b = s.max[order[k]] + 1u;
		r.out_min[k] = s.changed ? (float)(a < n ? a : n) : 0.f;
		r.out_max[k] = s.changed ? (float)(b < n ? b : n) : 0.f;
	}
	r.changed = s.changed;
	return r;
}

} // namespace tv
