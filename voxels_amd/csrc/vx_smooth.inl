// vx_smooth.inl — vx_grid_smooth (include/voxels_hip.h, "smoothing"): ordered Jacobi smoothing passes over boxes of the resident
// grid; included by vx_hip.hip after vx_island.inl (HIP only).  DESIGN.md §17.  The arithmetic and the per-lane logic are
// tv_smooth.h, shared with the host build of the tests.
//
// Per op, per iteration (a tile = a 16^3 grid block clipped to the op's box, one workgroup each, lane = one x-row):
//   k_smooth_eval    stages the tile's (16 + 2)^3 neighbourhood into LDS with the edge clamps resolved, computes the 16 new values
//                    of every row from it and writes them to the byte volume; reads the grid only, writes the volume only
//   k_smooth_commit  the volume into the grid inside the clip.  The first of several iterations keeps the grid's values in a
//                    second byte volume; the last iteration compares with them (a single iteration: with the grid's values it
//                    replaces), reduces the changed voxels' count and bounds per wave, then per workgroup, and issues one set of
//                    integer atomics into the op's slot
// Per op, after its last commit: k_box_ids, k_edit_flags and rebrick_blocks over the blocks of its box.
// Per call: k_smooth_results turns the slots into the result records and their union; one copy, one wait.
#include "tv_smooth.h"

namespace {

struct SmoothState {
	void* volume = nullptr;    // the new values of one iteration, 4096 bytes per tile
	size_t volumeCap = 0;
	void* original = nullptr;  // the op's original values (ops of more than one iteration)
	size_t originalCap = 0;
	void* ids = nullptr;       // the block ids of one op's box
	size_t idsCap = 0;
	void* perOp = nullptr;     // slots, then the result records and the union
	size_t perOpCap = 0;

	void release(vx_ctx* c)
	{
		c->be.free(volume); c->be.free(original); c->be.free(ids); c->be.free(perOp);
	}
};

struct SmoothParams { float center[3], radius, strength; };

__global__ __launch_bounds__(WG) void k_smooth_eval(GridView g, SmoothRegion r, SmoothParams p, i8* volume)
{
	__shared__ u32 staged[SMOOTH_STAGE_WORDS];
	const u32 t = threadIdx.x;
	const SmoothTile T = smooth_tile(r, blockIdx.x);
	for (u32 row = t; row < (u32)SMOOTH_STAGE_ROWS; row += WG) smooth_stage_row(g.dist, r.n, T, row, staged);
	__syncthreads();
	if (!smooth_row_inside(T, t & 15u, t >> 4)) return;
	u32 out[4];
	smooth_eval_row(staged, T, t, p.center, p.radius, p.strength, out);
	*(uint4*)(volume + (size_t)blockIdx.x * 4096u + t * 16u) = make_uint4(out[0], out[1], out[2], out[3]);
}

__global__ __launch_bounds__(WG) void k_smooth_commit(GridView g, SmoothRegion r, const i8* volume, i8* original, u32 mode, SmoothSlot* slot)
{
	__shared__ u32 sRed[WG / 64][7];
	const u32 t = threadIdx.x;
	const SmoothTile T = smooth_tile(r, blockIdx.x);
	const size_t at = (size_t)blockIdx.x * 4096u + t * 16u;
	const u32 changed = smooth_commit_row(const_cast<i8*>(g.dist), r.n, T, t, volume + at, original ? original + at : nullptr, mode);
	if (!(mode & (u32)(SMOOTH_COMPARE_GRID | SMOOTH_COMPARE_ORIGINAL))) return; // (uniform)
	// [0..2] ~min, [3..5] max, [6] count: zeros where nothing changed, all combined by max / sum
	u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 };
	if (changed) {
		v[0] = ~(T.org[0] + (u32)__builtin_ctz(changed)); v[1] = ~(T.org[1] + (t & 15u)); v[2] = ~(T.org[2] + (t >> 4));
		v[3] = T.org[0] + 31u - (u32)__builtin_clz(changed); v[4] = ~v[1]; v[5] = ~v[2];
		v[6] = (u32)__builtin_popcount(changed);
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
		for (int k = 0; k < 6; ++k) v[k] = max(v[k], (u32)__shfl_xor((int)v[k], d));
		v[6] += (u32)__shfl_xor((int)v[6], d);
	}
	if ((t & 63u) == 0) {
#pragma unroll
		for (int k = 0; k < 7; ++k) sRed[t >> 6][k] = v[k];
	}
	__syncthreads();
	if (t < 7) {
		u32 a = sRed[0][t], any = sRed[0][6];
#pragma unroll
		for (u32 w = 1; w < WG / 64; ++w) { a = t < 6 ? max(a, sRed[w][t]) : a + sRed[w][t]; any += sRed[w][6]; }
		if (any) {
			if (t < 3) atomicMax(&slot->notMin[t], a);
			else if (t < 6) atomicMax(&slot->max[t - 3], a);
			else atomicAdd(&slot->changed, (unsigned long long)a);
		}
	}
}

// slots -> out[0 .. count): the result records; out[count]: the union box and the sum.  One workgroup.
__global__ __launch_bounds__(WG) void k_smooth_results(const SmoothSlot* slots, u32 count, u32 n, SmoothResult* out)
{
	__shared__ SmoothSlot all;
	const u32 t = threadIdx.x;
	if (t == 0) { all.notMin[0] = all.notMin[1] = all.notMin[2] = 0; all.max[0] = all.max[1] = all.max[2] = 0; all.changed = 0; }
	__syncthreads();
	for (u32 i = t; i < count; i += WG) {
		const SmoothSlot s = slots[i];
		out[i] = smooth_result(n, s);
		if (!s.changed) continue;
		for (int k = 0; k < 3; ++k) { atomicMax(&all.notMin[k], s.notMin[k]); atomicMax(&all.max[k], s.max[k]); }
		atomicAdd(&all.changed, s.changed);
	}
	__syncthreads();
	if (t == 0) out[count] = smooth_result(n, all);
}

} // namespace

extern "C" {

static_assert(sizeof(vx_smooth) == 48 && sizeof(vx_smooth_result) == 32, "vx_smooth / vx_smooth_result layout");
static_assert(sizeof(SmoothSlot) == 32 && sizeof(SmoothResult) == sizeof(vx_smooth_result), "tv_smooth.h records");
static_assert(VX_SMOOTH_MAX_ITERATIONS == tv::SMOOTH_MAX_ITERATIONS && VX_SMOOTH_MAX_COUNT == tv::SMOOTH_MAX_COUNT, "smoothing limits");

int vx_grid_smooth(vx_ctx* c, const vx_smooth* ops, uint32_t count, vx_smooth_result* results, float union_min[3], float union_max[3],
                   uint64_t* changed_voxels)
{
	VX_ENTER(c);
	const char* what = "vx_grid_smooth";
	if (union_min) union_min[0] = union_min[1] = union_min[2] = 0.f;
	if (union_max) union_max[0] = union_max[1] = union_max[2] = 0.f;
	if (changed_voxels) *changed_voxels = 0;
	if (!c) return VX_ERR_INVALID;
	if (!count) return VX_OK;
	if (!ops) return fail(c, VX_ERR_INVALID, std::string(what) + ": null op array");
	if (count > VX_SMOOTH_MAX_COUNT) return fail(c, VX_ERR_INVALID, std::string(what) + ": more than VX_SMOOTH_MAX_COUNT ops");
	if (!c->ownsGrid || !c->n || (c->zBegin != 0 || c->zEnd != c->n || c->yBegin != 0 || c->yEnd != c->n)) return fail(c, VX_ERR_INVALID, std::string(what) + ": needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	size_t maxTiles = 0;
	bool anyActive = false, anyOriginal = false;
	for (u32 i = 0; i < count; ++i) {
		const vx_smooth& o = ops[i];
		for (int k = 0; k < 3; ++k)
			if (!(o.lo[k] < o.hi[k] && o.hi[k] <= c->n)) return fail(c, VX_ERR_INVALID, std::string(what) + ": the box needs lo < hi <= n on every axis in op " + std::to_string(i));
		if (!std::isfinite(o.center[0]) || !std::isfinite(o.center[1]) || !std::isfinite(o.center[2]) || !std::isfinite(o.radius) || !std::isfinite(o.strength))
			return fail(c, VX_ERR_INVALID, std::string(what) + ": field that is not finite in op " + std::to_string(i));
		if (o.radius < 0.f) return fail(c, VX_ERR_INVALID, std::string(what) + ": negative radius in op " + std::to_string(i));
		if (o.strength < 0.f || o.strength > 1.f) return fail(c, VX_ERR_INVALID, std::string(what) + ": strength outside 0..1 in op " + std::to_string(i));
		if (o.iterations > VX_SMOOTH_MAX_ITERATIONS) return fail(c, VX_ERR_INVALID, std::string(what) + ": more than VX_SMOOTH_MAX_ITERATIONS iterations in op " + std::to_string(i));
		if (!o.iterations || o.strength == 0.f) continue;
		anyActive = true;
		anyOriginal = anyOriginal || o.iterations > 1;
		maxTiles = std::max(maxTiles, (size_t)smooth_tiles(smooth_region(c->n, o.lo, o.hi)));
	}
	if (results) memset(results, 0, (size_t)count * sizeof(vx_smooth_result));
	if (!anyActive) return VX_OK;

	SmoothState* s = module_state<SmoothState>(c, MOD_SMOOTH);
	const size_t atResults = (size_t)count * sizeof(SmoothSlot);
	if (!dev_grow(c, s->volume, s->volumeCap, maxTiles * 4096) || (anyOriginal && !dev_grow(c, s->original, s->originalCap, maxTiles * 4096))
	    || !dev_grow(c, s->ids, s->idsCap, maxTiles * 4) || !dev_grow(c, s->perOp, s->perOpCap, atResults + ((size_t)count + 1) * sizeof(SmoothResult)))
		return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());

	SmoothSlot* slots = (SmoothSlot*)s->perOp;
	SmoothResult* dResults = (SmoothResult*)((char*)s->perOp + atResults);
	const GridView g = resident_view(c);
	hipStream_t st = c->be.stream;
	bool ok = c->be.fill(slots, 0, atResults);
	for (u32 i = 0; i < count && ok; ++i) {
		const vx_smooth& o = ops[i];
		if (!o.iterations || o.strength == 0.f) continue;
		const SmoothRegion r = smooth_region(c->n, o.lo, o.hi);
		const u32 tiles = smooth_tiles(r);
		const SmoothParams p = { { o.center[0], o.center[1], o.center[2] }, o.radius, o.strength };
		for (u32 it = 0; it < o.iterations; ++it) {
			const u32 mode = o.iterations == 1 ? (u32)SMOOTH_COMPARE_GRID : it == 0 ? (u32)SMOOTH_SAVE_ORIGINAL : it + 1 == o.iterations ? (u32)SMOOTH_COMPARE_ORIGINAL : 0u;
			hipLaunchKernelGGL(k_smooth_eval, dim3(tiles), dim3(WG), 0, st, g, r, p, (i8*)s->volume);
			hipLaunchKernelGGL(k_smooth_commit, dim3(tiles), dim3(WG), 0, st, g, r, (const i8*)s->volume, o.iterations > 1 ? (i8*)s->original : (i8*)nullptr, mode, slots + i);
		}
		// the flags and the mirrors of the blocks of the box follow, as after an edit (the id list is reused op after op: the
		// stream orders its writers behind its readers)
		c->be.run_box_ids((u32*)s->ids, r.tb0, r.tn, c->n / 16);
		hipLaunchKernelGGL(k_edit_flags, dim3(tiles), dim3(WG), 0, st, g, (u8*)c->dFlags, (const u32*)s->ids, tiles);
		ok = c->be.check(hipGetLastError(), "k_smooth launch");
		if (ok) rebrick_blocks(c, (const u32*)s->ids, tiles);
	}
	std::vector<SmoothResult> host((size_t)count + 1);
	if (ok) {
		hipLaunchKernelGGL(k_smooth_results, dim3(1), dim3(WG), 0, st, (const SmoothSlot*)slots, count, c->n, dResults);
		ok = c->be.check(hipGetLastError(), "k_smooth_results launch") && c->be.d2h_async(host.data(), dResults, host.size() * sizeof(SmoothResult));
	}
	ok = c->be.sync_ok() && ok;
	if (!ok) return fail(c, VX_ERR_DEVICE, std::string(what) + ": device edit failed: " + c->be.error());
	if (results) memcpy(results, host.data(), (size_t)count * sizeof(vx_smooth_result));
	const SmoothResult& all = host[count];
	for (int k = 0; k < 3; ++k) { if (union_min) union_min[k] = all.out_min[k]; if (union_max) union_max[k] = all.out_max[k]; }
	if (changed_voxels) *changed_voxels = all.changed;
	return VX_OK;
}

} // extern "C"
