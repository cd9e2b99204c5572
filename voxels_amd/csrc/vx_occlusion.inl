// vx_occlusion.inl — ambient occlusion (include/voxels_hip.h, "ambient occlusion"): vx_occlusion and vx_occlusion_device, one byte
// per vertex of a level's meshes from probes into the resident grid; included by vx_hip.hip after vx_height.inl (HIP only).
// DESIGN.md §25.  The rule is tv_occlusion.h, shared with the host build of the tests.
//
// The work item is a table entry.  One launch:
//   k_occlusion_bake  one workgroup of 256 lanes per entry of the level's block table; an entry the filter box does not visit
//                     leaves at once (uniform).  Phase 1: a lane per (y, z) row of the block's neighbourhood - the lattice points
//                     from 16 b - (steps + 2) to 16 b + 16 + (steps + 2) per axis - forms the row's sign bits as one 64-bit mask
//                     in LDS (at most 45 x 45 rows, 16.2 KB): at level 0 out of the 16-byte distance rows of the blocks the row
//                     crosses, a block of one sign without a read where the sign summaries are current; above, a strided read.
//                     Phase 2: a lane per vertex of the entry's regular range and, with VX_OCCLUSION_TRANSITIONS, of its six
//                     transition ranges - quantise, walk the 98 directions (the table sits in constant memory: the index is the
//                     same in every lane, the read a scalar load) with one bit test in LDS per sample, one byte stored.  A sample
//                     outside the staged region is read from the grid itself, so no result depends on the staging.
//                     The counts are reduced per workgroup and go out as two 64-bit adds, two 32-bit adds and one 32-bit maximum.
//   k_occlusion_counts  only where the caller wants counts in device memory: one lane turns the slot into vx_occlusion_counts.
// Every atomic is an integer sum or maximum, so the results do not depend on an order or a schedule.  The calls only read the
// grid, the pools and the tables.
#include "tv_occlusion.h"

namespace {

struct OcclusionState {
	void* buf = nullptr;       // the slot and the host form's counts (256 bytes), behind them the host form's staging of the bytes
	size_t bufCap = 0;
	bool shortcuts = true;     // the sign summaries may stand in for distance rows (vx_debug_occlusion_shortcuts)

	void release(vx_ctx* c)
	{
		c->be.free(buf);
	}
};

struct OcclusionArgs {
	const ListedBlock* table;
	const u32* countDev;       // the table's count in the run's device header (after a full run), or null
	u32 count;                 // the count the host knows (launch width)
	u32 level, cnt;            // blocks per axis of the level
	u32 n;
	const u8* dist;
	const u16* sign;           // sign summaries of the level-0 blocks, or null
	const PolyVertex* verts;
	u8* out;
	OcclSlot* slot;            // or null: no counts
	OcclParams prm;
};

__device__ __forceinline__ u32 occlusion_entries(const OcclusionArgs& a) { return a.countDev ? min(*a.countDev, a.count) : a.count; }

__global__ __launch_bounds__(WG) void k_occlusion_bake(OcclusionArgs a)
{
	__shared__ u64 sMask[OCCL_MAX_ROWS];
	__shared__ u32 sRed[WG / 64][9];
	const u32 e = blockIdx.x, t = threadIdx.x;
	if (e >= occlusion_entries(a)) return;
	const ListedBlock& b = a.table[e];
	if (!occl_box_meets(a.prm, b.minc, b.maxc)) return;             // (uniform)

	// phase 1: the neighbourhood's sign bits
	const u32 coord = b.rec.coordId, steps = a.prm.steps;
	const OcclRegion R = occl_region(coord % a.cnt, (coord / a.cnt) % a.cnt, coord / (a.cnt * a.cnt), steps + 2u);
	for (u32 row = t; row < R.edge * R.edge; row += WG) sMask[row] = occl_row_mask(a.dist, a.n, a.level, a.sign, R, row);
	__syncthreads();

	// phase 2: the vertices
	const u32 lim = occl_limit(a.n, a.level);
	const u32 ranges = (a.prm.flags & OCCL_TRANSITIONS) ? 7u : 1u;
	u32 v[9] = { 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	for (u32 r = 0; r < ranges; ++r) {                              // (uniform)
		const u32 off = r ? b.rec.tvOff[r - 1u] : b.rec.vOff, cnt = r ? b.rec.tvCount[r - 1u] : b.rec.vCount;
		for (u32 i = t; i < cnt; i += WG) {
			float pos[3], nrm[3];
			occl_vertex_read(a.verts + off + i, pos, nrm);
			OcclVertex q;
			u32 byte = 255u;
			if (occl_quantise(pos, nrm, a.level, q)) {
				byte = occl_byte(q, steps, lim, [&](int cx, int cy, int cz) {
					u32 row, bit;
					if (occl_region_holds(R, cx, cy, cz, row, bit)) return ((sMask[row] >> bit) & 1ull) != 0ull;
					return occl_grid_solid(a.dist, a.n, a.level, cx, cy, cz);
				});
				occl_vertex_counts(byte, v);
			}
			a.out[off + i] = (u8)byte;
		}
	}
	if (!a.slot) return;                                            // (uniform)
	measure_reduce<3>(v, sRed, t);
	if (t < 9) {
		const u32 x = v[0];
		if (t == 1) atomicAdd(&a.slot->visited, 1u);
		else if (x) {
			if (t == 0) atomicMax(&a.slot->notDarkest, x);
			else if (t == 6) atomicAdd(&a.slot->vertices, (u64)x);
			else if (t == 7) atomicAdd(&a.slot->sum, (u64)x);
			else if (t == 8) atomicAdd(&a.slot->open, x);
		}
	}
}

// the slot as vx_occlusion_counts, in device memory
__global__ void k_occlusion_counts(OcclusionArgs a, OcclCounts* out)
{
	if (threadIdx.x == 0 && blockIdx.x == 0) *out = occl_finish(*a.slot, occlusion_entries(a));
}

// the checks of both forms; VX_OK = go on
int occlusion_check_call(vx_ctx* c, uint32_t level, const vx_occlusion_params* prm, const void* ao, uint64_t capacity, const std::string& what)
{
	if (!c) return VX_ERR_INVALID;
	if (const char* bad = occl_check(undo_whole_grid(c), c->haveSurface, c->levelsRun, level, (const OcclParams*)prm, ao, capacity, c->poolVerts))
		return fail(c, VX_ERR_INVALID, what + bad);
	return VX_OK;
}

// The launches of one bake on the context's stream.  dSlot: zeroed by the caller, or null; dCounts (device): written from the
// slot by a launch of its own, or null.
int occlusion_launch(vx_ctx* c, const OcclusionState* s, uint32_t level, const OcclParams& prm, u8* dOut, OcclSlot* dSlot, OcclCounts* dCounts, const std::string& what)
{
	const vx_listed_block* tab = nullptr;
	u32 nb = 0;
	const int rc = vx_device_block_table(c, level, &tab, &nb);
	if (rc != VX_OK) return rc;
	OcclusionArgs a;
	memset(&a, 0, sizeof(a));
	a.table = (const ListedBlock*)tab;
	a.countDev = c->meshEpoch == c->fullRunEpoch ? (const u32*)c->dHeader + HDR_LISTS + level : nullptr;
	a.count = nb;
	a.level = level; a.cnt = c->lv[level].cnt;
	a.n = c->n;
	a.dist = (const u8*)c->dDist;
	a.sign = s->shortcuts && level == 0u ? grid_block_signs(c) : nullptr;
	a.verts = (const PolyVertex*)c->dVerts;
	a.out = dOut;
	a.slot = dSlot;
	a.prm = prm;
	bool ok = true;
	if (nb) {
		hipLaunchKernelGGL(k_occlusion_bake, dim3(nb), dim3(WG), 0, c->be.stream, a);
		ok = c->be.check(hipGetLastError(), "k_occlusion_bake launch");
	}
	if (ok && dCounts) {
		hipLaunchKernelGGL(k_occlusion_counts, dim3(1), dim3(64), 0, c->be.stream, a, dCounts);
		ok = c->be.check(hipGetLastError(), "k_occlusion_counts launch");
	}
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error());
}

} // namespace

extern "C" {

static_assert(sizeof(vx_occlusion_params) == 48 && sizeof(vx_occlusion_counts) == 32, "vx_occlusion_params / vx_occlusion_counts layout");
static_assert(sizeof(OcclParams) == sizeof(vx_occlusion_params) && sizeof(OcclCounts) == sizeof(vx_occlusion_counts) && sizeof(OcclSlot) == 32, "tv_occlusion.h records");
static_assert(VX_OCCLUSION_MAX_STEPS == tv::OCCL_MAX_STEPS && VX_OCCLUSION_TRANSITIONS == tv::OCCL_TRANSITIONS, "occlusion constants");
static_assert(sizeof(PolyVertex) == 48, "a vertex is 48 bytes");

// test hook: whether the sign summaries may stand in for distance rows (the default); nothing of a result depends on it
int vx_debug_occlusion_shortcuts(vx_ctx* c, uint32_t enable)
{
	if (!c) return VX_ERR_INVALID;
	module_state<OcclusionState>(c, MOD_OCCLUSION)->shortcuts = enable != 0;
	return VX_OK;
}

int vx_occlusion_device(vx_ctx* c, uint32_t level, const vx_occlusion_params* params, uint8_t* d_ao, uint64_t capacity, vx_occlusion_counts* d_counts)
{
	VX_ENTER(c);
	const std::string what = "vx_occlusion_device: ";
	const int rc = occlusion_check_call(c, level, params, d_ao, capacity, what);
	if (rc != VX_OK) return rc;
	if ((uintptr_t)d_counts & 7u) return fail(c, VX_ERR_INVALID, what + "counts must be 8-byte aligned");
	OcclusionState* s = module_state<OcclusionState>(c, MOD_OCCLUSION);
	OcclSlot* slot = nullptr;
	if (d_counts) {
		if (!dev_grow(c, s->buf, s->bufCap, 256)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
		slot = (OcclSlot*)s->buf;
		if (!c->be.fill(slot, 0, sizeof(OcclSlot))) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error());
	}
	return occlusion_launch(c, s, level, *(const OcclParams*)params, d_ao, slot, (OcclCounts*)d_counts, what);
}

int vx_occlusion(vx_ctx* c, uint32_t level, const vx_occlusion_params* params, uint8_t* ao, uint64_t capacity, vx_occlusion_counts* counts)
{
	VX_ENTER(c);
	const std::string what = "vx_occlusion: ";
	int rc = occlusion_check_call(c, level, params, ao, capacity, what);
	if (rc != VX_OK) return rc;
	OcclusionState* s = module_state<OcclusionState>(c, MOD_OCCLUSION);
	const size_t nv = c->poolVerts;
	if (!dev_grow(c, s->buf, s->bufCap, 256 + nv)) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	OcclSlot* dSlot = (OcclSlot*)s->buf;
	OcclCounts* dCounts = (OcclCounts*)((char*)s->buf + 64);   // (the table's count is the device's: the header word behind a full run)
	u8* dOut = (u8*)s->buf + 256;
	OcclCounts res;
	if (!(c->be.fill(dSlot, 0, sizeof(OcclSlot)) && (!nv || c->be.fill(dOut, 255, nv)))) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error());
	if ((rc = occlusion_launch(c, s, level, *(const OcclParams*)params, dOut, dSlot, dCounts, what)) != VX_OK) { c->be.sync(); return rc; }
	bool ok = !nv || c->be.d2h_async(ao, dOut, nv);
	ok = ok && c->be.d2h_async(&res, dCounts, sizeof(res));
	if (!ok) { c->be.sync(); return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	if (!c->be.sync_ok()) return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); // (the call's one wait)
	if (counts) memcpy(counts, &res, sizeof(res));
	return VX_OK;
}

} // extern "C"
