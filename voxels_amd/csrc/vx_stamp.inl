// vx_stamp.inl — the stamps (include/voxels_hip.h, "stamps"): capture, upload and read of dense voxel boxes, and vx_grid_paste, an
// ordered batch of oriented pastes applied to the resident grid in one device pass; included by vx_hip.hip after vx_brush.inl
// (HIP only).  DESIGN.md §22.  The per-voxel and per-block logic is tv_stamp.h, shared with the host build of the tests.
//
// A batch follows the scheme of the brush batches (vx_brush.inl) and uses its pieces - BrushBin, k_brush_offsets, brush_sort,
// BRUSH_LIST_CAP.  The paste array and the table of the stamps go up in one copy each.  Then, per chunk of consecutive pastes:
//   k_paste_count    one wave per paste (a large paste: up to 64 of them, blockIdx.y): its clipped box (paste_box), one count per
//                    block of it; the first paste to reach a block gives it a slot
//   k_brush_offsets  one lane per slot: room for the block's list
//   k_paste_fill     one wave per paste again: its index into the list of every block it touches (in any order)
//   k_paste_apply    one workgroup per slot: sorts the block's list (ascending paste index - the array order), stages the block's
//                    three fields into LDS, and per paste of the list reads the box of the stamp that the block needs along the
//                    stamp's x into a second LDS tile and applies it from there with the permuted index; writes the block back
//                    once, compares it with what it staged (tv_undo.h's row masks and bounds, one slot of atomics as k_rec_swap)
//                    and takes BF_Empty from the LDS copy where a paste other than PAINT touched (block_empty_rows)
// and one rebrick_blocks over the chunk's blocks.  The call waits once, at its end, for the slot.  Blocks do not share voxels and
// a block's pastes are applied in array order, so the grid is what `count` single-paste calls leave.  The counts compare the grid
// before and after the whole batch: a block that more than one chunk touches keeps what its first chunk staged in a snapshot and
// is compared with that by its last chunk (PastePlan of tv_stamp.h), so nothing depends on where the chunk borders fall.
#include "tv_stamp.h"

struct vx_stamp {
	vx_ctx* owner = nullptr;
	u32 size[3] = { 0, 0, 0 };
	void* mem = nullptr;            // distance, material, blend: `voxels` bytes each
	size_t voxels = 0;
};

namespace {

enum { STAMP_COPY_BLOCKS = 8192 };

struct StampState {
	std::vector<vx_stamp*> stamps;
	u32* count = nullptr;      // per block of the grid: zero between chunks and calls (k_paste_apply clears it)
	u32* slotOf = nullptr;
	size_t blocks = 0;
	void* buf = nullptr;       // everything sized by the call
	size_t bufCap = 0;
	void* slot = nullptr;      // RecSwapSlot
	size_t listCap = BRUSH_LIST_CAP;
	PastePlan plan;            // host: kept, so that a small batch on a large grid does not pay for every block of the grid

	void release(vx_ctx* c)
	{
		for (vx_stamp* st : stamps) { c->be.free(st->mem); delete st; }
		c->be.free(count); c->be.free(slotOf); c->be.free(buf); c->be.free(slot);
	}
};

bool stamp_owned(const vx_ctx* c, const vx_stamp* st)
{
	const StampState* s = module_peek<StampState>(c, MOD_STAMP);
	return s && st && std::find(s->stamps.begin(), s->stamps.end(), st) != s->stamps.end();
}

// Grid box -> stamp, one field per blockIdx.y.  `wide`: the box starts at a multiple of 16 along x and its x-size is one, so
// every row of both sides is whole 16-byte pieces; otherwise bytes, consecutive lanes along x.
__global__ __launch_bounds__(WG) void k_stamp_capture(RecGrid g, RecBox box, u8* dst, size_t voxels, u32 wide)
{
	const u8* src = blockIdx.y == 0 ? g.dist : blockIdx.y == 1 ? g.mat : g.blend;
	u8* out = dst + voxels * blockIdx.y;
	const u32 sx = box.hi[0] - box.lo[0], sy = box.hi[1] - box.lo[1], n = g.n;
	const u32 perRow = wide ? sx >> 4 : sx;
	const size_t total = wide ? voxels >> 4 : voxels;
	for (size_t q = (size_t)blockIdx.x * WG + threadIdx.x; q < total; q += (size_t)gridDim.x * WG) {
		const u32 x = (u32)(q % perRow);
		const size_t row = q / perRow;
		const u32 y = (u32)(row % sy), z = (u32)(row / sy);
		const size_t from = ((size_t)(box.lo[2] + z) * n + box.lo[1] + y) * n + box.lo[0];
		if (wide) rec_store16(out + row * sx + x * 16u, rec_load16(src + from + x * 16u));
		else out[row * sx + x] = src[from + x];
	}
}

// what the apply pass needs beside the bin: the chunk, and for a batch of several chunks the plan's per-block arrays
struct PasteMulti {
	const u32 *first, *last, *snapOf;   // nullptr: one chunk
	u8* snaps;                          // per snapshot 12 289 bytes in a stride of 12 304 (rows stay 16-byte aligned): three fields, the flag byte
	u32 chunk;
};
enum : u32 { PASTE_SNAP_BYTES = 12304 };

// the blocks of paste i: false = it misses the grid
__device__ __forceinline__ bool paste_blocks(const Paste& p, const StampView* stamps, u32 n, u32 first[3], u32 cnt[3])
{
	RecBox box;
	if (!paste_box(p, stamps[p.stamp].size, n, &box)) return false;
	paste_box_blocks(box, first, cnt);
	return true;
}

__global__ __launch_bounds__(WG) void k_paste_count(BrushBin p, const Paste* pastes, const StampView* stamps)
{
	const u32 lane = threadIdx.x & 63u, i = p.begin + blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (i >= p.end) return;
	u32 first[3], cnt[3];
	if (!paste_blocks(pastes[i], stamps, p.nb * 16u, first, cnt)) return;
	const u32 total = cnt[0] * cnt[1] * cnt[2];
	for (u32 q = blockIdx.y * 64u + lane; q < total; q += gridDim.y * 64u) {
		const u32 x = first[0] + q % cnt[0], y = first[1] + (q / cnt[0]) % cnt[1], z = first[2] + q / (cnt[0] * cnt[1]);
		const u32 id = (z * p.nb + y) * p.nb + x;
		if (atomicAdd(&p.count[id], 1u) == 0u) {
			const u32 slot = atomicAdd(&p.counters[0], 1u);
			if (slot < p.slots) { p.ids[slot] = id; p.slotOf[id] = slot; }
		}
	}
}

__global__ __launch_bounds__(WG) void k_paste_fill(BrushBin p, const Paste* pastes, const StampView* stamps)
{
	const u32 lane = threadIdx.x & 63u, i = p.begin + blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (i >= p.end) return;
	u32 first[3], cnt[3];
	if (!paste_blocks(pastes[i], stamps, p.nb * 16u, first, cnt)) return;
	const u32 total = cnt[0] * cnt[1] * cnt[2];
	for (u32 q = blockIdx.y * 64u + lane; q < total; q += gridDim.y * 64u) {
		const u32 x = first[0] + q % cnt[0], y = first[1] + (q / cnt[0]) % cnt[1], z = first[2] + q / (cnt[0] * cnt[1]);
		const u32 slot = p.slotOf[(z * p.nb + y) * p.nb + x];
		if (slot >= p.slots) continue;
		const u32 at = atomicAdd(&p.cursor[slot], 1u);
		if (at < p.listCap) p.list[at] = i;
	}
}

__global__ __launch_bounds__(WG) void k_paste_apply(RecGrid g, BrushBin p, const Paste* pastes, const StampView* stamps, PasteMulti multi, RecSwapSlot* out)
{
	__shared__ __attribute__((aligned(16))) i8 sDist[4096];
	__shared__ __attribute__((aligned(16))) u8 sMat[4096];
	__shared__ __attribute__((aligned(16))) u8 sBlend[4096];
	__shared__ __attribute__((aligned(16))) u8 sTile[3][4096];
	__shared__ u32 sList[BRUSH_SORT_LDS];
	__shared__ u32 sRed[WG / 64][7];
	__shared__ i8 lastOfRow[WG];
	__shared__ int waveMax[WG / 64];
	__shared__ u32 runs;

	const u32 t = threadIdx.x, slot = blockIdx.x;
	if (slot >= p.counters[0]) return; // (cannot happen: the host counted the same blocks)
	const u32 nb = p.nb, n = nb * 16u, id = p.ids[slot], L = p.count[id];
	if (p.offset[slot] + L > p.listCap) return;
	const u32 bc[3] = { id % nb, (id / nb) % nb, id / (nb * nb) };
	u32* glist = p.list + p.offset[slot];
	const u32* lst = glist;
	if (L <= BRUSH_SORT_LDS) {
		for (u32 i = t; i < L; i += WG) sList[i] = glist[i];
		__syncthreads();
		brush_sort(sList, L, t);
		lst = sList;
	} else {
		__syncthreads();
		brush_sort(glist, L, t);
	}
	__syncthreads();
	int carves = 0;
	for (u32 i = t; i < L; i += WG) if (paste_mode_writes_distance(pastes[lst[i]].mode)) carves = 1;
	const bool anyCarve = __syncthreads_or(carves) != 0;

	// row t of the block = (y = t & 15, z = t >> 4): 16 bytes of every dense field (a whole grid: pitch n, origin 0)
	const size_t rowAt = rec_grid_row(n, id, t);
	RecRow d0 = rec_load16(g.dist + rowAt), m0 = rec_load16(g.mat + rowAt), b0 = rec_load16(g.blend + rowAt);
	rec_store16((u8*)sDist + t * 16u, d0); rec_store16(sMat + t * 16u, m0); rec_store16(sBlend + t * 16u, b0);
	u8 flag0 = g.flags[id];

	for (u32 k = 0; k < L; ++k) {
		const Paste ps = pastes[lst[k]];        // (uniform)
		const StampView sv = stamps[ps.stamp];
		PasteSection s;
		if (!paste_section(ps, sv.size, bc, s)) continue;
		const size_t voxels = stamp_voxels(sv.size);
		const bool mats = paste_mode_reads_materials(ps.mode);
		__syncthreads(); // every lane is through with the tile of the paste before (and, the first time, the block is staged)
		const u32 tiles = paste_tile_count(s);
		for (u32 q = t; q < tiles; q += WG) {
			u32 at;
			const size_t from = paste_tile_source(s, sv.size, q, at);
			sTile[0][at] = sv.base[from];
			if (mats) { sTile[1][at] = sv.base[voxels + from]; sTile[2][at] = sv.base[2u * voxels + from]; }
		}
		__syncthreads();
		const u32 total = paste_voxel_count(s);
		for (u32 v = t; v < total; v += WG) {
			u32 li;
			const u32 at = paste_tile_index(s, v, li);
			i8 d = sDist[li];
			u8 m = sMat[li], b = sBlend[li];
			paste_combine(ps.mode, (i8)sTile[0][at], mats ? sTile[1][at] : (u8)0, mats ? sTile[2][at] : (u8)0, d, m, b);
			sDist[li] = d; sMat[li] = m; sBlend[li] = b;
		}
	}
	if (t == 0) p.count[id] = 0; // the counter is clean for the next chunk and the next call
	__syncthreads();

	const RecRow d1 = rec_load16((const u8*)sDist + t * 16u), m1 = rec_load16(sMat + t * 16u), b1 = rec_load16(sBlend + t * 16u);
	rec_store16(g.dist + rowAt, d1); rec_store16(g.mat + rowAt, m1); rec_store16(g.blend + rowAt, b1);
	u8 flag1 = flag0;
	if (anyCarve) { // (uniform)
		uint4 raw;
		memcpy(&raw, d1.w, 16);
		flag1 = block_empty_rows(raw, sDist[0], t, lastOfRow, waveMax, &runs) ? 1 : 0;
		if (t == 0) g.flags[id] = flag1;
	}

	// the comparison with the grid from before the batch: what this chunk staged, or what the block's first chunk kept
	bool compare = true;
	if (multi.first) {
		const u32 first = multi.first[id], last = multi.last[id];
		if (first != last) { // (uniform)
			u8* snap = multi.snaps + (size_t)multi.snapOf[id] * PASTE_SNAP_BYTES;
			if (multi.chunk == first) {
				rec_store16(snap + t * 16u, d0); rec_store16(snap + 4096u + t * 16u, m0); rec_store16(snap + 8192u + t * 16u, b0);
				if (t == 0) snap[12288] = flag0;
			} else if (multi.chunk == last) {
				d0 = rec_load16(snap + t * 16u); m0 = rec_load16(snap + 4096u + t * 16u); b0 = rec_load16(snap + 8192u + t * 16u);
				flag0 = snap[12288];
			}
			compare = multi.chunk == last;
		}
	}
	if (!compare) return; // (uniform)
	// [0..2] ~min, [3..5] max, [6] count: zeros where nothing differed, all combined by max / sum (as k_rec_swap)
	u32 v[7] = { 0, 0, 0, 0, 0, 0, 0 };
	rec_row_bounds(n, id, t, rec_row_diff(d0, d1) | rec_row_diff(m0, m1) | rec_row_diff(b0, b1), v);
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
		u32 a = sRed[0][t], count = sRed[0][6];
#pragma unroll
		for (u32 w = 1; w < WG / 64; ++w) { a = t < 6 ? max(a, sRed[w][t]) : a + sRed[w][t]; count += sRed[w][6]; }
		if (count) {
			if (t < 3) atomicMax(&out->notMin[t], a);
			else if (t < 6) atomicMax(&out->max[t - 3], a);
			else atomicAdd(&out->changed, (unsigned long long)a);
		}
		if (t == 0 && (count || flag0 != flag1)) atomicAdd(&out->blocks, 1u);
		if (t == 0 && flag0 != flag1) atomicAdd(&out->flagChanges, 1u);
	}
}

} // namespace

extern "C" {

static_assert(sizeof(vx_stamp_info) == 32 && sizeof(vx_paste) == 32 && sizeof(vx_paste_result) == 32 && sizeof(vx_paste_counts) == 48, "stamp record layouts");
static_assert(sizeof(Paste) == sizeof(vx_paste) && sizeof(PasteResult) == sizeof(vx_paste_result) && sizeof(PasteCounts) == sizeof(vx_paste_counts) && sizeof(StampView) == 24, "tv_stamp.h records");
static_assert(VX_STAMP_MAX_EDGE == tv::STAMP_MAX_EDGE && VX_STAMP_MAX_VOXELS == tv::STAMP_MAX_VOXELS && VX_PASTE_MAX_COUNT == tv::PASTE_MAX_COUNT && VX_PASTE_MAX_STAMPS == tv::PASTE_MAX_STAMPS, "stamp limits");
static_assert(VX_PASTE_REPLACE == tv::PASTE_REPLACE && VX_PASTE_UNION == tv::PASTE_UNION && VX_PASTE_SUBTRACT == tv::PASTE_SUBTRACT && VX_PASTE_PAINT == tv::PASTE_PAINT, "paste modes");

static vx_stamp* stamp_new(vx_ctx* c, const u32 size[3])
{
	vx_stamp* st = new vx_stamp();
	st->owner = c;
	for (int k = 0; k < 3; ++k) st->size[k] = size[k];
	st->voxels = stamp_voxels(size);
	st->mem = c->be.alloc(st->voxels * 3u);
	if (!st->mem) { delete st; return nullptr; }
	return st;
}

int vx_stamp_capture(vx_ctx* c, const vx_box* box, vx_stamp** out)
{
	VX_ENTER(c);
	const std::string what = "vx_stamp_capture: ";
	if (out) *out = nullptr;
	if (!c) return VX_ERR_INVALID;
	if (!out) return fail(c, VX_ERR_INVALID, what + "null out pointer");
	if (!undo_whole_grid(c)) return fail(c, VX_ERR_INVALID, what + "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (const char* bad = stamp_check_box(c->n, (const RecBox*)box)) return fail(c, VX_ERR_INVALID, what + bad);
	RecBox b;
	memcpy(&b, box, sizeof(b));
	const u32 size[3] = { b.hi[0] - b.lo[0], b.hi[1] - b.lo[1], b.hi[2] - b.lo[2] };
	StampState* s = module_state<StampState>(c, MOD_STAMP);
	vx_stamp* st = stamp_new(c, size);
	if (!st) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	const u32 wide = (b.lo[0] % 16u == 0u && size[0] % 16u == 0u) ? 1u : 0u;
	const size_t items = wide ? st->voxels / 16u : st->voxels;
	const u32 wgs = (u32)std::min<size_t>((items + WG - 1) / WG, (size_t)STAMP_COPY_BLOCKS);
	hipLaunchKernelGGL(k_stamp_capture, dim3(wgs, 3), dim3(WG), 0, c->be.stream, undo_grid(c), b, (u8*)st->mem, st->voxels, wide);
	if (!c->be.check(hipGetLastError(), "k_stamp_capture launch")) { c->be.free(st->mem); delete st; return fail(c, VX_ERR_DEVICE, what + "device pass failed: " + c->be.error()); }
	s->stamps.push_back(st);
	*out = st;
	return VX_OK;
}

int vx_stamp_upload(vx_ctx* c, const uint32_t size[3], const int8_t* dist, const uint8_t* mat, const uint8_t* blend, vx_stamp** out)
{
	VX_ENTER(c);
	const std::string what = "vx_stamp_upload: ";
	if (out) *out = nullptr;
	if (!c) return VX_ERR_INVALID;
	if (!out) return fail(c, VX_ERR_INVALID, what + "null out pointer");
	if (const char* bad = stamp_check_size(size)) return fail(c, VX_ERR_INVALID, what + bad);
	if (!dist) return fail(c, VX_ERR_INVALID, what + "null distance array");
	StampState* s = module_state<StampState>(c, MOD_STAMP);
	vx_stamp* st = stamp_new(c, size);
	if (!st) return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error());
	u8* base = (u8*)st->mem;
	bool ok = c->be.h2d_async(base, dist, st->voxels);
	ok = ok && (mat ? c->be.h2d_async(base + st->voxels, mat, st->voxels) : c->be.fill(base + st->voxels, 0, st->voxels));
	ok = ok && (blend ? c->be.h2d_async(base + 2u * st->voxels, blend, st->voxels) : c->be.fill(base + 2u * st->voxels, 0, st->voxels));
	if (!ok) { c->be.sync(); c->be.free(st->mem); delete st; return fail(c, VX_ERR_DEVICE, what + "copy failed: " + c->be.error()); }
	s->stamps.push_back(st);
	*out = st;
	return VX_OK;
}

int vx_stamp_read(vx_ctx* c, const vx_stamp* st, int8_t* dist, uint8_t* mat, uint8_t* blend)
{
	VX_ENTER(c);
	const std::string what = "vx_stamp_read: ";
	if (!c) return VX_ERR_INVALID;
	if (!st) return fail(c, VX_ERR_INVALID, what + "null stamp");
	if (!stamp_owned(c, st)) return fail(c, VX_ERR_INVALID, what + "the stamp belongs to another context");
	const u8* base = (const u8*)st->mem;
	bool ok = true;
	if (dist) ok = ok && c->be.d2h_async(dist, base, st->voxels);
	if (mat) ok = ok && c->be.d2h_async(mat, base + st->voxels, st->voxels);
	if (blend) ok = ok && c->be.d2h_async(blend, base + 2u * st->voxels, st->voxels);
	ok = ok && c->be.sync_ok();
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, what + "copy failed: " + c->be.error());
}

int vx_stamp_info_get(vx_ctx* c, const vx_stamp* st, vx_stamp_info* info)
{
	VX_ENTER(c);
	const std::string what = "vx_stamp_info_get: ";
	if (info) memset(info, 0, sizeof(*info));
	if (!c) return VX_ERR_INVALID;
	if (!st || !info) return fail(c, VX_ERR_INVALID, what + "null argument");
	if (!stamp_owned(c, st)) return fail(c, VX_ERR_INVALID, what + "the stamp belongs to another context");
	for (int k = 0; k < 3; ++k) info->size[k] = st->size[k];
	info->voxels = st->voxels; info->bytes = st->voxels * 3u;
	return VX_OK;
}

void vx_stamp_free(vx_ctx* c, vx_stamp* st)
{
	VX_ENTER(c);
	if (!c || !st || !module_peek<StampState>(c, MOD_STAMP)) return;
	StampState* s = module_peek<StampState>(c, MOD_STAMP);
	auto it = std::find(s->stamps.begin(), s->stamps.end(), st);
	if (it == s->stamps.end()) return;
	s->stamps.erase(it);
	c->be.sync(); // (a capture, an upload or a paste of the stamp may still be queued)
	c->be.free(st->mem);
	delete st;
}

int vx_paste_box(const vx_paste* paste, const uint32_t stamp_size[3], uint32_t n, vx_box* out)
{
	if (out) memset(out, 0, sizeof(*out));
	if (!paste || !stamp_size || !out || n < 16u || n % 16u || n > (u32)VX_MAX_GRID) return VX_ERR_INVALID;
	if (!stamp_size[0] || !stamp_size[1] || !stamp_size[2] || paste->orient > 7u) return VX_ERR_INVALID;
	Paste p;
	memcpy(&p, paste, sizeof(p));
	return paste_box(p, stamp_size, n, (RecBox*)out);
}

// test hook: the capacity of the (paste, block) lists of this context's batches (0 = the default), so that tests reach the
// chunked path at small sizes
int vx_debug_paste_list_cap(vx_ctx* c, uint32_t cap)
{
	if (!c) return VX_ERR_INVALID;
	module_state<StampState>(c, MOD_STAMP)->listCap = cap ? cap : (size_t)BRUSH_LIST_CAP;
	return VX_OK;
}

int vx_grid_paste(vx_ctx* c, vx_stamp* const* stamps, uint32_t n_stamps, const vx_paste* pastes, uint32_t count, vx_paste_result* results, vx_paste_counts* counts)
{
	VX_ENTER(c);
	const std::string what = "vx_grid_paste: ";
	if (counts) memset(counts, 0, sizeof(*counts));
	if (results && count <= VX_PASTE_MAX_COUNT) memset(results, 0, (size_t)count * sizeof(*results));
	if (!c) return VX_ERR_INVALID;
	if (!undo_whole_grid(c)) return fail(c, VX_ERR_INVALID, what + "needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	if (n_stamps && !stamps) return fail(c, VX_ERR_INVALID, what + "null stamp array");
	if (n_stamps > VX_PASTE_MAX_STAMPS) return fail(c, VX_ERR_INVALID, what + "more than VX_PASTE_MAX_STAMPS stamps");
	std::vector<u32> sizes((size_t)n_stamps * 3u + 3u, 0u);
	for (u32 i = 0; i < n_stamps; ++i) {
		if (!stamps[i]) continue;
		if (!stamp_owned(c, stamps[i])) return fail(c, VX_ERR_INVALID, what + "a stamp belongs to another context");
		for (int k = 0; k < 3; ++k) sizes[(size_t)i * 3u + k] = stamps[i]->size[k];
	}
	const u32 (*size3)[3] = (const u32 (*)[3])sizes.data();
	if (const char* bad = paste_check((const Paste*)pastes, count, size3, n_stamps)) return fail(c, VX_ERR_INVALID, what + bad);
	if (!count) return VX_OK;

	StampState* s = module_state<StampState>(c, MOD_STAMP);
	const u32 nb = c->n / 16;
	const size_t blocks = (size_t)nb * nb * nb;
	PastePlan& plan = s->plan;
	paste_plan((const Paste*)pastes, count, size3, c->n, s->listCap, (PasteResult*)results, plan);
	if (!plan.distinct) return VX_OK;
	const bool several = plan.chunks.size() > 1;

	// device buffers: the per-block counters (zero between calls), the slot, and one buffer for everything sized by the call
	auto noMemory = [&]() { return fail(c, VX_ERR_DEVICE, what + "allocation failed: " + c->be.error()); };
	if (s->blocks != blocks) {
		c->be.free(s->count); c->be.free(s->slotOf);
		s->count = (u32*)c->be.alloc(blocks * 4);
		s->slotOf = (u32*)c->be.alloc(blocks * 4);
		s->blocks = 0;
		if (!s->count || !s->slotOf || !c->be.fill(s->count, 0, blocks * 4)) return noMemory();
		s->blocks = blocks;
	}
	if (!s->slot && !(s->slot = c->be.alloc(sizeof(RecSwapSlot)))) return noMemory();
	auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t atPastes = 0, atStamps = pad((size_t)count * sizeof(Paste)), atCounters = atStamps + pad((size_t)n_stamps * sizeof(StampView));
	const size_t atIds = atCounters + pad(plan.chunks.size() * 8), atOffset = atIds + pad((size_t)plan.maxSlots * 4), atCursor = atOffset + pad((size_t)plan.maxSlots * 4);
	const size_t atList = atCursor + pad((size_t)plan.maxSlots * 4), atFirst = atList + pad(plan.maxEntries * 4);
	const size_t perBlock = several ? pad(blocks * 4) : 0, atSnaps = atFirst + 3u * perBlock;
	const size_t need = atSnaps + pad((size_t)plan.snaps * PASTE_SNAP_BYTES);
	if (need > s->bufCap) {
		c->be.free(s->buf);
		s->bufCap = need + need / 2;
		s->buf = c->be.alloc(s->bufCap);
		if (!s->buf) { s->bufCap = 0; return noMemory(); }
	}
	char* base = (char*)s->buf;
	std::vector<StampView> views(n_stamps);
	for (u32 i = 0; i < n_stamps; ++i) {
		memset(&views[i], 0, sizeof(StampView));
		if (!stamps[i]) continue;
		views[i].base = (const u8*)stamps[i]->mem;
		for (int k = 0; k < 3; ++k) views[i].size[k] = stamps[i]->size[k];
	}
	bool ok = c->be.h2d_async(base + atPastes, pastes, (size_t)count * sizeof(Paste)) && c->be.h2d_async(base + atStamps, views.data(), (size_t)n_stamps * sizeof(StampView))
	       && c->be.fill(base + atCounters, 0, plan.chunks.size() * 8) && c->be.fill(s->slot, 0, sizeof(RecSwapSlot));
	PasteMulti multi;
	memset(&multi, 0, sizeof(multi));
	if (several && ok) {
		ok = c->be.h2d_async(base + atFirst, plan.first.data(), blocks * 4) && c->be.h2d_async(base + atFirst + perBlock, plan.last.data(), blocks * 4)
		  && c->be.h2d_async(base + atFirst + 2u * perBlock, plan.snapOf.data(), blocks * 4);
		multi.first = (const u32*)(base + atFirst); multi.last = (const u32*)(base + atFirst + perBlock); multi.snapOf = (const u32*)(base + atFirst + 2u * perBlock);
		multi.snaps = (u8*)(base + atSnaps);
	}
	// what rebrick_blocks marks on the host holds only where a byte or a flag changed (as vx_record_swap)
	const bool storeValid = c->matStoreValid, mapStale = c->cellMapStale, planValid = c->planValid;
	const Paste* dPastes = (const Paste*)(base + atPastes);
	const StampView* dStamps = (const StampView*)(base + atStamps);
	for (size_t k = 0; k < plan.chunks.size() && ok; ++k) {
		const PasteChunk& ch = plan.chunks[k];
		if (!ch.slots) continue;
		BrushBin p;
		p.brushes = nullptr;
		p.begin = ch.begin; p.end = ch.end; p.nb = nb;
		p.count = s->count; p.slotOf = s->slotOf;
		p.ids = (u32*)(base + atIds); p.offset = (u32*)(base + atOffset); p.cursor = (u32*)(base + atCursor);
		p.counters = (u32*)(base + atCounters) + 2 * k;
		p.list = (u32*)(base + atList);
		p.slots = ch.slots; p.listCap = (u32)ch.entries;
		multi.chunk = (u32)k;
		const u32 waves = ch.end - ch.begin, perWg = WG / 64, split = std::min<u32>((ch.most + 63u) / 64u, 64u); // (waves over the blocks of the largest paste)
		hipLaunchKernelGGL(k_paste_count, dim3((waves + perWg - 1) / perWg, split), dim3(WG), 0, c->be.stream, p, dPastes, dStamps);
		hipLaunchKernelGGL(k_brush_offsets, dim3((ch.slots + WG - 1) / WG), dim3(WG), 0, c->be.stream, p);
		hipLaunchKernelGGL(k_paste_fill, dim3((waves + perWg - 1) / perWg, split), dim3(WG), 0, c->be.stream, p, dPastes, dStamps);
		hipLaunchKernelGGL(k_paste_apply, dim3(ch.slots), dim3(WG), 0, c->be.stream, undo_grid(c), p, dPastes, dStamps, multi, (RecSwapSlot*)s->slot);
		ok = c->be.check(hipGetLastError(), "k_paste launch");
		if (ok) rebrick_blocks(c, p.ids, ch.slots);
	}
	RecSwapSlot slot;
	memset(&slot, 0, sizeof(slot));
	ok = ok && c->be.d2h(&slot, s->slot, sizeof(slot)); // (the call's one wait)
	if (!ok) { c->be.sync(); s->blocks = 0; return fail(c, VX_ERR_DEVICE, what + "device edit failed: " + c->be.error()); }
	if (!slot.blocks) { c->matStoreValid = storeValid; c->cellMapStale = mapStale; c->planValid = planValid; }
	if (counts) {
		const PasteCounts r = paste_counts(c->n, slot, plan.distinct);
		memcpy(counts, &r, sizeof(r));
	}
	return VX_OK;
}

} // extern "C"
