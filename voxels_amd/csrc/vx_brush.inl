// vx_brush.inl — vx_grid_inject_brushes (include/voxels_hip.h, "edits on the device"): an ordered batch of brushes applied
// to the resident grid in one device pass; included by vx_hip.hip after vx_host.inl (HIP only).  DESIGN.md §15.
//
// The brush array goes up in one copy.  Then, per chunk of consecutive brushes (one chunk unless the lists below would
// outgrow BRUSH_LIST_CAP entries):
//   k_brush_count    one wave per brush: its box of blocks (the reference's per-axis float tests, edit_touched_box of
//                    vx_host.inl), one count per touched block; the first brush to reach a block gives it a slot
//   k_brush_offsets  one lane per slot: room for the block's list
//   k_brush_fill     one wave per brush again: its index into the list of every block it touches (in any order)
//   k_brush_apply    one workgroup per slot: sorts the block's list (ascending brush index - the array order), stages the
//                    block into LDS, applies the brushes of the list one after the other there, writes the block back once
//                    and computes its BF_Empty flag from the LDS copy
// and one rebrick_blocks over the chunk's blocks.  The call waits once, at its end.  Blocks do not share voxels and a
// block's brushes are applied in array order, so the result is what `count` single-brush calls leave; nothing of it
// depends on the order in which the atomics of the binning were served (slots and list positions are only places).
#include "tv_brush.h"

namespace {

enum { BRUSH_LIST_CAP = 1u << 22, BRUSH_SORT_LDS = 1024, BRUSH_TILE = 16, BRUSH_STEPS = 18 };

struct BrushBin {
	const vx_brush* brushes;
	u32 begin, end;       // the chunk's brushes
	u32 nb;
	u32* count;           // per block of the grid: brushes of the chunk that touch it (zero between chunks: k_brush_apply clears it)
	u32* slotOf;          // per block: its slot in this chunk (valid where count != 0)
	u32* ids;             // per slot: the block
	u32* offset;          // per slot: where its list starts
	u32* cursor;          // per slot: fill position
	u32* counters;        // [0] slots handed out, [1] list entries handed out
	u32* list;
	u32 slots, listCap;   // what the host counted: the bounds of ids / offset / cursor and of list
};

struct BrushState {
	u32* count = nullptr;
	u32* slotOf = nullptr;
	size_t blocks = 0;
	void* buf = nullptr;
	size_t bufCap = 0;
	std::vector<u32> stamp; // host: per block, the last chunk that counted it (distinct blocks of a chunk)
	u32 stampNow = 0;

	void release(vx_ctx* c)
	{
		c->be.free(count); c->be.free(slotOf); c->be.free(buf);
	}
};

// The blocks brush b touches, per axis first .. first + cnt - 1: the tests of edit_touched_box (vx_host.inl), which are
// the reference's expressions; the lanes of a wave take the blocks of an axis 64 at a time.
__device__ __forceinline__ bool brush_blocks(const vx_brush& b, u32 nb, u32 lane, u32 first[3], u32 cnt[3])
{
	bool any = true;
	for (int k = 0; k < 3; ++k) {
		u32 lo = 0, hi = 0, hits = 0;
		for (u32 b0 = 0; b0 < nb; b0 += 64) {
			const u32 blk = b0 + lane;
			const float bmin = (float)(blk * 16), bmax = (bmin + 8.f) + 8.f;
			const bool hit = blk < nb && !(b.position[k] - b.extents[k] > bmax || bmin > b.position[k] + b.extents[k]);
			const unsigned long long m = __ballot(hit);
			if (!m) continue;
			if (!hits) lo = b0 + (u32)__builtin_ctzll(m);
			hi = b0 + 63u - (u32)__builtin_clzll(m);
			hits += (u32)__builtin_popcountll(m);
		}
		if (!hits || hi - lo + 1 != hits) any = false;
		first[k] = lo; cnt[k] = hits;
	}
	return any;
}

__global__ __launch_bounds__(WG) void k_brush_count(BrushBin p)
{
	const u32 lane = threadIdx.x & 63u, i = p.begin + blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (i >= p.end) return;
	u32 first[3], cnt[3];
	if (!brush_blocks(p.brushes[i], p.nb, lane, first, cnt)) return;
	const u32 total = cnt[0] * cnt[1] * cnt[2];
	for (u32 q = lane; q < total; q += 64) {
		const u32 x = first[0] + q % cnt[0], y = first[1] + (q / cnt[0]) % cnt[1], z = first[2] + q / (cnt[0] * cnt[1]);
		const u32 id = (z * p.nb + y) * p.nb + x;
		if (atomicAdd(&p.count[id], 1u) == 0u) {
			const u32 slot = atomicAdd(&p.counters[0], 1u);
			if (slot < p.slots) { p.ids[slot] = id; p.slotOf[id] = slot; }
		}
	}
}

__global__ __launch_bounds__(WG) void k_brush_offsets(BrushBin p)
{
	const u32 slot = blockIdx.x * WG + threadIdx.x;
	if (slot >= p.slots || slot >= p.counters[0]) return;
	const u32 off = atomicAdd(&p.counters[1], p.count[p.ids[slot]]);
	p.offset[slot] = off;
	p.cursor[slot] = off;
}

__global__ __launch_bounds__(WG) void k_brush_fill(BrushBin p)
{
	const u32 lane = threadIdx.x & 63u, i = p.begin + blockIdx.x * (WG / 64) + (threadIdx.x >> 6);
	if (i >= p.end) return;
	u32 first[3], cnt[3];
	if (!brush_blocks(p.brushes[i], p.nb, lane, first, cnt)) return;
	const u32 total = cnt[0] * cnt[1] * cnt[2];
	for (u32 q = lane; q < total; q += 64) {
		const u32 x = first[0] + q % cnt[0], y = first[1] + (q / cnt[0]) % cnt[1], z = first[2] + q / (cnt[0] * cnt[1]);
		const u32 slot = p.slotOf[(z * p.nb + y) * p.nb + x];
		if (slot >= p.slots) continue;
		const u32 at = atomicAdd(&p.cursor[slot], 1u);
		if (at < p.listCap) p.list[at] = i;
	}
}

// Ascending sort of a[0 .. L) by the whole workgroup: the bitonic network whose comparators all point the same way, over the
// next power of two; the missing tail counts as +infinity, which such comparators never move, so pairs that reach beyond L
// are skipped.
__device__ __forceinline__ void brush_sort(u32* a, u32 L, u32 tid)
{
	u32 half = 1;
	while (half * 2 < L) half *= 2; // pairs per pass = (next power of two) / 2
	for (u32 k = 2; (k >> 1) < L; k <<= 1) {
		for (u32 q = tid; q < half; q += WG) {
			const u32 h = k >> 1, lo = (q / h) * k + q % h, hi = (q / h) * k + (k - 1u - q % h);
			if (hi < L) { const u32 u = a[lo], v = a[hi]; if (u > v) { a[lo] = v; a[hi] = u; } }
		}
		__syncthreads();
		for (u32 j = k >> 2; j > 0; j >>= 1) {
			for (u32 q = tid; q < half; q += WG) {
				const u32 lo = (q / j) * 2u * j + q % j, hi = lo + j;
				if (hi < L) { const u32 u = a[lo], v = a[hi]; if (u > v) { a[lo] = v; a[hi] = u; } }
			}
			__syncthreads();
		}
	}
}

// The per-block section of an edit (edit_section of tv_block.h) as tables.  Per axis k the reference runs two float loops: the
// grid's `for (x = b0; x < b1; ++x)` over the voxels and the brush's `for (x = s0; x < s1; x += 1)` over the samples.  Entry i
// of a table is the loop variable after i steps (edit_step), the count is the number of entries before the first that fails
// the loop's test - the trip count.  Groups 0..2 = voxel loops of x, y, z; 3..5 = sample loops.
struct BrushTables {
	float v[6][BRUSH_STEPS];
	int n[6];
};

__global__ __launch_bounds__(WG) void k_brush_apply(GridView g, u8* flags, BrushBin p)
{
	__shared__ __attribute__((aligned(16))) i8 sDist[4096];
	__shared__ __attribute__((aligned(16))) u8 sMat[4096];
	__shared__ __attribute__((aligned(16))) u8 sBlend[4096];
	__shared__ u32 sList[BRUSH_SORT_LDS];
	__shared__ __attribute__((aligned(16))) vx_brush sBrush[BRUSH_TILE];
	__shared__ BrushTables sTab[2];
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
	int hasMat = 0, hasDist = 0;
	for (u32 i = t; i < L; i += WG) { if (p.brushes[lst[i]].shape == (u32)BRUSH_MATERIAL) hasMat = 1; else hasDist = 1; }
	const bool anyMat = __syncthreads_or(hasMat) != 0;
	const bool anyDist = __syncthreads_or(hasDist) != 0;

	// row t of the block = (y = t & 15, z = t >> 4): 16 bytes of the dense fields (a whole grid: pitch n, origin 0)
	const size_t rowAt = ((size_t)(bc[2] * 16u + (t >> 4)) * n + bc[1] * 16u + (t & 15u)) * n + bc[0] * 16u;
	((uint4*)sDist)[t] = *(const uint4*)(g.dist + rowAt);
	if (anyMat) {
		((uint4*)sMat)[t] = *(const uint4*)(g.mat + rowAt);
		((uint4*)sBlend)[t] = *(const uint4*)(g.blend + rowAt);
	}

	u32 par = 0;
	for (u32 tile = 0; tile < L; tile += BRUSH_TILE) {
		__syncthreads(); // the previous tile is used up (and, the first time, the block is staged)
		if (t < BRUSH_TILE * 4u && tile + (t >> 2) < L) ((uint4*)sBrush)[t] = ((const uint4*)p.brushes)[(size_t)lst[tile + (t >> 2)] * 4u + (t & 3u)];
		__syncthreads();
		const u32 inTile = L - tile < (u32)BRUSH_TILE ? L - tile : (u32)BRUSH_TILE;
		for (u32 j = 0; j < inTile; ++j, par ^= 1u) {
			const vx_brush& b = sBrush[j];
			BrushTables& T = sTab[par];
			if (t < 192u) {
				const u32 grp = t >> 5, i = t & 31u, k = grp % 3u;
				const float bmin = (float)(bc[k] * 16u);
				const float q = b.position[k] - b.extents[k] / 2;
				const float b0 = edit_clampf(q, bmin, bmin + 16.f) - bmin;
				const float b1 = edit_clampf(q + b.extents[k], bmin, bmin + 16.f) - bmin;
				const float start = grp < 3u ? b0 : (bmin + b0) - b.position[k];
				const float end = grp < 3u ? b1 : (bmin + b1) - b.position[k];
				const float x = edit_step(start, (int)(i < (u32)BRUSH_STEPS ? i : (u32)BRUSH_STEPS - 1u));
				const unsigned long long m = __ballot(i < (u32)BRUSH_STEPS && x < end);
				const u32 mine = (u32)(m >> (t & 32u)); // the 32 lanes of this group
				if (i < (u32)BRUSH_STEPS) T.v[grp][i] = x;
				if (i == 0) T.n[grp] = __builtin_ctz(~mine);
			}
			__syncthreads(); // tables ready; every lane is through with the brush before
			const int c0 = T.n[0], c1 = T.n[1], c2 = T.n[2], total = c0 * c1 * c2;
			if (b.shape != (u32)BRUSH_MATERIAL) {
				const int s0 = T.n[3], s1 = T.n[4], s2 = T.n[5], plane = s0 * s1, samples = plane * s2;
				for (int v = (int)t; v < total; v += WG) {
					const int ix = v % c0, iy = (v / c0) % c1, iz = v / (c0 * c1);
					const u32 li = ((u32)T.v[2][iz] * 16u + (u32)T.v[1][iy]) * 16u + (u32)T.v[0][ix];
					// the voxel's sample is the one its running index meets in the brush's output (edit_voxel of tv_block.h)
					float sv = 0.f;
					if (plane > 0 && v < samples) {
						const int jz = v / plane, rem = v - jz * plane, jy = rem / s0, jx = rem - jy * s0;
						sv = brush_sample(b.shape, T.v[3][jx], T.v[4][jy], T.v[5][jz], b.a, b.b, b.radius);
					}
					const float value = (float)sDist[li];
					float r;
					if (b.type == 0u) r = value < sv ? value : sv;        // IT_Add: min
					else if (b.type == 1u) r = value > sv ? value : sv;   // IT_SubtractAddInner: max
					else r = (-sv > value) ? -sv : value;                 // IT_Subtract: max(-surface, value)
					sDist[li] = edit_round_distance(r);
				}
			} else {
				const float coeff = (b.extents[0] / 2.0f) * 0.75f;
				const float m0 = (float)(bc[0] * 16u), m1 = (float)(bc[1] * 16u), m2 = (float)(bc[2] * 16u);
				const u8 material = (u8)b.material;
				for (int v = (int)t; v < total; v += WG) {
					const int ix = v % c0, iy = (v / c0) % c1, iz = v / (c0 * c1);
					const float x = T.v[0][ix], y = T.v[1][iy], z = T.v[2][iz];
					const u32 li = ((u32)z * 16u + (u32)y) * 16u + (u32)x;
					const float cx = (x + m0) - b.position[0], cy = (y + m1) - b.position[1], cz = (z + m2) - b.position[2];
					const float d = sqrtf((cx * cx + cy * cy) + cz * cz) / coeff;
					float w = 1 - d;
					w = w > 0.f ? w : 0.f; w = w < 1.f ? w : 1.f;
					const u8 outBlend = (u8)(w * 255.f);
					if (sMat[li] == material) {
						int s = (b.type ? 1 : -1) * (int)outBlend + (int)sBlend[li];
						s = s < 255 ? s : 255; s = s > 0 ? s : 0;
						sBlend[li] = (u8)s;
					} else {
						sMat[li] = material;
						sBlend[li] = outBlend;
					}
				}
			}
		}
	}
	if (t == 0) p.count[id] = 0; // the counter is clean for the next chunk and the next call
	__syncthreads();

	const uint4 raw = ((const uint4*)sDist)[t];
	if (anyDist) *(uint4*)(const_cast<i8*>(g.dist) + rowAt) = raw;
	if (anyMat) {
		*(uint4*)(const_cast<u8*>(g.mat) + rowAt) = ((const uint4*)sMat)[t];
		*(uint4*)(const_cast<u8*>(g.blend) + rowAt) = ((const uint4*)sBlend)[t];
	}
	if (!anyDist) return; // (uniform) blocks that only material brushes touch keep their flag

	// BF_Empty by the codec's rule from the LDS copy (block_empty_rows of vx_hip.hip, as k_edit_flags)
	const bool empty = block_empty_rows(raw, sDist[0], t, lastOfRow, waveMax, &runs);
	if (t == 0) flags[id] = empty ? 1 : 0;
}

// host: the blocks of one axis that a brush touches.  The test of edit_touched_box is monotone in the block (the first
// comparison holds for the low blocks only, the second for the high ones), so the hits are one interval: an arithmetic
// guess at its start is corrected with the very test, then the test is walked to the interval's end.
bool brush_axis_range(u32 nb, float pos, float ext, u32& first, u32& count)
{
	auto below = [&](u32 b) { const float bmin = (float)(b * 16), bmax = (bmin + 8.f) + 8.f; return pos - ext > bmax; };
	auto above = [&](u32 b) { const float bmin = (float)(b * 16); return bmin > pos + ext; };
	const float guess = (pos - ext) / 16.f - 1.f;
	u32 b = guess > 0.f ? (guess < (float)nb ? (u32)guess : nb) : 0u;
	while (b > 0 && !below(b - 1)) --b;
	while (b < nb && below(b)) ++b;
	first = b;
	count = 0;
	while (b < nb && !above(b)) { ++b; ++count; }
	return count != 0;
}

struct BrushChunk { u32 begin, end, slots; size_t entries; };

bool brush_finite(const float* f, int n) { for (int i = 0; i < n; ++i) if (!std::isfinite(f[i])) return false; return true; }

} // namespace

extern "C" {

static_assert(sizeof(vx_brush) == 64 && sizeof(vx_brush_result) == 32, "vx_brush / vx_brush_result layout");
static_assert(VX_BRUSH_BALL == tv::BRUSH_BALL && VX_BRUSH_CAPSULE == tv::BRUSH_CAPSULE && VX_BRUSH_BOX == tv::BRUSH_BOX && VX_BRUSH_MATERIAL == tv::BRUSH_MATERIAL, "brush shapes");

int vx_grid_inject_brushes(vx_ctx* c, const vx_brush* brushes, uint32_t count, vx_brush_result* results,
                           float union_min[3], float union_max[3], uint32_t* touched_blocks)
{
	VX_ENTER(c);
	const char* what = "vx_grid_inject_brushes";
	if (union_min) union_min[0] = union_min[1] = union_min[2] = 0.f;
	if (union_max) union_max[0] = union_max[1] = union_max[2] = 0.f;
	if (touched_blocks) *touched_blocks = 0;
	if (!c) return VX_ERR_INVALID;
	if (!count) return VX_OK;
	if (!brushes) return fail(c, VX_ERR_INVALID, std::string(what) + ": null brush array");
	if (count > VX_BRUSH_MAX_COUNT) return fail(c, VX_ERR_INVALID, std::string(what) + ": more than VX_BRUSH_MAX_COUNT brushes");
	if (!c->ownsGrid || !c->n || (c->zBegin != 0 || c->zEnd != c->n || c->yBegin != 0 || c->yEnd != c->n)) return fail(c, VX_ERR_INVALID, std::string(what) + ": needs a whole grid owned by the context (vx_grid_upload / vx_grid_upload_packed)");
	for (u32 i = 0; i < count; ++i) {
		const vx_brush& b = brushes[i];
		if (b.shape >= (u32)BRUSH_SHAPES) return fail(c, VX_ERR_INVALID, std::string(what) + ": unknown shape in brush " + std::to_string(i));
		if (b.type > (b.shape == VX_BRUSH_MATERIAL ? 1u : 2u)) return fail(c, VX_ERR_INVALID, std::string(what) + ": unknown type in brush " + std::to_string(i));
		if (!brush_finite(b.position, 3) || !brush_finite(b.extents, 3) || !brush_finite(b.a, 3) || !brush_finite(b.b, 3) || !brush_finite(&b.radius, 1))
			return fail(c, VX_ERR_INVALID, std::string(what) + ": field that is not finite in brush " + std::to_string(i));
		if (b.shape == VX_BRUSH_MATERIAL && b.material > 255u) return fail(c, VX_ERR_INVALID, std::string(what) + ": material above 255 in brush " + std::to_string(i));
	}

	BrushState* s = module_state<BrushState>(c, MOD_BRUSH);
	const u32 nb = c->n / 16;
	const size_t blocks = (size_t)nb * nb * nb;
	if (s->stamp.size() != blocks) { s->stamp.assign(blocks, 0); s->stampNow = 0; }

	// per brush: the box it hands back and its blocks; chunks of consecutive brushes whose lists fit BRUSH_LIST_CAP entries
	// (a single brush has at most `blocks` <= 2^21 of them), and per chunk the number of distinct blocks
	std::vector<BrushChunk> chunks;
	BrushChunk cur = { 0, 0, 0, 0 };
	auto open_chunk = [&](u32 at) {
		cur = BrushChunk{ at, at, 0, 0 };
		if (++s->stampNow == 0) { std::fill(s->stamp.begin(), s->stamp.end(), 0u); s->stampNow = 1; }
	};
	open_chunk(0);
	float umin[3] = { 0, 0, 0 }, umax[3] = { 0, 0, 0 };
	bool any = false;
	size_t distinctAll = 0, maxEntries = 0;
	u32 maxSlots = 0;
	std::vector<unsigned char> seenAll; // distinct blocks over all chunks (only needed when there is more than one)
	for (u32 i = 0; i < count; ++i) {
		const vx_brush& b = brushes[i];
		float mn[3], mx[3];
		edit_modified_box(c->n, b.position, b.extents, mn, mx);
		u32 first[3] = { 0, 0, 0 }, cnt[3] = { 0, 0, 0 };
		bool hit = true;
		for (int k = 0; k < 3; ++k) hit = brush_axis_range(nb, b.position[k], b.extents[k], first[k], cnt[k]) && hit;
		const size_t touched = hit ? (size_t)cnt[0] * cnt[1] * cnt[2] : 0;
		if (results) {
			for (int k = 0; k < 3; ++k) { results[i].out_min[k] = mn[k]; results[i].out_max[k] = mx[k]; }
			results[i].touched_blocks = (u32)touched;
			results[i].reserved = 0;
		}
		if (touched) {
			for (int k = 0; k < 3; ++k) { umin[k] = any ? std::min(umin[k], mn[k]) : mn[k]; umax[k] = any ? std::max(umax[k], mx[k]) : mx[k]; }
			any = true;
			if (cur.entries && cur.entries + touched > (size_t)BRUSH_LIST_CAP) {
				cur.end = i;
				chunks.push_back(cur);
				if (seenAll.empty()) { seenAll.assign(blocks, 0); for (size_t q = 0; q < blocks; ++q) seenAll[q] = s->stamp[q] == s->stampNow; }
				open_chunk(i);
			}
			for (u32 z = first[2]; z < first[2] + cnt[2]; ++z)
			for (u32 y = first[1]; y < first[1] + cnt[1]; ++y)
			for (u32 x = first[0]; x < first[0] + cnt[0]; ++x) {
				const size_t id = ((size_t)z * nb + y) * nb + x;
				if (s->stamp[id] != s->stampNow) { s->stamp[id] = s->stampNow; ++cur.slots; }
				if (!seenAll.empty()) seenAll[id] = 1;
			}
			cur.entries += touched;
		}
	}
	cur.end = count;
	chunks.push_back(cur);
	if (!any) return VX_OK;
	for (const BrushChunk& k : chunks) { maxEntries = std::max(maxEntries, k.entries); maxSlots = std::max(maxSlots, k.slots); }
	if (chunks.size() == 1) distinctAll = cur.slots;
	else for (unsigned char f : seenAll) distinctAll += f;
	if (union_min) for (int k = 0; k < 3; ++k) union_min[k] = umin[k];
	if (union_max) for (int k = 0; k < 3; ++k) union_max[k] = umax[k];
	if (touched_blocks) *touched_blocks = (u32)distinctAll;

	// device buffers: the per-block counters (zero between calls) and one buffer for everything sized by the call
	if (s->blocks != blocks) {
		c->be.free(s->count); c->be.free(s->slotOf);
		s->count = (u32*)c->be.alloc(blocks * 4);
		s->slotOf = (u32*)c->be.alloc(blocks * 4);
		s->blocks = 0;
		if (!s->count || !s->slotOf || !c->be.fill(s->count, 0, blocks * 4)) return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
		s->blocks = blocks;
	}
	auto pad = [](size_t v) { return (v + 255) & ~(size_t)255; };
	const size_t atBrushes = 0, atCounters = pad((size_t)count * sizeof(vx_brush)), atIds = atCounters + pad(chunks.size() * 8);
	const size_t atOffset = atIds + pad((size_t)maxSlots * 4), atCursor = atOffset + pad((size_t)maxSlots * 4), atList = atCursor + pad((size_t)maxSlots * 4);
	const size_t need = atList + pad(maxEntries * 4);
	if (need > s->bufCap) {
		c->be.free(s->buf);
		s->bufCap = need + need / 2;
		s->buf = c->be.alloc(s->bufCap);
		if (!s->buf) { s->bufCap = 0; return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error()); }
	}
	char* base = (char*)s->buf;
	bool ok = c->be.h2d_async(base + atBrushes, brushes, (size_t)count * sizeof(vx_brush)) && c->be.fill(base + atCounters, 0, chunks.size() * 8);
	const GridView g = resident_view(c);
	for (size_t k = 0; k < chunks.size() && ok; ++k) {
		const BrushChunk& ch = chunks[k];
		if (!ch.slots) continue;
		BrushBin p;
		p.brushes = (const vx_brush*)(base + atBrushes);
		p.begin = ch.begin; p.end = ch.end; p.nb = nb;
		p.count = s->count; p.slotOf = s->slotOf;
		p.ids = (u32*)(base + atIds); p.offset = (u32*)(base + atOffset); p.cursor = (u32*)(base + atCursor);
		p.counters = (u32*)(base + atCounters) + 2 * k;
		p.list = (u32*)(base + atList);
		p.slots = ch.slots; p.listCap = (u32)ch.entries;
		const u32 waves = ch.end - ch.begin, perWg = WG / 64;
		hipLaunchKernelGGL(k_brush_count, dim3((waves + perWg - 1) / perWg), dim3(WG), 0, c->be.stream, p);
		hipLaunchKernelGGL(k_brush_offsets, dim3((ch.slots + WG - 1) / WG), dim3(WG), 0, c->be.stream, p);
		hipLaunchKernelGGL(k_brush_fill, dim3((waves + perWg - 1) / perWg), dim3(WG), 0, c->be.stream, p);
		hipLaunchKernelGGL(k_brush_apply, dim3(ch.slots), dim3(WG), 0, c->be.stream, g, (u8*)c->dFlags, p);
		ok = c->be.check(hipGetLastError(), "k_brush launch");
		if (ok) rebrick_blocks(c, p.ids, ch.slots);
	}
	ok = c->be.sync_ok() && ok;
	if (!ok) s->blocks = 0; // the per-block counters may be left half used: cleared again before the next call
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, std::string(what) + ": device edit failed: " + c->be.error());
}

} // extern "C"
