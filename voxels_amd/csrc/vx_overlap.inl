// vx_overlap.inl — a level's regular triangles that meet query boxes (include/voxels_hip.h, "overlap queries"); included by
// vx_hip.hip after vx_shape.inl and vx_scatter.inl: it reads the index of vx_ray.inl and shares the scan helpers of the LOD
// selection and the scattering (HIP only, like the ray casts).
//
// Three launches, the shape of k_scatter_count / k_scatter_scan / k_scatter_write:
//   k_overlap_count  one wave per query, four queries per workgroup.  The wave walks the blocks of the query's candidate range
//                    in coord_id order, 64 candidates at a time: a lane's block -> the dilated-box test and the level's map,
//                    then the meshed ones in lane order.  Per block: a lane per bucket (dilated-box test, not empty), and per
//                    run of candidate buckets the lanes go over the run's slice of the permutation: three positions, the
//                    predicate, counted by ballot.  One record per query: matches, and blocks with a match.
//   k_overlap_scan   one workgroup: exclusive scan of the per-query counts in 64 bits -> the first result of every query, the
//                    ranges and vx_overlap_counts.
//   k_overlap_write  the walk of the count pass again (nothing is cached between the passes).  The order inside a bucket's
//                    slice of the permutation is decided by atomics in k_ray_index, so nothing is emitted in traversal order:
//                    per block the wave marks the matches in its own LDS bitmap over the triangle ordinals (atomicOr), then
//                    the lanes take a word each, a wave prefix of the popcounts gives every word its place, and a lane emits
//                    the set bits of its word ascending, at first + offset while that is below the capacity.
// The order is query, coord_id, tri, with no atomic on it.  Every loop is bounded by a table or bucket size; the waves of a
// workgroup share nothing (no barrier: a wave's LDS accesses are served in program order).  Lane logic: tv_overlap.h.
#include "tv_overlap.h"

namespace {

struct OverlapQuery {       // per query, 16 bytes
	unsigned long long first;   // k_overlap_scan: matches of the queries before
	u32 count;                  // matches
	u32 pairs;                  // entries with a match
};

struct OverlapParams {
	const float4* boxes;    // vx_overlap_box: two float4 each
	u32 n;
	u32 empty;              // the level's table is empty: no count pass ran, every count is 0
	const ListedBlock* table;
	const u32* map;
	const u16* starts;
	const u16* perm;
	const PolyVertex* verts;
	const u32* idx;
	u32 cnt;                // blocks per axis of the level
	float size;             // block edge in voxels
	OverlapQuery* per;
	uint4* tris;            // vx_overlap_tri
	float4* corners;        // three float4 per result, or null
	uint2* ranges;          // vx_overlap_range, or null
	vx_overlap_counts* counts;
	u32 capacity;
};

__device__ __forceinline__ void overlap_position(const PolyVertex* v, u32 i, float P[3])
{
	const float4 q = *(const float4*)&v[i];
	P[0] = q.x; P[1] = q.y; P[2] = q.z;
}

// what one wave's lanes wrote to its part of the LDS is read by other lanes of the same wave
__device__ __forceinline__ void overlap_wave_sync()
{
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the walk of one query by one wave; WRITE = false counts, WRITE = true writes
template <bool WRITE> __device__ __forceinline__ void overlap_query(const OverlapParams& p)
{
	__shared__ u32 bitmaps[WRITE ? (WG / 64) * OVERLAP_WORDS : 1];
	const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	const u32 q = blockIdx.x * (WG / 64) + wave;
	if (q >= p.n) return;   // (the whole wave)
	u32* bits = bitmaps + (WRITE ? wave * OVERLAP_WORDS : 0u);
	u32 first = 0, written = 0;
	if (WRITE) {
		// nothing is written when the total does not fit 32 bits, and nothing of a query without matches or beyond the capacity
		if (p.counts->triangles > 0xFFFFFFFFull) return;
		const OverlapQuery mine = p.per[q];
		if (mine.count == 0u || mine.first >= (unsigned long long)p.capacity) return;
		first = (u32)mine.first;
	}
	const float4 b0 = p.boxes[2 * q], b1 = p.boxes[2 * q + 1];
	const float lo[3] = { b0.x, b0.y, b0.z }, hi[3] = { b1.x, b1.y, b1.z };
	u32 count = 0, pairs = 0;   // uniform in the wave
	if (overlap_box_valid(lo, hi)) {
		int c0[3];
		u32 ext[3];
		for (int a = 0; a < 3; ++a) {
			int c1;
			overlap_block_range(lo[a], hi[a], p.size, p.cnt, c0[a], c1);
			ext[a] = c1 >= c0[a] ? (u32)(c1 - c0[a] + 1) : 0u;
		}
		const u32 total = ext[0] * ext[1] * ext[2];   // (<= cnt^3, which the map's size already bounds by 2^32)
		const float sub = p.size / (float)RAY_SUB;
		for (u32 base = 0; base < total; base += 64u) {
			u32 e = RAY_NONE;
			if (base + lane < total) {
				int m[3];
				overlap_candidate_cell(base + lane, c0, ext, m);
				const float org[3] = { (float)m[0] * p.size, (float)m[1] * p.size, (float)m[2] * p.size };
				if (overlap_block_meets(lo, hi, org, sub)) e = p.map[ray_coord_id(m, p.cnt)];
			}
			unsigned long long blocks = __ballot(e != RAY_NONE);
			while (blocks) {
				const int src = __builtin_ctzll(blocks);
				blocks &= blocks - 1ull;
				const u32 eb = (u32)__builtin_amdgcn_readfirstlane(__shfl((int)e, src, 64));   // (the same in every lane: kept in a scalar register)
				const ListedBlock& b = p.table[eb];
				const u32 nTri = b.rec.iCount / 3u;
				const PolyVertex* v = p.verts + b.rec.vOff;
				const u32* ix = p.idx + b.rec.iOff;
				const u16* perm = p.perm + b.rec.iOff / 3u;
				const u16* starts = p.starts + (size_t)eb * (RAY_BUCKETS + 1);
				float org[3];
				ray_block_origin(b.rec.coordId, p.cnt, p.size, org);
				// a lane per bucket
				unsigned long long buckets = __ballot(overlap_bucket_meets(lo, hi, org, sub, lane) && starts[lane] < starts[lane + 1u]);
				if (!buckets) continue;
				const u32 nWords = min(overlap_words(nTri), (u32)OVERLAP_WORDS);
				if (WRITE) {
					for (u32 w = lane; w < nWords; w += 64u) bits[w] = 0u;
					overlap_wave_sync();
				}
				u32 inBlock = 0;
				while (buckets) {
					u32 s0, s1;
					overlap_next_run(buckets, s0, s1);
					const u32 k1 = starts[s1];
					for (u32 k0 = starts[s0]; k0 < k1; k0 += 64u) {
						const u32 k = k0 + lane;
						bool hit = false;
						u32 tri = 0;
						if (k < k1) {
							tri = perm[k];
							float A[3], B[3], C[3];
							overlap_position(v, ix[3u * tri], A);
							overlap_position(v, ix[3u * tri + 1u], B);
							overlap_position(v, ix[3u * tri + 2u], C);
							hit = overlap_matches(lo, hi, A, B, C);
						}
						if (WRITE) {
							u32 word;
							const u32 bit = overlap_mark(tri, word);
							if (hit && word < nWords) atomicOr(&bits[word], bit);
						} else {
							inBlock += (u32)__popcll(__ballot(hit));
						}
					}
				}
				if (!WRITE) {
					count += inBlock;
					pairs += inBlock ? 1u : 0u;
					continue;
				}
				overlap_wave_sync();
				for (u32 w0 = 0; w0 < nWords; w0 += 64u) {
					const u32 w = w0 + lane;
					u32 word = w < nWords ? bits[w] : 0u;
					const u32 pc = (u32)__popc(word), incl = wave_inclusive_scan(pc);
					u32 at = first + written + incl - pc;   // (no wrap: the total fits 32 bits)
					while (word) {
						const u32 tri = (w << 5) + (u32)__builtin_ctz(word);
						word &= word - 1u;
						if (at < p.capacity) {
							p.tris[at] = make_uint4(q, eb, b.id, tri);
							if (p.corners) {
								float4* o = p.corners + 3 * (size_t)at;
								for (u32 j = 0; j < 3u; ++j) {
									float4 c = *(const float4*)&v[ix[3u * tri + j]];
									c.w = 0.f;
									o[j] = c;
								}
							}
						}
						++at;
					}
					written += (u32)__shfl((int)incl, 63, 64);
				}
				if (first + written >= p.capacity) return;   // (the whole wave: every later match lies beyond the capacity)
			}
		}
	}
	if (!WRITE && lane == 0) {
		OverlapQuery r;
		r.first = 0ull; r.count = count; r.pairs = pairs;
		p.per[q] = r;
	}
}

__global__ __launch_bounds__(WG) void k_overlap_count(OverlapParams p) { overlap_query<false>(p); }
__global__ __launch_bounds__(WG) void k_overlap_write(OverlapParams p) { overlap_query<true>(p); }

// one workgroup: the first result of every query (exclusive scan of the counts in 64 bits), the ranges, the counts
__global__ __launch_bounds__(LOD_SCAN_WG) void k_overlap_scan(OverlapParams p)
{
	__shared__ unsigned long long waveTot[LOD_SCAN_WG / 64];
	__shared__ unsigned long long running, pairSum;
	__shared__ u32 hitSum, maxCount;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 n = p.empty ? 0u : p.n;
	if (tid == 0) { running = pairSum = 0; hitSum = maxCount = 0; }
	__syncthreads();
	unsigned long long pairs = 0;
	u32 hits = 0, most = 0;
	for (u32 base = 0; base < n; base += LOD_SCAN_WG) {
		const u32 k = base + tid;
		unsigned long long cnt = 0;
		if (k < n) {
			const OverlapQuery t = p.per[k];
			cnt = t.count; pairs += t.pairs; hits += t.count ? 1u : 0u; most = max(most, t.count);
		}
		const unsigned long long incl = scatter_wave_scan64(cnt);
		if (lane == 63) waveTot[wave] = incl;
		__syncthreads();
		unsigned long long before = 0, sum = 0;
		for (u32 w = 0; w < LOD_SCAN_WG / 64; ++w) { const unsigned long long s = waveTot[w]; before += w < wave ? s : 0ull; sum += s; }
		if (k < n) p.per[k].first = running + before + incl - cnt;
		__syncthreads();
		if (tid == 0) running += sum;
		__syncthreads();
	}
	for (int o = 32; o > 0; o >>= 1) { pairs += __shfl_xor(pairs, o, 64); hits += __shfl_xor(hits, o, 64); most = max(most, (u32)__shfl_xor((int)most, o, 64)); }
	if (lane == 0) { atomicAdd(&pairSum, pairs); atomicAdd(&hitSum, hits); atomicMax(&maxCount, most); }
	__syncthreads();
	const unsigned long long total = running;
	if (tid == 0) {
		vx_overlap_counts* o = p.counts;
		o->triangles = total;
		o->pairs = pairSum;
		o->queries = n;
		o->hit_queries = hitSum;
		o->max_per_query = maxCount;
		o->reserved = 0;
	}
	if (p.ranges && total <= 0xFFFFFFFFull) {
		if (p.empty) for (u32 k = tid; k < p.n; k += LOD_SCAN_WG) p.ranges[k] = make_uint2(0u, 0u);
		else for (u32 k = tid; k < n; k += LOD_SCAN_WG) p.ranges[k] = make_uint2((u32)p.per[k].first, p.per[k].count); // (a lane reads back its own stores)
	}
}

struct OverlapState {
	OverlapQuery* per = nullptr;
	size_t perCap = 0;          // bytes
	void* io = nullptr;         // vx_overlap_boxes: the boxes and the output arrays on their way through the device
	size_t ioCap = 0;

	void release(vx_ctx* c)
	{
		c->be.free(per); c->be.free(io);
	}
};

int overlap_check(vx_ctx* c, uint32_t level, const void* boxes, uint32_t n, uint32_t capacity, const void* tris, const void* corners,
                  const void* counts, const char* what)
{
	const int rc = ray_check(c, level, what);
	if (rc != VX_OK) return rc;
	const std::string w(what);
	if (!counts) return fail(c, VX_ERR_INVALID, w + ": null counts");
	if (n && !boxes) return fail(c, VX_ERR_INVALID, w + ": null boxes");
	if (n > VX_OVERLAP_MAX_QUERIES) return fail(c, VX_ERR_INVALID, w + ": more than VX_OVERLAP_MAX_QUERIES queries");
	if (capacity && !tris) return fail(c, VX_ERR_INVALID, w + ": null result array with a non-zero capacity");
	if (corners && !tris) return fail(c, VX_ERR_INVALID, w + ": corners without a result array");
	return VX_OK;
}

// the launches of one call on the context's stream; builds the level's index if it is not current, and allocates only when
// the per-query scratch does not fit yet
int overlap_launch(vx_ctx* c, uint32_t level, const vx_overlap_box* dBoxes, uint32_t n, uint32_t capacity, vx_overlap_tri* dTris,
                   float* dCorners, vx_overlap_range* dRanges, vx_overlap_counts* dCounts, const char* what)
{
	OverlapState* s = module_state<OverlapState>(c, MOD_OVERLAP);
	int rc = ray_prepare(c, level);
	if (rc != VX_OK) return rc;
	if (n && !dev_grow(c, s->per, s->perCap, (size_t)n * sizeof(OverlapQuery)))
		return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
	const RayState* rs = module_peek<RayState>(c, MOD_RAY);
	const RayLevel& l = rs->lv[level];
	OverlapParams p;
	memset(&p, 0, sizeof(p));
	p.boxes = (const float4*)dBoxes;
	p.n = n;
	p.empty = l.entries == 0u;
	p.table = l.table;
	p.map = l.map;
	p.starts = l.starts;
	p.perm = rs->perm;
	p.verts = (const PolyVertex*)c->dVerts;
	p.idx = (const u32*)c->dIdx;
	p.cnt = c->lv[level].cnt;
	p.size = (float)(16u << level);
	p.per = s->per;
	p.tris = (uint4*)dTris;
	p.corners = (float4*)dCorners;
	p.ranges = (uint2*)dRanges;
	p.counts = dCounts;
	p.capacity = capacity;
	hipStream_t st = c->be.stream;
	const bool walk = n && !p.empty;
	const u32 groups = (n + WG / 64 - 1) / (WG / 64);
	bool ok = true;
	if (walk) {
		hipLaunchKernelGGL(k_overlap_count, dim3(groups), dim3(WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_overlap_count launch");
	}
	if (ok) {
		hipLaunchKernelGGL(k_overlap_scan, dim3(1), dim3(LOD_SCAN_WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_overlap_scan launch");
	}
	if (ok && walk && capacity) {
		hipLaunchKernelGGL(k_overlap_write, dim3(groups), dim3(WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_overlap_write launch");
	}
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, std::string(what) + ": " + c->be.error());
}

} // namespace

extern "C" {

static_assert(sizeof(vx_overlap_box) == 32 && sizeof(vx_overlap_tri) == 16 && sizeof(vx_overlap_range) == 8 && sizeof(vx_overlap_counts) == 32,
              "vx_overlap_* layout");

int vx_overlap_boxes_device(vx_ctx* c, uint32_t level, const vx_overlap_box* d_boxes, uint32_t n, uint32_t capacity, vx_overlap_tri* d_tris,
                            float* d_corners, vx_overlap_range* d_ranges, vx_overlap_counts* d_counts)
{
	VX_ENTER(c);
	const int rc = overlap_check(c, level, d_boxes, n, capacity, d_tris, d_corners, d_counts, "vx_overlap_boxes_device");
	if (rc != VX_OK) return rc;
	if ((((uintptr_t)d_boxes | (uintptr_t)d_tris | (uintptr_t)d_corners | (uintptr_t)d_counts) & 15u) || ((uintptr_t)d_ranges & 7u))
		return fail(c, VX_ERR_INVALID, "vx_overlap_boxes_device: arrays must be 16-byte aligned (ranges: 8)");
	return overlap_launch(c, level, d_boxes, n, capacity, d_tris, d_corners, d_ranges, d_counts, "vx_overlap_boxes_device");
}

int vx_overlap_boxes(vx_ctx* c, uint32_t level, const vx_overlap_box* boxes, uint32_t n, uint32_t capacity, vx_overlap_tri* tris,
                     float* corners, vx_overlap_range* ranges, vx_overlap_counts* counts)
{
	VX_ENTER(c);
	int rc = overlap_check(c, level, boxes, n, capacity, tris, corners, counts, "vx_overlap_boxes");
	if (rc != VX_OK) return rc;
	OverlapState* s = module_state<OverlapState>(c, MOD_OVERLAP);
	const size_t boxBytes = (size_t)n * sizeof(vx_overlap_box), rangeBytes = lod_align16((size_t)n * sizeof(vx_overlap_range));
	const size_t triBytes = (size_t)capacity * sizeof(vx_overlap_tri), cornerBytes = corners ? (size_t)capacity * 48u : 0u;
	if (!dev_grow(c, s->io, s->ioCap, sizeof(vx_overlap_counts) + boxBytes + rangeBytes + triBytes + cornerBytes))
		return fail(c, VX_ERR_DEVICE, "vx_overlap_boxes: allocation failed: " + c->be.error());
	char* io = (char*)s->io;   // (every part is a multiple of 16 bytes)
	vx_overlap_counts* dCounts = (vx_overlap_counts*)io;
	vx_overlap_box* dBoxes = (vx_overlap_box*)(io + sizeof(vx_overlap_counts));
	vx_overlap_range* dRanges = (vx_overlap_range*)((char*)dBoxes + boxBytes);
	vx_overlap_tri* dTris = (vx_overlap_tri*)((char*)dRanges + rangeBytes);
	float* dCorners = (float*)((char*)dTris + triBytes);
	if (n && !c->be.h2d(dBoxes, boxes, boxBytes)) return fail(c, VX_ERR_DEVICE, "vx_overlap_boxes: upload failed: " + c->be.error());
	rc = overlap_launch(c, level, dBoxes, n, capacity, capacity ? dTris : nullptr, corners ? dCorners : nullptr, ranges ? dRanges : nullptr,
	                    dCounts, "vx_overlap_boxes");
	if (rc != VX_OK) return rc;
	if (!c->be.d2h(counts, dCounts, sizeof(vx_overlap_counts))) return fail(c, VX_ERR_DEVICE, "vx_overlap_boxes: download failed: " + c->be.error());
	const bool fits = counts->triangles <= 0xFFFFFFFFull;
	const size_t filled = fits ? (size_t)std::min<uint64_t>(counts->triangles, capacity) : 0;
	bool ok = true;
	if (fits && ranges && n) ok = c->be.d2h(ranges, dRanges, (size_t)n * sizeof(vx_overlap_range));
	if (ok && filled) ok = c->be.d2h(tris, dTris, filled * sizeof(vx_overlap_tri));
	if (ok && filled && corners) ok = c->be.d2h(corners, dCorners, filled * 48u);
	if (!ok) return fail(c, VX_ERR_DEVICE, "vx_overlap_boxes: download failed: " + c->be.error());
	if (counts->triangles > capacity) return fail(c, VX_ERR_OVERFLOW, "vx_overlap_boxes: capacity too small (counts.triangles says how much is needed)");
	return VX_OK;
}

} // extern "C"
