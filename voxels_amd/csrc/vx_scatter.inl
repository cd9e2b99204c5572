// vx_scatter.inl — seeded instance points on the regular meshes of one LOD level (include/voxels_hip.h, "scattering"); included
// by vx_hip.hip after vx_lod.inl (HIP only, like the ray casts: the CPU emulation does not export these entry points).
//
// Three launches, the shape of k_lod_classify / k_lod_scan / k_lod_write:
//   k_scatter_count  one workgroup per table entry.  An entry whose box misses the filter box is done at once.  Otherwise, per
//                    chunk of 256 triangles: a lane's triangle -> its candidate count, an inclusive scan of the counts in LDS,
//                    then the lanes stride over the chunk's candidate SLOTS (a coarse level's triangle carries hundreds of
//                    candidates: a lane per triangle would serialise them); the slot's triangle by binary search in the scan.
//                    Kept candidates are counted by ballot.  One total per entry: kept, candidates, triangles.
//   k_scatter_scan   one workgroup: exclusive scan of the entries' kept counts -> first point of every entry, vx_scatter_counts,
//                    and the ranges.
//   k_scatter_write  the walk of the count pass again (the candidates are recomputed, nothing is cached between the passes);
//                    kept candidates compacted in slot order - ballot prefix in the wave, running offset in the workgroup - and
//                    written at first + offset while that is below the capacity.
// The order is entry, triangle, k, with no atomics on it.
#include "tv_scatter.h"

namespace {

struct ScatterTotal {       // per table entry, 32 bytes
	unsigned long long kept, candidates;
	u32 triangles;          // of a visited entry, passing the texture mask
	u32 visited;
	u32 first;              // k_scatter_scan: kept points of the entries before (meaningful when all points fit 32 bits)
	u32 pad;
};

struct ScatterParams {
	const ListedBlock* table;
	const u32* countDev;    // the table's count in the run's device header (after a full run), or null
	u32 count;              // the count the host knows (launch width)
	u32 level;
	const PolyVertex* verts;
	const u32* idx;
	ScatterTotal* totals;
	uint2* ranges;          // vx_scatter_range, or null
	uint4* points;          // vx_scatter_point: three uint4 each
	vx_scatter_counts* counts;
	u32 capacity;
	ScatterRules rules;
};

__device__ __forceinline__ u32 scatter_entries(const ScatterParams& p) { return p.countDev ? min(*p.countDev, p.count) : p.count; }

// the walk over one entry's candidates; WRITE = false counts, WRITE = true writes the kept ones
template <bool WRITE> __device__ __forceinline__ void scatter_entry(const ScatterParams& p)
{
	__shared__ u32 scan[WG];            // inclusive scan of the chunk's candidate counts
	__shared__ u32 waveTot[WG / 64];
	__shared__ u32 keptTot[2][WG / 64]; // kept candidates per wave of a batch of slots (two batches in flight)
	__shared__ unsigned long long keptSum[WG / 64];
	__shared__ u32 triSum;
	const u32 e = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	if (e >= scatter_entries(p)) return;
	const ListedBlock& b = p.table[e];
	u32 first = 0;
	if (WRITE) {
		// nothing is written when the points do not fit 32 bits, and nothing of an entry without points or beyond the capacity
		if (p.counts->points > 0xFFFFFFFFull || p.totals[e].kept == 0ull) return;
		first = p.totals[e].first;
		if (first >= p.capacity) return;
	} else if (!scatter_box_meets(p.rules, b.minc, b.maxc)) {
		if (tid == 0) {
			ScatterTotal t = {};
			p.totals[e] = t;
		}
		return;
	}
	const u32 nTri = b.rec.iCount / 3u, blockId = b.id;
	const PolyVertex* v = p.verts + b.rec.vOff;
	const u32* ix = p.idx + b.rec.iOff;
	const u32 hb = scatter_block_hash(p.rules.seed, p.level, b.rec.coordId);
	if (tid == 0) triSum = 0;
	unsigned long long candidates = 0, keptWave = 0; // uniform in the workgroup / in the wave
	u32 triLane = 0, written = 0, batch = 0;         // written: uniform in the workgroup
	for (u32 base = 0; base < nTri; base += WG) {
		u32 cnt = 0;
		const u32 t = base + tid;
		if (t < nTri) {
			const ScatterVertex a = scatter_vertex(&v[ix[3 * t]], false, true);
			if (scatter_mask_passes(p.rules, a.tex0, a.tex1)) {
				++triLane;
				const ScatterVertex b1 = scatter_vertex(&v[ix[3 * t + 1]], false, false), c1 = scatter_vertex(&v[ix[3 * t + 2]], false, false);
				cnt = scatter_count(a.p, b1.p, c1.p, p.rules.density, scatter_tri_hash(hb, t));
			}
		}
		const u32 incl = wave_inclusive_scan(cnt);
		if (lane == 63) waveTot[wave] = incl;
		__syncthreads();
		u32 before = 0, chunkTotal = 0; // (256 x 65535 fits)
		for (u32 w = 0; w < WG / 64; ++w) { const u32 s = waveTot[w]; before += w < wave ? s : 0u; chunkTotal += s; }
		scan[tid] = before + incl;
		__syncthreads();
		candidates += chunkTotal;
		for (u32 s0 = 0; s0 < chunkTotal; s0 += WG) {
			const u32 s = s0 + tid;
			bool kept = false;
			ScatterSample smp;
			u32 tri = 0, tex0 = 0, tex1 = 0;
			if (s < chunkTotal) {
				u32 i = 0; // triangles of the chunk whose candidates end at or before slot s: the slot's triangle
				for (u32 step = WG / 2; step; step >>= 1) i += scan[i + step - 1] <= s ? step : 0u;
				tri = base + i;
				const u32 k = s - (i ? scan[i - 1] : 0u);
				const ScatterVertex a = scatter_vertex(&v[ix[3 * tri]], true, true), b1 = scatter_vertex(&v[ix[3 * tri + 1]], true, true);
				const ScatterVertex c1 = scatter_vertex(&v[ix[3 * tri + 2]], true, true);
				smp = scatter_sample(a, b1, c1, scatter_tri_hash(hb, tri), k);
				kept = scatter_keeps(p.rules, smp);
				tex0 = a.tex0; tex1 = a.tex1;
			}
			const unsigned long long ballot = __ballot(kept);
			const u32 inWave = (u32)__popcll(ballot);
			if (!WRITE) {
				keptWave += inWave;
			} else {
				if (lane == 0) keptTot[batch & 1u][wave] = inWave;
				__syncthreads(); // (one barrier per batch: the batch after the next reuses this half, behind the next one's barrier)
				u32 wavesBefore = 0, total = 0;
				for (u32 w = 0; w < WG / 64; ++w) { const u32 q = keptTot[batch & 1u][w]; wavesBefore += w < wave ? q : 0u; total += q; }
				const u32 at = first + written + wavesBefore + (u32)__popcll(ballot & ((1ull << lane) - 1ull));
				if (kept && at < p.capacity) {
					uint4* o = p.points + 3 * (size_t)at;
					o[0] = make_uint4(scatter_word(smp.pos.x), scatter_word(smp.pos.y), scatter_word(smp.pos.z), scatter_word(smp.rand));
					o[1] = make_uint4(scatter_word(smp.nrm.x), scatter_word(smp.nrm.y), scatter_word(smp.nrm.z), e);
					o[2] = make_uint4(blockId, tri, tex0, tex1);
				}
				written += total;
				++batch;
				if (first + written >= p.capacity) return; // (uniform: every later point lies beyond the capacity)
			}
		}
		__syncthreads(); // the scan is rewritten by the next chunk
	}
	if (!WRITE) {
		for (int o = 32; o > 0; o >>= 1) triLane += __shfl_xor(triLane, o, 64);
		if (lane == 0) { keptSum[wave] = keptWave; atomicAdd(&triSum, triLane); }
		__syncthreads();
		if (tid == 0) {
			ScatterTotal t = {};
			for (u32 w = 0; w < WG / 64; ++w) t.kept += keptSum[w];
			t.candidates = candidates;
			t.triangles = triSum;
			t.visited = 1;
			p.totals[e] = t;
		}
	}
}

__global__ __launch_bounds__(WG) void k_scatter_count(ScatterParams p) { scatter_entry<false>(p); }
__global__ __launch_bounds__(WG) void k_scatter_write(ScatterParams p) { scatter_entry<true>(p); }

// one workgroup: the first point of every entry (exclusive scan of the kept counts), the counts, the ranges
__global__ __launch_bounds__(LOD_SCAN_WG) void k_scatter_scan(ScatterParams p)
{
	__shared__ unsigned long long waveTot[LOD_SCAN_WG / 64];
	__shared__ unsigned long long running, candSum;
	__shared__ u32 triSum, visitedSum;
	const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u32 count = scatter_entries(p);
	if (tid == 0) { running = candSum = 0; triSum = visitedSum = 0; }
	__syncthreads();
	unsigned long long cand = 0;
	u32 tri = 0, visited = 0;
	for (u32 base = 0; base < count; base += LOD_SCAN_WG) {
		const u32 k = base + tid;
		unsigned long long kept = 0;
		if (k < count) {
			const ScatterTotal& t = p.totals[k];
			kept = t.kept; cand += t.candidates; tri += t.triangles; visited += t.visited;
		}
		const unsigned long long incl = scatter_wave_scan64(kept);
		if (lane == 63) waveTot[wave] = incl;
		__syncthreads();
		unsigned long long before = 0, sum = 0;
		for (u32 w = 0; w < LOD_SCAN_WG / 64; ++w) { const unsigned long long q = waveTot[w]; before += w < wave ? q : 0ull; sum += q; }
		if (k < count) p.totals[k].first = (u32)(running + before + incl - kept);
		__syncthreads();
		if (tid == 0) running += sum;
		__syncthreads();
	}
	for (int o = 32; o > 0; o >>= 1) { cand += __shfl_xor(cand, o, 64); tri += __shfl_xor(tri, o, 64); visited += __shfl_xor(visited, o, 64); }
	if (lane == 0) { atomicAdd(&candSum, cand); atomicAdd(&triSum, tri); atomicAdd(&visitedSum, visited); }
	__syncthreads();
	const unsigned long long points = running;
	if (tid == 0) {
		vx_scatter_counts* o = p.counts;
		o->points = points;
		o->candidates = candSum;
		o->triangles = triSum;
		o->entries = count;
		o->visited_entries = visitedSum;
		o->reserved = 0;
	}
	if (p.ranges && points <= 0xFFFFFFFFull)
		for (u32 k = tid; k < count; k += LOD_SCAN_WG) p.ranges[k] = make_uint2(p.totals[k].first, (u32)p.totals[k].kept); // (a lane reads back its own stores)
}

struct ScatterState {
	ScatterTotal* totals = nullptr;
	size_t totalsCap = 0;       // bytes
	void* io = nullptr;         // vx_scatter: the output arrays on their way to the host
	size_t ioCap = 0;

	void release(vx_ctx* c)
	{
		c->be.free(totals); c->be.free(io);
	}
};

int scatter_check(vx_ctx* c, uint32_t level, const vx_scatter_params* prm, uint32_t capacity, const void* points, const void* counts, const char* what)
{
	if (!c) return VX_ERR_INVALID;
	const std::string w(what);
	if (!c->haveSurface) return fail(c, VX_ERR_INVALID, w + ": no surface (run vx_polygonize first)");
	if (level >= c->levelsRun) return fail(c, VX_ERR_INVALID, w + ": no such level");
	if (!prm || !counts) return fail(c, VX_ERR_INVALID, w + ": null parameters or counts");
	if (capacity && !points) return fail(c, VX_ERR_INVALID, w + ": null point array with a non-zero capacity");
	if (!(prm->density > 0.f && prm->density <= VX_SCATTER_MAX_DENSITY)) return fail(c, VX_ERR_INVALID, w + ": density must be finite, above 0 and at most VX_SCATTER_MAX_DENSITY");
	bool nan = lod_nan(prm->min_up) || lod_nan(prm->max_up);
	for (int a = 0; a < 3; ++a) nan = nan || lod_nan(prm->box_min[a]) || lod_nan(prm->box_max[a]);
	if (nan) return fail(c, VX_ERR_INVALID, w + ": NaN slope or box");
	if (prm->min_up > prm->max_up) return fail(c, VX_ERR_INVALID, w + ": min_up > max_up");
	for (int a = 0; a < 3; ++a) if (prm->box_min[a] > prm->box_max[a]) return fail(c, VX_ERR_INVALID, w + ": box_min > box_max");
	if (prm->texture_slot > 7u) return fail(c, VX_ERR_INVALID, w + ": texture_slot > 7");
	if (prm->reserved) return fail(c, VX_ERR_INVALID, w + ": reserved must be 0");
	return VX_OK;
}

// the launches of one scattering on the context's stream; allocates only when the per-entry totals do not fit yet
int scatter_launch(vx_ctx* c, uint32_t level, const vx_scatter_params* prm, uint32_t capacity, vx_scatter_point* dPoints,
                   vx_scatter_range* dRanges, vx_scatter_counts* dCounts, const char* what)
{
	ScatterState* s = module_state<ScatterState>(c, MOD_SCATTER);
	const vx_listed_block* tab = nullptr;
	u32 nb = 0;
	const int rc = vx_device_block_table(c, level, &tab, &nb);
	if (rc != VX_OK) return rc;
	size_t entryCap = nb; // (sized for the levels' table capacities: allocated once per grid)
	for (u32 L = 0; L < c->levelsRun; ++L) entryCap = std::max<size_t>(entryCap, c->lv[L].cap);
	if (!dev_grow(c, s->totals, s->totalsCap, entryCap * sizeof(ScatterTotal)))
		return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
	ScatterParams p;
	memset(&p, 0, sizeof(p));
	p.table = (const ListedBlock*)tab;
	p.countDev = c->meshEpoch == c->fullRunEpoch ? (const u32*)c->dHeader + HDR_LISTS + level : nullptr;
	p.count = nb;
	p.level = level;
	p.verts = (const PolyVertex*)c->dVerts;
	p.idx = (const u32*)c->dIdx;
	p.totals = s->totals;
	p.ranges = (uint2*)dRanges;
	p.points = (uint4*)dPoints;
	p.counts = dCounts;
	p.capacity = capacity;
	static_assert(sizeof(ScatterRules) == sizeof(vx_scatter_params), "ScatterRules mirrors vx_scatter_params");
	memcpy(&p.rules, prm, sizeof(p.rules));
	hipStream_t st = c->be.stream;
	bool ok = true;
	if (nb) {
		hipLaunchKernelGGL(k_scatter_count, dim3(nb), dim3(WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_scatter_count launch");
	}
	if (ok) {
		hipLaunchKernelGGL(k_scatter_scan, dim3(1), dim3(LOD_SCAN_WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_scatter_scan launch");
	}
	if (ok && nb && capacity) {
		hipLaunchKernelGGL(k_scatter_write, dim3(nb), dim3(WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_scatter_write launch");
	}
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, std::string(what) + ": " + c->be.error());
}

} // namespace

extern "C" {

static_assert(sizeof(vx_scatter_params) == 80 && sizeof(vx_scatter_point) == 48 && sizeof(vx_scatter_range) == 8 && sizeof(vx_scatter_counts) == 32,
              "vx_scatter_* layout");

int vx_scatter_device(vx_ctx* c, uint32_t level, const vx_scatter_params* prm, uint32_t capacity, vx_scatter_point* d_points,
                      vx_scatter_range* d_ranges, vx_scatter_counts* d_counts)
{
	VX_ENTER(c);
	const int rc = scatter_check(c, level, prm, capacity, d_points, d_counts, "vx_scatter_device");
	if (rc != VX_OK) return rc;
	if ((((uintptr_t)d_points | (uintptr_t)d_counts) & 15u) || ((uintptr_t)d_ranges & 7u))
		return fail(c, VX_ERR_INVALID, "vx_scatter_device: arrays must be 16-byte aligned (ranges: 8)");
	return scatter_launch(c, level, prm, capacity, d_points, d_ranges, d_counts, "vx_scatter_device");
}

int vx_scatter(vx_ctx* c, uint32_t level, const vx_scatter_params* prm, uint32_t capacity, vx_scatter_point* points,
               vx_scatter_range* ranges, vx_scatter_counts* counts)
{
	VX_ENTER(c);
	int rc = scatter_check(c, level, prm, capacity, points, counts, "vx_scatter");
	if (rc != VX_OK) return rc;
	ScatterState* s = module_state<ScatterState>(c, MOD_SCATTER);
	const vx_listed_block* tab = nullptr;
	u32 nb = 0;
	if ((rc = vx_device_block_table(c, level, &tab, &nb)) != VX_OK) return rc;
	const size_t rangeBytes = lod_align16((size_t)nb * sizeof(vx_scatter_range)), pointBytes = (size_t)capacity * sizeof(vx_scatter_point);
	if (!dev_grow(c, s->io, s->ioCap, sizeof(vx_scatter_counts) + rangeBytes + pointBytes))
		return fail(c, VX_ERR_DEVICE, "vx_scatter: allocation failed: " + c->be.error());
	char* io = (char*)s->io;
	vx_scatter_counts* dCounts = (vx_scatter_counts*)io;
	vx_scatter_range* dRanges = (vx_scatter_range*)(io + sizeof(vx_scatter_counts));
	vx_scatter_point* dPoints = (vx_scatter_point*)(io + sizeof(vx_scatter_counts) + rangeBytes);
	if ((rc = scatter_launch(c, level, prm, capacity, dPoints, ranges ? dRanges : nullptr, dCounts, "vx_scatter")) != VX_OK) return rc;
	if (!c->be.d2h(counts, dCounts, sizeof(vx_scatter_counts))) return fail(c, VX_ERR_DEVICE, "vx_scatter: download failed: " + c->be.error());
	const bool fits = counts->points <= 0xFFFFFFFFull;
	const size_t nPoints = fits ? (size_t)std::min<uint64_t>(counts->points, capacity) : 0;
	bool ok = true;
	if (fits && ranges && counts->entries) ok = c->be.d2h(ranges, dRanges, (size_t)counts->entries * sizeof(vx_scatter_range));
	if (ok && nPoints) ok = c->be.d2h(points, dPoints, nPoints * sizeof(vx_scatter_point));
	if (!ok) return fail(c, VX_ERR_DEVICE, "vx_scatter: download failed: " + c->be.error());
	if (counts->points > capacity) return fail(c, VX_ERR_OVERFLOW, "vx_scatter: capacity too small (counts.points says how much is needed)");
	return VX_OK;
}

} // extern "C"
