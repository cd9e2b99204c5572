// vx_lod.inl — LOD selection with frustum culling and indirect draw lists (include/voxels_hip.h, "LOD selection"); included
// by vx_hip.hip after vx_ray.inl (HIP only, like the ray casts: the CPU emulation does not export these entry points).
//
// The least set O of opened nodes (header: rules 1-3) in one fine-to-coarse sweep, one launch per level (k_lod_open).  A node
// X of level L is in O exactly when
//   (a) rule 1 holds for X itself: ranges[L] > 0 and d^2 < ranges[L]^2;
//   (b) a level L-1 node next to X's children is in O: one of the 8 children, or one of the 24 nodes that share a face with
//       a child from outside X.  A node Y in O has leaves of level <= L-2 on every face; the same-level neighbour N of Y
//       must therefore be active, so parent(N) is in O (rule 3), and closure is the case Y = N;
//   (c) a band root B of level L-2 (odd sizes) touches X's children from across the band face: B is active whatever happens
//       to it, so the child next to it must be active too (this is the case (b) misses: B has no parent);
//   (d) X is the one node of level R-1 (no transition meshes), it is a root, and the grid has a band: a band leaf of level
//       <= R-2 then always touches it.
// (a), (c) and (d) are forced outright and (b) only reads level L-1, which is final when level L runs; what the sweep
// yields satisfies rules 2 and 3, so it is the least fixed point (DESIGN.md §13 has the argument at length).
//
// k_lod_leaves counts the leaves of every level (count and volume, one partial sum per workgroup).  Emission is three
// launches over the block tables of all levels, one lane per entry in level order: k_lod_classify keeps the leaves the
// frustum does not cull and counts their records and commands per workgroup, k_lod_scan (one workgroup) turns the counts
// into workgroup offsets and writes vx_lod_counts, k_lod_write writes records and commands at workgroup offset + lane scan.
// The order is the tables' order, with no atomics on it.
#include "tv_lod.h"

namespace {

enum { LOD_SCAN_WG = 1024 };

struct LodParams {
	u8* open[MAX_LEVELS];       // per level >= 1: cnt^3 flags, 1 = node opened (split); level 0 has none
	u32 cnt[MAX_LEVELS];        // nodes per axis
	u32 T, R, c0;               // coarsest level of the run, the reference's level count, level-0 blocks per axis
	float cam[3];
	float ranges[MAX_LEVELS];
};

__device__ __forceinline__ bool lod_open_at(const LodParams& p, u32 L, int x, int y, int z)
{
	const int n = (int)p.cnt[L];
	if (L == 0 || x < 0 || y < 0 || z < 0 || x >= n || y >= n || z >= n) return false;
	return p.open[L][((u32)z * (u32)n + (u32)y) * (u32)n + (u32)x] != 0;
}

// a node without a parent: the run's coarsest level, or a band node of odd sizes (c >> 1 beyond the next level on some axis)
__device__ __forceinline__ bool lod_is_root(const LodParams& p, u32 L, const u32 c[3])
{
	if (L >= p.T) return true;
	const u32 m = p.cnt[L + 1];
	return (c[0] >> 1) >= m || (c[1] >> 1) >= m || (c[2] >> 1) >= m;
}

__device__ __forceinline__ bool lod_is_leaf(const LodParams& p, u32 L, const u32 c[3])
{
	if (lod_open_at(p, L, (int)c[0], (int)c[1], (int)c[2])) return false;
	return lod_is_root(p, L, c) || lod_open_at(p, L + 1, (int)(c[0] >> 1), (int)(c[1] >> 1), (int)(c[2] >> 1));
}

__global__ __launch_bounds__(WG) void k_lod_open(LodParams p, u32 L)
{
	const u32 n = p.cnt[L], i = blockIdx.x * WG + threadIdx.x;
	if (i >= n * n * n) return;
	const u32 c[3] = { i % n, (i / n) % n, i / (n * n) };
	float mn[3], mx[3];
	lod_box(c, L, mn, mx);
	const float r = p.ranges[L];
	bool open = r > 0.f && lod_dist2(mn, mx, p.cam) < r * r;                                     // (a)
	if (L + 1 == p.R && L == p.T && (p.c0 & (p.c0 - 1u))) open = true;                          // (d)
	if (L >= 2) {
		if ((p.cnt[L - 2] & 1u) && !(p.cnt[L - 1] & 1u) && (c[0] == n - 1 || c[1] == n - 1 || c[2] == n - 1)) open = true; // (c)
		const int b[3] = { 2 * (int)c[0], 2 * (int)c[1], 2 * (int)c[2] };
		for (int k = 0; k < 8 && !open; ++k) open = lod_open_at(p, L - 1, b[0] + (k & 1), b[1] + ((k >> 1) & 1), b[2] + (k >> 2)); // (b)
		for (int a = 0; a < 3 && !open; ++a) {
			const int u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2;
			for (int k = 0; k < 8 && !open; ++k) {
				int q[3];
				q[a] = b[a] + ((k & 4) ? 2 : -1);
				q[u] = b[u] + (k & 1);
				q[v] = b[v] + ((k >> 1) & 1);
				open = lod_open_at(p, L - 1, q[0], q[1], q[2]);
			}
		}
	}
	p.open[L][i] = open ? 1 : 0;
}

struct LodLeafParams {
	LodParams s;
	u32 base[MAX_LEVELS + 1];   // first flattened node of each level (levels 0..T)
	unsigned long long* partials; // per workgroup: leaves, leaf volume in level-0 blocks
};

__global__ __launch_bounds__(WG) void k_lod_leaves(LodLeafParams p)
{
	__shared__ unsigned long long sum[2][WG / 64];
	const u32 i = blockIdx.x * WG + threadIdx.x;
	bool leaf = false;
	u32 L = 0;
	if (i < p.base[p.s.T + 1]) {
		while (i >= p.base[L + 1]) ++L;
		const u32 n = p.s.cnt[L], j = i - p.base[L];
		const u32 c[3] = { j % n, (j / n) % n, j / (n * n) };
		leaf = lod_is_leaf(p.s, L, c);
	}
	unsigned long long cnt = leaf ? 1ull : 0ull, vol = leaf ? 1ull << (3 * L) : 0ull;
	for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o, 64); vol += __shfl_xor(vol, o, 64); }
	if ((threadIdx.x & 63) == 0) { sum[0][threadIdx.x >> 6] = cnt; sum[1][threadIdx.x >> 6] = vol; }
	__syncthreads();
	if (threadIdx.x == 0) {
		unsigned long long a = 0, b = 0;
		for (int w = 0; w < WG / 64; ++w) { a += sum[0][w]; b += sum[1][w]; }
		p.partials[2 * blockIdx.x] = a;
		p.partials[2 * blockIdx.x + 1] = b;
	}
}

struct LodEmitParams {
	LodParams s;
	const ListedBlock* table[MAX_LEVELS];
	const u32* countDev[MAX_LEVELS]; // the tables' counts in the run's device header (after a full run), or null
	u32 count[MAX_LEVELS];           // the counts the host knows
	u32 base[MAX_LEVELS + 1];        // first flattened entry of each level (host counts); base[T + 1] = lanes of the launch
	u32 nPlanes;
	float planes[6][4];
	u32* words;                      // per flattened entry: bit 0 drawn, bits 1-6 transitions, bits 8-10 transition commands
	uint4* wgTotals;                 // per workgroup of k_lod_classify: records, transition commands, meshed leaves, culled leaves
	uint2* wgPrefix;                 // per workgroup: records and transition commands of the workgroups before it
	u32 nWg;
	const unsigned long long* partials; // k_lod_leaves: per workgroup leaves, leaf volume
	u32 nPartials;
	u32 drawCap, trCap;
	uint4* draws;                    // vx_lod_draw: two uint4 each
	u32* regular;                    // vx_draw_indexed: five u32 each
	u32* transition;
	vx_lod_counts* counts;
};

__device__ __forceinline__ void lod_put_command(u32* out, u32 k, u32 count, u32 first, u32 vertexOffset, u32 record)
{
	u32* o = out + 5 * (size_t)k;
	o[0] = count; o[1] = 1u; o[2] = first; o[3] = vertexOffset; o[4] = record;
}

// level and table entry of flattened lane i; false past the end of its level's table (after a full run the device count
// may be below the host's launch width)
__device__ __forceinline__ bool lod_entry(const LodEmitParams& p, u32 i, u32& L, u32& e)
{
	if (i >= p.base[p.s.T + 1]) return false;
	L = 0;
	while (i >= p.base[L + 1]) ++L;
	e = i - p.base[L];
	const u32 count = p.countDev[L] ? min(*p.countDev[L], p.count[L]) : p.count[L];
	return e < count;
}

// (records, transition commands) of one entry packed in a word: a 256-lane workgroup has at most 256 and 1536
__device__ __forceinline__ u32 lod_packed(u32 word) { return ((word & 1u) << 16) | ((word >> 8) & 7u); }

// WG-lane exclusive scan of v; `total` = the workgroup's sum (all lanes must call)
__device__ __forceinline__ u32 lod_wg_scan(u32 v, u32& total)
{
	__shared__ u32 waveTot[WG / 64];
	const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const u32 incl = wave_inclusive_scan(v);
	if (lane == 63) waveTot[wave] = incl;
	__syncthreads();
	u32 before = 0;
	total = 0;
	for (u32 w = 0; w < WG / 64; ++w) { const u32 t = waveTot[w]; before += w < wave ? t : 0u; total += t; }
	return before + incl - v;
}

// one lane per table entry of all levels: leaf or not, culled or not, its transition faces and commands
__global__ __launch_bounds__(WG) void k_lod_classify(LodEmitParams p)
{
	__shared__ u32 meshedSum, culledSum;
	const u32 i = blockIdx.x * WG + threadIdx.x;
	if (threadIdx.x == 0) meshedSum = culledSum = 0;
	__syncthreads();
	u32 L, e, word = 0;
	bool meshed = false, culled = false;
	if (lod_entry(p, i, L, e)) {
		const ListedBlock& b = p.table[L][e];
		const u32 n = p.s.cnt[L], coord = b.rec.coordId;
		const u32 c[3] = { coord % n, (coord / n) % n, coord / (n * n) };
		if (coord < n * n * n && lod_is_leaf(p.s, L, c)) {
			meshed = true;
			float mn[3], mx[3];
			lod_box(c, L, mn, mx);
			for (u32 k = 0; k < p.nPlanes; ++k) culled = culled || lod_outside(mn, mx, p.planes[k]);
			if (!culled) {
				u32 bits = 0, nTr = 0;
				for (int f = 0; f < 6; ++f) {
					const int a = lod_face_axis(f);
					int q[3] = { (int)c[0], (int)c[1], (int)c[2] };
					q[a] += lod_face_dir(f);
					// beyond the level's extent on the + side lie band roots of finer levels (odd sizes)
					const bool finer = q[a] >= (int)n ? (n << L) < p.s.c0 : lod_open_at(p.s, L, q[0], q[1], q[2]);
					if (finer) {
						bits |= 1u << f;
						nTr += b.rec.tiCount[f] ? 1u : 0u;
					}
				}
				word = 1u | (bits << 1) | (nTr << 8);
			}
		}
	}
	if (i < p.base[p.s.T + 1]) p.words[i] = word;
	u32 total;
	(void)lod_wg_scan(lod_packed(word), total);
	if (meshed) atomicAdd(&meshedSum, 1u);
	if (culled) atomicAdd(&culledSum, 1u);
	__syncthreads();
	if (threadIdx.x == 0) p.wgTotals[blockIdx.x] = make_uint4(total >> 16, total & 0xFFFFu, meshedSum, culledSum);
}

// one workgroup: workgroup offsets (exclusive scan of the classify totals) and the counts
__global__ __launch_bounds__(LOD_SCAN_WG) void k_lod_scan(LodEmitParams p)
{
	__shared__ u32 waveTot[2][LOD_SCAN_WG / 64];
	__shared__ u32 running[2], sums[2];
	__shared__ unsigned long long leafSum[2];
	const u32 tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid == 0) { running[0] = running[1] = sums[0] = sums[1] = 0; leafSum[0] = leafSum[1] = 0; }
	__syncthreads();
	{
		unsigned long long a = 0, b = 0;
		for (u32 k = tid; k < p.nPartials; k += LOD_SCAN_WG) { a += p.partials[2 * k]; b += p.partials[2 * k + 1]; }
		for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
		if (lane == 0) { atomicAdd(&leafSum[0], a); atomicAdd(&leafSum[1], b); } // (one atomic per wave: 1024 on one LDS word serialise)
	}
	u32 meshed = 0, culled = 0;
	for (u32 base = 0; base < p.nWg; base += LOD_SCAN_WG) {
		const u32 k = base + tid;
		const uint4 t = k < p.nWg ? p.wgTotals[k] : make_uint4(0u, 0u, 0u, 0u);
		meshed += t.z;
		culled += t.w;
		const u32 inclR = wave_inclusive_scan(t.x), inclT = wave_inclusive_scan(t.y);
		if (lane == 63) { waveTot[0][wave] = inclR; waveTot[1][wave] = inclT; }
		__syncthreads();
		u32 bR = 0, bT = 0, sR = 0, sT = 0;
		for (u32 w = 0; w < LOD_SCAN_WG / 64; ++w) {
			const u32 r = waveTot[0][w], q = waveTot[1][w];
			bR += w < wave ? r : 0u; bT += w < wave ? q : 0u; sR += r; sT += q;
		}
		if (k < p.nWg) p.wgPrefix[k] = make_uint2(running[0] + bR + inclR - t.x, running[1] + bT + inclT - t.y);
		__syncthreads();
		if (tid == 0) { running[0] += sR; running[1] += sT; }
		__syncthreads();
	}
	for (int o = 32; o > 0; o >>= 1) { meshed += __shfl_xor(meshed, o, 64); culled += __shfl_xor(culled, o, 64); }
	if (lane == 0) { atomicAdd(&sums[0], meshed); atomicAdd(&sums[1], culled); }
	__syncthreads();
	if (tid == 0) {
		vx_lod_counts* o = p.counts;
		o->records = running[0];
		o->regular = running[0];
		o->transition = running[1];
		o->leaves = (uint32_t)leafSum[0];
		o->meshed_leaves = sums[0];
		o->culled_leaves = sums[1];
		o->leaf_volume = leafSum[1];
	}
}

// one lane per table entry again: the record and commands of a drawn entry at its offsets (workgroup prefix + lane scan)
__global__ __launch_bounds__(WG) void k_lod_write(LodEmitParams p)
{
	const u32 i = blockIdx.x * WG + threadIdx.x;
	const u32 word = i < p.base[p.s.T + 1] ? p.words[i] : 0u;
	u32 total;
	const u32 excl = lod_wg_scan(lod_packed(word), total);
	if (!(word & 1u)) return;
	u32 L, e;
	if (!lod_entry(p, i, L, e)) return;
	const ListedBlock& b = p.table[L][e];
	const uint2 pre = p.wgPrefix[blockIdx.x];
	const u32 rec = pre.x + (excl >> 16), bits = (word >> 1) & 63u;
	if (rec < p.drawCap) {
		p.draws[2 * (size_t)rec] = make_uint4(L, e, b.id, b.rec.coordId);
		p.draws[2 * (size_t)rec + 1] = make_uint4(bits, lod_adjacency(bits), 0u, 0u);
		lod_put_command(p.regular, rec, b.rec.iCount, b.rec.iOff, b.rec.vOff, rec);
	}
	u32 t = pre.y + (excl & 0xFFFFu);
	for (int f = 0; f < 6; ++f) {
		if (!(bits & (1u << f)) || !b.rec.tiCount[f]) continue;
		if (t < p.trCap) lod_put_command(p.transition, t, b.rec.tiCount[f], b.rec.tiOff[f], b.rec.tvOff[f], rec);
		++t;
	}
}

struct LodState {
	u8* open = nullptr;
	size_t openCap = 0;         // bytes
	unsigned long long* partials = nullptr;
	size_t partialsCap = 0;     // bytes
	u32* words = nullptr;       // k_lod_classify -> k_lod_write, one word per table entry
	size_t wordsCap = 0;        // bytes
	void* wgSums = nullptr;     // per classify workgroup: totals (uint4), then offsets (uint2)
	size_t wgSumsCap = 0;       // bytes
	void* io = nullptr;         // vx_lod_select: the output arrays on their way to the host
	size_t ioCap = 0;

	void release(vx_ctx* c)
	{
		c->be.free(open); c->be.free(partials); c->be.free(words); c->be.free(wgSums); c->be.free(io);
	}
};

bool lod_nan(float v) { return v != v; }

int lod_check(vx_ctx* c, const vx_lod_params* prm, uint32_t drawCap, uint32_t trCap, const void* draws, const void* regular,
              const void* transition, const void* counts, const char* what)
{
	if (!c) return VX_ERR_INVALID;
	const std::string w(what);
	if (!c->haveSurface) return fail(c, VX_ERR_INVALID, w + ": no surface (run vx_polygonize first)");
	if (c->firstMeshedLevel) return fail(c, VX_ERR_INVALID, w + ": the last run left levels unmeshed (vx_polygonize_from)");
	if (!prm || !counts) return fail(c, VX_ERR_INVALID, w + ": null parameters or counts");
	if (prm->n_planes > 6) return fail(c, VX_ERR_INVALID, w + ": more than 6 planes");
	bool nan = lod_nan(prm->camera[0]) || lod_nan(prm->camera[1]) || lod_nan(prm->camera[2]);
	for (u32 k = 0; k < prm->n_planes; ++k) for (int j = 0; j < 4; ++j) nan = nan || lod_nan(prm->planes[k][j]);
	for (int L = 1; L < 16; ++L) nan = nan || lod_nan(prm->ranges[L]);
	if (nan) return fail(c, VX_ERR_INVALID, w + ": NaN camera, plane or range");
	if ((drawCap && (!draws || !regular)) || (trCap && !transition)) return fail(c, VX_ERR_INVALID, w + ": null array with a non-zero capacity");
	return VX_OK;
}

// the launches of one selection on the context's stream; allocates only when the flags or partial sums do not fit yet
int lod_launch(vx_ctx* c, const vx_lod_params* prm, uint32_t drawCap, uint32_t trCap, vx_lod_draw* dDraws,
               vx_draw_indexed* dRegular, vx_draw_indexed* dTransition, vx_lod_counts* dCounts, const char* what)
{
	LodState* s = module_state<LodState>(c, MOD_LOD);
	const u32 T = c->levelsRun - 1;
	LodEmitParams e;
	memset(&e, 0, sizeof(e));
	LodParams& p = e.s;
	LodLeafParams lp;
	memset(&lp, 0, sizeof(lp));
	size_t flagBytes = 0, nodes = 0;
	u32 flagOff[MAX_LEVELS] = {};
	for (u32 L = 0; L <= T; ++L) {
		const u32 n = c->lv[L].cnt;
		const size_t cube = (size_t)n * n * n;
		p.cnt[L] = n;
		lp.base[L] = (u32)nodes;
		nodes += cube;
		if (L) { flagOff[L] = (u32)flagBytes; flagBytes += cube; }
	}
	lp.base[T + 1] = (u32)nodes;
	const u32 wgs = (u32)((nodes + WG - 1) / WG);
	if (!dev_grow(c, s->open, s->openCap, flagBytes) || !dev_grow(c, s->partials, s->partialsCap, (size_t)wgs * 16))
		return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
	for (u32 L = 1; L <= T; ++L) p.open[L] = s->open + flagOff[L];
	p.T = T;
	p.R = c->refLevels;
	p.c0 = c->n >> 4;
	for (int a = 0; a < 3; ++a) p.cam[a] = prm->camera[a];
	for (u32 L = 0; L < MAX_LEVELS; ++L) p.ranges[L] = L ? prm->ranges[L] : 0.f;
	for (u32 L = 0; L <= T; ++L) {
		const vx_listed_block* tab = nullptr;
		u32 nb = 0;
		const int rc = vx_device_block_table(c, L, &tab, &nb);
		if (rc != VX_OK) return rc;
		e.table[L] = (const ListedBlock*)tab;
		e.count[L] = nb;
		e.countDev[L] = c->meshEpoch == c->fullRunEpoch ? (const u32*)c->dHeader + HDR_LISTS + L : nullptr;
	}
	u32 width = 0;
	size_t entryCap = 0;      // (sized for the levels' table capacities: the buffers are allocated once per grid)
	for (u32 L = 0; L <= T; ++L) { e.base[L] = width; width += e.count[L]; entryCap += std::max<size_t>(c->lv[L].cap, e.count[L]); }
	e.base[T + 1] = width;
	const u32 nWg = (width + WG - 1) / WG;
	const size_t wgCap = (entryCap + WG - 1) / WG + 1;
	if (!dev_grow(c, s->words, s->wordsCap, entryCap * 4) || !dev_grow(c, s->wgSums, s->wgSumsCap, wgCap * 24))
		return fail(c, VX_ERR_DEVICE, std::string(what) + ": allocation failed: " + c->be.error());
	e.words = s->words;
	e.wgTotals = (uint4*)s->wgSums;
	e.wgPrefix = (uint2*)((char*)s->wgSums + wgCap * 16);
	e.nWg = nWg;
	lp.s = p;
	lp.partials = s->partials;
	e.partials = s->partials;
	e.nPartials = wgs;
	e.nPlanes = prm->n_planes;
	for (u32 k = 0; k < prm->n_planes; ++k) for (int j = 0; j < 4; ++j) e.planes[k][j] = prm->planes[k][j];
	e.drawCap = drawCap;
	e.trCap = trCap;
	e.draws = (uint4*)dDraws;
	e.regular = (u32*)dRegular;
	e.transition = (u32*)dTransition;
	e.counts = dCounts;
	hipStream_t st = c->be.stream;
	bool ok = true;
	for (u32 L = 1; L <= T && ok; ++L) {
		const u32 cube = p.cnt[L] * p.cnt[L] * p.cnt[L];
		hipLaunchKernelGGL(k_lod_open, dim3((cube + WG - 1) / WG), dim3(WG), 0, st, p, L);
		ok = c->be.check(hipGetLastError(), "k_lod_open launch");
	}
	if (ok) {
		hipLaunchKernelGGL(k_lod_leaves, dim3(wgs), dim3(WG), 0, st, lp);
		ok = c->be.check(hipGetLastError(), "k_lod_leaves launch");
	}
	if (ok && nWg) {
		hipLaunchKernelGGL(k_lod_classify, dim3(nWg), dim3(WG), 0, st, e);
		ok = c->be.check(hipGetLastError(), "k_lod_classify launch");
	}
	if (ok) {
		hipLaunchKernelGGL(k_lod_scan, dim3(1), dim3(LOD_SCAN_WG), 0, st, e);
		ok = c->be.check(hipGetLastError(), "k_lod_scan launch");
	}
	if (ok && nWg) {
		hipLaunchKernelGGL(k_lod_write, dim3(nWg), dim3(WG), 0, st, e);
		ok = c->be.check(hipGetLastError(), "k_lod_write launch");
	}
	return ok ? VX_OK : fail(c, VX_ERR_DEVICE, std::string(what) + ": " + c->be.error());
}

size_t lod_align16(size_t v) { return (v + 15) & ~(size_t)15; }

} // namespace

extern "C" {

static_assert(sizeof(vx_lod_params) == 176 && sizeof(vx_lod_draw) == 32 && sizeof(vx_draw_indexed) == 20 && sizeof(vx_lod_counts) == 32,
              "vx_lod_* layout");

int vx_lod_select_device(vx_ctx* c, const vx_lod_params* prm, uint32_t draw_capacity, uint32_t transition_capacity,
                         vx_lod_draw* d_draws, vx_draw_indexed* d_regular, vx_draw_indexed* d_transition, vx_lod_counts* d_counts)
{
	VX_ENTER(c);
	int rc = lod_check(c, prm, draw_capacity, transition_capacity, d_draws, d_regular, d_transition, d_counts, "vx_lod_select_device");
	if (rc != VX_OK) return rc;
	if (((uintptr_t)d_draws | (uintptr_t)d_regular | (uintptr_t)d_transition | (uintptr_t)d_counts) & 15u)
		return fail(c, VX_ERR_INVALID, "vx_lod_select_device: arrays must be 16-byte aligned");
	return lod_launch(c, prm, draw_capacity, transition_capacity, d_draws, d_regular, d_transition, d_counts, "vx_lod_select_device");
}

int vx_lod_select(vx_ctx* c, const vx_lod_params* prm, uint32_t draw_capacity, uint32_t transition_capacity,
                  vx_lod_draw* draws, vx_draw_indexed* regular, vx_draw_indexed* transition, vx_lod_counts* counts)
{
	VX_ENTER(c);
	int rc = lod_check(c, prm, draw_capacity, transition_capacity, draws, regular, transition, counts, "vx_lod_select");
	if (rc != VX_OK) return rc;
	LodState* s = module_state<LodState>(c, MOD_LOD);
	const size_t drawBytes = (size_t)draw_capacity * sizeof(vx_lod_draw), regBytes = lod_align16((size_t)draw_capacity * sizeof(vx_draw_indexed));
	const size_t trBytes = lod_align16((size_t)transition_capacity * sizeof(vx_draw_indexed));
	if (!dev_grow(c, s->io, s->ioCap, sizeof(vx_lod_counts) + drawBytes + regBytes + trBytes))
		return fail(c, VX_ERR_DEVICE, "vx_lod_select: allocation failed: " + c->be.error());
	char* io = (char*)s->io;
	vx_lod_counts* dCounts = (vx_lod_counts*)io;
	vx_lod_draw* dDraws = (vx_lod_draw*)(io + sizeof(vx_lod_counts));
	vx_draw_indexed* dRegular = (vx_draw_indexed*)(io + sizeof(vx_lod_counts) + drawBytes);
	vx_draw_indexed* dTransition = (vx_draw_indexed*)(io + sizeof(vx_lod_counts) + drawBytes + regBytes);
	if ((rc = lod_launch(c, prm, draw_capacity, transition_capacity, dDraws, dRegular, dTransition, dCounts, "vx_lod_select")) != VX_OK) return rc;
	if (!c->be.d2h(counts, dCounts, sizeof(vx_lod_counts))) return fail(c, VX_ERR_DEVICE, "vx_lod_select: download failed: " + c->be.error());
	const u32 nRec = std::min(counts->records, draw_capacity), nTr = std::min(counts->transition, transition_capacity);
	bool ok = true;
	if (nRec) ok = c->be.d2h(draws, dDraws, (size_t)nRec * sizeof(vx_lod_draw)) && c->be.d2h(regular, dRegular, (size_t)nRec * sizeof(vx_draw_indexed));
	if (ok && nTr) ok = c->be.d2h(transition, dTransition, (size_t)nTr * sizeof(vx_draw_indexed));
	if (!ok) return fail(c, VX_ERR_DEVICE, "vx_lod_select: download failed: " + c->be.error());
	if (counts->records > draw_capacity || counts->transition > transition_capacity)
		return fail(c, VX_ERR_OVERFLOW, "vx_lod_select: capacity too small (the counts say how much is needed)");
	return VX_OK;
}

} // extern "C"
