// vx_ray.inl — ray casts against the regular meshes of one LOD level (include/voxels_hip.h, "ray casts"); included by
// vx_hip.hip after vx_host.inl (HIP only: the CPU emulation of the tests compiles vx_host.inl without this file and does not
// export these entry points).
//
// The index of a level, built on demand (k_ray_index, one workgroup per entry of the level's block table):
//   map     u32 per block of the level: block coordinate id -> table entry, RAY_NONE = no mesh
//   starts  65 u16 per entry: bucket starts over the 4 x 4 x 4 sub-bricks of the block, starts[64] = its triangle count
//   perm    u16 per triangle: the block's triangle ordinals in bucket order (counting sort in LDS), a triangle in the bucket
//           of the sub-brick that holds its centroid.  Indexed by the triangle's place in the index pool (iOff / 3 + k), so
//           the levels share one array: their ranges of the pool are disjoint.
// The traversal (k_raycast, one lane per ray) relies on every triangle lying inside the closed box of the cell that made it,
// hence inside its bucket's sub-brick; the build counts the triangles for which that fails (`straddling`, must be 0).
#include "tv_ray.h"

namespace {

struct RayIndexParams {
	const ListedBlock* table;
	const u32* countDev;        // the table's count in the run's device header (after a full run), or null
	u32 count;                  // the count the host knows (launch width)
	const PolyVertex* verts;
	const u32* idx;
	u32* map;
	u16* starts;
	u16* perm;
	unsigned long long* stats;  // [0] triangles, [1] straddling triangles
	u32 cnt;                    // blocks per axis of the level
	float size;                 // block edge in voxels
};

// bucket of triangle k of a block; `outside` counts it when a vertex lies outside the bucket's box (+-1/256)
__device__ __forceinline__ u32 ray_tri_bucket(const PolyVertex* v, const u32* ix, const float org[3], float sub, u32& outside)
{
	float P[3][3];
	for (int j = 0; j < 3; ++j) {
		const float4 q = *(const float4*)&v[ix[j]];
		P[j][0] = q.x; P[j][1] = q.y; P[j][2] = q.z;
	}
	int s[3];
	bool in = true;
	for (int a = 0; a < 3; ++a) {
		s[a] = ray_sub_of((P[0][a] + P[1][a] + P[2][a]) / 3.f, org[a], sub);
		const float lo = org[a] + (float)s[a] * sub - (1.f / 256.f), hi = org[a] + (float)(s[a] + 1) * sub + (1.f / 256.f);
		for (int j = 0; j < 3; ++j) in = in && P[j][a] >= lo && P[j][a] <= hi;
	}
	outside += in ? 0u : 1u;
	return ray_bucket(s);
}

__global__ __launch_bounds__(WG) void k_ray_index(RayIndexParams p)
{
	__shared__ u32 hist[RAY_BUCKETS], cursor[RAY_BUCKETS];
	const u32 e = blockIdx.x, tid = threadIdx.x;
	const u32 count = p.countDev ? min(*p.countDev, p.count) : p.count;
	if (e >= count) return;
	const ListedBlock& b = p.table[e];
	const u32 coord = b.rec.coordId, iOff = b.rec.iOff, nTri = b.rec.iCount / 3;
	const PolyVertex* v = p.verts + b.rec.vOff;
	const u32* ix = p.idx + iOff;
	if (tid < RAY_BUCKETS) hist[tid] = 0;
	if (tid == 0 && coord < p.cnt * p.cnt * p.cnt) p.map[coord] = e;
	__syncthreads();
	float org[3];
	ray_block_origin(coord, p.cnt, p.size, org);
	const float sub = p.size / (float)RAY_SUB;
	u32 outside = 0;
	for (u32 k = tid; k < nTri; k += WG) atomicAdd(&hist[ray_tri_bucket(v, ix + 3 * k, org, sub, outside)], 1u);
	__syncthreads();
	u16* starts = p.starts + (size_t)e * (RAY_BUCKETS + 1);
	if (tid == 0) {
		u32 sum = 0;
		for (u32 i = 0; i < RAY_BUCKETS; ++i) { starts[i] = (u16)sum; cursor[i] = sum; sum += hist[i]; }
		starts[RAY_BUCKETS] = (u16)sum;
		atomicAdd(&p.stats[0], (unsigned long long)nTri);
	}
	__syncthreads();
	u16* perm = p.perm + iOff / 3;
	u32 ignored = 0;
	for (u32 k = tid; k < nTri; k += WG) perm[atomicAdd(&cursor[ray_tri_bucket(v, ix + 3 * k, org, sub, ignored)], 1u)] = (u16)k;
	if (outside) atomicAdd(&p.stats[1], (unsigned long long)outside);
}

struct RayCastParams {
	const float4* rays;   // vx_ray: two float4 each
	float4* hits;         // vx_ray_hit: three float4 each
	u32 n;
	const ListedBlock* table;
	const u32* map;
	const u16* starts;
	const u16* perm;
	const PolyVertex* verts;
	const u32* idx;
	u32 cnt;
	float size;
};

struct RayBest {
	float t, u, v;
	u32 e, tri;
};

// the triangles of one bucket of table entry e against the ray; the nearest hit in [tLo, tHi] (ties: smallest (e, tri))
__device__ __forceinline__ void ray_test_bucket(const RayCastParams& p, const RayShear& sh, const float o[3], float tLo, float tHi, u32 e, u32 bucket, RayBest& best)
{
	const ListedBlock& b = p.table[e];
	const PolyVertex* v = p.verts + b.rec.vOff;
	const u32* ix = p.idx + b.rec.iOff;
	const u16* perm = p.perm + b.rec.iOff / 3;
	const u16* starts = p.starts + (size_t)e * (RAY_BUCKETS + 1);
	const u32 k1 = starts[bucket + 1];
	for (u32 k = starts[bucket]; k < k1; ++k) {
		const u32 tri = perm[k];
		float P[3][3];
		for (int j = 0; j < 3; ++j) {
			const float4 q = *(const float4*)&v[ix[3 * tri + j]];
			P[j][0] = q.x; P[j][1] = q.y; P[j][2] = q.z;
		}
		float t, u, w;
		if (!ray_triangle(sh, o, P[0], P[1], P[2], t, u, w) || !(t >= tLo && t <= tHi)) continue;
		if (t < best.t || (t == best.t && (e < best.e || (e == best.e && tri < best.tri)))) {
			best.t = t; best.u = u; best.v = w; best.e = e; best.tri = tri;
		}
	}
}

__global__ __launch_bounds__(WG) void k_raycast(RayCastParams p)
{
	const u32 i = blockIdx.x * WG + threadIdx.x;
	if (i >= p.n) return;
	const float4 r0 = p.rays[2 * i], r1 = p.rays[2 * i + 1];
	const float o[3] = { r0.x, r0.y, r0.z }, d[3] = { r1.x, r1.y, r1.z };
	RayBest best = { ray_inf(), 0.f, 0.f, RAY_NONE, RAY_NONE };
	float t0 = r0.w, t1 = r1.w;
	const bool valid = !(o[0] != o[0] || o[1] != o[1] || o[2] != o[2] || d[0] != d[0] || d[1] != d[1] || d[2] != d[2])
	                   && (d[0] != 0.f || d[1] != 0.f || d[2] != 0.f) && t0 <= t1;
	const float inv[3] = { d[0] != 0.f ? 1.f / d[0] : 0.f, d[1] != 0.f ? 1.f / d[1] : 0.f, d[2] != 0.f ? 1.f / d[2] : 0.f };
	const float extent = (float)p.cnt * p.size;
	if (valid && ray_clip_cube(o, d, inv, extent, t0, t1)) {
		const RayShear sh = ray_shear(d);
		const float tLo = r0.w, tHi = r1.w, sub = p.size / (float)RAY_SUB;
		const float eps = extent * 1e-5f; // (rounding of the watertight test at these coordinates is far below this)
		const float zero[3] = { 0.f, 0.f, 0.f };
		RayDda blk;
		blk.init(o, d, inv, t0, zero, p.size, (int)p.cnt);
		float tEnter = t0;
		bool done = false;
		for (;;) {
			const float tBlockExit = fminf(blk.exit_t(), t1);
			const u32 e = p.map[ray_coord_id(blk.cell, p.cnt)];
			if (e != RAY_NONE) {
				const float org[3] = { (float)blk.cell[0] * p.size, (float)blk.cell[1] * p.size, (float)blk.cell[2] * p.size };
				RayDda sb;
				sb.init(o, d, inv, tEnter, org, sub, (int)RAY_SUB);
				float tIn = tEnter;
				int entryAxis = blk.axis;
				for (;;) {
					const float tSubExit = fminf(sb.exit_t(), tBlockExit);
					ray_test_bucket(p, sh, o, tLo, tHi, e, ray_bucket(sb.cell), best);
					const float lo[3] = { org[0] + (float)sb.cell[0] * sub, org[1] + (float)sb.cell[1] * sub, org[2] + (float)sb.cell[2] * sub };
					const int exitAxis = tSubExit < t1 ? (sb.next[0] <= sb.next[1] ? (sb.next[0] <= sb.next[2] ? 0 : 2) : (sb.next[1] <= sb.next[2] ? 1 : 2)) : -1;
					int near[3];
					if (ray_near_faces(o, d, tIn, tSubExit, lo, sub, sb.step, entryAxis, exitAxis, eps, near)) {
						for (int dz = near[2] < 0 ? -1 : 0; dz <= (near[2] > 0 ? 1 : 0); ++dz)
							for (int dy = near[1] < 0 ? -1 : 0; dy <= (near[1] > 0 ? 1 : 0); ++dy)
								for (int dx = near[0] < 0 ? -1 : 0; dx <= (near[0] > 0 ? 1 : 0); ++dx) {
									if (!dx && !dy && !dz) continue;
									int s[3] = { sb.cell[0] + dx, sb.cell[1] + dy, sb.cell[2] + dz };
									int c[3] = { blk.cell[0], blk.cell[1], blk.cell[2] };
									bool inside = true;
									for (int a = 0; a < 3; ++a) {
										if (s[a] < 0) { s[a] += RAY_SUB; --c[a]; }
										else if (s[a] >= (int)RAY_SUB) { s[a] -= RAY_SUB; ++c[a]; }
										inside = inside && c[a] >= 0 && c[a] < (int)p.cnt;
									}
									if (!inside) continue;
									const u32 e2 = (c[0] == blk.cell[0] && c[1] == blk.cell[1] && c[2] == blk.cell[2]) ? e : p.map[ray_coord_id(c, p.cnt)];
									if (e2 != RAY_NONE) ray_test_bucket(p, sh, o, tLo, tHi, e2, ray_bucket(s), best);
								}
					}
					// a later sub-brick holds only triangles hit at t >= this exit
					if (best.t <= tSubExit + fabsf(tSubExit) * (1.f / 4194304.f)) { done = true; break; }
					if (tSubExit >= tBlockExit || !sb.advance(o, inv, org, sub, (int)RAY_SUB)) break;
					tIn = tSubExit;
					entryAxis = sb.axis;
				}
			}
			if (done || tBlockExit >= t1 || !blk.advance(o, inv, zero, p.size, (int)p.cnt)) break;
			tEnter = tBlockExit;
		}
	}
	const float bestT = best.t, bestU = best.u, bestV = best.v;
	const u32 bestE = best.e, bestTri = best.tri;
	float4 h0 = make_float4(bestT, 0.f, 0.f, 0.f), h1 = make_float4(0.f, 0.f, 0.f, 0.f), h2;
	if (bestE != RAY_NONE) {
		const ListedBlock& b = p.table[bestE];
		const PolyVertex* v = p.verts + b.rec.vOff;
		const u32* ix = p.idx + b.rec.iOff + 3 * bestTri;
		const float4 A = *(const float4*)&v[ix[0]], B = *(const float4*)&v[ix[1]], C = *(const float4*)&v[ix[2]];
		const double ex = (double)B.x - A.x, ey = (double)B.y - A.y, ez = (double)B.z - A.z;
		const double fx = (double)C.x - A.x, fy = (double)C.y - A.y, fz = (double)C.z - A.z;
		const double nx = ey * fz - ez * fy, ny = ez * fx - ex * fz, nz = ex * fy - ey * fx;
		const double len = sqrt(nx * nx + ny * ny + nz * nz);
		const double s = len > 0.0 ? 1.0 / len : 0.0;
		h0 = make_float4(bestT, o[0] + bestT * d[0], o[1] + bestT * d[1], o[2] + bestT * d[2]);
		h1 = make_float4((float)(nx * s), (float)(ny * s), (float)(nz * s), bestU);
		h2 = make_float4(bestV, __uint_as_float(bestE), __uint_as_float(b.id), __uint_as_float(bestTri));
	} else {
		h2 = make_float4(0.f, __uint_as_float(RAY_NONE), __uint_as_float(RAY_NONE), __uint_as_float(RAY_NONE));
	}
	p.hits[3 * i] = h0;
	p.hits[3 * i + 1] = h1;
	p.hits[3 * i + 2] = h2;
}

struct RayLevel {
	u32* map = nullptr;
	size_t mapCap = 0;          // bytes
	u16* starts = nullptr;
	size_t startsCap = 0;       // bytes
	const ListedBlock* table = nullptr;
	u32 entries = 0;
	uint64_t epoch = 0;         // vx_ctx::meshEpoch the index was built for
	bool built = false;
	vx_ray_index_info info = {};
};

struct RayState {
	RayLevel lv[MAX_LEVELS];
	u16* perm = nullptr;
	size_t permCap = 0;         // bytes
	unsigned long long* stats = nullptr;
	unsigned long long* statsHost = nullptr;
	void* io = nullptr;         // vx_raycast: rays and hits on their way through the device
	size_t ioCap = 0;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;

	bool setup(vx_ctx* c)
	{
		stats = (unsigned long long*)c->be.alloc(16);
		statsHost = (unsigned long long*)c->be.alloc_pinned(16);
		return stats && statsHost && c->be.check(hipEventCreate(&ev0), "hipEventCreate") && c->be.check(hipEventCreate(&ev1), "hipEventCreate");
	}
	void release(vx_ctx* c)
	{
		for (RayLevel& l : lv) { c->be.free(l.map); c->be.free(l.starts); }
		c->be.free(perm); c->be.free(stats); c->be.free(io);
		c->be.free_pinned(statsHost);
		if (ev0) (void)hipEventDestroy(ev0);
		if (ev1) (void)hipEventDestroy(ev1);
	}
};

int ray_check(vx_ctx* c, uint32_t level, const char* what)
{
	if (!c) return VX_ERR_INVALID;
	if (!c->haveSurface) return fail(c, VX_ERR_INVALID, std::string(what) + ": no surface (run vx_polygonize first)");
	if (level >= c->levelsRun) return fail(c, VX_ERR_INVALID, std::string(what) + ": no such level");
	return VX_OK;
}

bool ray_current(vx_ctx* c, uint32_t level)
{
	const RayState* s = module_peek<RayState>(c, MOD_RAY);
	return s && s->lv[level].built && s->lv[level].epoch == c->meshEpoch;
}

int ray_prepare(vx_ctx* c, uint32_t level)
{
	if (ray_current(c, level)) return VX_OK;
	RayState* s = module_state<RayState>(c, MOD_RAY, &RayState::setup);
	if (!s) return fail(c, VX_ERR_DEVICE, "vx_raycast_prepare: allocation failed: " + c->be.error());
	const vx_listed_block* tab = nullptr;
	u32 nb = 0;
	const int rc = vx_device_block_table(c, level, &tab, &nb);
	if (rc != VX_OK) return rc;
	RayLevel& l = s->lv[level];
	l.built = false;
	const u32 cnt = c->lv[level].cnt;
	const size_t mapBytes = (size_t)cnt * cnt * cnt * 4, startsBytes = (size_t)nb * (RAY_BUCKETS + 1) * 2;
	const size_t permBytes = ((size_t)c->poolIdx / 3 + 1) * 2;
	if (permBytes > s->permCap || !s->perm) {
		for (RayLevel& o : s->lv) o.built = false; // (the other levels' parts of the permutation are gone)
		if (!dev_grow(c, s->perm, s->permCap, permBytes)) return fail(c, VX_ERR_DEVICE, "vx_raycast_prepare: allocation failed: " + c->be.error());
	}
	if (!dev_grow(c, l.map, l.mapCap, mapBytes) || !dev_grow(c, l.starts, l.startsCap, startsBytes))
		return fail(c, VX_ERR_DEVICE, "vx_raycast_prepare: allocation failed: " + c->be.error());
	RayIndexParams p;
	p.table = (const ListedBlock*)tab;
	p.countDev = c->meshEpoch == c->fullRunEpoch ? (const u32*)c->dHeader + HDR_LISTS + level : nullptr;
	p.count = nb;
	p.verts = (const PolyVertex*)c->dVerts;
	p.idx = (const u32*)c->dIdx;
	p.map = l.map;
	p.starts = l.starts;
	p.perm = s->perm;
	p.stats = s->stats;
	p.cnt = cnt;
	p.size = (float)(16u << level);
	hipStream_t st = c->be.stream;
	bool ok = c->be.check(hipEventRecord(s->ev0, st), "hipEventRecord") && c->be.fill(l.map, 0xFF, mapBytes) && c->be.fill(s->stats, 0, 16);
	if (ok && nb) {
		hipLaunchKernelGGL(k_ray_index, dim3(nb), dim3(WG), 0, st, p);
		ok = c->be.check(hipGetLastError(), "k_ray_index launch");
	}
	ok = ok && c->be.check(hipEventRecord(s->ev1, st), "hipEventRecord") && c->be.d2h(s->statsHost, s->stats, 16);
	if (!ok) return fail(c, VX_ERR_DEVICE, "vx_raycast_prepare: " + c->be.error());
	float ms = 0.f;
	(void)hipEventElapsedTime(&ms, s->ev0, s->ev1);
	l.table = (const ListedBlock*)tab;
	l.entries = nb;
	l.epoch = c->meshEpoch;
	l.built = true;
	l.info.triangles = s->statsHost[0];
	l.info.straddling = (u32)s->statsHost[1];
	l.info.blocks = nb;
	l.info.bytes = mapBytes + startsBytes + 2 * s->statsHost[0];
	l.info.build_ms = ms;
	return VX_OK;
}

int ray_launch(vx_ctx* c, uint32_t level, const vx_ray* dRays, uint32_t n, vx_ray_hit* dHits)
{
	const RayState* s = module_peek<RayState>(c, MOD_RAY);
	const RayLevel& l = s->lv[level];
	RayCastParams p;
	p.rays = (const float4*)dRays;
	p.hits = (float4*)dHits;
	p.n = n;
	p.table = l.table;
	p.map = l.map;
	p.starts = l.starts;
	p.perm = s->perm;
	p.verts = (const PolyVertex*)c->dVerts;
	p.idx = (const u32*)c->dIdx;
	p.cnt = c->lv[level].cnt;
	p.size = (float)(16u << level);
	hipLaunchKernelGGL(k_raycast, dim3((n + WG - 1) / WG), dim3(WG), 0, c->be.stream, p);
	return c->be.check(hipGetLastError(), "k_raycast launch") ? VX_OK : fail(c, VX_ERR_DEVICE, "vx_raycast: " + c->be.error());
}

} // namespace

extern "C" {

static_assert(sizeof(vx_ray) == 32 && sizeof(vx_ray_hit) == 48, "vx_ray / vx_ray_hit layout");

int vx_raycast_prepare(vx_ctx* c, uint32_t level, vx_ray_index_info* info)
{
	VX_ENTER(c);
	int rc = ray_check(c, level, "vx_raycast_prepare");
	if (rc == VX_OK) rc = ray_prepare(c, level);
	if (rc == VX_OK && info) *info = module_peek<RayState>(c, MOD_RAY)->lv[level].info;
	return rc;
}

int vx_raycast_device(vx_ctx* c, uint32_t level, const vx_ray* d_rays, uint32_t n, vx_ray_hit* d_hits)
{
	VX_ENTER(c);
	int rc = ray_check(c, level, "vx_raycast_device");
	if (rc != VX_OK) return rc;
	if (n && (!d_rays || !d_hits)) return fail(c, VX_ERR_INVALID, "vx_raycast_device: null array");
	if (((uintptr_t)d_rays | (uintptr_t)d_hits) & 15u) return fail(c, VX_ERR_INVALID, "vx_raycast_device: arrays must be 16-byte aligned");
	if (!n) return VX_OK;
	if ((rc = ray_prepare(c, level)) != VX_OK) return rc;
	return ray_launch(c, level, d_rays, n, d_hits);
}

int vx_raycast(vx_ctx* c, uint32_t level, const vx_ray* rays, uint32_t n, vx_ray_hit* hits)
{
	VX_ENTER(c);
	int rc = ray_check(c, level, "vx_raycast");
	if (rc != VX_OK) return rc;
	if (n && (!rays || !hits)) return fail(c, VX_ERR_INVALID, "vx_raycast: null array");
	if (!n) return VX_OK;
	if ((rc = ray_prepare(c, level)) != VX_OK) return rc;
	RayState* s = module_peek<RayState>(c, MOD_RAY);
	const size_t rayBytes = (size_t)n * sizeof(vx_ray), hitBytes = (size_t)n * sizeof(vx_ray_hit);
	if (!dev_grow(c, s->io, s->ioCap, rayBytes + hitBytes)) return fail(c, VX_ERR_DEVICE, "vx_raycast: allocation failed: " + c->be.error());
	vx_ray* dRays = (vx_ray*)s->io;
	vx_ray_hit* dHits = (vx_ray_hit*)((char*)s->io + rayBytes);
	if (!c->be.h2d(dRays, rays, rayBytes)) return fail(c, VX_ERR_DEVICE, "vx_raycast: upload failed: " + c->be.error());
	if ((rc = ray_launch(c, level, dRays, n, dHits)) != VX_OK) return rc;
	if (!c->be.d2h(hits, dHits, hitBytes)) return fail(c, VX_ERR_DEVICE, "vx_raycast: download failed: " + c->be.error());
	return VX_OK;
}

} // extern "C"
