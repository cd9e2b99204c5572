// Host side of the tests of the overlap queries (include/voxels_hip.h, "overlap queries"): a level's ray-cast index built on the
// host by the centroid rule of k_ray_index (ray_sub_of / ray_bucket of voxels_amd/csrc/tv_ray.h), and the three passes of
// vx_overlap.inl - count, scan, write - run sequentially with the functions of voxels_amd/csrc/tv_overlap.h, a lane at a time -
// tests only (tests/test_overlap.py, tests/test_abi_overlap.py).  A seed shuffles every bucket's slice of the permutation:
// the device fills it with atomics, and the output must not depend on its order.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_ray.h"
#include "../../voxels_amd/csrc/tv_overlap.h"

using namespace tv;

namespace {

struct HostIndex {
	std::vector<u32> map;       // coord_id -> entry, RAY_NONE = no mesh
	std::vector<u32> starts;    // 65 per entry
	std::vector<u32> perm;      // per triangle of the index pool (i_off / 3 + k)
	uint64_t straddling = 0;
};

const float* position(const vx_vertex* v, u32 i) { return (const float*)(v + i); }   // (pos is the first field)

// bucket of a triangle: k_ray_index's ray_tri_bucket
u32 tri_bucket(const vx_vertex* v, const u32* ix, const float org[3], float sub, uint64_t& outside)
{
	const float* P[3] = { position(v, ix[0]), position(v, ix[1]), position(v, ix[2]) };
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

u32 next_random(u32& state)
{
	state ^= state << 13; state ^= state >> 17; state ^= state << 5;
	return state;
}

void build_index(const vx_listed_block* table, u32 nEntries, const vx_vertex* verts, const u32* idx, u32 cnt, float size, u32 seed, HostIndex& ix)
{
	ix.map.assign((size_t)cnt * cnt * cnt, RAY_NONE);
	ix.starts.assign((size_t)nEntries * (RAY_BUCKETS + 1), 0u);
	size_t pool = 0;
	for (u32 e = 0; e < nEntries; ++e) pool = std::max<size_t>(pool, table[e].i_off / 3u + table[e].i_count / 3u);
	ix.perm.assign(pool, 0u);
	u32 rnd = seed * 2654435761u + 1u;
	const float sub = size / (float)RAY_SUB;
	for (u32 e = 0; e < nEntries; ++e) {
		const vx_listed_block& b = table[e];
		if (b.coord_id < ix.map.size()) ix.map[b.coord_id] = e;
		float org[3];
		ray_block_origin(b.coord_id, cnt, size, org);
		const vx_vertex* v = verts + b.v_off;
		const u32* tix = idx + b.i_off;
		const u32 nTri = b.i_count / 3u;
		std::vector<u32> bucketOf(nTri);
		u32 hist[RAY_BUCKETS] = {};
		for (u32 k = 0; k < nTri; ++k) ++hist[bucketOf[k] = tri_bucket(v, tix + 3 * k, org, sub, ix.straddling)];
		u32* starts = &ix.starts[(size_t)e * (RAY_BUCKETS + 1)];
		u32 cursor[RAY_BUCKETS], sum = 0;
		for (u32 i = 0; i < RAY_BUCKETS; ++i) { starts[i] = cursor[i] = sum; sum += hist[i]; }
		starts[RAY_BUCKETS] = sum;
		u32* perm = &ix.perm[b.i_off / 3u];
		for (u32 k = 0; k < nTri; ++k) perm[cursor[bucketOf[k]]++] = k;
		if (seed)
			for (u32 i = 0; i < RAY_BUCKETS; ++i)
				for (u32 k = starts[i + 1]; k > starts[i] + 1u; --k) std::swap(perm[k - 1u], perm[starts[i] + next_random(rnd) % (k - starts[i])]);
	}
}

struct Walk {
	const vx_listed_block* table;
	const vx_vertex* verts;
	const u32* idx;
	u32 cnt;
	float size;
	const HostIndex* ix;
};

// the walk of one query: the matches of every block in coord_id order, each block's in ascending tri; emit(entry, tri)
template <typename Emit> void walk_query(const Walk& w, const float lo[3], const float hi[3], Emit emit)
{
	if (!overlap_box_valid(lo, hi)) return;
	int c0[3];
	u32 ext[3];
	for (int a = 0; a < 3; ++a) {
		int c1;
		overlap_block_range(lo[a], hi[a], w.size, w.cnt, c0[a], c1);
		ext[a] = c1 >= c0[a] ? (u32)(c1 - c0[a] + 1) : 0u;
	}
	const u32 total = ext[0] * ext[1] * ext[2];
	const float sub = w.size / (float)RAY_SUB;
	std::vector<u32> bits(OVERLAP_WORDS);
	for (u32 k = 0; k < total; ++k) {
		int m[3];
		overlap_candidate_cell(k, c0, ext, m);
		const float cellOrg[3] = { (float)m[0] * w.size, (float)m[1] * w.size, (float)m[2] * w.size };
		if (!overlap_block_meets(lo, hi, cellOrg, sub)) continue;
		const u32 e = w.ix->map[ray_coord_id(m, w.cnt)];
		if (e == RAY_NONE) continue;
		const vx_listed_block& b = w.table[e];
		const vx_vertex* v = w.verts + b.v_off;
		const u32* tix = w.idx + b.i_off;
		const u32* perm = &w.ix->perm[b.i_off / 3u];
		const u32* starts = &w.ix->starts[(size_t)e * (RAY_BUCKETS + 1)];
		float org[3];
		ray_block_origin(b.coord_id, w.cnt, w.size, org);
		unsigned long long buckets = 0;
		for (u32 s = 0; s < RAY_BUCKETS; ++s)
			if (overlap_bucket_meets(lo, hi, org, sub, s) && starts[s] < starts[s + 1]) buckets |= 1ull << s;
		if (!buckets) continue;
		const u32 nWords = std::min<u32>(overlap_words(b.i_count / 3u), OVERLAP_WORDS);
		std::fill(bits.begin(), bits.begin() + nWords, 0u);
		while (buckets) {
			u32 s0, s1;
			overlap_next_run(buckets, s0, s1);
			for (u32 j = starts[s0]; j < starts[s1]; ++j) {
				const u32 tri = perm[j];
				if (!overlap_matches(lo, hi, position(v, tix[3 * tri]), position(v, tix[3 * tri + 1]), position(v, tix[3 * tri + 2]))) continue;
				u32 word;
				const u32 bit = overlap_mark(tri, word);
				if (word < nWords) bits[word] |= bit;
			}
		}
		for (u32 word = 0; word < nWords; ++word)
			for (u32 rest = bits[word]; rest; rest &= rest - 1u) emit(e, (word << 5) + (u32)__builtin_ctz(rest));
	}
}

} // namespace

extern "C" {

// sizes (k = 0..5) and field offsets (k >= 6) as this compiler lays out the header's structs
uint32_t ov_layout(uint32_t k)
{
	const uint32_t s[] = {
		sizeof(vx_overlap_box), sizeof(vx_overlap_tri), sizeof(vx_overlap_range), sizeof(vx_overlap_counts), sizeof(vx_vertex), sizeof(vx_listed_block),
		offsetof(vx_overlap_box, lo), offsetof(vx_overlap_box, reserved0), offsetof(vx_overlap_box, hi), offsetof(vx_overlap_box, reserved1),
		offsetof(vx_overlap_tri, query), offsetof(vx_overlap_tri, entry), offsetof(vx_overlap_tri, block_id), offsetof(vx_overlap_tri, tri),
		offsetof(vx_overlap_range, first), offsetof(vx_overlap_range, count),
		offsetof(vx_overlap_counts, triangles), offsetof(vx_overlap_counts, pairs), offsetof(vx_overlap_counts, queries),
		offsetof(vx_overlap_counts, hit_queries), offsetof(vx_overlap_counts, max_per_query), offsetof(vx_overlap_counts, reserved),
		VX_OVERLAP_MAX_QUERIES,
	};
	return k < sizeof(s) / sizeof(s[0]) ? s[k] : 0xFFFFFFFFu;
}

// vx_overlap_boxes on host arrays: `verts` and `idx` are the pools the table's offsets point into, cnt the level's blocks per
// axis.  Returns 0, or -3 when triangles > capacity (everything the header promises is written first).  `straddling` (may be
// null) receives the index build's count of triangles outside their bucket's dilated box.
int ov_overlap(uint32_t level, const vx_listed_block* table, uint32_t nEntries, const vx_vertex* verts, const uint32_t* idx, uint32_t cnt,
               const vx_overlap_box* boxes, uint32_t n, uint32_t capacity, vx_overlap_tri* tris, float* corners, vx_overlap_range* ranges,
               vx_overlap_counts* counts, uint32_t seed, uint64_t* straddling)
{
	HostIndex ix;
	const float size = (float)(16u << level);
	build_index(table, nEntries, verts, idx, cnt, size, seed, ix);
	if (straddling) *straddling = ix.straddling;
	const Walk w = { table, verts, idx, cnt, size, &ix };
	vx_overlap_counts c;
	memset(&c, 0, sizeof(c));
	if (nEntries == 0u) {   // an empty table: zero counts, zero ranges
		*counts = c;
		if (ranges) memset(ranges, 0, (size_t)n * sizeof(vx_overlap_range));
		return 0;
	}
	c.queries = n;
	// count
	std::vector<uint64_t> count(n, 0), first(n, 0);
	for (u32 q = 0; q < n; ++q) {
		u32 last = RAY_NONE;
		walk_query(w, boxes[q].lo, boxes[q].hi, [&](u32 e, u32) { ++count[q]; if (e != last) { ++c.pairs; last = e; } });
	}
	// scan
	for (u32 q = 0; q < n; ++q) {
		first[q] = c.triangles;
		c.triangles += count[q];
		c.hit_queries += count[q] ? 1u : 0u;
		c.max_per_query = std::max<uint32_t>(c.max_per_query, (uint32_t)count[q]);
	}
	*counts = c;
	if (c.triangles > 0xFFFFFFFFull) return -3;
	if (ranges) for (u32 q = 0; q < n; ++q) { ranges[q].first = (uint32_t)first[q]; ranges[q].count = (uint32_t)count[q]; }
	// write
	for (u32 q = 0; q < n && capacity; ++q) {
		uint64_t at = first[q];
		walk_query(w, boxes[q].lo, boxes[q].hi, [&](u32 e, u32 tri) {
			if (at < capacity) {
				const vx_listed_block& b = table[e];
				tris[at].query = q; tris[at].entry = e; tris[at].block_id = b.id; tris[at].tri = tri;
				if (corners)
					for (u32 j = 0; j < 3u; ++j) {
						float* o = corners + 12 * at + 4 * j;
						memcpy(o, position(verts + b.v_off, idx[b.i_off + 3 * tri + j]), 12);
						o[3] = 0.f;
					}
			}
			++at;
		});
	}
	return c.triangles > capacity ? -3 : 0;
}

} // extern "C"
