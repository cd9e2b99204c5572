// brush_host.cpp — host oracle of vx_grid_inject_brushes (tests only; built by voxels_amd/build.py build_brush_host()).
//
// A vx_brush array is applied to a host grid SEQUENTIALLY, one Voxels::VoxelGrid::InjectSurface / InjectMaterial call per
// brush (voxels_amd/csrc/vx_grid_host.cpp, the class behind Voxels::Grid).  The distance brushes are a VoxelSurface whose
// GetSurface runs the reference's triple float loop and calls the sample function of voxels_amd/csrc/tv_brush.h.  The
// sample function is all this shares with the device path: sections, the pairing of voxels with samples and the rounding
// come from the host grid class, not from tv_block.h.
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/Voxels.h"
#include "../../include/voxels_hip.h"
#include "../../voxels_amd/csrc/tv_brush.h"
#include "../../voxels_amd/csrc/vx_grid_host.h"

namespace {

struct BrushSurface : public Voxels::VoxelSurface
{
	const vx_brush* b;
	void GetSurface(float xStart, float xEnd, float xStep, float yStart, float yEnd, float yStep, float zStart, float zEnd, float zStep,
	                float* output, unsigned char*, unsigned char*) override
	{
		// what InjectSurface allocated (:405-441): the product of the rounded-up lengths, plus one
		const size_t room = (size_t)ceilf(xEnd - xStart) * (size_t)ceilf(yEnd - yStart) * (size_t)ceilf(zEnd - zStart) + 1;
		size_t o = 0;
		for (float z = zStart; z < zEnd; z += zStep)
		for (float y = yStart; y < yEnd; y += yStep)
		for (float x = xStart; x < xEnd; x += xStep) {
			if (o < room) output[o] = tv::brush_sample(b->shape, x, y, z, b->a, b->b, b->radius);
			++o;
		}
	}
};

} // namespace

extern "C" {

// dist / mat / blend: dense n^3 fields (x fastest, Z up), rewritten in place.  flags: BF_Empty per block by the codec's rule
// (every block, as the host grid keeps it).  distTouched: per block, 1 when at least one distance brush touched it.
// boxes: 6 floats per brush (out_min, out_max), touched: blocks per brush.  pack: the grid file when pack != NULL and
// packCap suffices; *packSize = its size.
int bh_apply(uint32_t n, int8_t* dist, uint8_t* mat, uint8_t* blend, const vx_brush* brushes, uint32_t count,
             uint8_t* flags, uint8_t* distTouched, float* boxes, uint32_t* touched, uint8_t* pack, size_t packCap, size_t* packSize)
{
	using Voxels::VoxelGrid;
	VoxelGrid g(n);
	const uint32_t nb = n / 16;
	std::vector<int8_t> bd(4096);
	std::vector<uint8_t> bm(4096), bb(4096);
	auto gather = [&](const uint8_t* src, uint32_t bx, uint32_t by, uint32_t bz, uint8_t* out) {
		for (uint32_t z = 0; z < 16; ++z) for (uint32_t y = 0; y < 16; ++y)
			memcpy(out + z * 256 + y * 16, src + g.Index(bx * 16, by * 16 + y, bz * 16 + z), 16);
	};
	for (uint32_t bz = 0; bz < nb; ++bz) for (uint32_t by = 0; by < nb; ++by) for (uint32_t bx = 0; bx < nb; ++bx) {
		gather((const uint8_t*)dist, bx, by, bz, (uint8_t*)bd.data());
		gather(mat, bx, by, bz, bm.data());
		gather(blend, bx, by, bz, bb.data());
		g.SetBlockDistances(bx, by, bz, bd.data());
		g.SetBlockMaterials(bx, by, bz, bm.data(), bb.data());
	}
	if (distTouched) memset(distTouched, 0, (size_t)nb * nb * nb);
	std::vector<uint32_t> dirty;
	for (uint32_t i = 0; i < count; ++i) {
		const vx_brush& b = brushes[i];
		const uint64_t before = g.Generation();
		float mn[3], mx[3];
		if (b.shape == VX_BRUSH_MATERIAL) {
			g.InjectMaterial(b.position, b.extents, (uint8_t)b.material, b.type != 0, mn, mx);
		} else {
			BrushSurface s;
			s.b = &b;
			g.InjectSurface(b.position, b.extents, &s, (int)b.type, mn, mx);
		}
		g.DirtySince(before, dirty);
		if (touched) touched[i] = (uint32_t)dirty.size();
		if (distTouched && b.shape != VX_BRUSH_MATERIAL) for (uint32_t id : dirty) distTouched[id] = 1;
		if (boxes) for (int k = 0; k < 3; ++k) { boxes[i * 6 + k] = mn[k]; boxes[i * 6 + 3 + k] = mx[k]; }
	}
	const size_t total = (size_t)n * n * n;
	memcpy(dist, g.Distances(), total);
	memcpy(mat, g.Materials(), total);
	memcpy(blend, g.Blends(), total);
	if (flags) { std::vector<uint8_t> f; g.EmptyFlags(f); memcpy(flags, f.data(), f.size()); }
	std::vector<char> file;
	g.Pack(file);
	if (packSize) *packSize = file.size();
	if (pack && packCap >= file.size()) memcpy(pack, file.data(), file.size());
	return 0;
}

// the sample functions at `count` points: p, a, b = 3 floats per point, radius = 1
void bh_sample(uint32_t shape, uint32_t count, const float* p, const float* a, const float* b, const float* radius, float* out)
{
	for (uint32_t i = 0; i < count; ++i) out[i] = tv::brush_sample(shape, p[3 * i], p[3 * i + 1], p[3 * i + 2], a + 3 * i, b + 3 * i, radius[i]);
}

} // extern "C"
