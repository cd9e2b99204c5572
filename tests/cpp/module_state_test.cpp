// tests/cpp/module_state_test.cpp — the module registry of vx_ctx (vx_host.inl: module_state, module_peek, the loop of
// vx_ctx_destroy) and dev_grow, on the CPU emulation's backend: what tests/emu/emu.cpp includes, plus two stand-in module
// states whose release() records that it ran.  Prints OK and returns 0, or says what failed (tests/test_module_state.py).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../voxels_amd/csrc/tv_block.h"
#include "../../voxels_amd/csrc/tv_fast0.h"
#include "../../voxels_amd/csrc/tv_fast1.h"
#include "../../voxels_amd/csrc/vx_terrain_math.h"

#define VX_BACKEND_NAME "emu:cpu (tests only)"

namespace {
using namespace tv;

template <typename T>
u32 exclusive_scan(T* a, u32 n)
{
	u32 run = 0;
	for (u32 i = 0; i < n; ++i) { const u32 v = a[i]; a[i] = (T)run; run += v; }
	return run;
}
}

#include "../emu/emu_backend.inl"
#include "../../voxels_amd/csrc/vx_host.inl"

namespace {

std::vector<int> dropped; // the slot of every state released, in order
int alive = 0;            // states constructed and not yet deleted

template <int Id>
struct FakeState {
	void* buf = nullptr;
	size_t bufCap = 0;
	FakeState() { ++alive; }
	~FakeState() { --alive; }
	bool setup(vx_ctx* c) { buf = c->be.alloc(64); return false; } // a set-up that fails after it has allocated
	void release(vx_ctx* c) { c->be.free(buf); dropped.push_back(Id); }
};
typedef FakeState<MOD_LOD> LodLike;
typedef FakeState<MOD_UNDO> UndoLike;
typedef FakeState<MOD_RAY> RayLike;

int failures = 0;
#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); ++failures; } } while (0)

vx_ctx* make_ctx()
{
	vx_ctx* c = nullptr;
	if (vx_ctx_create(0, &c) != VX_OK || !c) { printf("FAILED: vx_ctx_create\n"); exit(1); }
	return c;
}

} // namespace

int main()
{
	// a context that never touched a module drops nothing
	vx_ctx* c = make_ctx();
	vx_ctx_destroy(c);
	CHECK(dropped.empty() && alive == 0);

	c = make_ctx();
	// peek before creation; first access creates, the second returns the same state
	CHECK(module_peek<UndoLike>(c, MOD_UNDO) == nullptr);
	UndoLike* u = module_state<UndoLike>(c, MOD_UNDO);
	CHECK(u && alive == 1);
	CHECK(module_state<UndoLike>(c, MOD_UNDO) == u && alive == 1);
	CHECK(module_peek<UndoLike>(c, MOD_UNDO) == u);
	CHECK(module_peek<LodLike>(c, MOD_LOD) == nullptr);
	// a failed set-up: released and deleted at once, the caller sees null, the slot stays empty - and can be tried again
	CHECK(module_state<RayLike>(c, MOD_RAY, &RayLike::setup) == nullptr);
	CHECK(module_peek<RayLike>(c, MOD_RAY) == nullptr && alive == 1);
	CHECK(dropped.size() == 1 && dropped[0] == MOD_RAY);
	CHECK(module_state<RayLike>(c, MOD_RAY, &RayLike::setup) == nullptr && dropped.size() == 2 && alive == 1);
	dropped.clear();
	// created after undo, dropped before it: enum order, not creation order
	LodLike* l = module_state<LodLike>(c, MOD_LOD);
	CHECK(l && (void*)l != (void*)u && alive == 2);
	// dev_grow: allocates for an empty buffer (a zero-byte request too), keeps one that is large enough, replaces one that is not
	CHECK(dev_grow(c, u->buf, u->bufCap, 0) && u->buf && u->bufCap == 256);
	void* first = u->buf;
	memset(first, 0x5a, 256);
	CHECK(dev_grow(c, u->buf, u->bufCap, 256) && u->buf == first && u->bufCap == 256);
	CHECK(dev_grow(c, u->buf, u->bufCap, 1000) && u->bufCap == 1000 + 250 + 256);
	memset(u->buf, 0x5a, u->bufCap);
	CHECK(dev_grow(c, l->buf, l->bufCap, 100) && l->bufCap == 100 + 25 + 256);
	vx_ctx_destroy(c);
	CHECK(dropped.size() == 2 && dropped[0] == MOD_LOD && dropped[1] == MOD_UNDO);
	CHECK(alive == 0);

	if (!failures) printf("OK\n");
	return failures ? 1 : 0;
}
