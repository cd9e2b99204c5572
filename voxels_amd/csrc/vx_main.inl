// vx_main.inl — k_main: everything a full run does between k_run_head (slots) and k_tail (lists) as ONE launch (gfx950).
// There is no classification pass in front of it.  Level-0 blocks and level-1 material blocks read the bitmaps they need by
// block coordinate from the cell map (MAP: Globals::cellMap, a mirror of the grid that is current before the run starts -
// MirrorState, ensure_cell_map); k_run_head has taken the blocks' cell counts from it.  Without the map (VX_CELLMAP=0) level-0
// blocks form their own bitmaps (f0_walk<.., SELF>) and level-1 material blocks their children's (mat_block, selfChild).
// Included by vx_hip.hip
// behind the passes whose per-block bodies it calls: f0_walk (table-driven regular cells of level-0 blocks, vx_fast0.inl),
// mat_block (the material vote of one block of a level >= 1, vx_hip.hip), f1_block (the table-driven regular cells of one
// block of a level 1..3, vx_fast1.inl), tr_block (the transition cells of one block, vx_hip.hip, with the table-driven body
// of vx_fastt.inl).
//
// The reference walks the levels one after the other (TransVoxelRun::Execute, src/TransVoxelImpl.cpp:492-531): the material
// cache of a level-L cell is a vote over its eight children on level L-1 (:753-838), a block's regular and transition
// cells read its own cache, and level 0 needs none of that.  As launches that is a chain - material L1, L2, L3, then the
// passes over the levels >= 1, the level-0 pass beside them on a second stream, stream events at the fork and at the join -
// whose fixed cost is the whole of a small run (a 128^3 grid, a rank's slab of an 8-GPU job).  Here the same work is two
// queues handed out by atomic counters to persistent workgroups:
//   * the upper queue, in dependency order:
//         [ material blocks of level 1 | of level 2 | ... | regular blocks of levels 1..3 | transition blocks ]
//     An item waits for exactly what it reads from other workgroups, as late as it can: a material block for its children's
//     caches right in front of its vote (sampling, classification and candidate selection need none of them), a regular block
//     for its own material behind the request of its lattice samples, a transition block for it behind planes,
//     classification and scans.  The flags are LevelDesc::matDone (publish_done_through / wait_done: write-through stores and
//     loads, placement-independent, every wait bounded).
//     On a grid that has not changed since a full run of this form filled the material store (MatStoreLevel, tv_block.h;
//     MainPlan::matMode) the material items are copy items (mat_copy_block): same queue position, same stores, same flag -
//     the regular and transition items behind them notice nothing - but no samples, no vote and nobody to wait for.
//     A run that also keeps the slot plan (matMode 3, "in place") has no material segment at all: every slot of the levels
//     >= 1 still holds the cache, bitmap, cell count and flat item that the run which left the plan wrote there (vx_host.inl,
//     where `kept` is decided, lists the writers), so the queue is [ regular | transition ] and nobody polls a flag.
//   * the level-0 queue: the active level-0 slots, taken in batches of consecutive slots (x-neighbour blocks: a batch is
//     walked with the register prefetch of f0_walk, and its blocks share halo lines in one XCD's L2).
// A workgroup prefers one of the queues (a share of the workgroups the upper one, so that the latency-bound dependency chain
// of the levels >= 1 starts at once and runs beside the bandwidth-hungry level-0 blocks on every CU) and moves on to the
// other when its own is empty: nobody idles while work is left, and no stream event or second stream is involved.
//
// Progress: an item only waits for items BEFORE it in the upper queue; those were dequeued earlier, by workgroups that are
// running (a workgroup dequeues while it runs, never before), and the first unfinished item of the queue waits for
// nothing.  So no co-residency of the whole grid is needed, and no order of dispatch is assumed.
namespace {

constexpr u32 UP_TAB_LDS = TR_TAB_LDS > F0_TAB_LDS ? TR_TAB_LDS : F0_TAB_LDS;      // one table image at a time: regular (F0) or transition
constexpr u32 UP_STATE_LDS = sizeof(TrState) > sizeof(Fast1State<REG_CAP_SMALL>)
	? (sizeof(TrState) > sizeof(MatLds) ? sizeof(TrState) : sizeof(MatLds))
	: (sizeof(Fast1State<REG_CAP_SMALL>) > sizeof(MatLds) ? sizeof(Fast1State<REG_CAP_SMALL>) : sizeof(MatLds));
constexpr u32 MAIN_STATE_LDS = sizeof(Fast0State<REG_CAP_SMALL>) > UP_STATE_LDS ? sizeof(Fast0State<REG_CAP_SMALL>) : UP_STATE_LDS;
static_assert((UP_TAB_LDS & 15u) == 0, "the state behind the tables stays 16-byte aligned");

struct MainPlan {
	u32 levels;     // levels of the run: material items for 1 .. levels - 1
	u32 fastEnd;    // regular items for the levels 1 .. fastEnd - 1 (the levels with a lattice copy)
	u32 level0;     // 1: the level-0 queue is part of the launch (its LDS then holds a Fast0State), and no classification pass ran
	                // (k_run_head<allocate>): level-0 blocks and level-1 material blocks read the bitmaps they need from the cell
	                // map (k_main<false, false, true>) or form them (k_main<false>)
	u32 batch;      // level-0 slots per dequeue (one head for the chip: a head per XCD over spatial granules - round 6,
	                // profiles/r06_xcd_heads.txt - fetched 9 % fewer lines and was no faster)
	u32 upperNum, upperDen; // workgroups with blockIdx % upperDen < upperNum prefer the upper queue
	// incremental runs (k_main<true>, vx_polygonize_dirty): the queues hand out the entries of the levels' work lists
	// (Globals::workItems / workCount, written by k_dirty_head); a material block only waits for the children that are part of
	// this run - those inside the dirty box of their level ([boxLo, boxHi) in block coordinates x, y, z)
	u32 boxLo[MAX_LEVELS][3], boxHi[MAX_LEVELS][3];
	// partial runs (k_main<false, true>, vx_polygonize_from): the levels below emitFrom keep their caches and bitmaps up to date
	// but produce no meshes (another device produces those, libVoxels.so with VOXELS_DEVICES): no level-0 queue, regular and
	// transition items only for the levels >= emitFrom
	u32 emitFrom;
	u32 trTables;   // 1: transition blocks take the table-driven body where they qualify (VX_FAST bit 2; vx_fastt.inl)
	// the material store (MAP form only; Globals::matStore is set for the run's levels where this is not 0): 1 = the material
	// blocks vote as always and also leave their results in the store (mat_block: capture), 2 = they are copy items
	// (mat_copy_block), 3 = in place: the run keeps the slot plan, and every slot still holds what the copy would write - the
	// upper queue has no material segment, and regular and transition items read their slots with ordinary loads and no
	// wait (the data is an earlier launch's).  Uniform at run time: not another instantiation of the kernel.
	u32 matMode;
	// 1 (only with matMode 3, in a run that keeps the slot plan): the run also keeps the MESH LAYOUT of the run before it on
	// these slots (vx_host.inl, where layoutValid is decided) - every slot's record, the block lists and their totals and the
	// final pool cursors are in memory already, byte for byte what this run would produce, because a block's ranges are the
	// only thing in them that depends on the order in which blocks arrive.  So a block takes its ranges from its record
	// (layout_ranges, vx_hip.hip) instead of reserving them, checks its totals against the record's counts, and stores
	// neither record nor list count nor - level 0 - the slot's bitmaps; nobody builds lists behind the kernel, and its last
	// workgroup does what is left of k_tail (LayoutEnd).  Uniform at run time, like matMode.
	// 2: the same, and the run keeps the INDEX POOL's bytes too (main_indices_kept).  An index is its cell's vertex base plus an
	// ordinal, or its owner's: the bases are the layout (the record's vOff and the scan of the per-cell counts), the ordinals
	// come from case codes and reuse decisions - signs and material ids of the grid, which has not changed or the plan and the
	// layout would be gone - and nothing in them depends on the material table.  The table-driven bodies (f0_walk, f1_block,
	// trf_block) cannot drop a triangle, so their cell phase alone yields the index counts that layout_ranges checks against
	// the record; they write no triangle descriptor, run no triangle lane and store no index.  The general phases of tr_block
	// (a zero on a staged plane: the degenerate filter decides the count) write their indices as ever - the same bytes.
	u32 layout;
	// 1 (only with layout != 0; main_geometry_kept): the run keeps the GEOMETRY of the regular vertices too - bytes 0..39 of a
	// vertex (position, secondary position, secW, normal) are a function of the grid alone, which has not changed or the layout
	// would be gone, and they lie where the record says.  f0_walk and f1_block then run the texture-only vertex forms
	// (f0_vertex_tex, f1_vertex_tex): the material rule and the table row - the one thing vx_material_lut changes - and one
	// 8-byte store at byte 40 of the record.  trf_block and the general phases of tr_block write whole vertices as ever, the
	// same bytes.  0: whole vertices everywhere.  Uniform at run time.
	u32 geometry;
};

// The end of a run that keeps the mesh layout (MainPlan::layout; pub.host == nullptr in every other run, which ends as ever):
// the workgroup that finishes last seeds the counters of the next run that keeps the slots (k_tail's SeedRanges), puts the
// cursors and list totals of the kept layout - the host's copies, taken from the header of the run that left it - into this
// run's header, marks the run if a block was handed to the general passes (nobody runs them), and publishes the header to the
// host.  Who is last is decided by a returning ticket on pub.done, drawn by every workgroup behind its own drained stores and
// atomics: nobody waits for anybody (k_dirty_head elects its last workgroup the same way).
struct LayoutEnd {
	HeaderPublish pub;
	SeedRanges seed;
	u32* lists;             // the header's list totals
	u32 cursors[2];         // vertices, indices
	u32 totals[MAX_LEVELS];
};

// The kernel's arguments by their places in the kernarg segment (every instantiation has the same four).  The mirror is tied
// to k_main's signature behind the kernel: KernargPlaces lays the parameter types of the kernel's own function type out by the
// kernarg rule (each at the next multiple of its alignment), and a static_assert compares that with this struct's offsets -
// an argument added, dropped or reordered there without the same change here does not compile.
struct MainKernargs {
	ExecParamsDev p;
	MainPlan plan;
	u32* clockStart;
	LayoutEnd end;
};
template <typename F> struct KernargPlaces;
template <typename... A> struct KernargPlaces<void(A...)> {
	static constexpr size_t count = sizeof...(A);
	static constexpr bool are(const size_t (&want)[sizeof...(A)], size_t total)
	{
		const size_t size[] = { sizeof(A)... }, align[] = { alignof(A)... };
		size_t off = 0;
		for (size_t i = 0; i < sizeof...(A); ++i) {
			off = (off + align[i] - 1) / align[i] * align[i];
			if (off != want[i]) return false;
			off += size[i];
		}
		return off <= total;
	}
};
__device__ __forceinline__ const MainKernargs& main_kernargs()
{
	typedef const __attribute__((address_space(4))) MainKernargs* KP;
	KP kp = (KP)__builtin_amdgcn_kernarg_segment_ptr();
	asm volatile("" : "+s"(kp));
	return *(const MainKernargs*)kp;
}
__device__ __forceinline__ bool main_layout_kept() { return r0_uniform(main_kernargs().plan.layout) != 0u; }
__device__ __forceinline__ bool main_indices_kept() { return r0_uniform(main_kernargs().plan.layout) == 2u; }
__device__ __forceinline__ bool main_geometry_kept() { return r0_uniform(main_kernargs().plan.geometry) != 0u; }

// DIRTY: the incremental run's form (TransVoxelRun::Execute with a Modification, src/TransVoxelImpl.cpp:429-465): the same two
// queues over the work lists k_dirty_head wrote - level-0 blocks with the bitmaps the head formed (no SELF), material blocks
// that keep the old cache contents where the reference does (mat_block: defineAll), and the levels beyond the lattice copies
// handed to the general pass of the run's last kernel through Globals::slowItems[1].
// PARTIAL: the levels below plan.emitFrom are somebody else's to mesh (the helper devices of a multi-device Execute): their
// material blocks run as always - the caches a later Modification continues from - and the level-1 material blocks also
// write the bitmaps of their level-0 children, which no level-0 walk forms in such a run.
// MAP (full runs with the level-0 queue only): the cell map is current - nobody forms a bitmap.
template <bool DIRTY, bool PARTIAL = false, bool MAP = false>
// clockStart: a run without k_run_head (the slot plan, vx_host.inl) - workgroup 0 leaves the 100 MHz clock here as it starts, the
// start of the run's device_ms (include/voxels_hip.h: "the first workgroup of the run"); nullptr in every other run.
__global__ __launch_bounds__(WG) __attribute__((amdgpu_waves_per_eu(4))) void k_main(ExecParamsDev pArg, MainPlan plan, u32* clockStart, LayoutEnd endArg)
{
	(void)endArg; // (read at the end of the kernel, through main_kernargs)
#define MAIN_PARAMS() (void)pArg; const ExecParamsDev& p = kernarg_params() // (vx_hip.hip: read afresh, per item)
	MAIN_PARAMS();
	if (clockStart && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(clockStart, run_clock(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (read by the publishing workgroup - of k_tail, or the last one of this kernel - possibly on another XCD)
	u8* tab = smem;
	u8* state = smem + UP_TAB_LDS;
	// (one 16-byte aligned block of statics in front of the dynamic region: its base stays aligned for the 16-byte LDS accesses)
	__shared__ __attribute__((aligned(16))) struct { u32 wgStats[20]; u32 scanScratch[8]; u32 zeroFlag[2]; u32 quietFaces[2]; u32 zeroFlag0[2]; u32 nextItem[2]; } sh;
	static_assert(sizeof(sh) % 16 == 0, "static LDS in front of the dynamic region");
	u32* const wgStats = sh.wgStats; u32* const scanScratch = sh.scanScratch; u32* const zeroFlag = sh.zeroFlag; u32* const quietFaces = sh.quietFaces;

	const int tid0 = (int)threadIdx.x;
	if (tid0 < 20) wgStats[tid0] = 0;
	if (tid0 < 2) { zeroFlag[tid0] = 0; quietFaces[tid0] = 0; sh.zeroFlag0[tid0] = 0; }
	// the upper queue's segments (the slot counts of all levels are final since the classification): matEnd[l] = end of level
	// l's material items; the regular and the transition items are prefixes of the same order
	u32 matEnd[MAX_LEVELS];
	u32 run = 0;
#pragma unroll
	for (u32 l = 0; l < MAX_LEVELS; ++l) {
		if (l >= 1 && l < plan.levels) run += DIRTY ? p.G.workCount[l] : p.G.slotCounts[l];
		matEnd[l] = r0_uniform(run);
	}
	const u32 matTotal = matEnd[MAX_LEVELS - 1];
	u32 regTotal = 0, trTotal = 0, skipItems = 0; // (PARTIAL: the blocks of the levels 1 .. emitFrom - 1 lead both segments and are left out)
#pragma unroll
	for (u32 l = 1; l < MAX_LEVELS; ++l) {
		if (l < plan.fastEnd) regTotal = matEnd[l];
		if (l < plan.levels && p.levels[l].hasTransitions) trTotal = matEnd[l];
		if (PARTIAL && l + 1u == plan.emitFrom) skipItems = matEnd[l];
	}
	if (PARTIAL) { regTotal = max(regTotal, skipItems) - skipItems; trTotal = max(trTotal, skipItems) - skipItems; }
	// (in place: matEnd still decodes a regular or transition item to (level, slot); only the segment itself leaves the queue)
	const bool inPlace = MAP && plan.matMode == 3u;
	const u32 matSeg = inPlace ? 0u : matTotal;
	const u32 upperTotal = matSeg + regTotal + trTotal;
	const u32 total0 = plan.level0 ? r0_uniform(DIRTY ? p.G.workCount[0] : p.G.slotCounts[0]) : 0u;

	u32 tabKind = 0;          // which table image the LDS holds: 0 none, 1 regular (F0), 2 transition
	F0Tables FT = {};
	Tables TT = {};
	u32 parity = 0, quietParity = 0, parity0 = 0;
	bool upperLeft = upperTotal != 0, level0Left = total0 != 0; // (this workgroup's knowledge: a queue is empty once a dequeue came back beyond its end)
	const bool preferUpper = (blockIdx.x % plan.upperDen) < plan.upperNum;
	// One barrier per item says both "the previous item is done with the LDS state" and "the ticket is there": the ticket travels
	// through sh.nextItem[item parity].  (Round 6: drawing the next ticket one item ahead - the returning atomic's 2 us round trip
	// behind the item instead of in front of it - was 2.5 % SLOWER for either queue: the answer comes back in order with the
	// item's first loads and is waited for with them, and a held upper item delays whoever depends on it.)
	u32 turn = 0;

	while (upperLeft || level0Left) {
		MAIN_PARAMS();
		int tid = tid0;
		asm volatile("" : "+v"(tid)); // (per item: what a lane derives from its index alone is not hoisted out of the loop and kept in registers)
		const bool takeUpper = upperLeft && (preferUpper || !level0Left);
		turn ^= 1u;
		if (tid0 == 0) sh.nextItem[turn] = takeUpper ? atomicAdd(p.G.upperHead, 1u) : atomicAdd(p.G.level0Head, plan.batch);
		__syncthreads(); // the previous item is done (with the LDS state), and the ticket is there
		if (!takeUpper) {
			// ---- a batch of consecutive level-0 slots -----------------------------------------------------------------
			const u32 first = r0_uniform(sh.nextItem[turn]);
			if (first >= total0) { level0Left = false; continue; }
			if (tabKind != 1u) { FT = f0_stage_tables(tab, p.tables, (u32)tid); tabKind = 1u; } // (visible after the walk's first barrier)
			f0_walk<REG_CAP_SMALL, false, !DIRTY && !MAP, MAP>(FT, *(Fast0State<REG_CAP_SMALL>*)state, wgStats, sh.zeroFlag0, parity0, total0, 0u, first, 1u, min(first + plan.batch, total0), tid);
			continue;
		}
		// ---- one item of the upper queue (a few thousand items per run) ---------------------------------------------------
		const u32 item = r0_uniform(sh.nextItem[turn]);
		if (item >= upperTotal) { upperLeft = false; continue; }
		// item -> (kind, level, slot): the position inside its segment, looked up in the level boundaries
		const bool isMat = item < matSeg, isReg = !isMat && item < matSeg + regTotal;
		const u32 f = isMat ? item : ((isReg ? item - matSeg : item - matSeg - regTotal) + (PARTIAL ? skipItems : 0u));
		u32 level = 1, base = 0;
#pragma unroll
		for (u32 l = 1; l + 1 < MAX_LEVELS; ++l) if (f >= matEnd[l]) { level = l + 1; base = matEnd[l]; }
		u32 slot = f - base;
		if (DIRTY) slot = r0_uniform(p.G.workItems[level][slot]);
		if (isMat) {
			if (DIRTY) {
				mat_block<true>(p, level, slot, *(MatLds*)state, tid, false, plan.boxLo[level - 1u], plan.boxHi[level - 1u]);
				// a level without a lattice copy has no table-driven regular pass: the general pass of the run's last kernel takes the block
				if (level >= plan.fastEnd && tid0 == 0) p.G.slowItems[1][atomicAdd(&p.G.slowCount[1], 1u)] = (level << 24) | slot;
			} else if (PARTIAL)
				mat_block<true, true>(p, level, slot, *(MatLds*)state, tid, true, nullptr, nullptr, plan.emitFrom);
			else if (MAP) {
				if (plan.matMode == 2u) { mat_copy_block(p, level, slot, tid); continue; }
				mat_block<true, false, true>(p, level, slot, *(MatLds*)state, tid, true, nullptr, nullptr, 0u, plan.matMode == 1u);
			} else
				mat_block<true>(p, level, slot, *(MatLds*)state, tid, plan.level0 != 0u);
			continue;
		}
		const LevelDesc& L = p.levels[level];
		const u32 coord = r0_uniform(L.slotCoord[slot]);
		const GridView& g = p.G.grid;
		const F1BrickSampler smp = { g.bDist, g.bMat, g.bBlend, g.n - 1, (u32)g.n >> 4, (u32)g.bRowsY, g.bYb0, g.bZb0 };
		if (isReg) {
			if (tabKind != 1u) { FT = f0_stage_tables(tab, p.tables, (u32)tid); tabKind = 1u; } // (behind the barriers of the dequeue; visible after the block's first barrier)
			// (in place: the cell count is the slot's own, requested with the coordinate)
			const u32 ntc = inPlace ? r0_uniform((u32)L.ntCount[slot]) : 0u;
			f1_block<REG_CAP_SMALL, true>(p, FT, smp, *(Fast1State<REG_CAP_SMALL>*)state, wgStats, zeroFlag, parity, level, slot, coord, ntc, 0u, tid, !inPlace);
		} else {
			if (tabKind != 2u) { TT = stage_transition_tables(tab, p.tables, (u32)tid); tabKind = 2u; }
			RegBlockCtx b;
			b.level = level; b.slot = slot;
			tr_block<false, true>(p, b, coord, *(TrState*)state, TT, scanScratch, quietFaces, quietParity, smp, tid, plan.trTables != 0u, wgStats + 2, inPlace);
		}
	}
	__syncthreads();
	{
		int tid = tid0;
		asm volatile("" : "+v"(tid)); // (the address is formed here, not carried through the kernel)
		// (no item of this kernel counts into the words 2 and 3: they hold the transition blocks by body, STAT_TR_PATHS)
		if (tid < 20 && wgStats[tid]) atomicAdd(&p.G.stats[(tid == 2 || tid == 3) ? (int)STAT_TR_PATHS + tid - 2 : tid], wgStats[tid]);
		// full runs: the material blocks by body (vx_material_path_counts).  Which body is the launch's (plan.matMode), so the
		// count is the length of the queue's material segment, added once - a counter per item would be kept by every workgroup
		// (in place the segment is not part of the queue; its blocks count as replayed all the same: left in their slots)
		if (!DIRTY && blockIdx.x == 0 && tid == 20 && matTotal) atomicAdd(&p.G.stats[STAT_MAT_PATHS + ((MAP && plan.matMode >= 2u) ? 1 : 0)], matTotal);
	}
	if (MAP && main_layout_kept()) { // (uniform over the launch)
		// (everything this needs is read here, from the kernarg segment: nothing of it is carried through the kernel)
		const MainKernargs& ka = main_kernargs();
		const ExecParamsDev& p = ka.p;
		const LayoutEnd& end = ka.end;
		// this workgroup's statistics, hand-overs and mesh stores have left before it counts as finished
#if defined(VX_CONSERVATIVE_SYNC)
		__threadfence();
#else
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
		__syncthreads();
		if (tid0 == 0) sh.nextItem[0] = atomicAdd(end.pub.done, 1u);
		__syncthreads();
		if (r0_uniform(sh.nextItem[0]) + 1u == gridDim.x) { // the last workgroup of the launch
#if defined(VX_CONSERVATIVE_SYNC)
			__threadfence();
#endif
			seed_words(end.seed, (u32)tid0, (u32)WG);
			if (tid0 == 0) {
				__hip_atomic_store(&p.P.cursors[CUR_V], end.cursors[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				__hip_atomic_store(&p.P.cursors[CUR_I], end.cursors[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				for (u32 l = 0; l < ka.plan.levels; ++l) __hip_atomic_store(&end.lists[l], end.totals[l], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				// blocks handed to the general passes (a zero sample where the run before met none): nobody takes them in this run
				if (TV_LOAD_THROUGH(p.G.slowCount) | TV_LOAD_THROUGH(p.G.slowCount + 1)) __hip_atomic_fetch_or(&p.G.stats[STAT_LAYOUT_MISS], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
			}
			// (the header words above are read back by other waves of this workgroup: publish_header_to_host loads past the caches)
#if defined(VX_CONSERVATIVE_SYNC)
			__threadfence();
#else
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
			__syncthreads();
			publish_header_to_host(end.pub, (u32)tid0, (u32)WG);
		}
	}
}

constexpr size_t MAIN_KERNARG_PLACES[] = { offsetof(MainKernargs, p), offsetof(MainKernargs, plan), offsetof(MainKernargs, clockStart), offsetof(MainKernargs, end) };
static_assert(KernargPlaces<decltype(k_main<false, false, true>)>::count == 4 && KernargPlaces<decltype(k_main<false, false, true>)>::are(MAIN_KERNARG_PLACES, sizeof(MainKernargs))
              && KernargPlaces<decltype(k_main<true>)>::are(MAIN_KERNARG_PLACES, sizeof(MainKernargs)) && KernargPlaces<decltype(k_main<false, true>)>::are(MAIN_KERNARG_PLACES, sizeof(MainKernargs))
              && KernargPlaces<decltype(k_main<false>)>::are(MAIN_KERNARG_PLACES, sizeof(MainKernargs)),
              "MainKernargs mirrors k_main's parameters: main_layout_kept and the end of the kernel read the kernarg segment through it");
static_assert(std::is_same<decltype(k_main<false, false, true>), void(decltype(MainKernargs::p), decltype(MainKernargs::plan), decltype(MainKernargs::clockStart), decltype(MainKernargs::end))>::value,
              "MainKernargs: a member per parameter of k_main, of the parameter's type, in the parameters' order");

} // namespace
