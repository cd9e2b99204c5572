"""vx_grid_walk_field without a GPU: the Dijkstra oracle of tests/walk/walk_host.cpp against answers written by hand, against a
brute-force Bellman-Ford in numpy and against the invariants of the definition; then the tile pipeline of
voxels_amd/csrc/tv_walk.h, run sequentially with its sweep loop, against that oracle byte for byte on the shared case list.
tests/test_gpu_walk.py runs the same list on the device."""
import numpy as np
import pytest

import walk_oracle as wo

CASES = wo.cases()
IDS = [c[0] for c in CASES]
U = wo.WALK_UNREACHED
INF = np.int64(1) << 40

_oracle = {}


def oracle(k):
    """the oracle's result of case k, computed once"""
    if k not in _oracle:
        _, dist, kw = CASES[k]
        _oracle[k] = wo.run("oracle", dist, **kw)
        assert _oracle[k].rc == 0
    return _oracle[k]


def params(kw):
    p = dict(clearance=2, step_up=1, step_down=1, cost_axial=10, cost_diagonal=14, cost_climb=0, max_cost=1 << 30)
    p.update({k: v for k, v in kw.items() if k in p})
    return p


def shifted(a, dx, dy, dz, fill):
    """b[z, y, x] = a[z + dz, y + dy, x + dx], `fill` where that lies outside"""
    b = np.full_like(a, fill)
    nz, ny, nx = a.shape

    def cut(d, n):
        return (slice(max(0, -d), min(n, n - d)), slice(max(0, d), min(n, n + d)))
    (tz, sz), (ty, sy), (tx, sx) = cut(dz, nz), cut(dy, ny), cut(dx, nx)
    b[tz, ty, tx] = a[sz, sy, sx]
    return b


def region_standable(dist, box, clearance):
    n = dist.shape[0]
    lo, hi = ((0, 0, 0), (n, n, n)) if box is None else box
    return wo.standable_numpy(dist, clearance)[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]], lo


def moves(S, p):
    """the moves of the definition on the region's standable cells S: (code, weight, dx, dy, dz, the cells that have the move)"""
    has = np.zeros_like(S)   # a standable in-region cell of the same column within the step range
    for dz in range(-p["step_down"], p["step_up"] + 1):
        has |= shifted(S, 0, 0, dz, False)
    for dz in range(-p["step_down"], p["step_up"] + 1):
        for o in range(8):
            dx, dy = wo.DX[o], wo.DY[o]
            exists = S & shifted(S, dx, dy, dz, False)
            if o >= 4:
                if not p["cost_diagonal"]:
                    continue
                exists &= shifted(has, dx, 0, 0, False) & shifted(has, 0, dy, 0, False)
            yield o | ((dz + 4) << 3), (p["cost_axial"] if o < 4 else p["cost_diagonal"]) + abs(dz) * p["cost_climb"], dx, dy, dz, exists


def used_goal_costs(S, lo, kw, p):
    """per region cell the least cost of a used goal, INF where there is none"""
    g = wo.walk_goals(kw.get("goals", ()))
    c = np.full(S.shape, INF, np.int64)
    for x, y, z, cost in zip(g["x"].tolist(), g["y"].tolist(), g["z"].tolist(), g["cost"].tolist()):
        i = (z - lo[2], y - lo[1], x - lo[0])
        if all(0 <= a < b for a, b in zip(i, S.shape)) and S[i] and cost <= p["max_cost"]:
            c[i] = min(c[i], cost)
    return c


def bellman_ford(dist, kw):
    p = params(kw)
    S, lo = region_standable(dist, kw.get("box"), p["clearance"])
    F = used_goal_costs(S, lo, kw, p)
    mv = list(moves(S, p))
    for _ in range(S.size + 2):
        new = F.copy()
        for _, w, dx, dy, dz, exists in mv:
            new = np.minimum(new, np.where(exists, shifted(F, dx, dy, dz, INF) + w, INF))
        if np.array_equal(new, F):
            break
        F = new
    # no limit while relaxing, the limit at the end: the header's claim that dropping candidates above max_cost is exact
    return np.where(F <= p["max_cost"], F, U).astype(np.uint32)


# ---- the oracle against answers written by hand ----

def test_flat_floor_four_neighbours_by_hand():
    r = oracle(IDS.index("flat floor 4-neighbour"))
    z, y, x = np.indices((32, 32, 32))
    want = np.where(z == 8, 10 * (abs(x - 5) + abs(y - 7)), U).astype(np.uint32)
    assert np.array_equal(r.field, want)
    # the least code among the moves towards the goal: -x is 1, +x is 0, +y is 2, -y is 3; dz = 0 -> | 4 << 3
    code = np.where(x < 5, 0, np.where(x > 5, 1, np.where(y < 7, 2, 3))) | 32
    code = np.where((x == 5) & (y == 7), 0xFE, code)
    assert np.array_equal(r.dirs, np.where(z == 8, code, 0xFF).astype(np.uint8))
    c = r.counts
    assert (c["standable"], c["reached"], c["goals_used"], c["goals_ignored"], c["max_distance"]) == (1024, 1024, 1, 0, 10 * (26 + 24))


def test_flat_floor_eight_neighbours_by_hand():
    r = oracle(IDS.index("flat floor 8-neighbour"))
    z, y, x = np.indices((32, 32, 32))
    a, b = abs(x - 5), abs(y - 7)
    want = np.where(z == 8, 14 * np.minimum(a, b) + 10 * abs(a - b), U).astype(np.uint32)
    assert np.array_equal(r.field, want)
    f, d = r.field[8], r.dirs[8]
    assert f[7, 5] == 0 and d[7, 5] == 0xFE
    assert f[9, 8] == 14 * 2 + 10 and d[9, 8] == 1 | 32     # 3 across, 2 up: the axial step -x (code 1) is as good as the diagonal
    assert f[10, 8] == 14 * 3 and d[10, 8] == 7 | 32        # on the diagonal only (-1, -1) will do
    assert f[4, 2] == 14 * 3 and d[4, 2] == 4 | 32          # (+1, +1)
    assert f[7, 0] == 50 and d[7, 0] == 0 | 32
    assert r.counts["max_distance"] == 14 * 24 + 10 * 2


def test_range_limit_by_hand():
    on, below = oracle(IDS.index("max_cost on a cell's distance")), oracle(IDS.index("max_cost one below a cell's distance"))
    assert on.field[8, 7, 10] == 50 and on.dirs[8, 7, 10] == 1 | 32 and on.counts["max_distance"] == 50
    assert below.field[8, 7, 10] == U and below.dirs[8, 7, 10] == 0xFF and below.counts["max_distance"] == 40
    # the cells within 5 (4) steps of the goal on an unbounded floor side: a diamond cut by the grid's edge at x = 0
    diamond = lambda k: sum(1 for x in range(32) for y in range(32) if abs(x - 5) + abs(y - 7) <= k)
    assert on.counts["reached"] == diamond(5) and below.counts["reached"] == diamond(4)
    zero = oracle(IDS.index("max_cost 0"))
    assert zero.counts["reached"] == 1 and zero.field[8, 7, 5] == 0 and zero.dirs[8, 7, 5] == 0xFE


def test_goals_by_hand():
    r = oracle(IDS.index("goals: costs, duplicates, ignored ones"))
    c = r.counts
    assert (c["goals_used"], c["goals_ignored"]) == (4, 4)
    f = r.field[8 - 4]     # the box starts at (2, 2, 4)
    assert f[7 - 2, 5 - 2] == 0 and f[20 - 2, 20 - 2] == 20
    assert f[20 - 2, 19 - 2] == 30 and r.dirs[8 - 4, 20 - 2, 19 - 2] == 0 | 32
    none = oracle(IDS.index("goals: none used"))
    assert (none.counts["goals_used"], none.counts["goals_ignored"], none.counts["reached"], none.counts["max_distance"]) == (0, 2, 0, 0)
    assert (none.field == U).all() and (none.dirs == 0xFF).all() and none.counts["standable"] == 1024
    assert oracle(IDS.index("goals: none given")).counts["reached"] == 0


def test_region_borders_by_hand():
    assert oracle(IDS.index("floor below lo.z")).counts["standable"] == 1024
    assert oracle(IDS.index("clearance reaches above hi.z, free")).counts["reached"] == 1024
    blocked = oracle(IDS.index("clearance reaches above hi.z, blocked"))
    assert blocked.counts["standable"] == 0 and blocked.counts["goals_ignored"] == 1
    assert oracle(IDS.index("clearance reaches above z = n")).counts["reached"] == 1024
    one = oracle(IDS.index("one-voxel region"))
    assert one.field.shape == (1, 1, 1) and one.field[0, 0, 0] == 9 and one.dirs[0, 0, 0] == 0xFE and one.counts["max_distance"] == 9
    assert oracle(IDS.index("region one voxel thick in x")).counts["max_distance"] == 10 * 28


def test_cliff_and_corner_by_hand():
    down, top = oracle(IDS.index("cliff, goal below")), oracle(IDS.index("cliff, goal on top"))
    assert down.counts["reached"] == 1024            # the plateau walks off the cliff
    assert down.field[12, 16, 15] == 14 * 10 + (10 + 3 * 2) and down.dirs[12, 16, 15] == 0 | ((-3 + 4) << 3)
    assert top.counts["reached"] == 16 * 32          # nobody climbs three
    assert top.field[9, 16, 16] == U
    diag, axial = oracle(IDS.index("wall corner at a tile corner")), oracle(IDS.index("wall corner at a tile corner, no diagonals"))
    # (15, 15) next to the wall's end at (16, 15): the way round is (15, 16) then (16, 16), never the diagonal
    assert diag.dirs[8, 15, 15] == 2 | 32 and diag.field[8, 15, 15] == diag.field[8, 16, 15] + 10
    assert diag.field[8, 16, 15] == diag.field[8, 16, 16] + 10
    assert diag.field[8, 15, 16] == U and diag.counts["standable"] == 1024 - 16
    assert axial.field[8, 15, 15] == 10 * (1 + 5 + 6)   # up to y = 16, across to x = 20, down to y = 10


def test_bridge_by_hand():
    r = oracle(IDS.index("bridge over a floor"))
    assert r.field[6, 16, 16] == 0 and r.field[14, 16, 16] != U and r.field[14, 16, 16] > 0
    assert r.field[10, 16, 16] == U


# ---- the oracle against brute force and against the definition's invariants ----

@pytest.mark.parametrize("k", [k for k, c in enumerate(CASES) if c[1].shape[0] == 32], ids=[c[0] for c in CASES if c[1].shape[0] == 32])
def test_the_oracle_equals_bellman_ford(k):
    _, dist, kw = CASES[k]
    assert np.array_equal(oracle(k).field, bellman_ford(dist, kw))


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_invariants_of_the_definition(k):
    _, dist, kw = CASES[k]
    p = params(kw)
    r = oracle(k)
    S, lo = region_standable(dist, kw.get("box"), p["clearance"])
    F = np.where(r.field == U, INF, r.field.astype(np.int64))
    goal = used_goal_costs(S, lo, kw, p)
    best = np.full(S.shape, INF, np.int64)
    least = np.full(S.shape, 0xFE, np.int64)
    for code, w, dx, dy, dz, exists in sorted(moves(S, p), key=lambda m: m[0]):
        cand = np.where(exists, shifted(F, dx, dy, dz, INF) + w, INF)
        better = cand < best
        best = np.where(better, cand, best)
        least = np.where(better, code, least)
    reached = r.field != U
    assert not (reached & ~S).any() and (F[reached] <= p["max_cost"]).all()
    assert (best[reached] >= F[reached]).all()                      # no move gives less
    own = reached & (best > F)                                      # a goal that is its own best
    assert (goal[own] == F[own]).all() and (r.dirs[own] == 0xFE).all()
    walk = reached & (best == F)
    assert (goal[walk] >= F[walk]).all() and np.array_equal(r.dirs[walk], least[walk].astype(np.uint8))   # the least such code
    lost = S & ~reached
    assert (np.minimum(best, goal)[lost] > p["max_cost"]).all() and (r.dirs[~reached] == 0xFF).all()
    c = r.counts
    assert c["standable"] == S.sum() and c["reached"] == reached.sum() and c["max_distance"] == (F[reached].max() if reached.any() else 0)
    g = wo.walk_goals(kw.get("goals", ()))
    assert c["goals_used"] + c["goals_ignored"] == g.size


# ---- the sequential tile pipeline against the oracle ----

@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_the_tile_pipeline_equals_the_oracle(k):
    _, dist, kw = CASES[k]
    got = wo.run("emulate", dist, **kw)
    ok, what = got.same_as(oracle(k))
    assert ok, what
    assert got.counts["sweeps"] <= got.counts["standable"] + 2


def test_the_serpentine_needs_many_sweeps():
    # the cheapest walk re-enters the same tiles again and again: one sweep per tile would stop early
    k = IDS.index("serpentine 48")
    assert wo.run("emulate", CASES[k][1], **CASES[k][2]).counts["sweeps"] > 9 and oracle(k).counts["reached"] == oracle(k).counts["standable"]


BAD = [dict(box=((4, 4, 4), (4, 8, 8))), dict(box=((4, 4, 4), (8, 8, 33))), dict(box=((9, 4, 4), (8, 8, 8))), dict(clearance=0), dict(clearance=33),
       dict(step_up=5), dict(step_down=5), dict(cost_axial=0), dict(cost_axial=65536), dict(cost_diagonal=65536), dict(cost_climb=65536),
       dict(max_cost=(1 << 30) + 1)]


@pytest.mark.parametrize("kind", ["oracle", "emulate"])
def test_argument_checks_of_the_host_entries(kind):
    flat = CASES[0][1]
    for kw in BAD:
        r = wo.run(kind, flat, goals=[(5, 7, 8)], **kw)
        assert r.rc == -1, kw
        assert (r.field == 0xDEADBEEF).all() and (r.dirs == 0xDD).all()
    fn = getattr(wo.load(), "wh_" + kind)
    q, g = wo.walk_query(), wo.walk_goals([(5, 7, 8)])
    counts = np.zeros(1, wo.WALK_COUNTS_DTYPE)
    field = np.zeros(32 ** 3 + 4, np.uint32)
    args = lambda **o: [o.get("q", q.ctypes.data), o.get("g", g.ctypes.data), o.get("n", 1), o.get("f", field.ctypes.data), None, o.get("c", counts.ctypes.data)]
    assert fn(32, flat.ctypes.data, *args()) == 0 and counts["reached"][0] == 1024
    assert fn(32, flat.ctypes.data, *args(q=None)) == -1 and fn(32, flat.ctypes.data, *args(c=None)) == -1
    assert fn(32, flat.ctypes.data, *args(g=None)) == -1 and fn(32, flat.ctypes.data, *args(n=wo.WALK_MAX_GOALS + 1)) == -1
    assert fn(32, flat.ctypes.data, *args(g=None, n=0)) == 0
    assert fn(32, flat.ctypes.data, *args(f=field.ctypes.data + 4)) == -1
    assert fn(32, flat.ctypes.data, *args(f=None)) == 0 and counts["reached"][0] == 1024   # both outputs NULL: the counts all the same
    flagged = q.copy()
    flagged["flags"] = 1
    assert fn(32, flat.ctypes.data, *args(q=flagged.ctypes.data)) == -1
