"""The fields of the tests of the steady-state full run (tests/test_steady_fields.py checks their premises in numpy on the CPU;
tests/test_gpu_steady.py and tests/test_gpu_steady_queries.py run them on the device): name -> (dist, mat, blend, the form the
kept runs behind the assigning run are expected to take).

The steady form - the slot plan kept, the material caches in their slots, the mesh layout kept: k_main alone - needs
  * every active block of every level within the first capacity class (LARGE_THRESHOLD non-trivial cells), or the context's
    full runs stay on the chain of launches, and
  * no block handed to the general passes (test_gpu_layout.hands_on: a meshed block that stages a sample that is exactly 0),
    or the run leaves no layout and the kept runs stay k_main | k_tail.
Both are functions of the distance field alone; per_level() restates the first for every level (the lattice of level L at
stride 2^L, coordinates clamped to the grid's last sample as in hands_on), which test_gpu_cellmap.numpy_cell_map does for
level 0 only.  (test_gpu_cellmap.gentle_field's docstring leaves the levels >= 1 of its fields to "the single-stream premise of
run_full", a check on the device; for the seeds and scales used here per_level is that check, on the CPU.)

Figures of the listed seeds, from numpy (fullest block's non-trivial cells per level / active blocks per level):
  gentle64_nozero    539 / 495 / 488          28 / 6 / 1
  gentle48_nozero    451 / 405                15 / 1
  gentle80_nozero    517 / 497 / 430          45 / 6 / 1
  gentle128_nozero   544 / 539 / 502 / 511    129 / 30 / 7 / 1
  plane64_*          256 in every active block of every level (16 / 4 / 1 of them; plane64_16.0 likewise, with zeros)
No seed or scale had to be changed."""
import numpy as np

import test_gpu_cellmap as cellmap
import test_gpu_layout as layout
import test_gpu_matstore as matstore

LARGE_THRESHOLD = cellmap.LARGE_THRESHOLD
HANDS_OUT, KEPT_ONE, KEPT_TWO = layout.HANDS_OUT, layout.KEPT_ONE, layout.KEPT_TWO


def level_count(n):
    """levels of a full run on an n^3 grid (as hands_on counts them)"""
    levels, v = 1, n >> 5
    while v:
        levels, v = levels + 1, v >> 1
    return levels


def per_level(d):
    """d: int8 [z][y][x] -> per level the non-trivial cell counts of its blocks, [bz][by][bx]: a cell is non-trivial unless its
    eight corner samples on the level's lattice agree in sign (0 counts as positive)"""
    d = np.asarray(d)
    n = d.shape[0]
    neg = d < 0
    out = []
    for lvl in range(level_count(n)):
        mult, cnt = 1 << lvl, (n >> 4) >> lvl
        at = np.minimum(np.arange(16 * cnt + 1) * mult, n - 1)
        s = neg[np.ix_(at, at, at)].astype(np.int8)
        corners = sum(s[a:a + 16 * cnt, b:b + 16 * cnt, c:c + 16 * cnt] for a in (0, 1) for b in (0, 1) for c in (0, 1))
        out.append(((corners > 0) & (corners < 8)).reshape(cnt, 16, cnt, 16, cnt, 16).sum(axis=(1, 3, 5)))
    return out


def _gentle(n, scale):
    d = cellmap.gentle_field(n, 16, scale=scale)
    zeros = np.argwhere(d == 0)
    d = d.copy()
    d[d == 0] = 1
    return d, zeros


def _gentle_nozero(n, scale):
    return (_gentle(n, scale)[0],) + matstore.mixed_materials(n, 5)


# Where gentle_field(64, 16, scale=40) is 0, [z][y][x]: the two of its zeros used below were found by a search over all of
# them - putting the first one back makes a meshed block stage it (hands_on), putting the second one back does not.
ZERO_STAGED = (0, 0, 33)
ZERO_UNSTAGED = (63, 0, 9)


def _gentle64_one_zero(at):
    d, zeros = _gentle(64, 40)
    assert any(tuple(z) == at for z in zeros), "gentle_field(64, 16, scale=40) has no 0 at %s" % (at,)
    d[at] = 0
    return (d,) + matstore.mixed_materials(64, 5)


def _plane(n, h):
    """clip((z - h) * 12): at h = 15.5, 31.5, 47.5 the sign changes between the last layer of one block and the first of the next,
    so every level-0 block holds samples of one sign, is flagged BF_Empty and is skipped (in the reference too): the surface
    is meshed on the levels >= 1 only.  At h = 16.0 layer 16 is exactly 0 and level 0 is meshed as well."""
    z = np.arange(n, dtype=np.float64)[:, None, None]
    d = np.clip((z - h) * 12, -127, 127).astype(np.int8)
    d = np.ascontiguousarray(np.broadcast_to(d, (n, n, n)))
    return (d,) + matstore.mixed_materials(n, 5)


def _constant(n, v):
    zero = np.zeros((n, n, n), np.uint8)
    return np.full((n, n, n), v, np.int8), zero, zero.copy()


def _terrain16():
    """the grid of test_gpu_parity.test_hip_single_block_grid: one block, one level"""
    import fields
    rng = np.random.RandomState(16)
    d = np.clip(np.round(fields.smooth_noise(16, 3, scale=6, amp=3.0)), -4, 4).astype(np.int8)
    return d, rng.randint(0, 3, (16, 16, 16)).astype(np.uint8), rng.randint(0, 256, (16, 16, 16)).astype(np.uint8)


# Which form do grids without an active block, and a grid of one level, take?  vx_polygonize (vx_host.inl): a run may leave the
# plan (planRun) when it is a single-stream one, it leaves the layout (layoutValid) when it was accepted with the plan valid, no
# block of the large class (HDR_LARGE), nothing handed to the general passes (HDR_SLOW) and no empty cache - and it keeps both
# when they are valid for its level count.  None of this asks for an active block; a single-stream run asks for more than one
# level (Backend::main_applies: levels > 1, and a lattice copy of level 1).  So
#   * empty64 and full64 (three levels, no active block on any: the corners of every cell agree) run like any other field: a
#     chain of launches, an assigning run that leaves a plan of no slots and a layout of empty lists, then one launch of
#     k_main per run, whose workgroups find both queues empty and whose last one publishes totals of 0 (the launch is sized
#     by the level tables' capacities, which are volumes and not 0);
#   * the 16^3 grid never takes the single-stream form: every one of its runs is the chain of launches and hands out its
#     slot.  (Its field is full of zeros and its block has 1 203 non-trivial cells, which would each keep it there as well.)
#     The same holds for any grid run with a level limit of 1.
# test_gpu_steady.py states these forms through the counters, so a wrong reading of the host code fails there, not silently.
FIELDS = {
    "gentle64_nozero": (lambda: _gentle_nozero(64, 40), KEPT_ONE),     # every transition face, non-trivial votes
    "gentle48_nozero": (lambda: _gentle_nozero(48, 40), KEPT_ONE),     # 3 blocks per edge: level 1 covers a prefix of each axis
    "gentle80_nozero": (lambda: _gentle_nozero(80, 64), KEPT_ONE),     # 5 blocks per edge
    "gentle128_nozero": (lambda: _gentle_nozero(128, 80), KEPT_ONE),   # four levels, planes from a lattice copy (mult 4)
    "gentle64_one_zero_staged": (lambda: _gentle64_one_zero(ZERO_STAGED), KEPT_TWO),
    "gentle64_one_zero_unstaged": (lambda: _gentle64_one_zero(ZERO_UNSTAGED), KEPT_ONE),
    "plane64_15.5": (lambda: _plane(64, 15.5), KEPT_ONE),              # axis-aligned planes: one case class, 256 cells a block
    "plane64_31.5": (lambda: _plane(64, 31.5), KEPT_ONE),
    "plane64_47.5": (lambda: _plane(64, 47.5), KEPT_ONE),
    "plane64_16.0": (lambda: _plane(64, 16.0), KEPT_TWO),              # the contrast: a layer of exact zeros on the surface
    "empty64": (lambda: _constant(64, 127), KEPT_ONE),
    "full64": (lambda: _constant(64, -127), KEPT_ONE),
    "terrain16": (_terrain16, HANDS_OUT),
}

NOZERO = ("gentle64_nozero", "gentle48_nozero", "gentle80_nozero", "gentle128_nozero")
PLANES = ("plane64_15.5", "plane64_31.5", "plane64_47.5")
NO_SURFACE = ("empty64", "full64")

_MADE = {}


def make(name):
    """(dist, mat, blend, kept form); built once, handed out read-only"""
    if name not in _MADE:
        d, m, b = FIELDS[name][0]()
        arrays = tuple(np.ascontiguousarray(a) for a in (d, m, b))
        for a in arrays:
            a.setflags(write=False)
        _MADE[name] = arrays + (FIELDS[name][1],)
    return _MADE[name]
