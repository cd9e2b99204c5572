"""The stamps without a GPU: the numpy statement of the header's text (tests/stamp_oracle.py) against answers written by hand, and
the host build of voxels_amd/csrc/tv_stamp.h (tests/stamp/stamp_host.cpp) - the plain loop and the kernels' pipeline with small
list capacities - against that statement, byte for byte."""
import numpy as np
import pytest

import stamp_oracle as sto
import undo_oracle as uo
from voxels_amd import binding

R, U, S, P = sto.MODES
CASES = sto.cases()


def flat_grid(n=16, d=10, m=1, b=2):
    return uo.Grid(np.full((n, n, n), d, np.int8), np.full((n, n, n), m, np.uint8), np.full((n, n, n), b, np.uint8), np.zeros((n // 16) ** 3, np.uint8))


def same_records(a, b):
    assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (a, b)


# ---- the oracle against answers written by hand -------------------------------------------------------------------------------

# the stamp    j=2: e f        (i to the right, j upwards, seen from +z)
#              j=1: c d
#              j=0: a b
# and what the grid holds at origin + (u, v), rows from v = 0 upwards, per orientation
LETTERS = np.array([[1, 2], [3, 4], [5, 6]], np.int8)   # [j, i]: a b / c d / e f
a, b, c, d, e, f = 1, 2, 3, 4, 5, 6
BY_HAND = {0: [[a, b], [c, d], [e, f]],          # as it is
           1: [[e, c, a], [f, d, b]],            # a quarter turn counter-clockwise: a goes to the +u end of row v = 0
           2: [[f, e], [d, c], [b, a]],          # a half turn
           3: [[b, d, f], [a, c, e]],            # three quarter turns
           4: [[b, a], [d, c], [f, e]],          # mirrored in x
           5: [[f, d, b], [e, c, a]],            # mirrored, then a quarter turn
           6: [[e, f], [c, d], [a, b]],          # mirrored, then a half turn = mirrored in y
           7: [[a, c, e], [b, d, f]]}            # mirrored, then three quarter turns = transposed


@pytest.mark.parametrize("orient", range(8))
def test_the_eight_orientations_of_a_2x3x1_stamp(orient):
    g = flat_grid()
    st = sto.St(LETTERS.reshape(1, 3, 2))
    results, counts = sto.paste(g, [st], [((4, 5, 6), 0, orient, R)])
    want = np.array(BY_HAND[orient], np.int8)
    assert np.array_equal(g.dist[6, 5:5 + want.shape[0], 4:4 + want.shape[1]], want)
    assert int((g.dist != 10).sum()) == 6 and int(counts["changed_voxels"]) == 6
    assert results[0]["box"]["lo"].tolist() == [4, 5, 6] and results[0]["box"]["hi"].tolist() == [4 + want.shape[1], 5 + want.shape[0], 7]
    assert sto.oriented_size(orient, (2, 3, 1)) == (want.shape[1], want.shape[0], 1)


def test_the_modes_by_hand():
    st = sto.St(np.array([[[-128, -5, 0, 5, 127]]], np.int8), np.full((1, 1, 5), 9, np.uint8), np.full((1, 1, 5), 8, np.uint8))
    for mode, dist, mat in ((R, [-128, -5, 0, 5, 127], [9, 9, 9, 9, 9]), (U, [-128, -5, 0, 3, 3], [9, 9, 9, 1, 1]),
                            (S, [127, 5, 3, 3, 3], [1, 1, 1, 1, 1]), (P, [3, 3, 3, 3, 3], [9, 9, 1, 1, 1])):
        g = flat_grid(d=3)
        sto.paste(g, [st], [((0, 0, 0), 0, 0, mode)])
        assert g.dist[0, 0, :5].tolist() == dist and g.mat[0, 0, :5].tolist() == mat and g.blend[0, 0, :5].tolist() == [8 if m == 9 else 2 for m in mat]


def test_counts_and_flags_by_hand():
    g = flat_grid(32, d=127)
    g.flags[:] = 1
    g.flags[7] = 0                                    # disagrees with the codec: block 7 is constant too
    st = sto.solid_stamp((4, 4, 4), -127)
    results, counts = sto.paste(g, [st], [((14, 2, 3), 0, 0, R), ((40, 0, 0), 0, 0, R), ((20, 20, 20), 0, 0, P)])
    assert results["touched_blocks"].tolist() == [2, 0, 1] and results[1]["box"]["hi"].tolist() == [0, 0, 0]
    assert results[0]["box"]["lo"].tolist() == [14, 2, 3] and results[0]["box"]["hi"].tolist() == [18, 6, 7]
    # the first paste carves blocks 0 and 1: no longer empty; the PAINT paste paints nothing (the stamp is solid: sd < 0 - it
    # does paint) and leaves the flag of block 7 alone
    assert g.flags.tolist() == [0, 0, 1, 1, 1, 1, 1, 0]
    assert counts["out_min"].tolist() == [14, 3, 2] and counts["out_max"].tolist() == [24, 24, 24]      # output order x, z, y
    assert (int(counts["changed_voxels"]), int(counts["changed_blocks"]), int(counts["flag_changes"]), int(counts["touched_blocks"])) == (128, 3, 2, 3)


def test_orientation_identities():
    rng = np.random.default_rng(3)
    for sx, sy in ((1, 1), (2, 3), (7, 4)):
        j, i = np.indices((sy, sx))
        for o in range(8):
            u, v = sto.oriented(o, sx, sy, i, j)
            ox, oy, _ = sto.oriented_size(o, (sx, sy, 1))
            assert u.min() == 0 and v.min() == 0 and u.max() == ox - 1 and v.max() == oy - 1
            assert len(set(zip(u.reshape(-1).tolist(), v.reshape(-1).tolist()))) == sx * sy
        # two mirrors give the identity: pasting the mirrored stamp mirrored again restores it; likewise four quarter turns
        st = sto.noise_stamp((sx, sy, 2), int(rng.integers(1000)))
        for turn, times in ((4, 2), (1, 4)):
            cur = st
            for _ in range(times):
                ox, oy, oz = sto.oriented_size(turn, cur.size)
                g = flat_grid(16)
                sto.paste(g, [cur], [((0, 0, 0), 0, turn, R)])
                cur = sto.capture(g, ((0, 0, 0), (ox, oy, oz)))
            assert np.array_equal(cur.dist, st.dist) and np.array_equal(cur.mat, st.mat) and np.array_equal(cur.blend, st.blend)


# ---- the host build against the oracle ------------------------------------------------------------------------------------------

def run_both(g0, stamps, ps, caps=((0, 0), (7, 0), (7, 5))):
    want = g0.copy()
    wres, wcounts = sto.paste(want, stamps, ps)
    runs = [(0, 0, 0)] + [(1, cap, seed) for cap, seed in caps]
    for path, cap, seed in runs:
        g = g0.copy()
        rc, res, counts = sto.host_paste(path, g, stamps, ps, cap, seed)
        assert rc == 0
        assert g.same_as(want), (path, cap, seed)
        same_records(res, wres)
        same_records(np.asarray(counts), np.asarray(wcounts))
    return want


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_build_on_the_case_list(case):
    g = case.grid()
    run_both(g, case.stamps(g), case.pastes)


def test_host_build_on_random_batches():
    g0 = sto.terrain_grid(48)
    g0.flags[::5] ^= 1        # flags that disagree with the codec: only carved blocks may change
    for seed in range(200):
        stamps, ps = sto.random_batch(48, seed + 1)
        run_both(g0, stamps, ps, caps=((7, seed + 1),))


def test_chunk_borders_inside_a_blocks_list():
    # a paste and its inverse in different chunks: the counts compare with the grid before the batch, not before the chunk
    g0 = sto.terrain_grid(48)
    src = sto.capture(g0, ((16, 16, 16), (24, 24, 24)))
    ps = [((16, 16, 16), 0, 0, R)] * 3 + [((16, 16, 16), 1, 0, R)] * 5 + [((0, 0, 0), 0, 0, P)]
    want = run_both(g0, [sto.noise_stamp((8, 8, 8), 1), src], ps, caps=((2, 0), (3, 9), (1, 0)))
    assert np.array_equal(want.dist, g0.dist)


def test_paste_box_against_the_oracle():
    lib = binding.HipLibrary().lib
    rng = np.random.default_rng(5)
    for k in range(10000):
        n = int(rng.choice([16, 48, 64, 1024, 2048]))
        size = np.array(rng.integers(1, [40, 40, 40][k % 3] if k % 7 else 2049, 3), np.uint32)
        span = 2 ** 31 if k % 11 == 0 else n + 50
        p = sto.pastes([(tuple(int(v) for v in rng.integers(-span, span, 3)), 0, int(rng.integers(8)), 0)])
        got = np.zeros(1, binding.BOX_DTYPE)
        rc = lib.vx_paste_box(p.ctypes.data, size.ctypes.data, n, got.ctypes.data)
        wrc, want = sto.paste_box(p[0], tuple(int(v) for v in size), n)
        assert rc == wrc and got[0].tobytes() == want.tobytes(), (p, size, n)
        host = np.zeros(1, binding.BOX_DTYPE)
        assert sto.load().sh_paste_box(p.ctypes.data, size.ctypes.data, n, host.ctypes.data) == wrc and host.tobytes() == got.tobytes()
    size = np.array([3, 4, 5], np.uint32)
    p = sto.pastes([((0, 0, 0), 0, 0, 0)])
    out = np.zeros(1, binding.BOX_DTYPE)
    args = (p.ctypes.data, size.ctypes.data, 48, out.ctypes.data)
    assert lib.vx_paste_box(*args) == 1
    for k in (0, 1, 3):
        assert lib.vx_paste_box(*[None if j == k else v for j, v in enumerate(args)]) == -1
    for n in (0, 8, 40, 2064):
        assert lib.vx_paste_box(args[0], args[1], n, args[3]) == -1
    assert lib.vx_paste_box(args[0], np.array([3, 0, 5], np.uint32).ctypes.data, 48, args[3]) == -1
    p["orient"] = 8
    assert lib.vx_paste_box(*args) == -1


def test_the_blocks_captured_from_paste_boxes_are_the_touched_blocks():
    for case in CASES:
        g = case.grid()
        stamps = case.stamps(g)
        boxes = binding.paste_boxes(case.pastes, [st.size for st in stamps], case.n)
        assert uo.block_set(case.n, boxes).tolist() == sto.touched_blocks(stamps, case.pastes, case.n).tolist(), case.name
        assert int(sto.paste(g, stamps, case.pastes)[1]["touched_blocks"]) == uo.block_set(case.n, boxes).size
