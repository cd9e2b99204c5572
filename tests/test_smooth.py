"""vx_grid_smooth without a GPU: the host build of voxels_amd/csrc/tv_smooth.h (tests/smooth/smooth_host.cpp) - the plain loop and
the tile pipeline of the kernels run sequentially - against the numpy statement of the header's text (tests/smooth_oracle.py),
byte for byte over the case list the GPU test runs too, and that statement against answers written out by hand."""
import numpy as np
import pytest

import smooth_oracle as so

CASES = so.cases()
F = np.float32


@pytest.fixture(scope="module")
def wanted():
    """the numpy oracle's answer per case, computed once"""
    return {name: so.apply(dist, ops) for name, dist, ops in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("kind", ["plain", "tiles"])
def test_the_host_build_equals_the_numpy_oracle(kind, case, wanted):
    name, dist, ops = case
    got = so.run(kind, dist, ops)
    assert got.rc == 0
    ok, what = got.same_as(wanted[name])
    assert ok, what


def test_the_cases_change_something(wanted):
    for name, dist, ops in CASES:
        assert wanted[name].changed > 0, name
        assert not np.array_equal(wanted[name].dist, dist), name


def all_three(dist, ops):
    out = [so.apply(dist, ops), so.run("plain", dist, ops), so.run("tiles", dist, ops)]
    for other in out[1:]:
        assert other.rc == 0
        ok, what = other.same_as(out[0])
        assert ok, what
    return out[0]


def test_a_constant_field_is_unchanged():
    for value in (-128, -3, 0, 127):
        d = np.full((16, 16, 16), value, np.int8)
        r = all_three(d, so.smooth_op(((0, 0, 0), (16, 16, 16)), strength=0.37, iterations=3))
        assert np.array_equal(r.dist, d) and r.changed == 0 and r.results["changed_voxels"][0] == 0
        assert not r.results["out_min"].any() and not r.results["out_max"].any() and not r.union_min.any() and not r.union_max.any()


def test_one_voxel_in_a_constant_field_by_hand():
    d = np.full((16, 16, 16), 127, np.int8)
    d[8, 9, 10] = -127                       # z = 8, y = 9, x = 10
    r = all_three(d, so.smooth_op(((0, 0, 0), (16, 16, 16))))
    # S = 64 * 127 - 254 k, k = the kernel weight of the offset: 8 centre, 4 face, 2 edge, 1 corner; new = rint(127 - 254 k / 64):
    # 127 - 31.75 = 95.25 -> 95, 127 - 15.875 = 111.125 -> 111, 127 - 7.9375 = 119.0625 -> 119, 127 - 3.96875 = 123.03125 -> 123
    want = np.full((16, 16, 16), 127, np.int8)
    want[7:10, 8:11, 9:12] = np.array([[[123, 119, 123], [119, 111, 119], [123, 119, 123]],
                                       [[119, 111, 119], [111, 95, 111], [119, 111, 119]],
                                       [[123, 119, 123], [119, 111, 119], [123, 119, 123]]], np.int8)
    assert np.array_equal(r.dist, want)
    assert r.changed == 27 and r.results["changed_voxels"][0] == 27
    # output order (x, z, y): x 9..11, z 7..9, y 8..10 -> [a, b + 1]
    assert r.results["out_min"][0].tolist() == [9.0, 7.0, 8.0] and r.results["out_max"][0].tolist() == [12.0, 10.0, 11.0]
    assert r.union_min.tolist() == [9.0, 7.0, 8.0] and r.union_max.tolist() == [12.0, 10.0, 11.0]


def test_the_grid_faces_clamp_by_hand():
    # the lone voxel in the corner (0, 0, 0): the clamp folds the neighbours beyond the faces onto it, k = (2 + 1)^3 = 27 there,
    # (2 + 1)^2 * 1 = 9 on a face neighbour, 3 on an edge neighbour, 1 on the corner neighbour
    d = np.full((16, 16, 16), 127, np.int8)
    d[0, 0, 0] = -127
    r = all_three(d, so.smooth_op(((0, 0, 0), (16, 16, 16))))
    # 127 - 254 * 27 / 64 = 19.84375 -> 20; 127 - 254 * 9 / 64 = 91.28125 -> 91; 127 - 254 * 3 / 64 = 115.09375 -> 115; 123
    assert r.dist[0, 0, 0] == 20 and r.dist[0, 0, 1] == 91 and r.dist[0, 1, 1] == 115 and r.dist[1, 1, 1] == 123
    assert r.changed == 8 and r.union_min.tolist() == [0.0, 0.0, 0.0] and r.union_max.tolist() == [2.0, 2.0, 2.0]


def test_ties_round_to_even_and_minus_zero_is_air():
    lib = so.load()
    # f = d + w (S / 64 - d): 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -0.5 -> 0 (air, not solid), -1.5 -> -2
    assert [lib.sh_value(0, s, 1.0) for s in (32, 96, 160, -32, -96)] == [0, 2, 2, 0, -2]
    assert lib.sh_value(-128, -128 * 64, 1.0) == -128 and lib.sh_value(127, 127 * 64, 1.0) == 127
    assert lib.sh_value(-128, 127 * 64, 0.5) == 0 and lib.sh_value(-128, 127 * 64, 0.0) == -128


def test_idle_ops_change_nothing():
    d = so.noise(16, 5)
    box = ((0, 0, 0), (16, 16, 16))
    for op in (so.smooth_op(box, strength=0.0, iterations=3), so.smooth_op(box, iterations=0), so.smooth_op(box, (8, 8, 8), 4.0, 0.0, 2)):
        r = all_three(d, op)
        assert np.array_equal(r.dist, d) and r.changed == 0 and not r.results["out_max"].any()
    r = all_three(d, np.zeros(0, so.SMOOTH_DTYPE))
    assert np.array_equal(r.dist, d) and r.changed == 0


def test_a_batch_equals_the_sequential_calls():
    d = so.terrain(48)[0]
    ops = so.stroke(12)
    batch = all_three(d, ops)
    cur, changed = d, 0
    for i in range(ops.size):
        one = so.run("tiles", cur, ops[i:i + 1])
        assert one.results[0].tobytes() == batch.results[i].tobytes()
        cur, changed = one.dist, changed + one.changed
    assert np.array_equal(cur, batch.dist) and changed == batch.changed


def test_the_order_of_overlapping_ops_matters():
    d = so.noise(48, 7)
    a = so.smooth_op(((4, 4, 4), (30, 30, 30)))
    b = so.smooth_op(((20, 20, 20), (44, 44, 44)), strength=0.37, iterations=2)
    ab, ba = all_three(d, so.stack([a, b])), all_three(d, so.stack([b, a]))
    assert not np.array_equal(ab.dist, ba.dist)
    # outside the overlap grown by the reach of the second op's reads, the order cannot matter
    same = ab.dist == ba.dist
    assert same[:17].all() and same[33:].all()


def test_iterations_read_the_previous_iteration_inside_and_the_grid_outside():
    d = so.noise(48, 8)
    once = so.smooth_op(so.UNALIGNED, strength=0.37)
    three = all_three(d, so.smooth_op(so.UNALIGNED, strength=0.37, iterations=3))
    cur = d
    for _ in range(3):
        cur = so.run("plain", cur, once).dist
    assert np.array_equal(cur, three.dist)
    lo, hi = so.UNALIGNED
    outside = np.ones(d.shape, bool)
    outside[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = False
    assert np.array_equal(three.dist[outside], d[outside])


def test_smooth_weight_on_random_inputs():
    rng = np.random.default_rng(11)
    count = 100000
    v = rng.integers(0, 2048, (count, 3)).astype(np.uint32)
    center = (rng.random((count, 3)) * 2200 - 100).astype(F)
    radius = (rng.random(count) * 3000 + 0.01).astype(F)
    radius[::17] = 0
    radius[1::17] = (rng.random(radius[1::17].size) * 4 + 0.01).astype(F)   # small balls: many weights clamp to 0
    strength = rng.random(count).astype(F)
    strength[::23] = 1
    got = np.zeros(count, F)
    so.load().sh_weight(count, so._ptr(v), so._ptr(center), so._ptr(radius), so._ptr(strength), so._ptr(got))
    p = v.astype(F) - center
    r = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    q = F(1.0) - r / np.where(radius == 0, F(1), radius)
    want = np.where(radius == 0, strength, strength * np.where(q > 0, q, F(0)))
    assert want.dtype == F and got.tobytes() == want.tobytes()
    assert (want == 0).sum() > 1000 and ((want > 0) & (want < strength)).sum() > 10000


def test_invalid_ops_are_refused_by_the_host_build_too():
    d = so.noise(16, 9)
    box = ((0, 0, 0), (16, 16, 16))
    bad = [so.smooth_op(((4, 4, 4), (4, 8, 8))), so.smooth_op(((4, 4, 4), (8, 8, 17))), so.smooth_op(box, (np.nan, 0, 0), 1.0),
           so.smooth_op(box, radius=np.inf), so.smooth_op(box, radius=-1.0), so.smooth_op(box, strength=1.5), so.smooth_op(box, strength=-0.1),
           so.smooth_op(box, strength=np.nan), so.smooth_op(box, iterations=65)]
    for op in bad:
        for kind in ("plain", "tiles"):
            r = so.run(kind, d, so.stack([so.smooth_op(box), op]))
            assert r.rc == -1 and np.array_equal(r.dist, d)
