"""CPU tests of the checker itself: oracle/port.cpp (the restatement) against
  (a) the committed fixtures generated from the unmodified reference (tests/golden/), and
  (b) the unmodified reference on seeded inputs: run live (oracle/_ref) where it could be built, and through the digests
      of its results stored in tests/golden/reference_digests.json (tests/reference_cases.py) everywhere.
Everything is compared bit-for-bit (the reference build and the port are both strict IEEE fp32)."""
import os
import subprocess

import numpy as np
import pytest

import fields
import reference_cases
import vxo
from golden_io import Golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def port():
    if not os.path.exists(vxo.PORT_SO):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "port"])
    return vxo.load_port()


@pytest.fixture(scope="module")
def ref():
    """The unmodified reference library, or None where it could not be built (its stored results stand in for it)."""
    return vxo.load_ref()


def assert_same(a, b):
    ok, msg = fields.surface_equal(a, b)
    assert ok, msg


def test_known_answer_hash_sphere64(port):
    """64^3 ball r=0.35N -> index hash 473e8b8c4d4f3c9d, counts and stats."""
    g = port.grid_from_float(vxo.sphere_field(64))
    s = port.execute(g)
    lv = s.all_levels()
    assert [l.totals() for l in lv] == [(32, 12024, 56904, 0, 0), (8, 2952, 14424, 1680, 4896), (1, 582, 3480, 0, 0)]
    assert list(s.stats()[:4]) == [73, 286528, 12480, 0]
    assert "%016x" % vxo.index_hash(lv) == "473e8b8c4d4f3c9d"


@pytest.mark.parametrize("name", ["sphere64", "terrain32_mat", "noise64_fullrange_mat"])
def test_port_matches_golden(port, name):
    gold = Golden(name)
    g = port.grid_from_dense(gold.dist, gold.mat, gold.blend)
    assert np.array_equal(g.block_flags(), gold.flags)
    assert g.memory_size() == int(gold["memory_size"][0])
    s = port.execute(g, threads=4)
    assert_same(s.all_levels(), gold.levels)
    assert np.array_equal(s.stats(), gold.stats)
    assert s.cache_bytes() == int(gold["cache_bytes"][0])


def test_port_quantisation_golden(port):
    z = np.load(os.path.join(ROOT, "tests", "golden", "quantize16.npz"))
    g = port.grid_from_float(np.ascontiguousarray(z["values"]))
    assert np.array_equal(g.read_dense()[0], z["dist"])


def test_port_carve_modify_golden(port):
    gold = Golden("terrain64_carve_modify")
    g = port.grid_from_dense(gold["pre_dist"], gold["pre_mat"], gold["pre_blend"])
    s = port.execute(g)
    mn, mx = g.inject_ball(gold["inject_pos"], gold["inject_ext"], float(gold["inject_radius"][0]), 2)
    assert np.array_equal(mn, gold["box_min"]) and np.array_equal(mx, gold["box_max"])
    d, m, b = g.read_dense()
    assert np.array_equal(d, gold.dist) and np.array_equal(m, gold.mat) and np.array_equal(b, gold.blend)
    assert np.array_equal(g.block_flags(), gold.flags)
    ids = port.execute_modify(g, s, mn, mx)
    assert np.array_equal(ids, gold["modified_ids"])
    assert_same(s.all_levels(), gold.levels)
    assert np.array_equal(s.stats(), gold.stats)


def test_port_thread_count_independent(port):
    gold = Golden("terrain32_mat")
    g = port.grid_from_dense(gold.dist, gold.mat, gold.blend)
    assert_same(port.execute(g, threads=1).all_levels(), port.execute(g, threads=8).all_levels())


def test_rle_empty_flag_edge_cases(port):
    """BF_Empty (VoxelGrid.cpp:622-667): uniform strict sign AND compressible; an all-zero block is NOT empty
    (the 255-run split multiplies 0*0), nor is a same-sign block whose run count overflows the codec."""
    n = 32
    d = np.full((n, n, n), 4, np.int8)
    d[:16, :16, :16] = 0            # block 0: all zero
    d[:16, :16, 16:] = -3           # block 1: uniform negative -> empty
    blk = np.tile(np.array([1, 2], np.int8), 2048).reshape(16, 16, 16)
    d[:16, 16:, :16] = blk          # block 2: same sign but 4096 runs -> stored raw -> not empty
    g = port.grid_from_dense(np.ascontiguousarray(d))
    fl = g.block_flags()
    assert fl[0] == 0 and fl[1] == 1 and fl[2] == 0 and fl[3] == 1


# ---- the port against the unmodified reference: live where oracle/_ref was built, its stored results everywhere else ------

def compare_with_reference(port, ref, case):
    """The port's results in one of tests/reference_cases.py's scenarios are the reference's, bit for bit: compared item by
    item with the live reference where oracle/_ref exists (whose results must then also be the stored ones), and with the
    reference's stored digests (tests/golden/reference_digests.json) in any case."""
    mine = reference_cases.CASES[case](port)
    if ref is not None:
        theirs = reference_cases.CASES[case](ref)
        assert [l for l, _ in mine] == [l for l, _ in theirs]
        for (label, a), (_, b) in zip(mine, theirs):
            if isinstance(a, list):
                ok, msg = fields.surface_equal(a, b)
                assert ok, "%s: %s" % (label, msg)
            else:
                assert np.array_equal(a, b), label
        reference_cases.assert_matches_stored(case, theirs)
    reference_cases.assert_matches_stored(case, mine)


@pytest.mark.parametrize("seed", [21, 22, 23])
def test_port_vs_reference_live(port, ref, seed):
    compare_with_reference(port, ref, "live_small_%d" % seed)


def test_port_vs_reference_live_256(port, ref):
    """The same pin at a size where every reference level (5 at 256^3) has interior blocks, transition faces on three
    levels and LOD chains of length 1..4: the bench generator's terrain (what the 512^3 / 1024^3 GPU parity tests compare
    the port with) and a full-range field (LOD chains that end on voxels, degenerate triangles)."""
    compare_with_reference(port, ref, "live_256")


def test_port_vs_reference_edit_and_pack(port, ref):
    compare_with_reference(port, ref, "edit_and_pack")


def test_port_heightmap_constructor_matches_reference(port, ref):
    """Grid::Create(w, heightmap): restatement == reference (dense data, flags, file bytes)."""
    compare_with_reference(port, ref, "heightmap")


@pytest.mark.parametrize("case", ["terrain_41_32", "terrain_42_64"])
def test_port_vs_reference_gpu_parity_inputs(port, ref, case):
    """The terrains tests/test_gpu_parity.py::test_hip_vs_oracle_terrain polygonizes: the port it compares the HIP path with
    gives the reference's bytes for them."""
    compare_with_reference(port, ref, case)


def test_port_vs_reference_odd_sizes(port, ref):
    """Edges 16, 48, 80, 112, 208 (tests/grid_sizes.py): coarse levels that cover only a prefix of each axis, a band meshed
    by finer levels alone, transition faces toward a level that stops short - every level and the statistics."""
    compare_with_reference(port, ref, "odd_sizes")


@pytest.mark.parametrize("n", [80, 208])
def test_port_vs_reference_odd_edits(port, ref, n):
    """Brushes in the band the coarsest levels leave uncovered (the incremental Execute floors and clamps its dirty box per
    level): boxes, modified ids, levels and statistics after each, then the grid file and a full Execute."""
    compare_with_reference(port, ref, "odd_edits_%d" % n)


def test_port_heightmap_constructor_odd_size(port, ref):
    compare_with_reference(port, ref, "odd_heightmap")
