"""The premises of tests/steady_fields.py in numpy, on the CPU, so that a failure of tests/test_gpu_steady.py or
tests/test_gpu_steady_queries.py on the device is never a broken premise: per field the count of exact zeros, whether a meshed
block stages one (test_gpu_layout.hands_on), the fullest block's non-trivial cell count on EVERY level against LARGE_THRESHOLD
(a block beyond it sends the context's full runs to the chain of launches, whatever the level), and an active block on every
level.  The figures of the listed seeds stand in steady_fields.py; asserted here are the conditions."""
import numpy as np
import pytest

import steady_fields as sf
from test_gpu_layout import hands_on

SURFACE = sf.NOZERO + ("gentle64_one_zero_staged", "gentle64_one_zero_unstaged") + sf.PLANES + ("plane64_16.0",)


def test_every_field_is_listed():
    assert set(sf.FIELDS) == set(SURFACE) | set(sf.NO_SURFACE) | {"terrain16"}


@pytest.mark.parametrize("name", SURFACE)
def test_premises_of_the_fields_with_a_surface(name):
    d, m, b, kept = sf.make(name)
    n = d.shape[0]
    assert d.dtype == np.int8 and m.dtype == np.uint8 and b.dtype == np.uint8 and d.shape == m.shape == b.shape == (n, n, n)
    zeros = int((d == 0).sum())
    want_zeros = {"gentle64_one_zero_staged": 1, "gentle64_one_zero_unstaged": 1, "plane64_16.0": 64 * 64}.get(name, 0)
    assert zeros == want_zeros
    handed = hands_on(d)
    assert handed == (name in ("gentle64_one_zero_staged", "plane64_16.0"))
    assert kept == (sf.KEPT_TWO if handed else sf.KEPT_ONE)
    counts = sf.per_level(d)
    assert len(counts) == sf.level_count(n) == {48: 2, 64: 3, 80: 3, 128: 4}[n]
    for lvl, c in enumerate(counts):
        assert c.shape == ((n >> 4) >> lvl,) * 3
        assert 0 < c.max() <= sf.LARGE_THRESHOLD, "%s, level %d: fullest block has %d non-trivial cells" % (name, lvl, c.max())
        assert (c > 0).sum() >= 1
    # (level 0 by the restatement the cell map is tested against)
    assert np.array_equal(counts[0], sf.cellmap.numpy_cell_map(d)[1])
    assert len(np.unique(m)) > 1 and len(np.unique(b)) > 100, "the votes are trivial"


@pytest.mark.parametrize("name", sf.NOZERO)
def test_zero_free_noise_covers_what_it_is_listed_for(name):
    d = sf.make(name)[0]
    n = d.shape[0]
    counts = sf.per_level(d)
    assert (counts[0] > 0).sum() > 8 and (counts[-1] > 0).sum() == 1
    if name == "gentle64_nozero":
        # every transition face: the level-1 blocks (2 per edge, all on the grid's boundary) are active in both halves of every axis
        act = counts[1] > 0
        assert all(act.take(i, axis=a).any() for a in range(3) for i in (0, 1))
    if n in (48, 80):
        assert (n >> 4) % 2 == 1  # the last level-0 layer of every axis has no ancestor: level 1 covers a prefix
        last = (n >> 4) - 1
        assert all((counts[0].take(last, axis=a) > 0).any() for a in range(3)), "no active block in a layer without ancestors"
    if name == "gentle128_nozero":
        assert len(counts) == 4 and (counts[0] > 0).sum() > 100


def test_one_zero_fields_differ_from_the_zero_free_one_in_one_sample():
    base = sf.make("gentle64_nozero")[0]
    for name, at in (("gentle64_one_zero_staged", sf.ZERO_STAGED), ("gentle64_one_zero_unstaged", sf.ZERO_UNSTAGED)):
        d = sf.make(name)[0]
        where = np.argwhere(d != base)
        assert len(where) == 1 and tuple(where[0]) == at and d[at] == 0 and base[at] == 1
    assert hands_on(sf.make("gentle64_one_zero_staged")[0]) and not hands_on(sf.make("gentle64_one_zero_unstaged")[0])


@pytest.mark.parametrize("name", sf.PLANES + ("plane64_16.0",))
def test_planes_have_256_cells_in_every_active_block(name):
    d = sf.make(name)[0]
    assert (d == d[:, :1, :1]).all(), "not a function of z alone"
    for lvl, c in enumerate(sf.per_level(d)):
        assert set(np.unique(c).tolist()) <= {0, 256}, (name, lvl)
        assert (c > 0).sum() == ((64 >> 4) >> lvl) ** 2  # one layer of blocks


@pytest.mark.parametrize("name", sf.NO_SURFACE)
def test_fields_without_a_surface(name):
    d, _, _, kept = sf.make(name)
    assert (d == (127 if name == "empty64" else -127)).all() and not hands_on(d)
    counts = sf.per_level(d)
    assert len(counts) == 3 and all(not c.any() for c in counts)
    assert kept == sf.KEPT_ONE  # (steady_fields.py says why)


def test_single_block_grid_has_one_level():
    d, m, b, kept = sf.make("terrain16")
    assert d.shape == (16, 16, 16) and sf.level_count(16) == 1 and len(sf.per_level(d)) == 1
    assert sf.per_level(d)[0].max() > 0
    assert kept == sf.HANDS_OUT  # (no single-stream run on one level: steady_fields.py)
