"""The premises of tests/index_keep_fields.py on the CPU, so that a failure of tests/test_gpu_index_keep.py on the device is never a
broken premise: every block of every level within the first capacity class (steady_fields.per_level), no block handed to the
general passes (test_gpu_layout.hands_on), and - from the oracle - one level-0 block whose mesh needs more than one descriptor
chunk.  Figures of the listed seed, from numpy and the oracle: fullest block's non-trivial cells per level 482 / 112 / 26; the
level-0 block has 2 042 vertices and 1 236 triangles (two chunks of each)."""
import numpy as np

import index_keep_fields as ikf
import steady_fields as sf
import vxo
from test_gpu_layout import hands_on


def test_chunks64_stays_in_the_first_capacity_class_and_hands_nothing_on():
    d, m, b = ikf.chunks64()
    assert d.shape == m.shape == b.shape == (64, 64, 64) and d.dtype == np.int8
    assert not (d == 0).any() and not hands_on(d)
    counts = sf.per_level(d)
    assert len(counts) == sf.level_count(64) == 3
    for lvl, c in enumerate(counts):
        assert 0 < c.max() <= 640 == sf.LARGE_THRESHOLD, "level %d: fullest block has %d non-trivial cells" % (lvl, c.max())
    # the cube lies inside level-0 block (0, 0, 0): one active block per level
    assert [int((c > 0).sum()) for c in counts] == [1, 1, 1] and counts[0][0, 0, 0] > 0
    outside = d.copy()
    outside[(slice(ikf.CUBE_AT, ikf.CUBE_AT + ikf.CUBE_EDGE),) * 3] = 127
    assert (outside == 127).all() and ikf.CUBE_AT + ikf.CUBE_EDGE < 16
    cube = d[(slice(ikf.CUBE_AT, ikf.CUBE_AT + ikf.CUBE_EDGE),) * 3]
    assert (cube < 0).any() and (cube > 0).any()


def test_chunks64_has_a_block_beyond_one_descriptor_chunk():
    port = vxo.load_port()
    assert port is not None, "oracle/libvoxels_port.so missing (run __graft_entry__.build())"
    d, m, b = ikf.chunks64()
    levels = port.execute(port.grid_from_dense(d, m, b)).all_levels()
    assert len(levels) == 3 and len(levels[0].infos) == 1
    info = levels[0].infos[0]
    assert int(info["id"]) == 0
    assert int(info["n_verts"]) > ikf.F0_VDESC and int(info["n_idx"]) // 3 > ikf.F0_TDESC, (int(info["n_verts"]), int(info["n_idx"]) // 3)
    # (the levels >= 1 have a mesh each, within one chunk)
    for lv in levels[1:]:
        assert len(lv.infos) == 1 and 0 < int(lv.infos[0]["n_verts"]) <= ikf.F0_VDESC
