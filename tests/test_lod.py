"""LOD selection (include/voxels_hip.h, "LOD selection") without a GPU: the invariants of the numpy oracle
(tests/lod_oracle.py) over grid sizes, level counts, cameras and ranges; the binding's dtypes against the header; the
library's exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lod_oracle import Selection, face_axis, ref_levels, select

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [16, 32, 48, 80, 112, 208, 256, 336, 1008]


def cameras(n, seed, count):
    """inside, outside, on block boundaries and on coarse node corners"""
    rs = np.random.RandomState(seed)
    cams = [rs.uniform(0, n, 3), rs.uniform(-n, 2 * n, 3), (rs.randint(0, n // 16 + 1, 3) * 16).astype(np.float32),
            np.float32([n / 2, n / 2, n / 2]), np.float32([-1e30, 5, 5]), np.float32([0, 0, 0])]
    while len(cams) < count:
        cams.append(rs.uniform(-n / 4, n * 1.25, 3))
    return [np.asarray(c, np.float32) for c in cams[:count]]


def range_sets(n, cam):
    base = np.float32([4.0 * 16 * (1 << L) for L in range(16)])
    unbalanced = base.copy()
    unbalanced[1], unbalanced[2] = 3.0 * n, 0.0
    deep = np.zeros(16, np.float32)
    deep[1] = 40.0                       # only level 1 split by distance: balance has to open everything above
    negative = np.full(16, -5.0, np.float32)
    # an exact tie: ranges[1] = the distance of some level-1 node (d^2 == r^2 does not split)
    tie = base.copy()
    d = np.abs(np.floor(cam / 32) * 32 - cam)
    tie[1] = np.float32(np.sqrt(np.float32(d[0] * d[0])))
    return [base, unbalanced, deep, negative, tie]


def check_invariants(sel, label):
    c0, T, R = sel.c0, sel.T, sel.R
    # leaves partition the grid
    assert (sel.cover == 1).all(), label
    assert sel.leaf_volume() == c0 ** 3, label
    lm = sel.level_map
    # face-adjacent leaves differ by at most 1; a level-(R-1) leaf touches no finer leaf
    for ax in range(3):
        a, b = np.moveaxis(lm, ax, 0)[:-1], np.moveaxis(lm, ax, 0)[1:]
        assert (np.abs(a - b) <= 1).all(), label
        if T == R - 1:
            assert not (((a == R - 1) & (b < R - 1)) | ((b == R - 1) & (a < R - 1))).any(), label
    for L in range(1, T + 1):
        o = sel.open[L]
        # minimality: an opened node with no opened child is forced by rule 1 or rule 3
        if L >= 2:
            m = sel.open[L - 1][:2 * sel.cnt[L], :2 * sel.cnt[L], :2 * sel.cnt[L]]
            child_open = m.reshape(sel.cnt[L], 2, sel.cnt[L], 2, sel.cnt[L], 2).any((1, 3, 5))
        else:
            child_open = np.zeros_like(o)
        g = 1 if L == R - 1 else 2
        rule3 = sel.active[L] & (sel.face_min[L].min(0) <= L - g)
        bare = o & ~child_open
        assert not (bare & ~sel.rule1[L] & ~rule3).any(), (label, L)
    # transition bit <=> a finer neighbour, and then the whole face is level L - 1
    for L in range(T + 1):
        leaf = sel.leaf[L]
        bits = sel.transitions(L)
        for f in range(6):
            on = leaf & ((bits >> f) & 1).astype(bool)
            assert (sel.face_min[L][f][on] == L - 1).all() and (sel.face_max[L][f][on] == L - 1).all(), (label, L, f)
            off = leaf & ~on
            assert (sel.face_min[L][f][off] >= L).all(), (label, L, f)
        if L == 0 or L == R - 1:
            assert not bits[leaf].any(), (label, L)


@pytest.mark.parametrize("n", SIZES)
def test_oracle_invariants(n):
    R = ref_levels(n)
    count = 3 if n >= 1000 else 6
    for levels in range(1, R + 1):
        for k, cam in enumerate(cameras(n, n + levels, count)):
            for j, ranges in enumerate(range_sets(n, cam)):
                if n >= 1000 and j not in (0, 1, 2):
                    continue
                check_invariants(Selection(n, levels, cam, ranges), "n=%d levels=%d cam=%d ranges=%d" % (n, levels, k, j))


def test_oracle_examples():
    """Hand-checked cases: a far camera keeps the coarsest level; a camera in a corner refines down to level 0 there."""
    from voxels_amd.binding import lod_ranges
    s = Selection(256, 5, [1e6, 1e6, 1e6], lod_ranges())
    assert s.leaf_count() == 1 and s.leaf[4].all()
    s = Selection(256, 5, [1, 1, 1], lod_ranges())
    assert s.level_map[0, 0, 0] == 0 and s.level_map[-1, -1, -1] >= 2
    # odd size: the coarsest level always opens (a band touches it), band roots stay
    s = Selection(80, 3, [1e6, 1e6, 1e6], lod_ranges())
    assert s.open[2].all() and s.leaf[0][:, :, 4].all()
    # unbalanced ranges: level 1 split everywhere, nothing coarser by distance -> all leaves level 0
    r = np.zeros(16, np.float32)
    r[1] = 1e9
    s = Selection(128, 4, [0, 0, 0], r)
    assert (s.level_map == 0).all()


def test_oracle_records_from_a_table():
    from voxels_amd.binding import LISTED_BLOCK_DTYPE, lod_ranges
    n = 64
    sel = Selection(n, 3, [3.0, 70.0, 3.0], lod_ranges(2.0))
    tables = []
    for L in range(3):
        c = sel.cnt[L]
        t = np.zeros(c ** 3, LISTED_BLOCK_DTYPE)
        t["coord_id"] = np.arange(c ** 3)
        t["i_count"], t["ti_count"] = 3, 6
        tables.append(t)
    draws, regular, transition, counts = select(sel, tables)
    assert counts["records"] == counts["leaves"] == len(draws)
    assert (regular["first_instance"] == np.arange(len(draws))).all()
    assert counts["transition"] == sum(bin(int(b)).count("1") for b in draws["transitions"])
    # a frustum that keeps nothing
    draws, _, _, counts = select(sel, tables, planes=[(0, 0, 0, -1)])
    assert len(draws) == 0 and counts["culled_leaves"] == counts["meshed_leaves"] == counts["leaves"]


def test_face_order():
    assert [face_axis(f) for f in range(6)] == [(2, -1), (1, -1), (0, -1), (2, 1), (1, 1), (0, 1)]


def test_dtypes_match_the_header(tmp_path):
    from voxels_amd.binding import DRAW_INDEXED_DTYPE, LOD_COUNTS_DTYPE, LOD_DRAW_DTYPE, LOD_PARAMS_DTYPE
    src = tmp_path / "sizes.c"
    fields = {"vx_lod_params": (LOD_PARAMS_DTYPE, ["camera", "n_planes", "planes", "ranges"]),
              "vx_lod_draw": (LOD_DRAW_DTYPE, ["level", "entry", "block_id", "coord_id", "transitions", "adjacency", "reserved"]),
              "vx_draw_indexed": (DRAW_INDEXED_DTYPE, ["index_count", "instance_count", "first_index", "vertex_offset", "first_instance"]),
              "vx_lod_counts": (LOD_COUNTS_DTYPE, ["records", "regular", "transition", "leaves", "meshed_leaves", "culled_leaves",
                                                   "leaf_volume"])}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "voxels_hip.h"', "int main(void) {"]
    for s, (_, names) in fields.items():
        lines.append('printf("%%zu\\n", sizeof(%s));' % s)
        for f in names:
            lines.append('printf("%%zu\\n", offsetof(%s, %s));' % (s, f))
    lines.append("return 0; }")
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    out = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    want = []
    for dt, names in fields.values():
        want.append(dt.itemsize)
        want += [dt.fields[f][1] for f in names]
    assert out == want


def test_library_exports_lod_selection():
    from voxels_amd import build
    lib = C.CDLL(build.build_hip())
    assert hasattr(lib, "vx_lod_select") and hasattr(lib, "vx_lod_select_device")
