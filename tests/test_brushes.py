"""The host side of vx_grid_inject_brushes (no GPU): the host oracle of the GPU tests (tests/brush/brush_host.cpp) is anchored
to the unmodified reference and to the port - ball and material lists through it equal the same lists through
tests/vxo.py, one call per brush, byte for byte - the sample functions of voxels_amd/csrc/tv_brush.h are checked against
float64 numpy, and the ABI of the new entry point is checked."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import brush_oracle as bo
import fields
import vxo
from grid_sizes import ODD_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracles():
    out = [o for o in (vxo.load_ref(), vxo.load_port()) if o is not None]
    assert out, "no CPU checker was built"
    return out


def terrain(n, seed):
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    return f, m, b


def check_against_sequential(n, brushes, seed):
    f, m, b = terrain(n, seed)
    for o in oracles():
        g = o.grid_from_float(f, m, b)
        d0, m0, b0 = g.read_dense()
        got = bo.apply(d0, m0, b0, brushes)
        boxes = bo.sequential(g, brushes)
        assert np.array_equal(got.boxes, boxes), (o.kind, n, len(brushes))
        assert np.array_equal(got.pack, g.pack()), "packed file after %d brushes on %d^3 (%s)" % (len(brushes), n, o.kind)
        assert np.array_equal(got.flags, g.block_flags()), (o.kind, n, len(brushes))
        d1, m1, b1 = g.read_dense()
        assert np.array_equal(got.dist, d1) and np.array_equal(got.mat, m1) and np.array_equal(got.blend, b1)


@pytest.mark.parametrize("n", [64, 80])
@pytest.mark.parametrize("count", [1, 2, 64])
def test_ball_lists_equal_the_reference_one_call_per_brush(n, count):
    assert 80 in ODD_SIZES
    brushes = bo.anywhere_balls(n, count, seed=100 + count)
    if count == 64:
        assert set(brushes["type"].tolist()) == {0, 1, 2}
        assert (bo.apply(*[a for a in _dense(n)], brushes).touched == 0).any(), "the list holds brushes that miss the grid"
    check_against_sequential(n, brushes, seed=3)


def _dense(n):
    f, m, b = terrain(n, 3)
    return vxo.load_port().grid_from_float(f, m, b).read_dense()


@pytest.mark.parametrize("n", [64, 80])
def test_material_lists_equal_the_reference_one_call_per_brush(n):
    balls = bo.anywhere_balls(n, 24, seed=9)
    items = []
    for k, b in enumerate(balls):
        items.append(bo.material(b["position"], b["extents"], 7 + k % 5, k % 4 < 2))
        if k % 3 == 0:
            items.append(b)
    # the same material twice over the same voxels: the second call adds to / subtracts from the blend of the first
    items.append(bo.material((30.0, 30.0, 30.0), (12.0, 12.0, 12.0), 9, True))
    items.append(bo.material((31.0, 30.0, 30.0), (12.0, 12.0, 12.0), 9, True))
    items.append(bo.material((30.0, 31.0, 30.0), (12.0, 12.0, 12.0), 9, False))
    check_against_sequential(n, bo.stack(items), seed=5)


def _f64_capsule(p, a, b, r):
    pa, ba = p - a, b - a
    bb = (ba * ba).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = np.where(bb == 0, 0.0, np.clip((pa * ba).sum(axis=1) / bb, 0.0, 1.0))
    v = pa - ba * h[:, None]
    return np.sqrt((v * v).sum(axis=1)) - r


def _f64_box(p, a, r):
    q = np.abs(p) - a
    return np.sqrt((np.maximum(q, 0.0) ** 2).sum(axis=1)) + np.minimum(q.max(axis=1), 0.0) - r


def test_sample_functions_against_float64():
    """|f32 - f64| <= 64 * 2^-23 * max(1, largest coordinate or parameter magnitude of the sample): each function is a handful
    of rounded operations, each within one ulp at that magnitude.  100 000 random points in [-64, 64]^3, nothing excluded."""
    rng = np.random.RandomState(2024)
    count = 100000
    p = rng.uniform(-64, 64, (count, 3)).astype(np.float32)
    a = rng.uniform(-64, 64, (count, 3)).astype(np.float32)
    b = rng.uniform(-64, 64, (count, 3)).astype(np.float32)
    b[::7] = a[::7] + rng.uniform(-1e-3, 1e-3, (len(a[::7]), 3)).astype(np.float32)  # short segments
    half = np.abs(rng.uniform(0, 64, (count, 3))).astype(np.float32)
    r = rng.uniform(0, 32, count).astype(np.float32)
    P, A, B, H, R = (x.astype(np.float64) for x in (p, a, b, half, r))
    cases = ((bo.BRUSH_BALL, a, b, np.sqrt((P * P).sum(axis=1)) - R, np.abs(P).max(axis=1)),
             (bo.BRUSH_CAPSULE, a, b, _f64_capsule(P, A, B, R), np.maximum(np.abs(P).max(axis=1), np.maximum(np.abs(A).max(axis=1), np.abs(B).max(axis=1)))),
             (bo.BRUSH_BOX, half, b, _f64_box(P, H, R), np.maximum(np.abs(P).max(axis=1), H.max(axis=1))))
    for shape, pa, pb, want, mag in cases:
        got = bo.sample(shape, p, pa, pb, r).astype(np.float64)
        tol = 64.0 * 2.0 ** -23 * np.maximum(1.0, np.maximum(mag, R))
        err = np.abs(got - want)
        print("shape %d: largest |error| / tolerance = %.4f" % (shape, float((err / tol).max())))
        assert (err <= tol).all(), (shape, int(np.argmax(err / tol)), float((err / tol).max()))


def test_degenerate_capsule_is_the_ball_exactly():
    rng = np.random.RandomState(7)
    count = 20000
    p = rng.uniform(-64, 64, (count, 3)).astype(np.float32)
    a = rng.uniform(-64, 64, (count, 3)).astype(np.float32)
    a[::2] = 0
    r = rng.uniform(0, 32, count).astype(np.float32)
    cap = bo.sample(bo.BRUSH_CAPSULE, p, a, a, r)
    ball = bo.sample(bo.BRUSH_BALL, (p - a).astype(np.float32), a, a, r)
    assert np.array_equal(cap, ball)


def test_a_capsule_of_equal_ends_edits_like_the_ball():
    n = 64
    d, m, b = _dense(n)
    balls = bo.anywhere_balls(n, 16, seed=4)
    caps = balls.copy()
    caps["shape"] = bo.BRUSH_CAPSULE
    assert np.array_equal(bo.apply(d, m, b, balls).pack, bo.apply(d, m, b, caps).pack)


def test_order_matters_in_the_oracle():
    n = 64
    d, m, b = _dense(n)
    pair = bo.stack([bo.ball((32.0, 32.0, 30.0), (20.0, 20.0, 20.0), 8.0, 0), bo.ball((33.0, 32.0, 30.0), (20.0, 20.0, 20.0), 8.0, 2)])
    assert not np.array_equal(bo.apply(d, m, b, pair).pack, bo.apply(d, m, b, pair[::-1]).pack)


def test_abi_of_the_brush_entry_point():
    from voxels_amd import binding
    so = os.path.join(ROOT, "voxels_amd", "csrc", "libvoxels_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT vx_grid_inject_brushes\b", syms)
    assert binding.BRUSH_DTYPE.itemsize == 64 and binding.BRUSH_RESULT_DTYPE.itemsize == 32
    # sizeof / offsetof as the C compiler sees the header
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "voxels_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu",'
           'sizeof(vx_brush),offsetof(vx_brush,position),offsetof(vx_brush,shape),offsetof(vx_brush,extents),offsetof(vx_brush,type),offsetof(vx_brush,a),'
           'offsetof(vx_brush,radius),offsetof(vx_brush,b),offsetof(vx_brush,material),sizeof(vx_brush_result),offsetof(vx_brush_result,out_max),'
           'offsetof(vx_brush_result,touched_blocks));return 0;}\n')
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "abi.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(tmp, "abi")
        subprocess.check_call(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), "-o", exe, c])
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    dt, rt = binding.BRUSH_DTYPE, binding.BRUSH_RESULT_DTYPE
    want = [64] + [dt.fields[k][1] for k in ("position", "shape", "extents", "type", "a", "radius", "b", "material")] + [32, rt.fields["out_max"][1], rt.fields["touched_blocks"][1]]
    assert got == want


def test_the_emulation_library_still_loads_without_the_entry_point():
    from emu_lib import emu_library
    from voxels_amd import Polygonizer
    from voxels_amd.binding import VoxelsHipError
    lib = emu_library()
    assert not lib.has_brushes
    p = Polygonizer(library=lib)
    with pytest.raises(VoxelsHipError):
        p.inject_brushes(bo.anywhere_balls(64, 2, 1))
