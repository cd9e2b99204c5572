"""The ABI of the ambient occlusion (include/voxels_hip.h, "ambient occlusion"): the exports, the layout of the structs as the C
compiler sees them, the constants, the prototypes and the rule's text in the header, and every listed error through the entry
checks of the host library."""
import os
import re

import numpy as np

import occlusion_oracle as oo
from voxels_amd import binding

EXPORTS = ("vx_occlusion", "vx_occlusion_device", "vx_debug_occlusion_shortcuts")


def layout(which):
    out = np.zeros(8, np.uint32)
    k = oo.load().oh_layout(which, out.ctypes.data)
    return out[:k].tolist()


def test_the_library_exports_the_occlusion():
    import voxels_amd
    lib = binding.HipLibrary()
    assert lib.has_occlusion and all(hasattr(lib.lib, name) for name in EXPORTS)
    for name in ("occlusion", "occlusion_device", "debug_occlusion_shortcuts"):
        assert hasattr(binding.Polygonizer, name)
    for name in ("OCCLUSION_PARAMS_DTYPE", "OCCLUSION_COUNTS_DTYPE", "OCCLUSION_MAX_STEPS", "OCCLUSION_TRANSITIONS", "occlusion_params"):
        assert getattr(voxels_amd, name) is getattr(binding, name) and name in voxels_amd.__all__


def test_record_sizes_and_offsets():
    # as the C compiler lays out the header's structs (tests/occlusion/occlusion_host.cpp includes include/voxels_hip.h)
    assert layout(0) == [48, 32, 48]
    assert [d.itemsize for d in (binding.OCCLUSION_PARAMS_DTYPE, binding.OCCLUSION_COUNTS_DTYPE, binding.VERTEX_DTYPE)] == [48, 32, 48]
    names = ("steps", "flags", "box_min", "box_max", "reserved")
    assert layout(1) == [binding.OCCLUSION_PARAMS_DTYPE.fields[k][1] for k in names] == [0, 4, 8, 20, 32]
    names = ("vertices", "sum", "entries", "visited_entries", "darkest", "open")
    assert layout(2) == [binding.OCCLUSION_COUNTS_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 20, 24, 28]
    assert layout(3) == [binding.VERTEX_DTYPE.fields[k][1] for k in ("pos", "nrm")] == [0, 28]


def test_the_header_states_the_constants_the_prototypes_and_the_rule():
    text = open(os.path.join(oo.ROOT, "include", "voxels_hip.h")).read()
    lib = oo.load()
    for k, (name, value) in enumerate((("VX_OCCLUSION_MAX_STEPS", "12"), ("VX_OCCLUSION_TRANSITIONS", "1u"))):
        assert re.search(r"#define %s %s\b" % (name, value), text), name
        assert lib.oh_limit(k) == int(value.rstrip("u")) == getattr(binding, name[3:])
    for proto in ("int  vx_occlusion_device(vx_ctx* ctx, uint32_t level, const vx_occlusion_params* params /* host */,",
                  "int  vx_occlusion(vx_ctx* ctx, uint32_t level, const vx_occlusion_params* params,",
                  "int  vx_debug_occlusion_shortcuts(vx_ctx* ctx, uint32_t enable);"):
        assert proto in text, proto
    flat = re.sub(r"\s*\n \*\s*", " ", text)
    for phrase in ("P[a] = (int32)floorf(g[a] * (256.0f / s) + 0.5f)", "N[a] = (int32)floorf(m[a] * 127.0f + 0.5f)", "max(|dx|, |dy|, |dz|) == 2",
                   "((dz + 2) * 5 + (dy + 2)) * 5 + (dx + 2)", "S[a] = floor(256 * d[a] / |d| + 0.5)", "w_k = max(0, (N . S_k) >> 8)", "O = P + 2 * N",
                   "c[a] = (Q[a] + 128) >> 8", "tot = steps * sum of w_k", "w_k * (steps + 1 - hit_k)", "ao = tot ? 255 - (255 * occ) / tot : 255",
                   "the grid as it is NOW", "old vertices against the new samples", "keeps its value"):
        assert phrase in flat, phrase


def test_a_null_context_is_invalid():
    lib = binding.HipLibrary().lib
    prm = oo.occlusion_params(steps=4)
    ao = np.full(64, 0xA5, np.uint8)
    for fn in (lib.vx_occlusion, lib.vx_occlusion_device):
        assert fn(None, 0, prm.ctypes.data, ao.ctypes.data, 64, None) == -1
    assert lib.vx_debug_occlusion_shortcuts(None, 1) == -1
    assert (ao == 0xA5).all()


def test_the_entry_checks_refuse_every_listed_error():
    lib = oo.load()
    good = oo.occlusion_params(steps=12, transitions=True, box_min=(0, -np.inf, 0), box_max=(8, np.inf, 8))

    def both(whole=1, surface=1, levels=3, level=2, prm=good, array=1, capacity=100, n_verts=100):
        rc = lib.oh_check(whole, surface, levels, level, None if prm is None else prm.ctypes.data, array, capacity, n_verts)
        assert rc == oo.check(whole, surface, levels, level, prm, array, capacity, n_verts), (whole, surface, levels, level, prm, array, capacity, n_verts)
        return rc

    assert both() == 0 and both(capacity=101) == 0 and both(n_verts=0, capacity=0) == 0
    assert both(prm=oo.occlusion_params(steps=1)) == 0
    assert both(whole=0) == -1                                   # no whole grid of the context's own
    assert both(surface=0) == -1                                 # no surface
    assert both(level=3) == -1 and both(levels=0, level=0) == -1  # level >= levels of the last run
    assert both(prm=None) == -1                                  # null params
    assert both(array=0) == -1                                   # a null array
    assert both(capacity=99) == -1                               # capacity < n_verts

    def bad(change):
        p = good.copy()
        change(p)
        assert both(prm=p) == -1, p

    for steps in (0, 13, 0xFFFFFFFF):
        bad(lambda p, s=steps: p.__setitem__("steps", s))
    for flags in (2, 3, 0x80000000):
        bad(lambda p, f=flags: p.__setitem__("flags", f))
    for k in range(4):
        def word(p, k=k):
            p["reserved"][0, k] = 1
        bad(word)
    for field in ("box_min", "box_max"):
        for a in range(3):
            def nan(p, field=field, a=a):
                p[field][0, a] = np.nan
            bad(nan)
    for a in range(3):
        def crossed(p, a=a):
            p["box_min"][0, a], p["box_max"][0, a] = 9.0, 8.0
        bad(crossed)
    # a bake with steps out of range writes nothing
    v = oo.vertices([(1, 1, 1)], [(0, 1, 0)])
    for steps in (0, 13):
        rc, out, _, _ = oo.host_bake(0, np.full((16, 16, 16), 100, np.int8), 0, steps, v)
        assert rc == -1 and (out == 0xA5).all()
