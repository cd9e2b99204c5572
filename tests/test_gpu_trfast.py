"""GPU tests of the table-driven transition body (vx_fastt.inl, VX_FAST bit 2): the fields of tests/trfast_fields.py on the
device against the port oracle with the body on (VX_FAST=7) and off (VX_FAST=3), the share of blocks that took it
(vx_transition_path_counts: a run cannot pass by falling back), and an incremental run compared between the two."""
import os

import numpy as np
import pytest

import fields
import trfast_fields
import vxo

pytestmark = pytest.mark.gpu

NRM_TOL = 1e-5  # (tests/test_gpu_parity.py: the device's normalisation against the host's)


@pytest.fixture(scope="module")
def port():
    o = vxo.load_port()
    assert o is not None, "oracle/libvoxels_port.so missing (run __graft_entry__.build())"
    return o


@pytest.fixture(scope="module")
def oracle_runs(port):
    """name -> (d, m, b, flags, oracle levels, oracle stats): computed once, shared by both knob values"""
    cache = {}

    def get(name):
        if name not in cache:
            d, m, b = trfast_fields.make(name)
            g = port.grid_from_dense(d, m, b)
            s = port.execute(g)
            cache[name] = (d, m, b, g.block_flags(), s.all_levels(), s.stats())
        return cache[name]
    return get


def make_poly(fast):
    import torch
    torch.cuda.init()
    from voxels_amd import Polygonizer
    os.environ["VX_FAST"] = fast  # (read once, when the context is created)
    try:
        p = Polygonizer(device=0)
    finally:
        del os.environ["VX_FAST"]
    assert p.backend == "hip:gfx950", "the native HIP library must be the one running"
    p.set_materials(vxo.default_lut())
    return p


@pytest.mark.parametrize("fast", ["7", "3"])
@pytest.mark.parametrize("name", sorted(trfast_fields.FIELDS))
def test_hip_transition_bodies_match_the_oracle(oracle_runs, name, fast):
    d, m, b, flags, ref, ref_stats = oracle_runs(name)
    p = make_poly(fast)
    try:
        p.upload(d, m, b, flags)
        p.execute(0)
        ok, msg = fields.surface_equal(p.all_levels(), ref, nrm_tol=NRM_TOL)
        assert ok, "%s, VX_FAST=%s: %s" % (name, fast, msg)
        assert np.array_equal(p.stats(), ref_stats)
        table_driven, fallback = p.transition_path_counts()
        print("%s VX_FAST=%s: %d table-driven, %d fallback" % (name, fast, table_driven, fallback))
        _, all_fast, some_fallback = trfast_fields.FIELDS[name]
        if fast == "3":
            assert (table_driven, fallback) == (0, 0)
        else:
            if all_fast:
                assert fallback == 0 and table_driven > 0, "%s: %d table-driven, %d fallback" % (name, table_driven, fallback)
            if some_fallback:
                assert fallback > 0, "%s: no block fell back" % name
    finally:
        p.close()


def test_hip_incremental_run_is_the_same_with_either_body():
    from voxels_amd import digest
    got, counts = [], []
    for fast in ("7", "3"):
        p = make_poly(fast)
        try:
            p.create_terrain(128, 21)
            p.execute(0)
            mn, mx = p.inject_ball((60.0, 64.0, 70.0), (24.0, 24.0, 24.0), 11.0, 2)
            p.execute_dirty(mn, mx)
            got.append(digest.surface_digest(p.all_levels()))
            counts.append(p.transition_path_counts())
        finally:
            p.close()
    assert digest.digests_equal(got[0], got[1]), "the incremental run differs between VX_FAST=7 and VX_FAST=3"
    assert counts[0][0] > 0 and counts[1] == (0, 0), counts
