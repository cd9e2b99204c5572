"""CPU tests of the table-driven transition body (voxels_amd/csrc/tv_fastt.h): the derived case rows against the general
phases for every case, reuse mask, material combination and winding, and trf_block_serial against the general serial phases
on whole runs (tests/trfast/trfast_host.cpp: the CPU emulation with either body) - vertices, indices and the per-face ranges
of every block record, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import fields
import trfast_fields
import vxo


@pytest.fixture(scope="module")
def host():
    from voxels_amd import build
    from voxels_amd.binding import HipLibrary
    lib = HipLibrary(build.build_trfast_host())
    assert lib.backend.startswith("emu:")
    lib.lib.trfh_check_tables.restype = C.c_uint32
    return lib


def test_case_rows_match_the_general_phases_exhaustively(host):
    bad = C.c_uint32(0)
    checked = host.lib.trfh_check_tables(2, C.byref(bad))
    assert checked == 510 * 4 * 4 * 2 * 2
    assert bad.value == 0, "%d of %d configurations differ (see stderr)" % (bad.value, checked)


def run(host, mode, d, m, b, flags):
    from voxels_amd.binding import Polygonizer
    host.lib.trfh_set_mode(mode)
    p = Polygonizer(library=host)
    p.set_materials(vxo.default_lut())
    p.upload(d, m, b, flags)
    p.execute()
    levels, stats = p.all_levels(), p.stats()
    counts = np.zeros(2, np.uint32)
    host.lib.trfh_counts(counts.ctypes.data_as(C.c_void_p))
    p.close()
    return levels, stats, (int(counts[0]), int(counts[1]))


@pytest.mark.parametrize("name", sorted(trfast_fields.FIELDS))
def test_serial_block_equals_the_general_phases(host, name):
    from voxels_amd import synth
    d, m, b = trfast_fields.make(name)
    flags = synth.block_empty_flags(d)
    general, gstats, _ = run(host, 0, d, m, b, flags)
    table, tstats, (fast, fallback) = run(host, 1, d, m, b, flags)
    assert sum(len(l.tidx) for l in general) > 0, "the field has no transition geometry"
    ok, msg = fields.surface_equal(table, general)
    assert ok, name + ": " + msg
    assert np.array_equal(gstats, tstats)
    _, all_fast, some_fallback = trfast_fields.FIELDS[name]
    if all_fast:
        assert fallback == 0 and fast > 0, "%s: %d table-driven, %d fallback" % (name, fast, fallback)
    if some_fallback:
        assert fallback > 0, "%s: no block fell back" % name
