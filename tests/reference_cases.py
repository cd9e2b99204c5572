"""What the unmodified reference produces where it cannot be run: tests/golden/reference_digests.json.

The oracle tests compare the port (oracle/port.cpp) with the unmodified reference (oracle/_ref) on seeded inputs.  The
reference library can only be built where its sources are, so tests/golden/make_golden.py (run there, `digests`) records
SHA-256 digests of everything those comparisons look at - every byte of every level's block infos, vertices, indices,
transition meshes, the statistics, block flags, dense fields, packed grid files - and of the dumps the reference build of
tests/cpp/dropin_test.cpp writes.  Where oracle/_ref exists the tests compare live as well, and check the stored digests
against the live reference."""
import hashlib
import json
import os

import numpy as np

import fields
import grid_sizes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_digests.json")
CHUNK = 1 << 20  # drop-in dumps: one digest per MiB besides the whole file's, so a mismatch still says where it starts


def array_digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %s;" % (a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def levels_digest(levels):
    h = hashlib.sha256()
    h.update(b"levels %d;" % len(levels))
    for lv in levels:
        for a in (lv.infos, lv.verts, lv.idx, lv.tverts, lv.tidx):
            h.update(array_digest(a).encode())
    return h.hexdigest()


def digest(value):
    return levels_digest(value) if isinstance(value, list) else array_digest(value)


# ---- the scenarios: each runs on one oracle (the reference or the port) and returns [(label, levels | array)] in order ---

def live_small(o, seed):
    """A terrain through Grid::Create's float path and a full-range int8 noise field, with materials."""
    n = 32 if seed != 23 else 64
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    g = o.grid_from_float(f, m, b)
    s = o.execute(g)
    out = [("terrain flags", g.block_flags()), ("terrain levels", s.all_levels()), ("terrain stats", s.stats())]
    q = fields.quantize_full_range(fields.smooth_noise(n, seed, scale=8, amp=3.0))
    s = o.execute(o.grid_from_dense(q, m, b))
    return out + [("noise levels", s.all_levels()), ("noise stats", s.stats())]


def live_256(o):
    """256^3: the bench generator's terrain and a full-range field (every reference level has interior blocks)."""
    from voxels_amd import synth
    n = 256
    d, m, b = synth.terrain(n)
    g = o.grid_from_dense(d, m, b)
    s = o.execute(g)
    out = [("terrain flags", g.block_flags()), ("terrain levels", s.all_levels()), ("terrain stats", s.stats())]
    s.destroy()
    q = fields.quantize_full_range(fields.smooth_noise(n, 77, scale=24, amp=3.0))
    s = o.execute(o.grid_from_dense(q, m, b))
    return out + [("noise levels", s.all_levels()), ("noise stats", s.stats())]


def edit_and_pack(o):
    """Three ball injections, each followed by the incremental Execute (Modification), a material injection, the grid's
    dense fields and its file (PackForSave), and a full Execute of the edited grid."""
    n = 64
    f = fields.terrain_field(n, 31)
    m, b = fields.materials_for(n, 31)
    g = o.grid_from_float(f, m, b)
    s = o.execute(g)
    out = []
    for k, (t, pos, ext, r) in enumerate(((2, (30.0, 33.5, 31.25), (20, 20, 20), 7.0), (0, (40, 20, 25), (16, 16, 16), 6.0),
                                          (1, (12, 40, 30), (10, 14, 12), 5.0))):
        box = g.inject_ball(pos, ext, r, t)
        ids = o.execute_modify(g, s, *box)
        out += [("edit %d box min" % k, box[0]), ("edit %d box max" % k, box[1]), ("edit %d modified ids" % k, ids),
                ("edit %d levels" % k, s.all_levels())]
    g.inject_material((20, 20, 30), (12, 12, 12), 5, True)
    out += [("dense %s" % name, a) for name, a in zip(("dist", "mat", "blend"), g.read_dense())]
    return out + [("pack", g.pack()), ("levels after the material edit", o.execute(g).all_levels())]


def heightmap(o):
    """Grid::Create(w, heightmap): dense data, flags, file bytes."""
    rng = np.random.RandomState(5)
    n = 64
    hm = (rng.randint(-40, 40, (n, n)) + (np.arange(n).reshape(n, 1) - 32)).clip(-128, 127).astype(np.int8)
    g = o.grid_from_heightmap(n, hm)
    out = [("dense %s" % name, a) for name, a in zip(("dist", "mat", "blend"), g.read_dense())]
    return out + [("flags", g.block_flags()), ("pack", g.pack())]


def terrain(o, seed, n):
    """tests/test_gpu_parity.py::test_hip_vs_oracle_terrain's inputs polygonized by the oracle."""
    f = fields.terrain_field(n, seed)
    m, b = fields.materials_for(n, seed)
    s = o.execute(o.grid_from_float(f, m, b))
    return [("levels", s.all_levels()), ("stats", s.stats())]


def odd_sizes(o):
    """Every edge of grid_sizes.ODD_SIZES (coarse levels covering a prefix of each axis): a terrain through the float path
    and a full-range int8 noise field, with materials."""
    out = []
    for n in grid_sizes.ODD_SIZES:
        f = fields.terrain_field(n, 60 + n)
        m, b = fields.materials_for(n, 60 + n)
        g = o.grid_from_float(f, m, b)
        s = o.execute(g)
        out += [("n=%d terrain flags" % n, g.block_flags()), ("n=%d terrain levels" % n, s.all_levels()),
                ("n=%d terrain stats" % n, s.stats())]
        s.destroy()
        q = fields.quantize_full_range(fields.smooth_noise(n, 70 + n, scale=8, amp=3.0))
        s = o.execute(o.grid_from_dense(q, m, b))
        out += [("n=%d noise levels" % n, s.all_levels()), ("n=%d noise stats" % n, s.stats())]
        s.destroy()
    return out


def odd_edits(o, n):
    """grid_sizes.edit_chain at an edge that is not a power of two: after every brush the box, the incremental Execute's
    modified ids, the levels and the statistics; at the end the grid's file and a full Execute."""
    f = fields.terrain_field(n, 90 + n)
    m, b = fields.materials_for(n, 90 + n)
    g = o.grid_from_float(f, m, b)
    s = o.execute(g)
    out = []
    for k, edit in enumerate(grid_sizes.edit_chain(n)):
        box = grid_sizes.apply_edit(g, edit)
        ids = o.execute_modify(g, s, *box)
        out += [("edit %d box min" % k, box[0]), ("edit %d box max" % k, box[1]), ("edit %d modified ids" % k, ids),
                ("edit %d levels" % k, s.all_levels()), ("edit %d stats" % k, s.stats())]
    s2 = o.execute(g)
    return out + [("pack", g.pack()), ("full run levels", s2.all_levels()), ("full run stats", s2.stats())]


def odd_heightmap(o):
    """Grid::Create(w, heightmap) at w = 80: dense data, flags, file bytes."""
    n = 80
    g = o.grid_from_heightmap(n, grid_sizes.heightmap_for(n, 8))
    out = [("dense %s" % name, a) for name, a in zip(("dist", "mat", "blend"), g.read_dense())]
    return out + [("flags", g.block_flags()), ("pack", g.pack())]


CASES = {
    "live_small_21": lambda o: live_small(o, 21),
    "live_small_22": lambda o: live_small(o, 22),
    "live_small_23": lambda o: live_small(o, 23),
    "live_256": live_256,
    "edit_and_pack": edit_and_pack,
    "heightmap": heightmap,
    "terrain_41_32": lambda o: terrain(o, 41, 32),
    "terrain_42_64": lambda o: terrain(o, 42, 64),
    "odd_sizes": odd_sizes,
    "odd_edits_80": lambda o: odd_edits(o, 80),
    "odd_edits_208": lambda o: odd_edits(o, 208),
    "odd_heightmap": odd_heightmap,
}


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def record(results):
    return [[label, digest(v)] for label, v in results]


def assert_matches_stored(case, results):
    """`results` (a scenario's output) must be, digest for digest, what the reference produced for it."""
    stored = load()["cases"][case]
    got = record(results)
    assert [l for l, _ in got] == [l for l, _ in stored], (case, [l for l, _ in got], [l for l, _ in stored])
    for (label, d), (_, want) in zip(got, stored):
        assert d == want, "%s: %s differs from the reference's (digest %s, stored %s)" % (case, label, d[:16], want[:16])


# ---- the drop-in application's dumps (tests/cpp/dropin_test.cpp) ---------------------------------------------------------

def dropin_key(n, variant="", gentle=False, edits=0):
    return "n=%d variant=%s gentle=%d edits=%d" % (n, variant or "-", int(bool(gentle)), int(edits))


def file_record(path):
    whole, chunks, size = hashlib.sha256(), [], 0
    with open(path, "rb") as f:
        while True:
            block = f.read(CHUNK)
            if not block:
                break
            whole.update(block)
            chunks.append(hashlib.sha256(block).hexdigest()[:16])
            size += len(block)
    return {"bytes": size, "sha256": whole.hexdigest(), "chunk_sha256_16": chunks}


def assert_dump_is_the_reference_s(path, key):
    """The dump at `path` must be, byte for byte, the one the reference build of the same application wrote."""
    want = load()["dropin_dumps"][key]
    got = file_record(path)
    assert got["bytes"] == want["bytes"], "%s: %d bytes, the reference's dump has %d" % (key, got["bytes"], want["bytes"])
    if got["sha256"] != want["sha256"]:
        first = next((i for i, (a, b) in enumerate(zip(got["chunk_sha256_16"], want["chunk_sha256_16"])) if a != b), 0)
        raise AssertionError("%s: dump differs from the reference's, first in bytes [%d, %d) of %d"
                             % (key, first * CHUNK, min((first + 1) * CHUNK, got["bytes"]), got["bytes"]))
