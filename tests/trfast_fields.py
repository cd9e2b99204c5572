"""The fields of the tests of the table-driven transition body (tests/test_trfast_tables.py on the CPU, tests/test_gpu_trfast.py
on the device): name -> (dist, mat, blend), and whether every transition block of the field must qualify for that body."""
import numpy as np

import fields


def _noise(n, seed, zeros):
    """Full-range band-limited noise (every 0 replaced by 1 unless `zeros`) under noise materials: the same-material bits of
    the reuse directions vary from cell to cell."""
    d = fields.quantize_full_range(fields.smooth_noise(n, seed, scale=16, amp=3.0))
    if not zeros:
        d[d == 0] = 1
    rng = np.random.RandomState(seed + 1)
    return d, rng.randint(0, 2, (n, n, n)).astype(np.uint8), rng.randint(0, 256, (n, n, n)).astype(np.uint8)


def _terrain(n, seed):
    from voxels_amd import synth
    return synth.terrain(n, seed=seed)


# name: (builder, every block table-driven, some block falls back)
FIELDS = {
    "noise64_nozero": (lambda: _noise(64, 7, False), True, False),      # levels 0-2, transition cells on level 1
    "noise128_nozero": (lambda: _noise(128, 11, False), True, False),   # level 2 as well: planes from a lattice copy, mult = 4
    "terrain64": (lambda: _terrain(64, 1337), True, False),
    "noise64_zeros": (lambda: _noise(64, 7, True), False, True),
}


def make(name):
    d, m, b = FIELDS[name][0]()
    return np.ascontiguousarray(d), np.ascontiguousarray(m), np.ascontiguousarray(b)
