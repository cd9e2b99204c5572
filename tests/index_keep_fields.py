"""The field of the index-keeping tests that steady_fields.py does not have (tests/test_index_keep_fields.py checks its premises
in numpy and against the oracle on the CPU; tests/test_gpu_index_keep.py runs it on the device): a level-0 block whose mesh needs
more than one descriptor chunk - more than F0_VDESC new vertices or more than F0_TDESC triangles (tv_fast0.h) - while every
block of every level stays within the first capacity class and no meshed block stages an exact zero, so that the context's full
runs reach the one-launch form.

chunks64: a 64^3 grid of +127 with a CUBE_EDGE^3 cube of zero-free noise of both signs inside level-0 block (0, 0, 0), under the
random materials of the steady fields (few vertices are reused across cells of different materials).  The cube's samples
lie at CUBE_AT .. CUBE_AT + CUBE_EDGE - 1 on every axis, so the non-trivial cells are the (CUBE_EDGE + 1)^3 cells around them:
512 of the block's 4096, all in one block.  On level 1 the lattice (stride 2) meets 4^3 of the cube's samples, on level 2 two per axis."""
import numpy as np

import test_gpu_matstore as matstore

F0_VDESC = F0_TDESC = 1024  # tv_fast0.h: vertices / triangles described per chunk
N, CUBE_AT, CUBE_EDGE, SEED = 64, 4, 7, 3

_MADE = {}


def chunks64():
    """(dist, mat, blend); built once, handed out read-only"""
    if "chunks64" not in _MADE:
        rng = np.random.RandomState(SEED)
        d = np.full((N, N, N), 127, np.int8)
        mag = rng.randint(1, 128, (CUBE_EDGE,) * 3)
        sign = rng.randint(0, 2, (CUBE_EDGE,) * 3) * 2 - 1
        cube = (slice(CUBE_AT, CUBE_AT + CUBE_EDGE),) * 3
        d[cube] = (mag * sign).astype(np.int8)
        arrays = tuple(np.ascontiguousarray(a) for a in (d,) + matstore.mixed_materials(N, 5))
        for a in arrays:
            a.setflags(write=False)
        _MADE["chunks64"] = arrays
    return _MADE["chunks64"]
