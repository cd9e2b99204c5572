"""numpy statement of the LOD selection of include/voxels_hip.h ("LOD selection"), independent of the device code.

The least set of opened nodes is found by plain iteration: start from rule 1 plus closure, then open every active node that a
leaf of level <= L - g(L) touches (rule 3, read off a dense level-0 array of leaf levels and the layers of cells beyond each
node face), close upwards again, and repeat until nothing changes.  Records and draw commands follow from a block table
(LISTED_BLOCK_DTYPE arrays, one per level)."""
import numpy as np

from voxels_amd.binding import DRAW_INDEXED_DTYPE, LOD_DRAW_DTYPE

FAR = 99  # leaf level of the cells outside the grid


def ref_levels(n):
    return (n // 16).bit_length()


def face_axis(f):
    """internal axis (x 0, y 1, z 2) and direction of TransitionFaceId f (-Y, -Z, -X, +Y, +Z, +X in mesh space)"""
    return (2, 1, 0)[f % 3], (-1 if f < 3 else 1)


# bit of vertex.sec[3] that marks a regular vertex on transition face f: the meshes put bit b on face b
# (tests/test_gpu_lod.py::test_adjacency_bits_from_the_meshes)
ADJ_BIT = (0, 1, 2, 3, 4, 5)


def adjacency(bits):
    bits = np.asarray(bits, np.uint32)
    a = np.zeros_like(bits)
    for f in range(6):
        a |= np.where(bits & (1 << f), np.uint32(1 << ADJ_BIT[f]), np.uint32(0))
    return a


def node_boxes(cnt, level):
    """mesh-space boxes of all nodes of a level, arrays indexed [z, y, x] (internal coordinates)"""
    s = np.float32(16 << level)
    z, y, x = np.meshgrid(np.arange(cnt), np.arange(cnt), np.arange(cnt), indexing="ij")
    mn = np.stack([x, z, y], -1).astype(np.float32) * s
    return mn, mn + s


def dist2(mn, mx, cam):
    cam = np.asarray(cam, np.float32)
    with np.errstate(over="ignore"):
        return _dist2(mn, mx, cam)


def _dist2(mn, mx, cam):
    d = np.maximum(np.maximum(mn - cam, np.float32(0)), cam - mx).astype(np.float32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(np.float32)


def culled(mn, mx, planes):
    out = np.zeros(mn.shape[:-1], bool)
    for pl in np.asarray(planes, np.float32).reshape(-1, 4):
        p = np.where(pl[:3] >= 0, mx, mn)
        s = (pl[0] * p[..., 0] + pl[1] * p[..., 1]).astype(np.float32) + (pl[2] * p[..., 2]).astype(np.float32)
        out |= (s.astype(np.float32) + pl[3]) < 0
    return out


class Selection:
    """The selection for grid edge n, levels_run levels, a camera and ranges (16 floats)."""

    def __init__(self, n, levels_run, camera, ranges):
        self.n, self.c0 = n, n // 16
        self.R, self.T = ref_levels(n), levels_run - 1
        self.cnt = [self.c0 >> L for L in range(self.T + 1)]
        ranges = np.asarray(ranges, np.float32)
        self.rule1 = [np.zeros((c, c, c), bool) for c in self.cnt]
        for L in range(1, self.T + 1):
            r = ranges[L]
            if r > 0:
                mn, mx = node_boxes(self.cnt[L], L)
                self.rule1[L] = dist2(mn, mx, camera) < np.float32(r * r)
        self.root = [self._roots(L) for L in range(self.T + 1)]
        self.open = [o.copy() for o in self.rule1]
        self._close()
        while True:
            self._leaves()
            grew = False
            for L in range(1, self.T + 1):
                g = 1 if L == self.R - 1 else 2
                force = self.active[L] & ~self.open[L] & (self.face_min[L].min(0) <= L - g)
                if force.any():
                    self.open[L] |= force
                    grew = True
            if not grew:
                break
            self._close()

    def _roots(self, L):
        c = self.cnt[L]
        if L == self.T:
            return np.ones((c, c, c), bool)
        i = np.arange(c) >> 1 >= self.cnt[L + 1]
        return i[:, None, None] | i[None, :, None] | i[None, None, :]

    def _parent_open(self, L):
        c, p = self.cnt[L], self.cnt[L + 1] if L < self.T else 0
        out = np.zeros((c, c, c), bool)
        if L < self.T:
            up = self.open[L + 1].repeat(2, 0).repeat(2, 1).repeat(2, 2)
            m = min(c, 2 * p)
            out[:m, :m, :m] = up[:m, :m, :m]
        return out & ~self.root[L]

    def _close(self):
        for L in range(1, self.T):
            c, p = self.cnt[L], self.cnt[L + 1]
            o = self.open[L] & ~self.root[L]
            m = 2 * p
            par = o[:m, :m, :m].reshape(p, 2, p, 2, p, 2).any((1, 3, 5))
            self.open[L + 1] |= par

    def _leaves(self):
        self.active = [self.root[L] | self._parent_open(L) for L in range(self.T + 1)]
        self.leaf = [self.active[L] & ~self.open[L] for L in range(self.T + 1)]
        lm = np.full((self.c0,) * 3, -1, np.int32)
        cover = np.zeros((self.c0,) * 3, np.int32)
        for L in range(self.T + 1):
            m, c = 1 << L, self.cnt[L]
            big = self.leaf[L].repeat(m, 0).repeat(m, 1).repeat(m, 2)
            e = c * m
            lm[:e, :e, :e][big] = L
            cover[:e, :e, :e] += big
        self.level_map, self.cover = lm, cover
        pad = np.full((self.c0 + 2,) * 3, FAR, np.int32)
        pad[1:-1, 1:-1, 1:-1] = lm
        self.face_min, self.face_max = [], []
        for L in range(self.T + 1):
            m, c = 1 << L, self.cnt[L]
            mins, maxs = np.zeros((6, c, c, c), np.int32), np.zeros((6, c, c, c), np.int32)
            for f in range(6):
                a, d = face_axis(f)
                ax = 2 - a  # array axis of internal axis a ([z, y, x])
                q = np.moveaxis(pad, ax, 0)
                pos = np.arange(c) * m + (0 if d < 0 else m + 1)
                layer = q[pos][:, 1:1 + c * m, 1:1 + c * m]          # [node along ax, other, other]
                blk = layer.reshape(c, c, m, c, m)
                lo, hi = blk.min((2, 4)), np.where(blk == FAR, -1, blk).max((2, 4))
                mins[f] = np.moveaxis(lo, 0, ax)
                maxs[f] = np.moveaxis(hi, 0, ax)
            self.face_min.append(mins)
            self.face_max.append(maxs)

    def transitions(self, L):
        """per node of level L: TransitionFaceId bits of the faces a finer leaf touches"""
        bits = np.zeros((self.cnt[L],) * 3, np.uint32)
        for f in range(6):
            bits |= np.where(self.face_min[L][f] < L, np.uint32(1 << f), np.uint32(0))
        return bits

    def leaf_count(self):
        return int(sum(l.sum() for l in self.leaf))

    def leaf_volume(self):
        return int(sum(int(l.sum()) << (3 * L) for L, l in enumerate(self.leaf)))


def select(sel, tables, planes=()):
    """(draws, regular, transition, counts) for the block tables (LISTED_BLOCK_DTYPE arrays, levels 0..T)"""
    draws, regular, transition = [], [], []
    meshed = culled_n = 0
    for L in range(sel.T + 1):
        tab = tables[L]
        if not len(tab):
            continue
        c = sel.cnt[L]
        coord = tab["coord_id"].astype(np.int64)
        z, y, x = coord // (c * c), (coord // c) % c, coord % c
        leaf = sel.leaf[L][z, y, x]
        mn, mx = node_boxes(c, L)
        cull = culled(mn[z, y, x], mx[z, y, x], planes) if len(planes) else np.zeros(len(tab), bool)
        bits = sel.transitions(L)[z, y, x]
        meshed += int(leaf.sum())
        culled_n += int((leaf & cull).sum())
        for e in np.nonzero(leaf & ~cull)[0]:
            rec = len(draws)
            b = tab[e]
            draws.append((L, e, b["id"], b["coord_id"], bits[e], adjacency(bits[e]), (0, 0)))
            regular.append((b["i_count"], 1, b["i_off"], b["v_off"], rec))
            for f in range(6):
                if bits[e] & (1 << f) and b["ti_count"][f] > 0:
                    transition.append((b["ti_count"][f], 1, b["ti_off"][f], b["tv_off"][f], rec))
    draws = np.array(draws, LOD_DRAW_DTYPE) if draws else np.zeros(0, LOD_DRAW_DTYPE)
    regular = np.array(regular, DRAW_INDEXED_DTYPE) if regular else np.zeros(0, DRAW_INDEXED_DTYPE)
    transition = np.array(transition, DRAW_INDEXED_DTYPE) if transition else np.zeros(0, DRAW_INDEXED_DTYPE)
    counts = dict(records=len(draws), regular=len(regular), transition=len(transition), leaves=sel.leaf_count(),
                  meshed_leaves=meshed, culled_leaves=culled_n, leaf_volume=sel.leaf_volume())
    return draws, regular, transition, counts
