"""A plain restatement of the rebuild contract (include/gpuart_build.h), in NumPy float32:

    build(prims) -> (quads, new_to_old)

`prims` are the primitives of a regular, orderly scene as tests/test_ray_queries.tree_prims lists them: (type, 16 floats of data quads) per
old ordinal. The result is the canonical compiled tree (the format tests/converter_ref.layout parses) of the Morton-order build:

    key      : per axis k, in fp32 as NumPy computes it (denormals kept, no contraction, IEEE division), with [Rmin, Rmax] the fold of all
               primitive boxes by refit_ref.fold from +-99e29:  c = lo_k*0.5f + hi_k*0.5f,  e = Rmax_k - Rmin_k,  t = (c - Rmin_k) / e,
               q_k = min(2^21 - 1, uint32(t * 2097152.0f)) if e > 0 and t > 0 else 0;   bit 3b+2 of the key = bit b of q_x, 3b+1 of q_y, 3b of q_z;
    order    : a stable sort by key; position p is the new ordinal, new_to_old[p] the old one;
    leaves   : leaf j holds positions 2j and 2j+1 (the last one alone when N is odd); its key K_j is its first primitive's;
    topology : delta(i, j) = clz64(K_i ^ K_j) if the keys differ else 64 + clz32(i ^ j); the node over leaves [a, b], a < b, splits behind the
               largest g in [a, b) with delta(a, g) > delta(a, b) (delta(a, a) is infinite): lower child [a, g], upper child [g + 1, b];
    boxes    : the refit rule (tests/refit_ref.py): a leaf's primitives' boxes folded in leaf order, an interior node's lower child's box
               folded with its upper child's;
    layout   : pre-order, lower child first.

A plain recursion; shares no code with the host library's RebuildMorton or with csrc/treebuild/build.hip (which constructs the tree in
parallel, every node from the keys alone).
"""
import sys

import numpy as np

from tests import converter_ref as CR
from tests import refit_ref as RR

F = np.float32
SCALE = F(2097152.0)   # 2^21
QMAX = (1 << 21) - 1


def boxes_of(prims):
    lo = np.zeros((len(prims), 3), F)
    hi = np.zeros((len(prims), 3), F)
    for i, (t, d) in enumerate(prims):
        lo[i], hi[i] = RR.prim_box(t, d)
    return lo, hi


def root_box(lo, hi):
    rlo, rhi = np.full(3, RR.START_LO, F), np.full(3, RR.START_HI, F)
    for a, b in zip(lo, hi):
        rlo, rhi = RR.fold(rlo, rhi, a, b)
    return rlo, rhi


def keys_of(lo, hi, rlo, rhi):
    """The 63-bit key of every primitive, as Python ints."""
    keys = []
    with np.errstate(all="ignore"):
        for a, b in zip(lo, hi):
            key = 0
            for k in range(3):
                c = F(F(a[k] * F(0.5)) + F(b[k] * F(0.5)))
                e = F(rhi[k] - rlo[k])
                t = F(F(c - rlo[k]) / e)
                q = 0
                if e > 0 and t > 0:
                    q = min(QMAX, int(F(t * SCALE)))
                for bit in range(21):
                    key |= ((q >> bit) & 1) << (3 * bit + 2 - k)
            keys.append(key)
    return keys


def delta(K, i, j):
    x = K[i] ^ K[j]
    if x:
        return 64 - x.bit_length()
    if i == j:
        return 1 << 30   # infinite
    return 64 + 32 - (i ^ j).bit_length()


def leaf_keys(keys, order):
    """K_j: the key of leaf j's first primitive."""
    return [keys[order[2 * j]] for j in range((len(order) + 1) // 2)]


def split(K, a, b):
    """The largest g in [a, b) with delta(a, g) > delta(a, b)."""
    d_ab = delta(K, a, b)
    return max(g for g in range(a, b) if delta(K, a, g) > d_ab)


def build(prims):
    n = len(prims)
    assert n >= 1 and all(0 <= t <= 3 for t, _ in prims)
    lo, hi = boxes_of(prims)
    rlo, rhi = root_box(lo, hi)
    keys = keys_of(lo, hi, rlo, rhi)
    order = sorted(range(n), key=lambda i: (keys[i], i))
    m = (n + 1) // 2
    K = leaf_keys(keys, order)
    quads = []

    def node(box_lo, box_hi, flags, parent):
        at = len(quads)
        quads.append([box_lo[0], box_lo[1], box_lo[2], 0.0])
        quads.append([box_hi[0], box_hi[1], box_hi[2], 0.0])
        quads.append(np.array([flags, 0, 0, parent], np.uint32).view(F).tolist())
        return at

    def patch(at, word, value):
        quads[at + 2][word] = float(np.array([value], np.uint32).view(F)[0])

    def emit(a, b, parent, flags):
        """Lays the subtree over leaves [a, b] out at the end of `quads`; returns its box."""
        if a == b:
            members = order[2 * a:2 * a + 2]
            blo, bhi = RR.leaf_box([(lo[i], hi[i]) for i in members])
            node(blo, bhi, CR.LEAF | flags | len(members), parent)
            for i in members:
                t, d = prims[i]
                quads.append(np.array([t, 0, 0, 0], np.uint32).view(F).tolist())
                quads.extend(np.asarray(d, F)[:4 * (t + 1)].reshape(-1, 4).tolist())
            return blo, bhi
        g = split(K, a, b)
        at = node((0, 0, 0), (0, 0, 0), flags, parent)
        patch(at, 1, at + 3)
        llo, lhi = emit(a, g, at, CR.IS_LOWER)
        patch(at, 2, len(quads))
        hlo, hhi = emit(g + 1, b, at, 0)
        blo, bhi = np.full(3, RR.START_LO, F), np.full(3, RR.START_HI, F)
        blo, bhi = RR.fold(blo, bhi, llo, lhi)
        blo, bhi = RR.fold(blo, bhi, hlo, hhi)
        quads[at][:3] = [float(v) for v in blo]
        quads[at + 1][:3] = [float(v) for v in bhi]
        return blo, bhi

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 4000))
    try:
        emit(0, m - 1, 0, CR.IS_ROOT)
    finally:
        sys.setrecursionlimit(limit)
    out = np.zeros((len(quads), 4), F)
    out.view(np.uint32)[:] = np.array(quads, F).view(np.uint32)   # (bit patterns of the uint words survive float32 -> list -> float32)
    return out, np.array(order, np.uint32)
