"""A plain restatement of the clustered rebuild's contract (include/gpuart_ploc.h), in NumPy float32:

    build(prims, radius=8) -> (quads, new_to_old)

with the signature and the canonical compiled-tree output of tests/build_ref.build. Locally-ordered clustering (Meister & Bittner 2018):

    order     : the Morton contract's keys (tests/build_ref.keys_of) and a stable sort by key; sorted position p is initial cluster p, which
                holds one primitive and has that primitive's box;
    iteration : over the cluster array C[0..c), c > 1:
      distance  d(i, j), i != j, |i - j| <= radius: the box of the cluster at the lower position folded with the other's (refit_ref.fold),
                e = hi - lo, d = (e.x*e.y + e.y*e.z) + e.z*e.x in fp32, denormals kept, no contraction;
      nearest   nn(i) = the j that minimises (d(i, j), i xor j) lexicographically;
      merge     every pair with nn(nn(i)) = i, i < nn(i), merges into i's slot: cluster i the lower child, nn(i) the upper, the box the fold
                above; two clusters of one primitive each become a leaf of two (i's primitive first), anything else an interior node;
      compact   the surviving clusters keep their order;
    end       : c = 1; more than MAX_ITERATIONS iterations are refused (ValueError);
    layout    : pre-order, lower child first; the primitives in the order of the leaves, which is new_to_old.

`info`, a dict, receives iterations, depth (of the deepest node, root = 0), n_recs and the refs (2 per record in pre-order, as the device
writes them: tree_rule::leaf_ref). The iteration is written with whole-array NumPy operations (one per window offset); it shares no
code with csrc/ploc/ploc.hip or the host library's AdoptTopology.
"""
import sys

import numpy as np

from tests import build_ref as BR
from tests import converter_ref as CR
from tests import refit_ref as RR

F = np.float32
RADIUS = 8               # GPUART_PLOC_RADIUS
MAX_ITERATIONS = 1024    # GPUART_PLOC_MAX_ITERATIONS
REF_LEAF, REF_TRIS, REF_TWO, REF_SMALL = 0x80000000, 0x40000000, 0x20000000, 0x10000000


def _nearest(lo, hi, radius):
    """nn(i) of every cluster of the array with boxes lo, hi (c x 3)."""
    c = len(lo)
    best_d = np.full(c, np.inf, F)
    best_x = np.full(c, 1 << 62, np.int64)
    nn = np.full(c, -1, np.int64)
    pos = np.arange(c, dtype=np.int64)

    def offer(i, j, d):
        x = i ^ j
        better = (d < best_d[i]) | ((d == best_d[i]) & (x < best_x[i]))
        i, j, d, x = i[better], j[better], d[better], x[better]
        best_d[i], best_x[i], nn[i] = d, x, j

    with np.errstate(all="ignore"):
        for off in range(1, min(radius, c - 1) + 1):
            a, b = pos[:c - off], pos[off:]
            flo, fhi = RR.fold(lo[a], hi[a], lo[b], hi[b])      # the lower position's box first
            e = (fhi - flo).astype(F)
            d = ((e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]).astype(F)
            offer(a, b, d)
            offer(b, a, d)
    return nn


def _slot(lower, upper):
    """The slots the merged clusters take: the lower partners'."""
    return lower


def _pair(a, b):
    """The node over clusters a (lower) and b (upper)."""
    return ("pair", a, b)


def build(prims, radius=RADIUS, info=None):
    n = len(prims)
    assert n >= 1 and radius >= 1 and all(0 <= t <= 3 for t, _ in prims)
    plo, phi = BR.boxes_of(prims)
    keys = BR.keys_of(plo, phi, *BR.root_box(plo, phi))
    order = sorted(range(n), key=lambda i: (keys[i], i))
    # a node: ("prim", old ordinal) or ("pair", lower node, upper node); a cluster: its node, its box and how many primitives it holds
    node = [("prim", o) for o in order]
    lo, hi = plo[order].copy(), phi[order].copy()
    count = np.ones(n, np.int64)
    iterations = 0
    while len(node) > 1:
        if iterations == MAX_ITERATIONS:
            raise ValueError("more than %d iterations" % MAX_ITERATIONS)
        iterations += 1
        c = len(node)
        nn = _nearest(lo, hi, radius)
        pos = np.arange(c)
        mutual = nn[nn] == pos
        lower = np.nonzero(mutual & (pos < nn))[0]
        assert len(lower) >= 1
        upper = nn[lower]
        into = _slot(lower, upper)
        keep = np.ones(c, bool)
        keep[lower + upper - into] = False
        for i, j, s in zip(lower, upper, into):
            node[s] = _pair(node[i], node[j])
        with np.errstate(all="ignore"):
            lo[into], hi[into] = RR.fold(lo[lower], hi[lower], lo[upper], hi[upper])
        count[into] = count[lower] + count[upper]
        node = [node[i] for i in np.nonzero(keep)[0]]
        lo, hi, count = lo[keep], hi[keep], count[keep]

    quads, new_to_old, refs, depths = [], [], [], [0]

    def header(box_lo, box_hi, flags, parent):
        at = len(quads)
        quads.append([box_lo[0], box_lo[1], box_lo[2], 0.0])
        quads.append([box_hi[0], box_hi[1], box_hi[2], 0.0])
        quads.append(np.array([flags, 0, 0, parent], np.uint32).view(F).tolist())
        return at

    def patch(at, word, value):
        quads[at + 2][word] = float(np.array([value], np.uint32).view(F)[0])

    def is_leaf(nd):
        return nd[0] == "prim" or (nd[1][0] == "prim" and nd[2][0] == "prim")

    def emit(nd, parent, flags, level):
        """Lays the subtree of `nd` out at the end of `quads`; returns (its box, its ref)."""
        depths[0] = max(depths[0], level)
        if is_leaf(nd):
            members = [nd[1]] if nd[0] == "prim" else [nd[1][1], nd[2][1]]
            blo, bhi = RR.leaf_box([(plo[o], phi[o]) for o in members])
            header(blo, bhi, CR.LEAF | flags | len(members), parent)
            tris = all(prims[o][0] == 2 for o in members)
            ref = REF_LEAF | len(new_to_old) | (REF_TRIS if tris else REF_SMALL) | (REF_TWO if len(members) == 2 else 0)
            for o in members:
                t, d = prims[o]
                new_to_old.append(o)
                quads.append(np.array([t, 0, 0, 0], np.uint32).view(F).tolist())
                quads.extend(np.asarray(d, F)[:4 * (t + 1)].reshape(-1, 4).tolist())
            return blo, bhi, ref
        rec = len(refs) // 2
        refs.extend([0, 0])
        at = header((0, 0, 0), (0, 0, 0), flags, parent)
        patch(at, 1, at + 3)
        llo, lhi, refs[2 * rec] = emit(nd[1], at, CR.IS_LOWER, level + 1)
        patch(at, 2, len(quads))
        hlo, hhi, refs[2 * rec + 1] = emit(nd[2], at, 0, level + 1)
        blo, bhi = np.full(3, RR.START_LO, F), np.full(3, RR.START_HI, F)
        blo, bhi = RR.fold(blo, bhi, llo, lhi)
        blo, bhi = RR.fold(blo, bhi, hlo, hhi)
        quads[at][:3] = [float(v) for v in blo]
        quads[at + 1][:3] = [float(v) for v in bhi]
        return blo, bhi, rec

    limit = sys.getrecursionlimit()
    sys.setrecursionlimit(max(limit, 3 * MAX_ITERATIONS + 1000))
    try:
        blo, bhi, root_ref = emit(node[0], 0, CR.IS_ROOT, 0)
    finally:
        sys.setrecursionlimit(limit)
    with np.errstate(all="ignore"):
        assert (blo == lo[0]).all() and (bhi == hi[0]).all()    # the refit rule's boxes are the boxes the clustering carried
    out = np.zeros((len(quads), 4), F)
    out.view(np.uint32)[:] = np.array(quads, F).view(np.uint32)
    if info is not None:
        info.update(iterations=iterations, depth=depths[0], n_recs=len(refs) // 2, refs=np.array(refs, np.uint32), root_ref=int(root_ref))
    return out, np.array(new_to_old, np.uint32)
