"""A plain restatement of the refit contract (include/gpuart_refit.h), in NumPy float32 on the canonical compiled tree:

    refit(quads, ordinals, payloads) -> quads'

replaces the data quads of the listed primitives — numbered as tests/test_ray_queries.tree_prims and tests/converter_ref.layout number
them: the leaves in pre-order, each leaf's primitives in order —, recomputes every node's box and changes nothing else:

    primitive : the box its constructor gives it (the reference's src/core.cpp): sphere and disc c -+ r; triangle the running minimum and
                maximum of its vertices from +-9e19; cone min(c1 - r1, c2 - r2) .. max(c1 + r1, c2 + r2) as std::min / std::max compute them;
    leaf      : the running minimum and maximum of its primitives' boxes in leaf order, from +-99e29, with `<` and `>` (the first of equal
                values stays, a NaN is skipped);
    interior  : its lower child's box folded with its upper child's by the same rule.

The device arrays after a refit are tests/converter_ref.convert(quads')'s recs and prims, byte for byte, and the host library's
BoundingVolumesHierarchy::Refit writes quads' itself. Shares no code with either.
"""
import numpy as np

from tests import converter_ref as CR

F = np.float32
PAYLOAD = 16
START_LO, START_HI = F(99.0e29), F(-99.0e29)


def prim_box(t, d):
    """(lo, hi) of a primitive of type t with data quads d (16 floats)."""
    d = np.asarray(d, F)
    if t in (0, 1):
        return d[0:3] - d[3], d[0:3] + d[3]
    if t == 2:
        lo, hi = np.full(3, 9e19, F), np.full(3, -9e19, F)
        for v in (d[0:3], d[4:7], d[8:11]):
            lo = np.where(v < lo, v, lo)
            hi = np.where(v > hi, v, hi)
        return lo, hi
    a, b = d[0:3] - d[3], d[4:7] - d[7]
    A, B = d[0:3] + d[3], d[4:7] + d[7]
    return np.where(b < a, b, a), np.where(A < B, B, A)


def fold(lo, hi, clo, chi):
    return np.where(clo < lo, clo, lo), np.where(chi > hi, chi, hi)


def leaf_box(boxes):
    """A leaf's box: its primitives' boxes, (lo, hi) each, folded in leaf order."""
    lo, hi = np.full(3, START_LO, F), np.full(3, START_HI, F)
    for a, b in boxes:
        lo, hi = fold(lo, hi, a, b)
    return lo, hi


def refit(quads, ordinals=(), payloads=()):
    q = np.array(quads, F).reshape(-1, 4).copy()
    lay = CR.layout(q)
    p_addr, p_type = lay["prim_addr"], lay["prim_type"]
    payloads = np.asarray(payloads, F).reshape(-1, PAYLOAD)
    for o, p in zip(ordinals, payloads):
        a, t = int(p_addr[o]), int(p_type[o])
        q[a + 1:a + 2 + t] = p[:4 * (t + 1)].reshape(-1, 4)
    addr, parent, leaf = lay["addr"], lay["parent"], lay["leaf"]
    n = len(addr)
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[parent[i]].append(i)            # pre-order: the lower child is met first
    leaf_of = np.searchsorted(addr, p_addr, "right") - 1
    members = [[] for _ in range(n)]
    for k, l in enumerate(leaf_of):
        members[l].append(k)
    lo_, hi_ = np.zeros((n, 3), F), np.zeros((n, 3), F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n - 1, -1, -1):
            lo, hi = np.full(3, START_LO, F), np.full(3, START_HI, F)
            if leaf[i]:
                boxes = []
                for k in members[i]:
                    a, t = int(p_addr[k]), int(p_type[k])
                    d = np.zeros(PAYLOAD, F)
                    d[:4 * (t + 1)] = q[a + 1:a + 2 + t].reshape(-1)
                    boxes.append(prim_box(t, d))
                lo, hi = leaf_box(boxes)
            else:
                for c in kids[i]:
                    lo, hi = fold(lo, hi, lo_[c], hi_[c])
            lo_[i], hi_[i] = lo, hi
            q[addr[i], 0:3], q[addr[i] + 1, 0:3] = lo, hi
    return q


# ---- making updates ---------------------------------------------------------------------------------------------------------------
def desc_of(t, d):
    """The description (gpuart_amd.binding.make_prims) of the primitive with data quads d."""
    d = [float(x) for x in d]
    return (t, {0: d[0:4], 1: d[0:3] + d[4:7] + d[3:4], 2: d[0:3] + d[4:7] + d[8:11], 3: d[0:3] + d[4:7] + [d[3], d[7]]}[t])


def payload_of(desc):
    """The 16 floats the host library's constructors and StoreDataIntoBVH make of a description (a cone's derived constants included)."""
    from gpuart_amd import binding as B
    from tests.test_ray_queries import tree_prims
    t, f = desc
    f = np.asarray(f, F)
    d = np.zeros(PAYLOAD, F)
    if t == 0:
        d[0:4] = f[0:4]
    elif t == 1:
        d[0:3], d[3], d[4:7] = f[0:3], f[6], f[3:6]
    elif t == 2:
        d[0:3], d[4:7], d[8:11] = f[0:3], f[3:6], f[6:9]
    else:
        (tt, d), = tree_prims(B.compile_bvh([(t, [float(x) for x in f])])[0])
        assert tt == 3
    return d


def moved(t, d, delta):
    """The payload of primitive (t, d) translated by delta: through its description, as a caller would make it."""
    t, f = desc_of(t, d)
    f = np.asarray(f, F).copy()
    delta = np.asarray(delta, F)
    for k in {0: (0,), 1: (0,), 2: (0, 3, 6), 3: (0, 3)}[t]:
        f[k:k + 3] = f[k:k + 3] + delta
    return payload_of((t, f))


def random_update(tree, rng, share, amount):
    """(ordinals, payloads) moving `share` of the tree's primitives by up to `amount` per axis."""
    from tests.test_ray_queries import tree_prims
    prims = tree_prims(tree)
    n = len(prims)
    k = max(1, int(round(share * n)))
    ordinals = np.sort(rng.choice(n, k, replace=False)).astype(np.uint32)
    payloads = np.stack([moved(prims[o][0], prims[o][1], rng.uniform(-amount, amount, 3)) for o in ordinals])
    return ordinals, payloads
