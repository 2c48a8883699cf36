"""A plain restatement of the box-overlap contract (include/gpuart_nearest.h, "Box overlap"), in NumPy float32, written from the header
and not from csrc/. The tree order and the leaves' members are tests/within_ref.py's and tests/nearest_ref.py's.

    inflate(boxes, margin)                                                     (qlo, qhi): lo - margin, hi + margin, one fp32 operation each
    box_ok(boxes)                                                              six finite words and lo <= hi on every axis
    brute(recs, prims, boxes, root, queries, margin, user_sphere=None)         the definition: every primitive's box tested, in tree order
    walk(recs, prims, boxes, root, queries, margin, user_sphere=None, first=)  the pruned walk, which child is entered first a parameter
    pairs(recs, prims, boxes, root, margin)                                    the pairs: query i = boxes[i], the items j > i

All return (offsets uint32 (n + 1,), items int32 (total,)). `recs` (R, 4, 4), `prims` (P, 3, 4) and `boxes` (P, 6) are the device's arrays,
`root` = (root_min, root_max, root_ref), `queries` (n, 6) = lo.xyz, hi.xyz.

item     primitive j is an item of query q iff qlo[k] <= bhi_j[k] and blo_j[k] <= qhi[k] for k = 0, 1, 2 — touching counts. The user sphere
         (c, R) takes part through the box c -+ R with ordinal -2. A query that is not box_ok has an empty list.
order    the user sphere first, then the unpruned depth-first walk, lower child first, a leaf's primitives by ascending ordinal.
walk     a child, and the root, is skipped iff its box fails the same test against (qlo, qhi); nothing else is, and what comes off the
         stack is not tested again.
pairs    list i = the list of the query boxes[i] without a user sphere, every j <= i removed; the LOWER ordinal's box is the inflated one.

The `mutant=` flags are the wrong rules the tests must tell from the right one: "strict" (< in place of <=, brute and walk),
"uninflated_child" (walk: the un-inflated box tested at a child and the root), "leaf_box" (walk: a leaf's box, as its parent holds it,
tested in place of its primitives' boxes), and for pairs "inflate_higher" (the higher ordinal's box inflated — which is the margin moved
to the other side of each comparison: lo_i <= hi_j + m in place of lo_i - m <= hi_j) and "pairs_ge" (j >= i listed)."""
import numpy as np

from tests import nearest_ref as NR
from tests import within_ref as WR

F = np.float32


def inflate(boxes, margin):
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    with np.errstate(all="ignore"):
        return boxes[:, :3] - F(margin), boxes[:, 3:] + F(margin)


def box_ok(boxes):
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return np.isfinite(boxes).all(1) & (boxes[:, :3] <= boxes[:, 3:]).all(1)


def margin_ok(margin):
    m = F(margin)
    return bool(m >= 0 and np.isfinite(m))


def overlap(qlo, qhi, blo, bhi, strict=False):
    """(n,) of queries (n, 3) against one box."""
    with np.errstate(invalid="ignore"):
        if strict:
            return ((qlo < bhi) & (blo < qhi)).all(-1)
        return ((qlo <= bhi) & (blo <= qhi)).all(-1)


def user_sphere_box(us):
    return NR.user_sphere_prim(us)[1]


def _csr(lists):
    offsets = np.zeros(len(lists) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64).astype(np.uint32)
    return offsets, np.array([k for l in lists for k in l], np.int32).reshape(-1)


def _arrays(recs, prims, boxes, queries):
    return (np.asarray(recs, F).reshape(-1, 4, 4), np.asarray(prims, F).reshape(-1, 3, 4), np.asarray(boxes, F).reshape(-1, 6),
            np.ascontiguousarray(queries, F).reshape(-1, 6))


def brute_lists(recs, prims, boxes, root, queries, margin, user_sphere=None, mutant=None):
    recs, prims, boxes, queries = _arrays(recs, prims, boxes, queries)
    assert margin_ok(margin)
    ok = box_ok(queries)
    qlo, qhi = inflate(queries, margin)
    strict = mutant == "strict"
    order = WR.tree_order(recs, prims, root[2]) if len(prims) else []
    lists = [[] for _ in range(len(queries))]
    if user_sphere is not None:
        b = user_sphere_box(user_sphere)
        for i in np.nonzero(ok & overlap(qlo, qhi, b[:3], b[3:], strict))[0]:
            lists[i].append(-2)
    for k in order:
        for i in np.nonzero(ok & overlap(qlo, qhi, boxes[k, :3], boxes[k, 3:], strict))[0]:
            lists[i].append(k)
    return lists


def brute(recs, prims, boxes, root, queries, margin, user_sphere=None, mutant=None):
    return _csr(brute_lists(recs, prims, boxes, root, queries, margin, user_sphere, mutant))


def walk(recs, prims, boxes, root, queries, margin, user_sphere=None, first="lower", mutant=None, stats=None):
    """stats (a dict) receives the deepest stack and the box steps."""
    recs, prims, boxes, queries = _arrays(recs, prims, boxes, queries)
    ru = recs.view(np.uint32)
    ok = box_ok(queries)
    qlo, qhi = inflate(queries, margin)
    strict = mutant == "strict"
    deepest = steps = 0
    lists = [[] for _ in range(len(queries))]
    root_lo, root_hi, root_ref = np.asarray(root[0], F), np.asarray(root[1], F), int(root[2])
    for i in range(len(queries)):
        if not ok[i]:
            continue
        lo, hi = qlo[i], qhi[i]
        # what a child is tested against: the inflated box, or — the mutant — the box as given
        clo, chi = (queries[i, :3], queries[i, 3:]) if mutant == "uninflated_child" else (lo, hi)
        if user_sphere is not None:
            b = user_sphere_box(user_sphere)
            if overlap(lo, hi, b[:3], b[3:], strict):
                lists[i].append(-2)
        if not len(prims) or not overlap(clo, chi, root_lo, root_hi, strict):
            continue
        stack = [(root_ref, root_lo, root_hi)]
        while stack:
            deepest = max(deepest, len(stack))
            ref, blo, bhi = stack.pop()
            if ref & NR.REF_LEAF:
                for k in NR.leaf_members(prims, ref):
                    if mutant == "leaf_box" or overlap(lo, hi, boxes[k, :3], boxes[k, 3:], strict):      # (the leaf's box was tested on the way in)
                        lists[i].append(k)
                continue
            steps += 1
            a = (int(ru[ref, 0, 3]), recs[ref, 0, :3], recs[ref, 1, :3])
            b = (int(ru[ref, 1, 3]), recs[ref, 2, :3], recs[ref, 3, :3])
            if first != "lower":
                a, b = b, a
            if overlap(clo, chi, b[1], b[2], strict):
                stack.append(b)
            if overlap(clo, chi, a[1], a[2], strict):
                stack.append(a)
    if stats is not None:
        stats["deepest"], stats["steps"] = deepest, steps
    return _csr(lists)


def pairs_lists(recs, prims, boxes, root, margin, mutant=None):
    recs, prims, boxes, _ = _arrays(recs, prims, boxes, np.zeros((0, 6), F))
    assert margin_ok(margin)
    n = len(boxes)
    order = WR.tree_order(recs, prims, root[2]) if n else []
    ok = box_ok(boxes)
    qlo, qhi = inflate(boxes, margin)
    lists = [[] for _ in range(n)]
    o = np.array(order, np.int64)       # every j at once, in the tree's order
    for i in range(n):
        if not ok[i]:
            continue
        if mutant == "inflate_higher":
            hit = ok[o] & overlap(qlo[o], qhi[o], boxes[i, :3], boxes[i, 3:])
        else:
            hit = overlap(qlo[i], qhi[i], boxes[o, :3], boxes[o, 3:])
        keep = hit & ((o >= i) if mutant == "pairs_ge" else (o > i))
        lists[i] = o[keep].tolist()
    return lists


def pairs(recs, prims, boxes, root, margin, mutant=None):
    return _csr(pairs_lists(recs, prims, boxes, root, margin, mutant))


def lists_of(res):
    o, it = res
    o = np.asarray(o).astype(np.int64)
    return [np.asarray(it)[o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


def as_pairs(res):
    """(total, 2) int32 of (i, j) from the CSR of the pairs."""
    o, it = res
    i = np.repeat(np.arange(len(o) - 1, dtype=np.int32), np.diff(np.asarray(o).astype(np.int64)))
    return np.stack([i, np.asarray(it, np.int32)], 1).reshape(-1, 2)
