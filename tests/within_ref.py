"""A plain restatement of the neighbour-list contract (include/gpuart_nearest.h, "Neighbour lists"), in NumPy float32, written from the
header and not from csrc/: the point rule, box_d2 and "is this a query" are tests/nearest_ref.py's.

    tree_order(recs, prims, root_ref, first="lower")                       the ordinals in the order of the unpruned depth-first walk
    brute(recs, prims, boxes, root, points, user_sphere=None)              the definition: every primitive tested, in tree order
    walk(recs, prims, boxes, root, points, user_sphere=None, first=)       the pruned walk, which child is entered first a parameter

Both return (offsets uint32 (n + 1), items HIT (total,)). `recs` (R, 4, 4), `prims` (P, 3, 4) and `boxes` (P, 6) are the device's arrays,
`root` = (root_min, root_max, root_ref), `points` (n, 4) = p.xyz, r.

list     r2 = r r in fp32. The list of (p, r) holds one record per primitive with d2 <= r2, d2 = dist2(p, closest_on_prim(..)): sqrt(d2), q, d2,
         the ordinal, the type, 0 — the record the closest-point query writes for that primitive alone. The user sphere (c, R) is the
         sphere record {c}{R} with box c -+ R, ordinal -2 and type 0, under the same acceptance. r NaN or negative, or a word of p that is
         not finite: an empty list.
order    the user sphere first; then the primitives as the unpruned depth-first walk from the root ref meets them, a record's lower child
         (word 3 of its first quad) before its upper one (word 3 of its second), a leaf's primitives by ascending ordinal.
walk     a child is skipped iff box_d2(child) > r2, the root likewise; nothing else is.
output   offsets[0] = 0, offsets[i + 1] - offsets[i] = the length of list i; items list after list.

The `mutant=` flags are the wrong rules the tests must tell from the right one: brute takes "strict_accept" (d2 < r2) and "no_clamp"; walk
takes "prune_ge" (a child at exactly r2 is skipped), "skip_second" (the second primitive of a leaf of two is not tested) and "best_so_far"
(the closest-point walk's prune: a child farther than the nearest item so far is skipped)."""
import numpy as np

from tests import nearest_ref as NR

F = np.float32
HIT = NR.HIT


def tree_order(recs, prims, root_ref, first="lower"):
    """The ordinals as the unpruned walk meets them. first: "lower" (the contract) or "upper"."""
    ru = np.asarray(recs, F).reshape(-1, 4, 4).view(np.uint32)
    prims = np.asarray(prims, F).reshape(-1, 3, 4)
    out, stack = [], [int(root_ref)]
    while stack:
        ref = stack.pop()
        if ref & NR.REF_LEAF:
            out.extend(NR.leaf_members(prims, ref))
            continue
        lo, hi = int(ru[ref, 0, 3]), int(ru[ref, 1, 3])
        stack.extend([hi, lo] if first == "lower" else [lo, hi])
    return out


def _candidates(prims, boxes, p, user_sphere, clamp=True):
    """ordinal -> (q (n, 3), d2 (n,), type) for every primitive, and -2 for the user sphere."""
    cand = {}
    if user_sphere is not None:
        rec, box = NR.user_sphere_prim(user_sphere)
        cand[-2] = NR.closest_on_prim(rec, box, p) + (0,)
    for k in range(len(prims)):
        cand[k] = NR.closest_on_prim(prims[k], boxes[k], p, clamp=clamp) + (NR._type(prims[k]),)
    return cand


def _csr(lists, cand):
    """(offsets, items) of per-query lists of ordinals."""
    offsets = np.zeros(len(lists) + 1, np.uint32)
    offsets[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64).astype(np.uint32)
    items = np.zeros(int(sum(len(l) for l in lists)), HIT)
    at = 0
    for i, l in enumerate(lists):
        for k in l:
            q, d2, t = cand[k]
            it = items[at]
            it["dist"], it["q"], it["d2"], it["prim"], it["type"] = np.sqrt(d2[i]), q[i], d2[i], k, t
            at += 1
    return offsets, items


def _arrays(recs, prims, boxes, points):
    return (np.asarray(recs, F).reshape(-1, 4, 4), np.asarray(prims, F).reshape(-1, 3, 4), np.asarray(boxes, F).reshape(-1, 6),
            np.ascontiguousarray(points, F).reshape(-1, 4))


def brute(recs, prims, boxes, root, points, user_sphere=None, mutant=None):
    recs, prims, boxes, points = _arrays(recs, prims, boxes, points)
    p = points[:, :3]
    ok = NR.query_ok(points)
    with np.errstate(all="ignore"):
        r2 = points[:, 3] * points[:, 3]
    cand = _candidates(prims, boxes, p, user_sphere, clamp=mutant != "no_clamp")
    order = ([-2] if user_sphere is not None else []) + (tree_order(recs, prims, root[2]) if len(prims) else [])
    lists = [[] for _ in range(len(points))]
    for k in order:
        d2 = cand[k][1]
        with np.errstate(invalid="ignore"):
            acc = ok & ((d2 < r2) if mutant == "strict_accept" else (d2 <= r2))
        for i in np.nonzero(acc)[0]:
            lists[i].append(k)
    return _csr(lists, cand)


def walk(recs, prims, boxes, root, points, user_sphere=None, first="lower", mutant=None, stats=None):
    """stats (a dict) receives the deepest stack."""
    recs, prims, boxes, points = _arrays(recs, prims, boxes, points)
    deepest = 0
    ru = recs.view(np.uint32)
    p = points[:, :3]
    n = len(points)
    ok = NR.query_ok(points)
    with np.errstate(all="ignore"):
        r2 = points[:, 3] * points[:, 3]
    cand = _candidates(prims, boxes, p, user_sphere)
    child_d2 = np.zeros((len(recs), 2, n), F)
    for r in range(len(recs)):
        child_d2[r, 0], child_d2[r, 1] = NR.box_d2(recs[r, 0, :3], recs[r, 1, :3], p), NR.box_d2(recs[r, 2, :3], recs[r, 3, :3], p)
    root_lo, root_hi, root_ref = root
    root_d2 = NR.box_d2(root_lo, root_hi, p)
    lists = [[] for _ in range(n)]
    for i in range(n):
        if not ok[i]:
            continue
        best = np.inf       # (only the "best_so_far" mutant looks at it)

        def pruned(b):
            if mutant == "prune_ge":
                return b >= r2[i]
            if mutant == "best_so_far":
                return b > r2[i] or b > best
            return b > r2[i]

        def offer(k):
            nonlocal best
            d2 = cand[k][1][i]
            if d2 <= r2[i]:
                lists[i].append(k)
                best = min(best, d2)

        if user_sphere is not None:
            offer(-2)
        if not len(prims) or pruned(root_d2[i]):
            continue
        stack = [(int(root_ref), root_d2[i])]
        while stack:
            deepest = max(deepest, len(stack))
            ref, b = stack.pop()
            if mutant == "best_so_far" and pruned(b):      # as the closest-point walk: tested again when it comes off the stack
                continue
            if ref & NR.REF_LEAF:
                members = NR.leaf_members(prims, ref)
                if mutant == "skip_second" and ref & NR.REF_TWO:
                    members = members[:1]
                for k in members:
                    offer(k)
                continue
            lo, hi = (int(ru[ref, 0, 3]), child_d2[ref, 0, i]), (int(ru[ref, 1, 3]), child_d2[ref, 1, i])
            a, b = (lo, hi) if first == "lower" else (hi, lo)
            if not pruned(b[1]):
                stack.append(b)
            if not pruned(a[1]):
                stack.append(a)
    if stats is not None:
        stats["deepest"] = deepest
    return _csr(lists, cand)
