"""A plain restatement of the k-nearest contract (include/gpuart_nearest.h, "k nearest"), in NumPy float32, written from the header and not
from csrc/: the point rule, box_d2 and "is this a query" are tests/nearest_ref.py's, a primitive's record is tests/within_ref.py's.

    brute(prims, boxes, points, k, user_sphere=None, mutant=None)                        the definition: every primitive tested, then sorted
    walk(recs, prims, boxes, root, points, k, user_sphere=None, order="nearer", mutant=None)   the pruned walk, child order a parameter

Both return HIT records (n, k). `prims` (P, 3, 4) and `boxes` (P, 6) are the device's primitive records and boxes, `recs` (R, 4, 4) its tree
records, `root` = (root_min, root_max, root_ref), `points` (n, 4) = p.xyz, r.

candidates  r2 = r r in fp32. Every primitive with d2 <= r2, d2 = dist2(p, closest_on_prim(..)), and the user sphere (c, R) — the sphere
            record {c}{R} with box c -+ R, ordinal -2, type 0 — under the same acceptance. r NaN or negative, or a word of p that is not
            finite: none.
order       ascending d2; equal d2 by ascending ordinal taken as uint32, so that the user sphere (0xfffffffe) is behind every primitive.
answer      row i: the first k candidates of query i in that order, each as sqrt(d2), q, d2, the ordinal, the type, 0; then misses:
            -1, 0, 0, 0, 0, -1, -1, 0.
walk        the kept: the (at most k) first candidates met so far. A child is skipped iff box_d2(child) > r2, or k are kept and
            box_d2(child) > the d2 of the last of them, strictly; tested when its parent's record is read and again when it comes off the
            stack; the root box likewise before the root. The user sphere is met first.

The `mutant=` flags are the wrong rules the tests must tell from the right one: brute takes "no_clamp"; walk takes "prune_ge" (a child at
exactly the worst kept d2 is skipped), "before_full" (the worst kept prunes while fewer than k are kept), "d2_only" (once k are kept a
candidate must be strictly nearer than the worst: a tie never evicts it) and "unsorted" (the kept are a binary max-heap, as a kernel
would keep them, and are written in the heap's order)."""
import numpy as np

from tests import nearest_ref as NR
from tests import within_ref as WR

F = np.float32
HIT = NR.HIT
ORDERS = NR.ORDERS


def _key(d2, ordinal):
    return (d2, ordinal & 0xffffffff)


def _records(lists, cand, k):
    """(n, k) HIT records of per-query lists of ordinals."""
    out = np.zeros((len(lists), k), HIT)
    out["dist"], out["prim"], out["type"] = F(-1), -1, -1
    for i, l in enumerate(lists):
        for j, o in enumerate(l):
            q, d2, t = cand[o]
            it = out[i, j]
            it["dist"], it["q"], it["d2"], it["prim"], it["type"] = np.sqrt(d2[i]), q[i], d2[i], o, t
    return out


def _queries(points):
    points = np.ascontiguousarray(points, F).reshape(-1, 4)
    with np.errstate(all="ignore"):
        return points, NR.query_ok(points), points[:, 3] * points[:, 3]


def brute(prims, boxes, points, k, user_sphere=None, mutant=None):
    prims = np.asarray(prims, F).reshape(-1, 3, 4)
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    points, ok, r2 = _queries(points)
    cand = WR._candidates(prims, boxes, points[:, :3], user_sphere, clamp=mutant != "no_clamp")
    lists = []
    for i in range(len(points)):
        accepted = [o for o, c in cand.items() if ok[i] and c[1][i] <= r2[i]]
        lists.append(sorted(accepted, key=lambda o: _key(cand[o][1][i], o))[:k])
    return _records(lists, cand, k)


def _heap_push(heap, e):
    """e into the binary max-heap (the last in the order at index 0)."""
    heap.append(e)
    i = len(heap) - 1
    while i and heap[(i - 1) // 2] < e:
        heap[i] = heap[(i - 1) // 2]
        i = (i - 1) // 2
    heap[i] = e


def _heap_replace_root(heap, e):
    i, m = 0, len(heap)
    while 2 * i + 1 < m:
        c = 2 * i + 1
        if c + 1 < m and heap[c] < heap[c + 1]:
            c += 1
        if not e < heap[c]:
            break
        heap[i] = heap[c]
        i = c
    heap[i] = e


def prepare(recs, prims, boxes, root, points, user_sphere=None):
    """What the walks of one scene and one query set share, whatever k, order and mutant: the candidates' points and the box distances."""
    recs = np.asarray(recs, F).reshape(-1, 4, 4)
    prims = np.asarray(prims, F).reshape(-1, 3, 4)
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    points, ok, r2 = _queries(points)
    p = points[:, :3]
    child_d2 = np.zeros((len(recs), 2, len(points)), F)
    for r in range(len(recs)):
        child_d2[r, 0], child_d2[r, 1] = NR.box_d2(recs[r, 0, :3], recs[r, 1, :3], p), NR.box_d2(recs[r, 2, :3], recs[r, 3, :3], p)
    return dict(ru=recs.view(np.uint32), prims=prims, ok=ok, r2=r2, cand=WR._candidates(prims, boxes, p, user_sphere), child_d2=child_d2,
                root_d2=NR.box_d2(root[0], root[1], p), root_ref=int(root[2]), us=user_sphere is not None, n=len(points))


def walk(recs, prims, boxes, root, points, k, user_sphere=None, order="nearer", mutant=None, ctx=None, stats=None):
    """ctx: prepare(...) of the same arguments, to share it between calls. stats (a dict) receives the leaves and records visited."""
    c = ctx if ctx is not None else prepare(recs, prims, boxes, root, points, user_sphere)
    ru, cand, child_d2, r2 = c["ru"], c["cand"], c["child_d2"], c["r2"]
    lists, visited = [], 0
    for i in range(c["n"]):
        kept = []      # a max-heap of (d2, ordinal as uint32, ordinal): kept[0] is the worst
        if not c["ok"][i]:
            lists.append([])
            continue

        def offer(o):
            d2 = cand[o][1][i]
            if not d2 <= r2[i]:
                return
            e = _key(d2, o) + (o,)
            if len(kept) < k:
                _heap_push(kept, e)
            elif (e[0] < kept[0][0]) if mutant == "d2_only" else (e < kept[0]):
                _heap_replace_root(kept, e)

        def pruned(b):
            if b > r2[i]:
                return True
            if mutant == "before_full":
                return bool(kept) and b > kept[0][0]
            if len(kept) < k:
                return False
            return b >= kept[0][0] if mutant == "prune_ge" else b > kept[0][0]

        if c["us"]:
            offer(-2)
        stack = [] if not len(c["prims"]) or pruned(c["root_d2"][i]) else [(c["root_ref"], c["root_d2"][i])]
        while stack:
            ref, b = stack.pop()
            if pruned(b):
                continue
            visited += 1
            if ref & NR.REF_LEAF:
                for o in NR.leaf_members(c["prims"], ref):
                    offer(o)
                continue
            lo, hi = (int(ru[ref, 0, 3]), child_d2[ref, 0, i]), (int(ru[ref, 1, 3]), child_d2[ref, 1, i])
            first, second = (hi, lo) if order == "upper" or (order == "nearer" and hi[1] < lo[1]) else (lo, hi)
            if not pruned(second[1]):
                stack.append(second)
            if not pruned(first[1]):
                stack.append(first)
        lists.append([e[2] for e in (kept if mutant == "unsorted" else sorted(kept))])
    if stats is not None:
        stats["visited"] = visited
    return _records(lists, cand, k)


def found(hits):
    """Per query, how many of its k slots hold a candidate."""
    return (np.asarray(hits)["prim"] != -1).sum(-1)
