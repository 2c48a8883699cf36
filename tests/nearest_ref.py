"""A plain restatement of the closest-point contract (include/gpuart_nearest.h), in NumPy float32, written from the header and not from
csrc/hip/nearest_rule.h:

    brute(prims, boxes, points, user_sphere=None) -> HIT records     the definition: every primitive, in ordinal order
    walk(recs, prims, boxes, root, points, user_sphere=None, order=) the pruned walk over the device records, child order a parameter

`prims` (P, 3, 4) and `boxes` (P, 6) are the device's primitive records and boxes, `recs` (R, 4, 4) its tree records, `root` =
(root_min, root_max, root_ref), `points` (n, 4) = p.xyz, r. Every operation is an fp32 +, -, *, /, sqrt, comparison or select in the order
the header gives (NumPy keeps denormals, never contracts, divides and roots correctly rounded), vectorised over the queries.

point    sphere {c, T}{r}: v = p - c, len = sqrt((vx vx + vy vy) + vz vz); len > 0: c + v (r / len), else (c.x + r, c.y, c.z).
         disc {c, T}{n, r}: h = v . n, w = v - n h, w2 = w . w; c + w s with s = 1 if w2 <= r r else r / sqrt(w2).
         triangle {v0, T}{e1}{e2}: ap = p - v0, bp = ap - e1, cp = ap - e2, d1 = e1.ap, d2 = e2.ap, d3 = e1.bp, d4 = e2.bp, d5 = e1.cp,
           d6 = e2.cp, vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4; the first region that holds, in this order:
           a (d1 <= 0, d2 <= 0): (0, 0); b (d3 >= 0, d4 <= d3): (1, 0); ab (vc <= 0, d1 >= 0, d3 <= 0): (d1 // (d1 - d3), 0);
           c (d6 >= 0, d5 <= d6): (0, 1); ac (vb <= 0, d2 >= 0, d6 <= 0): (0, d2 // (d2 - d6));
           bc (va <= 0, d4 - d3 >= 0, d5 - d6 >= 0): t = (d4 - d3) // ((d4 - d3) + (d5 - d6)), s = 1 - t;
           else the face: den = (va + vb) + vc, (vb // den, vc // den);   q_raw = (v0 + e1 s) + e2 t.   a // b = a / b if b > 0 else 0.
         cone {c1, T}{axis, len}{r1, wc, ..}: t = v . axis, w = v - axis t, rho0 = sqrt(w . w); if rho0 > 0: u0 = w / rho0,
           u1 = u0 - axis (u0 . axis), n = sqrt(u1 . u1), else n = 0; if n >= 0.5: u = u1 / n, rho = rho0 n; else u = the fixed
           perpendicular (axis x the coordinate axis of its smallest component: (0, az, -ay), (-az, 0, ax) or (ay, -ax, 0), ties to the
           earlier), divided by its length ((1, 0, 0) if that is 0), and rho = 0; dr = wc len,
           s = clamp((t len + (rho - r1) dr) // (len len + dr dr), 0, 1); q_raw = (c1 + axis (len s)) + u (r1 + dr s).
clamp    clamp(x, lo, hi) = min'(max'(x, lo), hi) with max'(x, lo) = x if x > lo else lo and min'(a, hi) = a if a < hi else hi.
         q = clamp(q_raw, box_lo, box_hi); d = p - q; d2 = (dx dx + dy dy) + dz dz.   box_d2(lo, hi, p): the same with q = clamp(p, lo, hi).
answer   r2 = r r. A candidate (d2, ordinal) replaces the best (best_d2, best_ordinal; at first +inf, 0xffffffff) iff d2 <= r2 and
         (d2 < best_d2 or (d2 == best_d2 and ordinal < best_ordinal)). The user sphere (c, R) is the sphere record {c}{R} with box c -+ R
         and ordinal 0xfffffffe (-2). A query with r NaN or negative or a non-finite word of p, or with nothing accepted, is a miss.
walk     a child is skipped iff box_d2(child) > best_d2 or box_d2(child) > r2, tested when its parent's record is read and again when
         it comes off the stack; the root box is tested the same way before the root.

The flags of brute and walk (`mutant=`) are the wrong rules the tests must tell from the right one.
"""
import numpy as np

F = np.float32
HIT = np.dtype([("dist", F), ("q", F, (3,)), ("d2", F), ("prim", np.int32), ("type", np.int32), ("zero", np.uint32)])
REF_LEAF, REF_TRIS, REF_TWO, REF_SMALL, REF_INDEX = 1 << 31, 1 << 30, 1 << 29, 1 << 28, (1 << 28) - 1
NO_PRIM, USER_SPHERE = 0xffffffff, 0xfffffffe
ORDERS = ("lower", "upper", "nearer")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _clamp(x, lo, hi):
    a = np.where(x > lo, x, lo)
    return np.where(a < hi, a, hi)


def _ratio(a, b):
    ok = b > 0
    return np.where(ok, a / np.where(ok, b, F(1)), F(0))


def _sphere(rec, p):
    c, r = rec[0, :3], rec[1, 0]
    v = p - c
    ln = np.sqrt(_dot(v, v))
    s = r / np.where(ln > 0, ln, F(1))
    at_centre = np.broadcast_to(np.array([c[0] + r, c[1], c[2]], F), p.shape)
    return np.where((ln > 0)[:, None], c + v * s[:, None], at_centre)


def _disc(rec, p):
    c, n, r = rec[0, :3], rec[1, :3], rec[1, 3]
    v = p - c
    h = _dot(v, n)
    w = v - n * h[:, None]
    w2 = _dot(w, w)
    inside = w2 <= r * r
    s = np.where(inside, F(1), r / np.sqrt(np.where(inside, F(1), w2)))
    return c + w * s[:, None]


def _triangle(rec, p):
    v0, e1, e2 = rec[0, :3], rec[1, :3], rec[2, :3]
    ap = p - v0
    bp, cp = ap - e1, ap - e2
    d1, d2, d3, d4, d5, d6 = _dot(e1, ap), _dot(e2, ap), _dot(e1, bp), _dot(e2, bp), _dot(e1, cp), _dot(e2, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    t_bc = _ratio(d4 - d3, (d4 - d3) + (d5 - d6))
    den = (va + vb) + vc
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    s = np.select(regions, [zero, one, _ratio(d1, d1 - d3), zero, zero, one - t_bc], _ratio(vb, den))
    t = np.select(regions, [zero, zero, zero, one, _ratio(d2, d2 - d6), t_bc], _ratio(vc, den))
    return (v0 + e1 * s[:, None]) + e2 * t[:, None]


def cone_radial(rec, p):
    """(t, n) of the cone rule for the points p: the axial parameter, and the length n of the unit radial vector after its second pass
    (0 where p - c1 has no radial part at all); n < 0.5 takes the fixed perpendicular."""
    c1, ax = rec[0, :3], rec[1, :3]
    v = p - c1
    t = _dot(v, ax)
    u = v - ax * t[:, None]
    rho = np.sqrt(_dot(u, u))
    some = rho > 0
    u = u / np.where(some, rho, F(1))[:, None]
    u = u - ax * _dot(u, ax)[:, None]
    return t, np.where(some, np.sqrt(_dot(u, u)), F(0))


def _cone(rec, p):
    c1, ax, ln, r1, wc = rec[0, :3], rec[1, :3], rec[1, 3], rec[2, 0], rec[2, 1]
    v = p - c1
    t = _dot(v, ax)
    u = v - ax * t[:, None]
    rho = np.sqrt(_dot(u, u))
    some = rho > 0
    u = u / np.where(some, rho, F(1))[:, None]
    u = u - ax * _dot(u, ax)[:, None]
    n = np.where(some, np.sqrt(_dot(u, u)), F(0))
    off = n >= F(0.5)
    a = np.abs(ax)
    if a[0] <= a[1] and a[0] <= a[2]:
        fixed = np.array([F(0), ax[2], -ax[1]], F)
    elif a[1] <= a[2]:
        fixed = np.array([-ax[2], F(0), ax[0]], F)
    else:
        fixed = np.array([ax[1], -ax[0], F(0)], F)
    fl = np.sqrt(_dot(fixed, fixed))
    if not fl > 0:
        fixed, fl = np.array([1, 0, 0], F), F(1)
    fixed = fixed / fl
    u = np.where(off[:, None], u / np.where(off, n, F(1))[:, None], fixed)
    rho = np.where(off, rho * n, F(0))
    dr = wc * ln
    s = _clamp(_ratio(t * ln + (rho - r1) * dr, np.full_like(t, ln * ln + dr * dr)), F(0), F(1))
    return (c1 + ax * (ln * s)[:, None]) + u * (r1 + dr * s)[:, None]


_POINT = (_sphere, _disc, _triangle, _cone)


def closest_on_prim(rec, box, p, clamp=True):
    """(q (n, 3), d2 (n,)) of the points p (n, 3) on the primitive with record rec (3, 4) and box (6,)."""
    rec = np.asarray(rec, F).reshape(3, 4)
    box = np.asarray(box, F)
    t = int(rec.view(np.uint32)[0, 3]) & 3
    with np.errstate(all="ignore"):
        q = _POINT[t](rec, p).astype(F)
        if clamp:
            q = _clamp(q, box[:3], box[3:])
        d = p - q
        return q, _dot(d, d)


def box_d2(lo, hi, p):
    with np.errstate(all="ignore"):
        d = p - _clamp(p, np.asarray(lo, F), np.asarray(hi, F))
        return _dot(d, d)


def query_ok(points):
    with np.errstate(invalid="ignore"):
        return (points[:, 3] >= 0) & (np.abs(points[:, :3]) < np.inf).all(1)


def user_sphere_prim(us):
    """(record, box) the user sphere takes part with."""
    us = np.asarray(us, F)
    rec = np.zeros((3, 4), F)
    rec[0, :3], rec[1, 0] = us[:3], us[3]
    return rec, np.concatenate([us[:3] - us[3], us[:3] + us[3]]).astype(F)


class _Best:
    """The best candidate of every query so far."""

    def __init__(self, points, mutant):
        with np.errstate(all="ignore"):
            self.r2 = points[:, 3] * points[:, 3]
        n = len(points)
        strict = mutant == "strict_accept"     # the wrong rule: best starts at r2 and a candidate must be strictly nearer
        self.d2 = self.r2.copy() if strict else np.full(n, np.inf, F)
        self.strict = strict
        self.ord = np.full(n, NO_PRIM, np.uint32)
        self.type = np.zeros(n, np.int32)
        self.q = np.zeros((n, 3), F)

    def offer(self, sel, q, d2, ordinal, t):
        """The candidate (q, d2) of the queries sel."""
        with np.errstate(invalid="ignore"):
            if self.strict:
                better = d2 < self.d2[sel]
            else:
                better = (d2 <= self.r2[sel]) & ((d2 < self.d2[sel]) | ((d2 == self.d2[sel]) & (np.uint32(ordinal) < self.ord[sel])))
        at = sel[better]
        self.d2[at], self.ord[at], self.type[at], self.q[at] = d2[better], ordinal, t, q[better]

    def hits(self, ok):
        out = np.zeros(len(ok), HIT)
        hit = ok & (self.ord != NO_PRIM)
        out["dist"], out["prim"], out["type"] = F(-1), -1, -1
        out["dist"][hit] = np.sqrt(self.d2[hit])
        out["q"][hit], out["d2"][hit], out["type"][hit] = self.q[hit], self.d2[hit], self.type[hit]
        out["prim"][hit] = self.ord[hit].view(np.int32)
        return out


def _type(rec):
    return int(np.asarray(rec, F).reshape(3, 4).view(np.uint32)[0, 3]) & 3


def brute(prims, boxes, points, user_sphere=None, mutant=None):
    """The definition: HIT records of the queries points (n, 4). mutant: None, "no_clamp" or "strict_accept"."""
    prims = np.asarray(prims, F).reshape(-1, 3, 4)
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    points = np.ascontiguousarray(points, F).reshape(-1, 4)
    p = points[:, :3]
    best = _Best(points, mutant)
    sel = np.arange(len(points))
    if user_sphere is not None:
        rec, box = user_sphere_prim(user_sphere)
        q, d2 = closest_on_prim(rec, box, p)
        best.offer(sel, q, d2, USER_SPHERE, 0)
    for k in range(len(prims)):
        q, d2 = closest_on_prim(prims[k], boxes[k], p, clamp=mutant != "no_clamp")
        best.offer(sel, q, d2, k, _type(prims[k]))
    return best.hits(query_ok(points))


def leaf_members(prims, ref):
    """The ordinals of the leaf `ref`."""
    first = ref & REF_INDEX
    if ref & (REF_TRIS | REF_SMALL):
        return list(range(first, first + (2 if ref & REF_TWO else 1)))
    return list(range(first, first + (int(prims.view(np.uint32)[first, 0, 3]) >> 2)))


def walk(recs, prims, boxes, root, points, user_sphere=None, order="nearer", mutant=None, stats=None):
    """The pruned walk, query by query. order: which child is entered first — "lower", "upper" or "nearer" (the smaller box_d2; equal:
    the lower). mutant: None, "prune_ge" (a child at exactly the best distance is skipped) or "skip_second" (the second primitive of a
    REF_TWO leaf is not tested). stats (a dict) receives the deepest stack."""
    recs = np.asarray(recs, F).reshape(-1, 4, 4)
    prims = np.asarray(prims, F).reshape(-1, 3, 4)
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    points = np.ascontiguousarray(points, F).reshape(-1, 4)
    ru = recs.view(np.uint32)
    p = points[:, :3]
    n = len(points)
    best = _Best(points, None)
    ok = query_ok(points)
    every = np.arange(n)
    if user_sphere is not None:
        rec, box = user_sphere_prim(user_sphere)
        q, d2 = closest_on_prim(rec, box, p)
        best.offer(every, q, d2, USER_SPHERE, 0)
    child_d2 = np.zeros((len(recs), 2, n), F)      # box_d2 of every record's two children, for every query
    for r in range(len(recs)):
        child_d2[r, 0], child_d2[r, 1] = box_d2(recs[r, 0, :3], recs[r, 1, :3], p), box_d2(recs[r, 2, :3], recs[r, 3, :3], p)
    cand = {}

    def candidate(k):
        if k not in cand:
            cand[k] = closest_on_prim(prims[k], boxes[k], p) + (_type(prims[k]),)
        return cand[k]

    def pruned(b, i):
        if mutant == "prune_ge":
            return b >= best.d2[i] or b > best.r2[i]
        return b > best.d2[i] or b > best.r2[i]

    root_lo, root_hi, root_ref = root
    root_d2 = box_d2(root_lo, root_hi, p)
    deepest = 0
    for i in range(n):
        if not ok[i] or pruned(root_d2[i], i):
            continue
        one = every[i:i + 1]
        stack = [(int(root_ref), root_d2[i])]
        while stack:
            deepest = max(deepest, len(stack))
            ref, b = stack.pop()
            if pruned(b, i):
                continue
            if ref & REF_LEAF:
                members = leaf_members(prims, ref)
                if mutant == "skip_second" and ref & REF_TWO:
                    members = members[:1]
                for k in members:
                    q, d2, t = candidate(k)
                    best.offer(one, q[i:i + 1], d2[i:i + 1], k, t)
                continue
            lo, hi = (int(ru[ref, 0, 3]), child_d2[ref, 0, i]), (int(ru[ref, 1, 3]), child_d2[ref, 1, i])
            first, second = (hi, lo) if order == "upper" or (order == "nearer" and hi[1] < lo[1]) else (lo, hi)
            if not pruned(second[1], i):
                stack.append(second)
            if not pruned(first[1], i):
                stack.append(first)
    if stats is not None:
        stats["deepest"] = deepest
    return best.hits(ok)


def from_tree(tree):
    """(recs, prims, boxes, root) of a canonical compiled tree, as the uploader lays it out (tests/converter_ref.py) with the boxes the
    primitives' constructors give them (tests/build_ref.boxes_of)."""
    from tests import build_ref as BR
    from tests import converter_ref as CR
    from tests.test_ray_queries import tree_prims
    cv = CR.convert(tree)
    lo, hi = BR.boxes_of(tree_prims(tree))
    return cv["recs"], cv["prims"], np.concatenate([lo, hi], 1).astype(F), (cv["root_min"], cv["root_max"], cv["root_ref"])
