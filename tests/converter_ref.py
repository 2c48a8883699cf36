"""A plain restatement of what gpuart_hip_upload_bvh makes of a compiled tree, written from the two FORMATS and not from csrc/hip/converter.h.

Canonical side (the reference's src/bvh.cpp, the comment in CompileFrom; Primitive::StoreIntoBVH and the StoreDataIntoBVH of the four
primitives in src/core.h / src/core.cpp). The tree is an array of RGBA32F quads. A node is three quads,

    { xmin, ymin, zmin, PAD }  { xmax, ymax, zmax, PAD }  { flags | num_primitives, lo_addr, hi_addr, parent_addr }

with addresses counted in quads and the words of the third quad read as uint32: LEAF = bit 31, IS_LOWER = bit 30, IS_ROOT = bit 29, the
primitive count below them. An interior node is followed at once by its lower child's subtree (lo_addr = its own address + 3), and that by
its upper child's (hi_addr = where the lower subtree ends): the tree is one contiguous pre-order run. A leaf is followed by its primitives,
each a header quad { type, PAD, PAD, PAD } and then its data quads:

    sphere   (0), 1 quad : { c.xyz, r }
    disc     (1), 2 quads: { c.xyz, r } { n.xyz, PAD }
    triangle (2), 3 quads: { v0.xyz, PAD } { v1.xyz, PAD } { v2.xyz, PAD }
    cone     (3), 4 quads: { c1.xyz, r1 } { c2.xyz, r2 } { axis.xyz, len } { widthCoeff, cosB, dotAxC1, PAD }

Device side (the header comment of csrc/hip/device_scene.h):

    recs  : one record of four quads per INTERIOR node, in pre-order: { lo.min, lo ref } { lo.max, hi ref } { hi.min, mark } { hi.max, 0 }.
            A ref is the record index of an interior child, or bit 31 | first primitive of a leaf — | bit 30 when the leaf holds one or two
            primitives, all triangles; | bit 28 when it holds one or two primitives, not all triangles; | bit 29 when it holds two.
            mark = 1 in the records of nodes above level top_depth (a counter's input, GPUART_HIP_TOP_DEPTH), else 0.
    prims : one record of three quads per primitive, in the order the leaves are met; an empty leaf keeps one record of zeros.
            sphere { c, T } { r, 0, 0, 0 } { 0 }; disc { c, T } { n, r } { 0 }; triangle { v0, T } { v1 - v0, 0 } { v2 - v0, 0 } (fp32);
            cone { c1, T } { axis, len } { r1, widthCoeff, cosB, dotAxC1 }.   T = type | count << 2 on a leaf's first primitive, else type.

WHAT THE DEVICE NEVER READS, and so what this restatement ignores: the parent address (word 3 of a node's third quad), IS_ROOT and IS_LOWER,
words 1 and 2 of a leaf's third quad, and every PAD word above (of the two box quads, of a primitive's header, of a disc's second quad, of
a triangle's three quads, of a cone's fourth) — and cone centre 2 / radius 2 beyond the box they bound.

The three classifications (csrc/hip/box_quick.h gq_plane_ok), over every node's box:
    irregular : some box has min > max on an axis, a NaN or an infinite bound;
    subnormal : some box plane is neither zero nor at least 2^-60 in magnitude (NaN included);
    disorderly: some child box is not inside its parent's (or is itself inverted), or some primitive is not inside its leaf's box by the
                formulas of the reference's constructors (src/core.cpp: sphere and disc c -+ r; triangle the extremes of its vertices; cone
                min(c1 - r1, c2 - r2) .. max(c1 + r1, c2 + r2)), or has a negative radius / length, or a non-pad data word beyond 2^20 in
                magnitude (NaN included). The uploader additionally holds a cone's derived constants to its centres and radii within
                tolerances; those are NOT restated here (tests/test_host_parity.py::test_uploader_classifies_trees_for_the_visiting_order pins
                them): for a tree with cones, `disorderly` here implies the uploader's, and equals it when the cones are honest.

Everything is iterative (one explicit stack) and shares no control flow with the uploader's recursion.
"""
import numpy as np

LEAF, IS_LOWER, IS_ROOT = 1 << 31, 1 << 30, 1 << 29
COUNT_MASK = (1 << 29) - 1
REF_LEAF, REF_TRIS, REF_TWO, REF_SMALL, REF_INDEX = 1 << 31, 1 << 30, 1 << 29, 1 << 28, (1 << 28) - 1
DATA_QUADS = (1, 2, 3, 4)            # StoreDataIntoBVH of sphere, disc, triangle, cone
NON_PAD = ([0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6], [0, 1, 2, 4, 5, 6, 8, 9, 10], list(range(15)))
MAX_DEPTH = 1024
MAX_PRIMS = 0x05555540               # 48 bytes x index and 64 bytes x index fit 32 bits on the device (device_scene.h trav_step_box and the leaf tests)
MAX_RECS = 0x03fffff0
COORD_LIMIT = np.float32(1048576.0)  # 2^20
PLANE_MIN = np.float32(2.0 ** -60)


class Rejected(Exception):
    """The tree is malformed; str(e) is the uploader's reason."""


def _scan(u, nq):
    """Numbers the nodes in pre-order. Returns per node (addr, depth, ref, parent node or -1) and per primitive (header address, type,
    the leaf's node, the T word), or raises Rejected."""
    addr_, depth_, ref_, parent_, hi_of = [], [], [], [], {}
    p_addr, p_type, p_leaf, p_T = [], [], [], []
    n_recs = n_prims = 0
    cursor = 0      # where the subtree met last ends
    stack = [("node", 0, 0, -1, False)]
    while stack:
        item = stack.pop()
        if item[0] == "upper starts":
            if item[1] != cursor:
                raise Rejected("upper child does not start where the lower subtree ends")
            continue
        _, addr, depth, parent, is_upper = item
        if addr + 3 > nq:
            raise Rejected("node address out of range")
        if depth > MAX_DEPTH:
            raise Rejected("tree deeper than 1024 levels")
        me = len(addr_)
        addr_.append(addr); depth_.append(depth); parent_.append(parent)
        if is_upper:
            hi_of[parent] = me
        flags = u[4 * addr + 8]
        if flags & LEAF:
            count = flags & COUNT_MASK
            if n_prims >= MAX_PRIMS:
                raise Rejected("too many primitives")
            a = addr + 3
            types = []
            for _k in range(count):
                if a + 1 > nq:
                    raise Rejected("primitive header out of range")
                t = u[4 * a]
                if t > 3:
                    raise Rejected("unknown primitive type")
                if a + 1 + DATA_QUADS[t] > nq:
                    raise Rejected("primitive data out of range")
                p_addr.append(a); p_type.append(t); p_leaf.append(me); p_T.append(t | (count << 2) if not types else t)
                types.append(t)
                a += 1 + DATA_QUADS[t]
            ref = REF_LEAF | n_prims
            if count in (1, 2):
                ref |= REF_TRIS if all(t == 2 for t in types) else REF_SMALL
            if count == 2:
                ref |= REF_TWO
            if count == 0:   # the one dummy record of an empty leaf
                p_addr.append(-1); p_type.append(-1); p_leaf.append(me); p_T.append(0)
            n_prims += max(count, 1)
            ref_.append(ref)
            cursor = a
        else:
            lo, hi = u[4 * addr + 9], u[4 * addr + 10]
            if lo != addr + 3:
                raise Rejected("lower child does not follow its parent")
            if hi <= lo or hi >= nq:
                raise Rejected("upper child address out of range")
            if n_recs >= MAX_RECS:
                raise Rejected("too many nodes")
            ref_.append(n_recs)
            n_recs += 1
            stack.append(("node", hi, depth + 1, me, True))
            stack.append(("upper starts", hi))
            stack.append(("node", lo, depth + 1, me, False))
    nodes = dict(addr=np.array(addr_, np.int64), depth=np.array(depth_, np.int64), ref=np.array(ref_, np.uint32), parent=np.array(parent_, np.int64))
    hi = np.full(len(addr_), -1, np.int64)
    if hi_of:
        hi[np.fromiter(hi_of.keys(), np.int64, len(hi_of))] = np.fromiter(hi_of.values(), np.int64, len(hi_of))
    nodes["hi"] = hi
    prims = dict(addr=np.array(p_addr, np.int64), type=np.array(p_type, np.int64), leaf=np.array(p_leaf, np.int64), T=np.array(p_T, np.uint32))
    return nodes, prims, n_recs, n_prims


def plane_ok(p):
    """Zero, or at least 2^-60 in magnitude (false for NaN)."""
    return (p == 0) | (np.abs(p) >= PLANE_MIN)


def _inside(cmin, cmax, bmin, bmax):
    """Rows of (n, 3): min >= the outer min, max <= the outer max, and ordered itself (any NaN fails)."""
    return ((cmin >= bmin) & (cmax <= bmax) & (cmin <= cmax)).all(1)


def convert(quads, nquads=None, top_depth=0):
    """The outputs of binding.convert_tree for the first `nquads` quads (default: all), or Rejected. One more key, `refs`: every node's ref in
    pre-order (the root's first) — what a test's conditions on its inputs are read from."""
    q = np.ascontiguousarray(quads, np.float32).reshape(-1)
    nq = q.size // 4 if nquads is None else int(nquads)
    f = q[:4 * nq]                    # nothing beyond nquads exists for the restatement
    uw = f.view(np.uint32)
    nodes, prims, n_recs, n_prims = _scan(uw.tolist(), nq)
    addr, depth, ref, parent, hi = nodes["addr"], nodes["depth"], nodes["ref"], nodes["parent"], nodes["hi"]
    base = 4 * addr
    bmin = f[base[:, None] + np.arange(3)]
    bmax = f[base[:, None] + 4 + np.arange(3)]

    # ---- records
    inner = np.flatnonzero((ref & np.uint32(REF_LEAF)) == 0)
    assert len(inner) == n_recs and (ref[inner] == np.arange(n_recs)).all()
    lo_i, hi_i = inner + 1, hi[inner]
    recs = np.zeros((n_recs, 4, 4), np.float32)
    ru = recs.view(np.uint32)
    recs[:, 0, :3], recs[:, 1, :3], recs[:, 2, :3], recs[:, 3, :3] = bmin[lo_i], bmax[lo_i], bmin[hi_i], bmax[hi_i]
    ru[:, 0, 3], ru[:, 1, 3] = ref[lo_i], ref[hi_i]
    ru[:, 2, 3] = (depth[inner] < top_depth).astype(np.uint32)

    # ---- primitives
    out = np.zeros((n_prims, 3, 4), np.float32)
    ou = out.view(np.uint32)
    assert len(prims["addr"]) == n_prims
    ou[:, 0, 3] = prims["T"]
    d_of = lambda sel, k: f[(4 * (prims["addr"][sel] + 1))[:, None] + np.asarray(k)]
    loose = np.zeros(n_prims, bool)
    lbmin, lbmax = bmin[prims["leaf"]], bmax[prims["leaf"]]
    for t in range(4):
        sel = np.flatnonzero(prims["type"] == t)
        if not len(sel):
            continue
        d = d_of(sel, np.arange(15 if t == 3 else 4 * DATA_QUADS[t]))
        out[sel, 0, :3] = d[:, 0:3]
        if t == 0:
            out[sel, 1, 0] = d[:, 3]
            ok = d[:, 3] >= 0
            lo, hi_ = d[:, 0:3] - d[:, 3:4], d[:, 0:3] + d[:, 3:4]
        elif t == 1:
            out[sel, 1, :3], out[sel, 1, 3] = d[:, 4:7], d[:, 3]
            ok = d[:, 3] >= 0
            lo, hi_ = d[:, 0:3] - d[:, 3:4], d[:, 0:3] + d[:, 3:4]
        elif t == 2:
            with np.errstate(invalid="ignore", over="ignore"):
                out[sel, 1, :3], out[sel, 2, :3] = d[:, 4:7] - d[:, 0:3], d[:, 8:11] - d[:, 0:3]
            ok = np.ones(len(sel), bool)
            v = np.stack([d[:, 0:3], d[:, 4:7], d[:, 8:11]])
            with np.errstate(invalid="ignore"):
                lo, hi_ = v.min(0), v.max(0)
        else:
            out[sel, 1, :], out[sel, 2, 0], out[sel, 2, 1:] = d[:, 8:12], d[:, 3], d[:, 12:15]
            ok = (d[:, 3] >= 0) & (d[:, 7] >= 0) & (d[:, 11] >= 0)
            with np.errstate(invalid="ignore", over="ignore"):
                lo = np.minimum(d[:, 0:3] - d[:, 3:4], d[:, 4:7] - d[:, 7:8])
                hi_ = np.maximum(d[:, 0:3] + d[:, 3:4], d[:, 4:7] + d[:, 7:8])
        with np.errstate(invalid="ignore", over="ignore"):
            ok &= (np.abs(d[:, NON_PAD[t]]) <= COORD_LIMIT).all(1)
            ok &= _inside(lo, hi_, lbmin[sel], lbmax[sel])
        loose[sel] = ~ok

    # ---- classification
    with np.errstate(invalid="ignore"):
        irregular = bool((~(bmin <= bmax) | np.isinf(bmin) | np.isinf(bmax)).any())
        subnormal = bool((~plane_ok(bmin) | ~plane_ok(bmax)).any())
        kids = np.flatnonzero(parent >= 0)
        disorderly = bool(loose.any() or (~_inside(bmin[kids], bmax[kids], bmin[parent[kids]], bmax[parent[kids]])).any())
    type_mask = 0
    for t in np.unique(prims["type"][prims["type"] >= 0]):
        type_mask |= 1 << int(t)
    return dict(recs=recs, prims=out, root_min=bmin[0].copy(), root_max=bmax[0].copy(), root_ref=int(ref[0]), num_nodes=len(addr),
                max_depth=int(depth.max()), type_mask=type_mask, irregular=irregular, disorderly=disorderly, subnormal=subnormal, refs=ref)


def layout(quads):
    """Where an accepted tree's nodes and primitives lie, in pre-order: dict(addr, depth, parent, leaf (bool) per node; prim_addr (header quad),
    prim_type per primitive) — for tests that edit a chosen node or word."""
    q = np.ascontiguousarray(quads, np.float32).reshape(-1)
    nodes, prims, _, _ = _scan(q.view(np.uint32).tolist(), q.size // 4)
    real = prims["type"] >= 0
    return dict(addr=nodes["addr"], depth=nodes["depth"], parent=nodes["parent"], leaf=(nodes["ref"] & np.uint32(REF_LEAF)) != 0,
                prim_addr=prims["addr"][real], prim_type=prims["type"][real])


def verdict(quads, nquads=None):
    """None if the tree is accepted, else the reason."""
    try:
        convert(quads, nquads)
        return None
    except Rejected as e:
        return str(e)
