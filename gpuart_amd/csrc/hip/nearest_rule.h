// nearest_rule.h — the closest-point rule of include/gpuart_nearest.h, stated once for the kernel (nearest/nearest.hip: k_nearest), the
// definition on host arrays (gpuart_nearest_brute_host) and whoever else wants it: the point of a primitive's surface nearest to a point,
// from the primitive's 48-byte device record and its box, the squared distance of a point to a box, and the order of two candidates.
// Host and device, plain C++ like prim_rule.h: fp32 with no contraction, IEEE division and square root, denormals kept (every includer is
// built so); only + - * / sqrtf, comparisons and selects, each in a fixed order, so that NumPy float32 restates it word for word
// (tests/nearest_ref.py, which does not read this file).
//
// THE LEMMA the pruned walk rests on. Let B = [lo, hi] be a finite, ordered box, q a point of B (every component lo <= q <= hi) and p any
// finite point. Then, computed in fp32 by the lines below,   box_d2(lo, hi, p) <= dist2(p, q),   bit for bit, with no margin.
//   Per axis, c = clamp(p, lo, hi) is p itself (inside), lo (below) or hi (above). Inside: p - c = 0. Below: q >= lo > p, so in the reals
//   0 < lo - p <= q - p; above likewise. Hence |p - c| <= |p - q| in the reals, the two differences have the same sign, and fp32
//   subtraction (correctly rounded, hence monotone in either operand) keeps the order: |fl(p - c)| <= |fl(p - q)|. Squaring a magnitude
//   is monotone under correct rounding, and so is each of the two additions of the fixed-order sum (dx*dx + dy*dy) + dz*dz in each operand;
//   an overflow to +inf keeps the order as well. No NaN arises: the operands are finite, and inf - inf, 0 * inf do not occur.
//   A box inside another (lo' <= lo, hi <= hi') has its clamp point inside the outer one, so the same argument gives
//   box_d2(outer) <= box_d2(inner): along a root-to-leaf path of a tree with nested boxes box_d2 never decreases, and it ends at or below the d2
//   of every primitive of the leaf, because closest_on_prim clamps its answer into the primitive's own box, which the leaf's box holds.
//   So a walk that skips a child only when box_d2(child) > best_d2 STRICTLY (or > r*r) never skips a primitive whose d2 is <= best_d2:
//   neither the winner nor one that ties with it. Equality does occur (a point on a face of both boxes; 7e5 of 1.6e7 random triples):
//   that is why the prune is strict, and why a walk in ANY child order returns the same record as the brute force over all primitives.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NR_FN __host__ __device__ static inline
#else
#define NR_FN static inline
#endif

namespace nearest_rule {

enum { SPHERE = 0, DISC = 1, TRIANGLE = 2, CONE = 3 };
constexpr uint32_t NO_PRIM = 0xffffffffu;      ///< "nothing accepted yet": above every ordinal
constexpr uint32_t USER_SPHERE = 0xfffffffeu;  ///< the user sphere's ordinal, -2: above every tree primitive's, so it loses every tie

/// x into [lo, hi] (lo <= hi): selects only. A NaN x goes to lo, so the result always lies in the box.
NR_FN float clamp1(float x, float lo, float hi) {
    const float a = x > lo ? x : lo;
    return a < hi ? a : hi;
}

NR_FN float dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

/// The squared distance of p to the clamped point q: d = p - q, (dx*dx + dy*dy) + dz*dz.
NR_FN float dist2(const float p[3], const float q[3]) {
    const float d[3] = {p[0] - q[0], p[1] - q[1], p[2] - q[2]};
    return dot3(d, d);
}

/// The squared distance of p to the box [lo, hi].
NR_FN float box_d2(const float lo[3], const float hi[3], const float p[3]) {
    const float q[3] = {clamp1(p[0], lo[0], hi[0]), clamp1(p[1], lo[1], hi[1]), clamp1(p[2], lo[2], hi[2])};
    return dist2(p, q);
}

/// a / b where b > 0, else 0: a degenerate primitive's zero denominator (or a NaN one) selects the start of its edge or axis.
NR_FN float ratio(float a, float b) { return b > 0.0f ? a / b : 0.0f; }

// ---- q_raw per type, from the record's twelve words (device_scene.h: the 48-byte records) ---------------------------------------------
/// Sphere {c, T}{r}: the surface point on the ray from c through p; a p at the centre (or so near that |p - c|^2 is 0) goes to +x.
NR_FN void sphere_point(const float *rec, const float p[3], float q[3]) {
    const float r = rec[4];
    const float v[3] = {p[0] - rec[0], p[1] - rec[1], p[2] - rec[2]};
    const float len = sqrtf(dot3(v, v));
    if (len > 0.0f) {
        const float s = r / len;
        for (int k = 0; k < 3; k++) q[k] = rec[k] + v[k] * s;
    } else {
        q[0] = rec[0] + r; q[1] = rec[1]; q[2] = rec[2];
    }
}

/// Disc {c, T}{n, r}: p projected into the plane, w = (p - c) - n (n . (p - c)); inside the radius (|w|^2 <= r*r) c + w, else the rim
/// c + w (r / |w|).
NR_FN void disc_point(const float *rec, const float p[3], float q[3]) {
    const float *n = rec + 4, r = rec[7];
    const float v[3] = {p[0] - rec[0], p[1] - rec[1], p[2] - rec[2]};
    const float h = dot3(v, n);
    const float w[3] = {v[0] - n[0] * h, v[1] - n[1] * h, v[2] - n[2] * h};
    const float w2 = dot3(w, w);
    const float s = w2 <= r * r ? 1.0f : r / sqrtf(w2);  // (w2 > r*r >= 0: the root is not 0)
    for (int k = 0; k < 3; k++) q[k] = rec[k] + w[k] * s;
}

/// Triangle {v0, T}{e1}{e2}: the seven Voronoi regions of a = v0, b = v0 + e1, c = v0 + e2, tested in the order a, b, ab, c, ac, bc,
/// face (Ericson, Real-Time Collision Detection 5.1.5, on the record's edges: bp = ap - e1, cp = ap - e2).
NR_FN void triangle_point(const float *rec, const float p[3], float q[3]) {
    const float *e1 = rec + 4, *e2 = rec + 8;
    const float ap[3] = {p[0] - rec[0], p[1] - rec[1], p[2] - rec[2]};
    const float d1 = dot3(e1, ap), d2 = dot3(e2, ap);
    float s = 0.0f, t = 0.0f;  // q_raw = v0 + e1 s + e2 t
    const float bp[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
    const float d3 = dot3(e1, bp), d4 = dot3(e2, bp);
    const float cp[3] = {ap[0] - e2[0], ap[1] - e2[1], ap[2] - e2[2]};
    const float d5 = dot3(e1, cp), d6 = dot3(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (d1 <= 0.0f && d2 <= 0.0f) { s = 0.0f; t = 0.0f; }                                       // a
    else if (d3 >= 0.0f && d4 <= d3) { s = 1.0f; t = 0.0f; }                                    // b
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { s = ratio(d1, d1 - d3); t = 0.0f; }      // edge ab
    else if (d6 >= 0.0f && d5 <= d6) { s = 0.0f; t = 1.0f; }                                    // c
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { s = 0.0f; t = ratio(d2, d2 - d6); }      // edge ac
    else if (va <= 0.0f && d4 - d3 >= 0.0f && d5 - d6 >= 0.0f) {                                // edge bc
        t = ratio(d4 - d3, (d4 - d3) + (d5 - d6));
        s = 1.0f - t;
    } else {                                                                                    // the face
        const float den = (va + vb) + vc;
        s = ratio(vb, den);
        t = ratio(vc, den);
    }
    for (int k = 0; k < 3; k++) q[k] = (rec[k] + e1[k] * s) + e2[k] * t;
}

/// Cone {c1, T}{axis, len}{r1, widthCoeff, ..}: the lateral surface between t = 0 and t = len, what cone_hit intersects (no caps). In the
/// half-plane (t, rho) of p — t = axis . (p - c1), rho the length of the part of p - c1 perpendicular to the axis — the surface is the
/// segment (0, r1) .. (len, r1 + wc len): p's projection on it, its parameter clamped to [0, 1]. The radial direction is p's, made
/// perpendicular to the axis a second time as a unit vector: near the axis w = (p - c1) - axis t is rounding noise of |p - c1|'s size in
/// any direction, the axis' own included, and a radial direction tilted out of the perpendicular plane would leave the surface. Where
/// that second pass removes more than half of the unit vector — p is on the axis as far as fp32 can tell — and for w = 0 the direction is
/// a fixed perpendicular: the axis crossed with the coordinate axis of its smallest component, normalised ((1, 0, 0) for a zero axis).
NR_FN void cone_point(const float *rec, const float p[3], float q[3]) {
    const float *ax = rec + 4, len = rec[7], r1 = rec[8], wc = rec[9];
    const float v[3] = {p[0] - rec[0], p[1] - rec[1], p[2] - rec[2]};
    const float t = dot3(v, ax);
    float u[3] = {v[0] - ax[0] * t, v[1] - ax[1] * t, v[2] - ax[2] * t};
    float rho = sqrtf(dot3(u, u)), n = 0.0f;
    if (rho > 0.0f) {
        for (int k = 0; k < 3; k++) u[k] = u[k] / rho;
        const float e = dot3(u, ax);
        for (int k = 0; k < 3; k++) u[k] = u[k] - ax[k] * e;
        n = sqrtf(dot3(u, u));
    }
    if (n >= 0.5f) {
        for (int k = 0; k < 3; k++) u[k] = u[k] / n;
        rho = rho * n;
    } else {
        const float a0 = fabsf(ax[0]), a1 = fabsf(ax[1]), a2 = fabsf(ax[2]);
        if (a0 <= a1 && a0 <= a2) { u[0] = 0.0f; u[1] = ax[2]; u[2] = -ax[1]; }
        else if (a1 <= a2) { u[0] = -ax[2]; u[1] = 0.0f; u[2] = ax[0]; }
        else { u[0] = ax[1]; u[1] = -ax[0]; u[2] = 0.0f; }
        n = sqrtf(dot3(u, u));
        if (!(n > 0.0f)) { u[0] = 1.0f; u[1] = 0.0f; u[2] = 0.0f; n = 1.0f; }
        for (int k = 0; k < 3; k++) u[k] = u[k] / n;
        rho = 0.0f;
    }
    const float dr = wc * len;
    const float s = clamp1(ratio(t * len + (rho - r1) * dr, len * len + dr * dr), 0.0f, 1.0f);
    const float ts = len * s, rs = r1 + dr * s;
    for (int k = 0; k < 3; k++) q[k] = (rec[k] + ax[k] * ts) + u[k] * rs;
}

/// The point q of the primitive's surface nearest to p, clamped into the primitive's own box (box: min xyz, max xyz), and d2 = dist2(p, q).
/// rec: the record's twelve words; word 3's low two bits are the type (the leaf count above them is ignored).
NR_FN float closest_on_prim(uint32_t type, const float *rec, const float *box, const float p[3], float q[3]) {
    float raw[3];
    type &= 3u;
    if (type == SPHERE) sphere_point(rec, p, raw);
    else if (type == DISC) disc_point(rec, p, raw);
    else if (type == TRIANGLE) triangle_point(rec, p, raw);
    else cone_point(rec, p, raw);
    for (int k = 0; k < 3; k++) q[k] = clamp1(raw[k], box[k], box[3 + k]);
    return dist2(p, q);
}

// ---- the query ------------------------------------------------------------------------------------------------------------------------
/// Is (p, r) a query at all: r neither NaN nor negative, every word of p finite.
NR_FN bool query_ok(const float p[3], float r) {
    return r >= 0.0f && fabsf(p[0]) < INFINITY && fabsf(p[1]) < INFINITY && fabsf(p[2]) < INFINITY;
}

/// Does the candidate (d2, ord) replace the best so far (best_d2, best_ord; nothing yet: +inf, NO_PRIM) of a query of squared radius r2:
/// accepted (d2 <= r2), and nearer or equally near with the lower ordinal. A NaN d2 loses.
NR_FN bool better(float d2, uint32_t ord, float r2, float best_d2, uint32_t best_ord) {
    return d2 <= r2 && (d2 < best_d2 || (d2 == best_d2 && ord < best_ord));
}

/// Is the child whose box is at squared distance b skipped: strictly beyond the best so far, or beyond the radius.
NR_FN bool pruned(float b, float r2, float best_d2) { return b > best_d2 || b > r2; }

// ---- the neighbour list: every primitive within r, not the nearest one (gpuart_nearest_within_*) -------------------------------------
/// Is the primitive at squared distance d2 an item of the list of a query of squared radius r2. A NaN d2 is not.
NR_FN bool within_accept(float d2, float r2) { return d2 <= r2; }

/// Is the child whose box is at squared distance b skipped by a list's walk: beyond the radius, strictly. There is no best so far. By the
/// lemma b <= d2 of everything below the child, so b > r2 implies d2 > r2 for all of it: the walk loses no item.
NR_FN bool within_pruned(float b, float r2) { return b > r2; }

// ---- box overlap: every primitive whose box meets a query box (gpuart_nearest_overlap_*, gpuart_nearest_pairs_*) ------------------------
// The query is a box [lo, hi] and one margin m >= 0 per call; what is tested is the INFLATED box qlo = fl(lo - m), qhi = fl(hi + m), each
// component one fp32 operation (an overflow to -+inf is allowed: such a side reaches everything). A primitive is an item if and only if
// its own box [blo, bhi] (prim_boxes) satisfies qlo <= bhi && blo <= qhi on all three axes: touching counts. Comparisons of stored
// numbers only: nothing rounds behind the two subtractions and additions that made q.
//   THE LEMMA of the overlap walk. If b = [blo, bhi] lies inside B = [Blo, Bhi] (Blo <= blo, bhi <= Bhi: what gpuart_nearest_bind checks
//   of every child and every leaf's primitives) and q overlaps b, then q overlaps B: qlo <= bhi <= Bhi and Blo <= blo <= qhi, per axis.
//   So a walk that skips a child — or the root — exactly when its box fails overlap_test against the same (qlo, qhi) loses no item.
//   The margin is on the QUERY's side, once: in fp32 fl(lo_i - m) <= hi_j and lo_i <= fl(hi_j + m) can disagree (lo_i = 1,
//   hi_j = 1 - 2^-24, m = 2^-25: false and true), so for pairs the contract says whose box is inflated — the lower ordinal's.
/// Is m a margin: neither NaN nor negative nor infinite.
NR_FN bool overlap_margin_ok(float m) { return m >= 0.0f && m < INFINITY; }

/// Is box (lo.xyz, hi.xyz) a query at all: six finite words, lo <= hi on every axis (tree_rule::box_ok, written out: a NaN fails).
NR_FN bool overlap_query_ok(const float box[6]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && box[k] <= box[3 + k] && fabsf(box[k]) < INFINITY && fabsf(box[3 + k]) < INFINITY;
    return ok;
}

/// The inflated query: qlo = lo - m, qhi = hi + m.
NR_FN void overlap_inflate(const float box[6], float m, float qlo[3], float qhi[3]) {
    for (int k = 0; k < 3; k++) {
        qlo[k] = box[k] - m;
        qhi[k] = box[3 + k] + m;
    }
}

/// Does the inflated query (qlo, qhi) meet the box (blo, bhi): the item test, and — negated — the walk's prune.
NR_FN bool overlap_test(const float qlo[3], const float qhi[3], const float blo[3], const float bhi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && qlo[k] <= bhi[k] && blo[k] <= qhi[k];
    return ok;
}

/// Is primitive j an item of the pair list of primitive i: strictly above it, so a pair {i, j} appears once, in the lower ordinal's list.
NR_FN bool pairs_keep(uint32_t i, uint32_t j) { return j > i; }

// ---- the k nearest: the first k of the accepted primitives in the order below (gpuart_nearest_knn_*) -----------------------------------
/// Does the candidate (d2a, orda) come before (d2b, ordb) in an answer: nearer, or equally near with the lower ordinal — `better` without
/// the acceptance. USER_SPHERE is above every tree ordinal, so the user sphere comes after every tree primitive of equal d2.
NR_FN bool knn_before(float d2a, uint32_t orda, float d2b, uint32_t ordb) { return d2a < d2b || (d2a == d2b && orda < ordb); }

/// Is the child whose box is at squared distance b skipped by a k-nearest walk: beyond the radius, or — only once k candidates are kept
/// (`full`) — strictly beyond the d2 of the worst kept. The lemma's corollary, extended: b <= d2 of everything below the child, so
/// b > worst_d2 puts all of it strictly behind every kept candidate, and what is kept later only comes before the worst of now: nothing
/// pruned can precede anything in the answer. At b == worst_d2 a primitive of lower ordinal may lie below: the prune is strict.
NR_FN bool knn_pruned(float b, float r2, bool full, float worst_d2) { return b > r2 || (full && b > worst_d2); }

}  // namespace nearest_rule
