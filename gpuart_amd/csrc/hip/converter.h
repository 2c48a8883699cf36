// converter.h — host side of gpuart_hip_upload_bvh: validates the reference's canonical compiled tree (RGBA32F quads,
// reference src/bvh.cpp:161-222) and re-lays it out as 64-byte two-children records + 48-byte primitive records
// (DESIGN.md section 3). Host code only; included by gpuart_hip.hip.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>
#include <vector>

#include "device_scene.h"
#include "prim_rule.h"

namespace {

using namespace gd;

// ---- canonical tree -> device layout ---------------------------------------------------------------
/// std::allocator whose value-less construct() leaves trivial elements uninitialised: the device arrays are touched for the first
/// time by the threads that fill them (every element is written), not zeroed by one thread beforehand.
template <class T>
struct UninitAlloc : std::allocator<T> {
    template <class U> struct rebind { using other = UninitAlloc<U>; };
    template <class U> void construct(U *p) { ::new ((void *)p) U; }
    template <class U, class A0, class... A> void construct(U *p, A0 &&a0, A &&...a) { ::new ((void *)p) U(std::forward<A0>(a0), std::forward<A>(a)...); }
};

struct Converter {
    const float *q;
    size_t nq;
    std::vector<float4, UninitAlloc<float4>> recs, prims;
    std::vector<float, UninitAlloc<float>> pbox;  ///< per device primitive its constructor's box (min xyz, max xyz): what a refit folds a leaf's box from
    size_t num_nodes = 0;
    uint32_t type_mask = 0;
    uint32_t max_depth = 0;
    uint32_t top_depth = 0;  ///< records of nodes above this level are marked (pad word of the record; counters only)
    std::string err;

    static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
    static float fbits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

    /// Appends the device record of one canonical primitive payload (type + data quads).
    static bool pack_prim(uint32_t type, const float *d, float4 rec[3]) {
        float T = fbits(type);
        switch (type) {
        case P_SPHERE:
            rec[0] = make_float4(d[0], d[1], d[2], T); rec[1] = make_float4(d[3], 0, 0, 0); rec[2] = make_float4(0, 0, 0, 0);
            return true;
        case P_DISC:
            rec[0] = make_float4(d[0], d[1], d[2], T); rec[1] = make_float4(d[4], d[5], d[6], d[3]); rec[2] = make_float4(0, 0, 0, 0);
            return true;
        case P_TRIANGLE:
            rec[0] = make_float4(d[0], d[1], d[2], T);
            rec[1] = make_float4(d[4] - d[0], d[5] - d[1], d[6] - d[2], 0);   // edge1 = v1 - v0
            rec[2] = make_float4(d[8] - d[0], d[9] - d[1], d[10] - d[2], 0);  // edge2 = v2 - v0
            return true;
        case P_CONE:
            rec[0] = make_float4(d[0], d[1], d[2], T);
            rec[1] = make_float4(d[8], d[9], d[10], d[11]);
            rec[2] = make_float4(d[3], d[12], d[13], d[14]);
            return true;
        }
        return false;
    }

    /// Result of converting one canonical node: its box and the ref its parent stores for it.
    struct Child {
        float bmin[3], bmax[3];
        uint32_t ref;
    };

    /// A box that is inverted (min > max on some axis: e.g. a sphere with a negative radius, or the empty scene) or holds
    /// a NaN is irregular: the device's fast box test (med3) assumes min <= max, while the reference's comparisons can
    /// still hit such a box through the two planes of its one irregular axis. An infinite bound is irregular too: a plane at
    /// +-inf gives the reference a legitimate candidate with parameter +inf ("intersected", entry stays 1e19), which the
    /// fast test cannot tell from no candidate. Boxes are uploaded as they are; a tree with an irregular box anywhere makes
    /// every box test take the comparison form (Scene::exact_boxes, device_scene.h). With finite, ordered bounds the two
    /// forms agree for every ray, NaN / infinite origins and directions included. (The condition is tree_rule.h box_ok.)
    bool irregular = false;
    void note(const Child &c) { irregular = irregular || !tree_rule::box_ok(c.bmin, c.bmax); }

    /// May the fast kernels visit this tree's nodes in their own order (nearer child first, device_scene.h "Visiting order")? Their
    /// certificate rests on boxes that bound what they hold: every child box inside its parent's, every primitive inside its
    /// leaf's box by the very formulas the reference's constructors use (reference src/core.cpp:36-65,80-90,136-150,217-225) —
    /// which only bound a primitive with radii >= 0 and, for a cone, with derived constants (axis, length, width coefficient)
    /// that agree with its two centres and radii. Hostile input (negative radii, NaN, a hand-made tree) fails this and keeps
    /// the reference's order throughout, like a tree with irregular boxes.
    bool disorderly = false;
    /// Some box plane lies within 2^-60 of zero without being zero (a subnormal number, which the device reads as zero, included): the
    /// quick box answers (box_quick.h: gq_plane_ok) are sized for planes that are zero or at least 2^-60 in magnitude — there the
    /// signs of a ray's plane parameters decide the inside test exactly —, such a tree runs its six face tests every time.
    bool subnormal = false;
    static bool tiny(const Child &c) {
        bool r = false;
        for (int k = 0; k < 3; k++) r = r || !gq_plane_ok(c.bmin[k]) || !gq_plane_ok(c.bmax[k]);
        return r;
    }
    static bool box_in_box(const float *cmin, const float *cmax, const float *bmin, const float *bmax) {
        bool ok = true;
        for (int k = 0; k < 3; k++) ok = ok && cmin[k] >= bmin[k] && cmax[k] <= bmax[k] && cmin[k] <= cmax[k];  // NaN fails
        return ok;
    }
    /// A primitive lies inside a box when it meets the preconditions of prim_rule.h (magnitudes, radii, a cone's derived constants) and
    /// the box its constructor gives it (lo, hi: prim_rule::prim_box, which the caller keeps) does.
    static bool prim_in_box(uint32_t type, const float *d, const float *lo, const float *hi, const float *bmin, const float *bmax) {
        return prim_rule::prim_ok(type, d) && box_in_box(lo, hi, bmin, bmax);
    }

    /// What the scan keeps of a canonical node: where it lies, the ref its parent stores for it, and (interior nodes) which
    /// entry of the table its upper child is — its lower child is the next entry (pre-order).
    struct NodeInfo {
        uint32_t addr, ref, hi_index, depth;
    };
    std::vector<NodeInfo> table;
    size_t n_recs = 0, n_prims = 0;

    /// Pass 1 — headers only: validates the subtree at quad address `addr` and numbers its records and primitives, in the
    /// order the device arrays keep them (interior nodes in pre-order, so an interior lower child's record directly follows
    /// its parent's; leaves append their primitives). `end` receives the address just past the subtree. Compile (reference
    /// src/bvh.cpp:161-222) lays subtrees out contiguously in pre-order, so an upper child must start exactly where its
    /// sibling's subtree ends: this is what rules out overlapping (DAG-shaped) inputs, whose conversion would otherwise take
    /// exponential time. Returns the node's entry in `table`.
    bool scan(size_t addr, uint32_t depth, uint32_t &index, size_t &end) {
        if (addr + 3 > nq) { err = "node address out of range"; return false; }
        if (depth > 1024) { err = "tree deeper than 1024 levels"; return false; }
        if (depth > max_depth) max_depth = depth;
        num_nodes++;
        index = (uint32_t)table.size();
        table.push_back(NodeInfo{(uint32_t)addr, 0, 0, depth});
        const float *b = q + 4 * addr;
        uint32_t flags = bits(b[8]);
        if (flags & 0x80000000u) {
            uint32_t n = flags & ~0xE0000000u;
            // (a primitive's byte offset, 48 x index, and a record's, 64 x index, fit 32 bits: the kernels address both as base + 32-bit
            //  offset, device_scene.h trav_step_box and the leaf tests — 89 million primitives / 67 million interior nodes; the reference's own format ends at
            //  2^31 floats = 76 million triangles with their leaves)
            if (n_prims >= 0x05555540u) { err = "too many primitives"; return false; }
            const uint32_t first = (uint32_t)n_prims;
            size_t a = addr + 3;
            static const int LEN[4] = {1, 2, 3, 4};
            bool all_tris = true;
            for (uint32_t i = 0; i < n; i++) {
                if (a + 1 > nq) { err = "primitive header out of range"; return false; }
                uint32_t type = bits(q[4 * a]);
                if (type > 3) { err = "unknown primitive type"; return false; }
                if (type != P_TRIANGLE) all_tris = false;
                type_mask |= 1u << type;
                if (a + 1 + LEN[type] > nq) { err = "primitive data out of range"; return false; }
                a += 1 + LEN[type];
            }
            n_prims += n ? n : 1;  // an empty leaf (empty scene) keeps one dummy record with count 0
            table[index].ref = tree_rule::leaf_ref(first, n, all_tris);
            end = a;
            return true;
        }
        uint32_t lo = bits(b[9]), hi = bits(b[10]);
        if (lo != addr + 3) { err = "lower child does not follow its parent"; return false; }
        if (hi <= lo || hi >= nq) { err = "upper child address out of range"; return false; }
        if (n_recs >= 0x03fffff0u) { err = "too many nodes"; return false; }
        table[index].ref = (uint32_t)n_recs++;
        uint32_t lo_index, hi_index;
        size_t lo_end = 0;
        if (!scan(lo, depth + 1, lo_index, lo_end)) return false;
        if (hi != lo_end) { err = "upper child does not start where the lower subtree ends"; return false; }
        if (!scan(hi, depth + 1, hi_index, end)) return false;
        table[index].hi_index = hi_index;
        return true;
    }

    Child child_of(const NodeInfo &n) const {
        Child c;
        const float *b = q + 4 * (size_t)n.addr;
        for (int k = 0; k < 3; k++) { c.bmin[k] = b[k]; c.bmax[k] = b[4 + k]; }
        c.ref = n.ref;
        return c;
    }

    /// Pass 2 — the entries [from, to) of the table into the device arrays (disjoint writes: any number of threads).
    /// Returns whether one of the boxes written is irregular.
    bool fill(size_t from, size_t to, bool &loose, bool &sub) {
        bool irr = false;
        auto bad = [](const Child &c) { return !tree_rule::box_ok(c.bmin, c.bmax); };
        static const int LEN[4] = {1, 2, 3, 4};
        for (size_t i = from; i < to; i++) {
            const NodeInfo &n = table[i];
            const float *b = q + 4 * (size_t)n.addr;
            if (n.ref & GD_REF_LEAF) {
                const uint32_t cnt = bits(b[8]) & ~0xE0000000u;
                float4 *dst = prims.data() + 3 * (size_t)(n.ref & GD_REF_INDEX);
                size_t a = (size_t)n.addr + 3;
                for (uint32_t k = 0; k < cnt; k++) {
                    const uint32_t type = bits(q[4 * a]);
                    pack_prim(type, q + 4 * (a + 1), dst + 3 * k);
                    float *pb = pbox.data() + 6 * ((size_t)(n.ref & GD_REF_INDEX) + k);
                    prim_rule::prim_box(type, q + 4 * (a + 1), pb, pb + 3);
                    loose = loose || !prim_in_box(type, q + 4 * (a + 1), pb, pb + 3, b, b + 4);
                    if (k == 0) dst[0].w = fbits(type | (cnt << 2));  // the first primitive carries the leaf's count
                    a += 1 + LEN[type];
                }
                if (cnt == 0) {
                    dst[0] = make_float4(0, 0, 0, fbits(0)); dst[1] = make_float4(0, 0, 0, 0); dst[2] = make_float4(0, 0, 0, 0);
                    float *pb = pbox.data() + 6 * (size_t)(n.ref & GD_REF_INDEX);
                    prim_rule::box_start(pb, pb + 3);
                }
            } else {
                const Child L = child_of(table[i + 1]), H = child_of(table[n.hi_index]);
                irr = irr || bad(L) || bad(H);
                sub = sub || tiny(L) || tiny(H);
                loose = loose || !box_in_box(L.bmin, L.bmax, b, b + 4) || !box_in_box(H.bmin, H.bmax, b, b + 4);
                float4 *r = recs.data() + 4 * (size_t)n.ref;
                r[0] = make_float4(L.bmin[0], L.bmin[1], L.bmin[2], fbits(L.ref));
                r[1] = make_float4(L.bmax[0], L.bmax[1], L.bmax[2], fbits(H.ref));
                r[2] = make_float4(H.bmin[0], H.bmin[1], H.bmin[2], fbits(n.depth < top_depth ? 1u : 0u));
                r[3] = make_float4(H.bmax[0], H.bmax[1], H.bmax[2], 0);
            }
        }
        return irr;
    }

    /// The whole conversion: scan, then fill on `threads` threads. `root` receives the root's box and ref.
    bool convert(Child &root, unsigned threads) {
        uint32_t index;
        size_t end = 0;
        table.reserve(nq / 6 + 1);
        if (!scan(0, 0, index, end)) return false;
        recs.resize(4 * n_recs);
        prims.resize(3 * n_prims);
        pbox.resize(6 * n_prims);
        root = child_of(table[0]);
        note(root);
        const size_t n = table.size();
        const unsigned parts = (unsigned)std::max<size_t>(1, std::min<size_t>(threads, n / 16384));
        std::vector<char> irr(parts, 0), loose(parts, 0), sub(parts, 0);
        subnormal = tiny(root);
        std::vector<std::thread> pool;
        auto work = [&](unsigned k) { bool l = false, t = false; irr[k] = fill(n * k / parts, n * (size_t)(k + 1) / parts, l, t) ? 1 : 0; loose[k] = l ? 1 : 0; sub[k] = t ? 1 : 0; };
        for (unsigned k = 1; k < parts; k++) {
            try { pool.emplace_back(work, k); } catch (const std::system_error &) { work(k); }
        }
        work(0);
        for (auto &t : pool) t.join();
        for (char v : irr) irregular = irregular || v;
        for (char v : loose) disorderly = disorderly || v;
        for (char v : sub) subnormal = subnormal || v;
        std::vector<NodeInfo>().swap(table);
        return true;
    }
};

}  // namespace
