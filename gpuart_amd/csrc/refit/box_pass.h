// box_pass.h — the box pass of a tree in device memory, shared by refit/refit.hip and treebuild/build.hip (each one translation unit that
// includes this once, after tree/tree_lib.h): one launch of k_rf_level per tree level, deepest first, then k_rf_root. A leaf's box is its
// primitives' boxes folded in leaf order, an interior node's its lower child's folded with its upper child's (include/gpuart_refit.h).
// Nothing is handed between workgroups inside a launch: a level reads what the launch before it wrote (DESIGN.md "Refit").
// ploc/ploc.hip takes the Status and k_rf_root from here.
#pragma once

namespace {

#define RF_FN __device__ __forceinline__

/// What the device sequence leaves for the host, in device memory; all zero before a run. `refused`: tree_lib.h's refusal word.
struct Status {
    uint32_t refused;
    uint32_t subnormal;  ///< some plane written fails tree_rule::plane_ok (a subnormal number is kept here, and fails it)
    float root_min[3], root_max[3];
};

RF_FN bool planes_ok(const float lo[3], const float hi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && tree_rule::plane_ok(lo[k]) && tree_rule::plane_ok(hi[k]);
    return ok;
}

/// The box of the leaf whose primitives start at `first`: its primitives' boxes folded in leaf order; the count is in the first record.
RF_FN void leaf_box(const float4 *prims, const float *pbox, uint32_t first, float lo[3], float hi[3]) {
    const uint32_t cnt = __float_as_uint(prims[3 * (size_t)first].w) >> 2;
    prim_rule::box_start(lo, hi);
    for (uint32_t k = 0; k < cnt; k++) {
        const float *b = pbox + 6 * ((size_t)first + k);
        prim_rule::box_fold(lo, hi, b, b + 3);
    }
}

/// The box of the interior node with record `r`: its lower child's box folded with its upper child's.
RF_FN void record_box(const float4 *recs, uint32_t r, float lo[3], float hi[3]) {
    const float4 *q = recs + 4 * (size_t)r;
    const float4 a = q[0], b = q[1], c = q[2], d = q[3];
    const float llo[3] = {a.x, a.y, a.z}, lhi[3] = {b.x, b.y, b.z}, hlo[3] = {c.x, c.y, c.z}, hhi[3] = {d.x, d.y, d.z};
    prim_rule::box_start(lo, hi);
    prim_rule::box_fold(lo, hi, llo, lhi);
    prim_rule::box_fold(lo, hi, hlo, hhi);
}

RF_FN void node_box(const float4 *recs, const float4 *prims, const float *pbox, uint32_t ref, float lo[3], float hi[3]) {
    if (ref & REF_LEAF) leaf_box(prims, pbox, ref & REF_INDEX, lo, hi);
    else record_box(recs, ref, lo, hi);
}

// 3. One level of the tree: one thread per child of each of the level's records (`order` lists them). A leaf child's box comes from its
// primitives' boxes, an interior child's from that child's own record, which a launch before this one wrote (it lies a level deeper).
// The thread writes the twelve box floats of its child's two quads and leaves their fourth words alone: the refs, the
// GPUART_HIP_TOP_DEPTH mark and the pad. Like the update it does nothing once an update is refused.
__global__ void __launch_bounds__(256) k_rf_level(const uint32_t *order, uint32_t count, float4 *recs, const float4 *prims, const float *pbox, Status *st) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= 2u * count || st->refused) return;
    const uint32_t r = order[t >> 1], c = t & 1u;
    float4 *q = recs + 4 * (size_t)r;
    const uint32_t ref = __float_as_uint(q[c].w);  // the lower child's ref is word 3 of quad 0, the upper child's of quad 1
    float lo[3], hi[3];
    node_box(recs, prims, pbox, ref, lo, hi);
    float *f = (float *)(q + 2 * c);  // (the fourth words are not stored to: the sibling's thread reads one of them)
    for (int k = 0; k < 3; k++) { f[k] = lo[k]; f[4 + k] = hi[k]; }
    if (!planes_ok(lo, hi)) atomicOr(&st->subnormal, 1u);
}

// 4. The root's box, after the top level: from record 0, or from the primitives when the root is a leaf.
__global__ void k_rf_root(const float4 *recs, const float4 *prims, const float *pbox, uint32_t root_ref, Status *st) {
    if (blockIdx.x || threadIdx.x || st->refused) return;
    float lo[3], hi[3];
    node_box(recs, prims, pbox, root_ref, lo, hi);
    for (int k = 0; k < 3; k++) { st->root_min[k] = lo[k]; st->root_max[k] = hi[k]; }
    if (!planes_ok(lo, hi)) atomicOr(&st->subnormal, 1u);
}

}  // namespace
