/* gpuart_build.h — C ABI of libgpuart_build.so: the tree of an uploaded scene rebuilt on the device, in Morton order (MI355X, gfx950).
 * Where a refit (include/gpuart_refit.h) keeps the topology and lets boxes loosen as primitives drift, a rebuild makes a new tree of
 * the primitives as they are now, device to device. The library reads the arrays gpuart_hip_scene_device hands out and writes the spare
 * set gpuart_hip_scene_reserve hands out; it knows nothing of contexts, frames or passes, and the caller tells the context afterwards
 * (gpuart_hip_scene_rebuilt). DESIGN.md "Rebuild" has the contract, the launches and the limits.
 *
 * The contract (tests/build_ref.py restates it in NumPy; the key and delta are written once for the device and the host library,
 * csrc/hip/tree_rule.h, and the host library's BoundingVolumesHierarchy::RebuildMorton is a second statement of the topology only, by
 * bisection). Primitive i has the box its constructor gave it (prim_boxes); R is the scene's root box. All in fp32 with denormals kept,
 * no contraction and IEEE division:
 *   key      per axis k: c = lo_k*0.5f + hi_k*0.5f, e = Rmax_k - Rmin_k, t = (c - Rmin_k) / e,
 *            q_k = e > 0 && t > 0 ? min(2^21 - 1, (uint32)(t * 2097152.0f)) : 0; bit 3b+2 of the key = bit b of q_x, 3b+1 of q_y, 3b of q_z;
 *   order    a stable sort by key: position p is the primitive's new device ordinal, new_to_old[p] its old one;
 *   leaves   leaf j holds positions 2j and 2j+1 (the last leaf one primitive when N is odd), M = ceil(N/2) leaves; K_j = the key of its first;
 *   topology delta(i,j) = clz64(K_i ^ K_j) if the keys differ, else 64 + clz32(i ^ j); the node over leaves [a,b], a < b, splits behind the
 *            largest g in [a,b) with delta(a,g) > delta(a,b): lower child [a,g], upper child [g+1,b]; M = 1: the root is a leaf;
 *   boxes    the refit rule: a leaf's primitives' boxes folded in leaf order, an interior node's lower child's box folded with its upper's;
 *   layout   pre-order, lower child first.
 * The device arrays after a run are what gpuart_hip_upload_bvh makes of that tree, byte for byte in every word the device reads.
 *
 * Device sequence, on the handle's stream; kernel boundaries are the only synchronisation between workgroups in the hand-written
 * launches: keys; a stable radix sort of (key, ordinal) (rocPRIM); permute; hierarchy (one thread per interior node, from the leaf keys
 * alone); number (every node walks its parent links to the root: depth and pre-order index); emit (refs, mark, pad, per-level lists);
 * one read-back of the per-level counts; the refit's level kernel per level, deepest first, and its root kernel; one small read-back.
 *
 * Conventions as gpuart_refit.h: 0 or a negative gpuart_hip_status; the last failure's message (per thread) from
 * gpuart_build_last_error(), beginning "build:". One handle per device; it owns its HIP stream and its scratch memory. */
#ifndef GPUART_BUILD_H
#define GPUART_BUILD_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_build gpuart_build;

#define GPUART_BUILD_MAX_LEVELS 128u /* 63 key bits + 32 index bits bound a tree's depth by 96 */

typedef struct gpuart_build_result {
    uint64_t n_recs;     /* ceil(n_prims / 2) - 1 */
    uint32_t root_ref;   /* 0, or the leaf ref when the root is a leaf */
    uint32_t max_depth;  /* level of the deepest node (root = 0) */
    uint32_t subnormal;  /* some box plane of the built tree is within 2^-60 of zero without being zero */
    uint32_t levels;     /* levels of the records = launches of the level kernel */
    float root_min[3], root_max[3];
} gpuart_build_result;

int gpuart_build_create(int device, gpuart_build **out);
int gpuart_build_destroy(gpuart_build *h);

/* Builds the tree of src's primitives into dst's arrays: reads src->prims, src->prim_boxes, src->n_prims and src's root box; writes
 * dst->recs (ceil(n_prims/2) - 1 records), dst->prims, dst->prim_boxes (n_prims each) and new_to_old (n_prims uint32, device memory,
 * 4-byte aligned). Synchronous. *result (may be NULL) is filled on success. GPUART_HIP_ERR_ARG, with nothing written, for a tree with
 * exact_boxes, an empty scene (the dummy leaf of count 0), an unknown layout, a root box that is not finite and ordered, NULL or
 * misaligned pointers, dst->n_recs or dst->n_prims too small, and dst arrays that alias src's. */
int gpuart_build_run(gpuart_build *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_build_result *result);
/* The same with new_to_old in host memory (n_prims uint32), staged through the handle's memory. */
int gpuart_build_run_host(gpuart_build *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_build_result *result);

/* The cost of the scene's tree: the sum over its records of (half-area of the lower box + half-area of the upper box), divided by the
 * half-area of the root box, in fp64 from the fp32 planes. Workgroups write partial sums in a fixed order and the host adds them in
 * index order: the value is deterministic. 0 for a tree without records or a root box of no area. */
int gpuart_build_cost(gpuart_build *h, const gpuart_hip_scene *scene, double *cost);
/* Device time in ms of the steps of the last run: keys, sort, permute, hierarchy, number, emit, levels (level launches and the root's). */
int gpuart_build_step_ms(gpuart_build *h, double ms[7]);
/* Waits for the handle's stream. */
int gpuart_build_finish(gpuart_build *h);
const char *gpuart_build_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_BUILD_H */
