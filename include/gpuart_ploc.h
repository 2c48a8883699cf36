/* gpuart_ploc.h — C ABI of libgpuart_ploc.so: the tree of an uploaded scene rebuilt on the device by locally-ordered clustering (PLOC,
 * Meister & Bittner 2018; MI355X, gfx950). Where the Morton rebuild (include/gpuart_build.h) takes its topology from the keys alone, this
 * one starts from the same order and lets neighbouring clusters merge by the area of their common box: a large primitive stays unmerged
 * until the top of the tree, and leaves pair what lies together. Like the Morton build the library reads the arrays
 * gpuart_hip_scene_device hands out and writes the spare set gpuart_hip_scene_reserve hands out (reserve n_prims - 1 records); the caller
 * tells the context afterwards (gpuart_hip_scene_rebuilt). gpuart_build_cost measures the result. DESIGN.md "Clustered rebuild".
 *
 * The contract (tests/ploc_ref.py restates it in NumPy). All in fp32 with denormals kept and no contraction:
 *   order     the Morton contract's keys (csrc/hip/tree_rule.h morton_key) and a stable sort by key; sorted position p is initial cluster
 *             p, which holds one primitive and has that primitive's box (prim_boxes);
 *   iteration over the cluster array C[0..c), c > 1, with radius r = GPUART_PLOC_RADIUS:
 *     distance  d(i,j), i != j, |i - j| <= r: the box of the cluster at the lower position folded with the other's by the refit rule's fold
 *               (`<` / `>`, the first of equal values stays), e = hi - lo, d = (e.x*e.y + e.y*e.z) + e.z*e.x;
 *     nearest   nn(i) = the j that minimises (d(i,j), i xor j) lexicographically (the xor breaks ties symmetrically: the smallest
 *               (d, i xor j, min(i,j)) of the array is a mutual pair, so every iteration merges at least once);
 *     merge     every pair with nn(nn(i)) = i, i < nn(i), merges into i's slot: cluster i the lower child, nn(i) the upper child, the box
 *               the fold above. Two clusters of one primitive each become a leaf of two (i's primitive first) and make no record;
 *               anything else is an interior node, and a one-primitive cluster merged with a larger one stays a leaf of one;
 *     compact   the surviving clusters keep their order;
 *   end       c = 1. n_prims = 1: the root is a leaf of one; 2: a leaf of two; else n_recs = leaves - 1 <= n_prims - 1 records. A build that
 *             needs more than GPUART_PLOC_MAX_ITERATIONS iterations is refused (a level needs an iteration: the depth stays within the
 *             uploader's 1024);
 *   layout    pre-order, lower child first; the primitives in the order of the leaves. The boxes are the refit rule's, which are the
 *             boxes the clustering carried; the refs tree_rule::leaf_ref's.
 * The device arrays after a run are what gpuart_hip_upload_bvh makes of that tree, byte for byte in every word the device reads.
 *
 * Device sequence, on the handle's stream; kernel boundaries are the only synchronisation between workgroups, a kernel reads only what
 * an earlier launch wrote, and atomics only count: keys; a stable radix sort of (key, ordinal) (rocPRIM); init (the initial clusters);
 * per iteration nearest (256 clusters and their 2r neighbours staged in LDS), merge (mutual pairs -> keep and new-node flags), an
 * exclusive scan of the flags (rocPRIM), scatter (the new nodes made, the survivors compacted) and a read-back of 8 bytes {c, nodes};
 * number (every node walks its parent links to the root: record index, first primitive, depth); permute; emit; one small read-back.
 *
 * Conventions as gpuart_build.h: 0 or a negative gpuart_hip_status; the last failure's message (per thread) from
 * gpuart_ploc_last_error(), beginning "ploc:". One handle per device; it owns its HIP stream and its scratch memory. */
#ifndef GPUART_PLOC_H
#define GPUART_PLOC_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_ploc gpuart_ploc;

#define GPUART_PLOC_RADIUS 8u
#define GPUART_PLOC_MAX_ITERATIONS 1024u

typedef struct gpuart_ploc_result {
    uint64_t n_recs;      /* leaves - 1 */
    uint32_t root_ref;    /* 0, or the leaf ref when the root is a leaf */
    uint32_t max_depth;   /* level of the deepest node (root = 0) */
    uint32_t subnormal;   /* some box plane of the built tree is within 2^-60 of zero without being zero */
    uint32_t iterations;  /* iterations of the clustering */
    float root_min[3], root_max[3];
} gpuart_ploc_result;

int gpuart_ploc_create(int device, gpuart_ploc **out);
int gpuart_ploc_destroy(gpuart_ploc *h);

/* Builds the tree of src's primitives into dst's arrays: reads src->prims, src->prim_boxes, src->n_prims and src's root box; writes
 * dst->recs (result->n_recs records; room for n_prims - 1 is asked for), dst->prims, dst->prim_boxes (n_prims each) and new_to_old
 * (n_prims uint32, device memory, 4-byte aligned). Synchronous. *result (may be NULL) is filled on success. GPUART_HIP_ERR_ARG, with
 * nothing of dst to be adopted, for a tree with exact_boxes, an empty scene (the dummy leaf of count 0), an unknown layout, a root box
 * that is not finite and ordered, NULL or misaligned pointers, dst->n_recs < n_prims - 1 or dst->n_prims too small, dst arrays that
 * alias src's, and a scene that needs more than GPUART_PLOC_MAX_ITERATIONS iterations. */
int gpuart_ploc_run(gpuart_ploc *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_ploc_result *result);
/* The same with new_to_old in host memory (n_prims uint32), staged through the handle's memory. */
int gpuart_ploc_run_host(gpuart_ploc *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_ploc_result *result);

/* Device time in ms of the steps of the last run: keys, sort, the iterations in total (with their read-backs), number, emit, permute. */
int gpuart_ploc_step_ms(gpuart_ploc *h, double ms[6]);
/* Waits for the handle's stream. */
int gpuart_ploc_finish(gpuart_ploc *h);
const char *gpuart_ploc_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_PLOC_H */
