/* gpuart_edit.h — C ABI of libgpuart_edit.so: primitives of an uploaded scene removed and new ones of any type appended, on the device
 * (MI355X, gfx950). Where the refit (include/gpuart_refit.h) keeps every primitive's type and the count, and the rebuilds
 * (include/gpuart_build.h, include/gpuart_ploc.h) reorder what is there, this library makes the primitive list with another count: the
 * step in front of a builder. It reads the arrays gpuart_hip_scene_device hands out, writes staging arrays of its own and knows nothing
 * of contexts; the caller builds the tree of the edited list into the context's spare set (gpuart_hip_scene_reserve_prims) and tells the
 * context (gpuart_hip_scene_replaced). DESIGN.md "Edit".
 *
 * The contract (tests/edit_ref.py restates it):
 *   list      the edited list holds the primitives of src that are not removed, in their old order, then the added ones in the order
 *             given: n_new = n_old - n_remove + n_add;
 *   record    a survivor's 48-byte record is copied; an added primitive's is written by the uploader's arithmetic from its payload (the
 *             16 floats of GPUART_REFIT_PAYLOAD: a triangle's edges subtracted in fp32 with denormals kept and no contraction, all else
 *             copied). Word 3 of the first quad carries the bare type with no leaf count — the builders write the counts of their
 *             leaves —, except in a list of one primitive, which is the leaf of one both builders take it for: it carries count 1 (a
 *             count of 0 there is the empty scene's dummy record, which the builders refuse);
 *   box       a survivor's box is copied, an added primitive's is the box its constructor gives it (csrc/hip/prim_rule.h);
 *   source    source[q] is the old ordinal of the survivor at q, or n_old + k for the k-th addition;
 *   edited    layout 1, exact_boxes 0, prims and prim_boxes the staging arrays, n_prims = n_new, recs NULL and n_recs 0, generation =
 *             src's, everything else zero but the root box: exactly what gpuart_build_run and gpuart_ploc_run read of their src (prims,
 *             prim_boxes, n_prims, the root box; layout, exact_boxes, recs and n_recs in their checks);
 *   root box  per axis the minimum of the n_new boxes' lower planes and the maximum of their upper planes, from +-99e29, where of two
 *             zeros -0 is the smaller for the minimum and +0 the larger for the maximum: a total order, so every grouping of a parallel
 *             reduction gives the same bits. The sequential fold with `<` and `>` (tests/build_ref.root_box) keeps the first of equal
 *             values instead; the two differ in nothing but the sign of a zero plane, and compare equal with ==. The keys do not depend
 *             on that sign (csrc/hip/tree_rule.h morton_key: c - root_lo and root_hi - root_lo come out the same, t > 0 is false for
 *             either zero), and the tree's own root box comes from the builder's box pass, not from here;
 *   type_mask the OR of 1 << type over the edited list.
 *
 * A run is refused as a whole with GPUART_HIP_ERR_ARG, and nothing outside the handle's own memory and `source` is written: a src with
 * exact_boxes, an empty src, an unknown layout, removals that are not strictly ascending or not below n_prims, a type above 3, a payload
 * outside the primitive rule's preconditions (a word that is not finite or beyond 2^20, a negative radius or length, a cone's derived
 * constants that contradict its centres and radii), n_new = 0, n_new >= 0x05555540 (the uploader's bound), NULL or misaligned pointers
 * where the matching count is above zero. An empty scene is not edited: upload one primitive and edit from there. n_remove = n_add = 0
 * is allowed and yields the scene's own list.
 *
 * Device sequence, on the handle's stream; kernel boundaries are the only synchronisation between workgroups, atomics only set the
 * status word: validate (one thread per removal and per addition); the keep flags; an exclusive scan (rocPRIM); compact (survivors,
 * their boxes, source); append; reduce (per workgroup, then one workgroup over the partial results); one small read-back.
 *
 * Conventions as gpuart_ploc.h: 0 or a negative gpuart_hip_status; the last failure's message (per thread) from
 * gpuart_edit_last_error(), beginning "edit:". One handle per device; it owns its HIP stream and its staging arrays, which the next run
 * overwrites. */
#ifndef GPUART_EDIT_H
#define GPUART_EDIT_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_edit gpuart_edit;

#define GPUART_EDIT_NONE 0xffffffffu
#define GPUART_EDIT_MAX_PRIMS 0x05555540u /* n_new stays below this (csrc/hip/converter.h) */

typedef struct gpuart_edit_result {
    int32_t status;     /* 0, or GPUART_HIP_ERR_ARG: the device sequence refused the edit */
    uint32_t first_bad; /* on such a refusal the first offender: i < n_remove is removal i, else addition i - n_remove; else GPUART_EDIT_NONE */
    uint64_t n_prims;   /* n_new */
    uint32_t type_mask; /* OR of 1 << type over the edited list */
    float root_min[3], root_max[3]; /* the fold of the edited list's boxes */
} gpuart_edit_result;

int gpuart_edit_create(int device, gpuart_edit **out);
int gpuart_edit_destroy(gpuart_edit *h);

/* remove: n_remove device ordinals of src, strictly ascending; add_types: n_add values 0..3; add_payload: n_add x 16 floats; source:
 * n_new int32 — all device memory, add_payload 16-byte aligned, the others 4. Pointers may be NULL where their count is 0. Synchronous.
 * *edited describes the handle's staging arrays and is valid until the handle's next run; *result (may be NULL) is filled whenever the
 * device sequence ran. */
int gpuart_edit_run(gpuart_edit *h, const gpuart_hip_scene *src, const uint32_t *remove, size_t n_remove, const uint32_t *add_types,
                    const float *add_payload, size_t n_add, int32_t *source, gpuart_hip_scene *edited, gpuart_edit_result *result);
/* The same with remove, add_types, add_payload and source in host memory (4-byte alignment), staged through the handle's memory. */
int gpuart_edit_run_host(gpuart_edit *h, const gpuart_hip_scene *src, const uint32_t *remove, size_t n_remove, const uint32_t *add_types,
                         const float *add_payload, size_t n_add, int32_t *source, gpuart_hip_scene *edited, gpuart_edit_result *result);
/* out[p] = source[perm[p]], p < n, on the device (all device memory, 4-byte aligned; out may not overlap the others): a build's
 * new_to_old expressed in old ordinals and addition indices. An entry of perm that is not below n yields -1. Synchronous. */
int gpuart_edit_compose(gpuart_edit *h, const int32_t *source, const uint32_t *perm, size_t n, int32_t *out);

/* Device time in ms of the steps of the last run: validate and flags, scan, compact and append, reduce. */
int gpuart_edit_step_ms(gpuart_edit *h, double ms[4]);
/* Waits for the handle's stream. */
int gpuart_edit_finish(gpuart_edit *h);
const char *gpuart_edit_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_EDIT_H */
