/* gpuart_refit.h — C ABI of libgpuart_refit.so: listed primitives of an uploaded scene replaced and the boxes of its tree refitted, on
 * the device and in place (MI355X, gfx950). The tree's topology stays: only the moved primitives' 48-byte records, their boxes and the
 * boxes above them change. The library works on the arrays gpuart_hip_scene_device hands out and knows nothing of contexts, frames or
 * passes; the caller tells the context afterwards (gpuart_hip_scene_refitted). DESIGN.md "Refit" has the contract and its limits.
 *
 * The contract (tests/refit_ref.py restates it in NumPy; the host library's BoundingVolumesHierarchy::Refit is a second statement):
 * in the canonical compiled tree the data quads of the listed primitives are replaced; every leaf's box becomes the running minimum and
 * maximum, from +-99e29 with `<` and `>`, of its primitives' boxes in leaf order, each the box the primitive's constructor gives it;
 * every interior node's box is its lower child's box folded with its upper child's by the same rule; nothing else changes. The device
 * arrays after a refit are what gpuart_hip_upload_bvh makes of that tree, byte for byte in every word the device reads. All in fp32
 * with denormals kept and no contraction, as the host uploader computes a triangle's edges and copies a box plane.
 *
 * An update is refused as a whole, with nothing written, unless its ordinals are strictly ascending and below n_prims and every
 * payload meets the preconditions under which the uploader says a box bounds its primitive (csrc/hip/prim_rule.h, the one statement
 * both use): every word the device reads finite and at most 2^20 in magnitude, radii and a cone's length >= 0, a cone's derived
 * constants consistent with its centres and radii. A primitive keeps its type. So a refitted tree stays regular and orderly.
 *
 * Device sequence, on the handle's stream: validate; update (returns at once when validation set the status word); one launch per
 * tree level, deepest first, over that level's records — no data is handed between workgroups inside a launch, kernel boundaries are
 * the synchronisation —; one launch for the root box; one small read-back.
 *
 * Conventions as the image libraries': 0 on success or a negative gpuart_hip_status; the message of the last failure (per thread)
 * from gpuart_refit_last_error(), which begins "refit:". One handle per device; it owns its HIP stream, the level lists and its
 * staging memory. */
#ifndef GPUART_REFIT_H
#define GPUART_REFIT_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_refit gpuart_refit;

#define GPUART_REFIT_PAYLOAD 16u /* floats per update: the primitive's data quads as Primitive::StoreDataIntoBVH writes them, zero-padded */
#define GPUART_REFIT_NO_UPDATE 0xffffffffu

typedef struct gpuart_refit_result {
    int32_t status;     /* 0, or GPUART_HIP_ERR_ARG: the update was refused and nothing was written */
    uint32_t first_bad; /* on refusal: index into the update list of the first offending update; else GPUART_REFIT_NO_UPDATE */
    uint32_t subnormal; /* some box plane of the refitted tree is within 2^-60 of zero without being zero */
    float root_min[3], root_max[3]; /* the refitted root box */
} gpuart_refit_result;

int gpuart_refit_create(int device, gpuart_refit **out);
int gpuart_refit_destroy(gpuart_refit *h);

/* Binds the handle to a scene: reads the records back once, checks every ref against the counts (record refs ascending in pre-order
 * and each used once, leaf ranges inside the primitive array), derives every record's level from the refs and uploads the record
 * indices sorted by level. Remembers scene->generation. GPUART_HIP_ERR_ARG for exact_boxes != 0 (an irregular or disorderly tree is not
 * refitted), an unknown layout, NULL arrays, or refs that do not form the tree the counts describe. */
int gpuart_refit_bind(gpuart_refit *h, const gpuart_hip_scene *scene);
/* Levels of the bound tree's records = launches of the level kernel per run (0 when the root is a leaf). */
int gpuart_refit_levels(gpuart_refit *h, uint32_t *levels);

/* Replaces n primitives and refits every box. ordinals: n device primitive ordinals, strictly ascending (the numbering
 * gpuart_hip_trace_rays returns), device memory, 4-byte aligned; payload: n x 16 floats, device memory, 16-byte aligned. n = 0 (the
 * pointers may be NULL) is a plain refit. Synchronous: when it returns the arrays are refitted, or untouched. *result (may be NULL)
 * is filled whenever the device sequence ran. GPUART_HIP_ERR_ARG for a handle that is not bound to this scene's arrays and generation,
 * NULL or misaligned pointers with n > 0, n > n_prims, and for a refused update (the message names the update and the reason). */
int gpuart_refit_run(gpuart_refit *h, const gpuart_hip_scene *scene, const uint32_t *ordinals, const float *payload, size_t n,
                     gpuart_refit_result *result);
/* The same with ordinals and payload in host memory (4-byte alignment), staged through the handle's memory. */
int gpuart_refit_run_host(gpuart_refit *h, const gpuart_hip_scene *scene, const uint32_t *ordinals, const float *payload, size_t n,
                          gpuart_refit_result *result);
/* Waits for the handle's stream. */
int gpuart_refit_finish(gpuart_refit *h);
const char *gpuart_refit_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_REFIT_H */
