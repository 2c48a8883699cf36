/* gpuart_edges.h — C ABI of libgpuart_edges.so: geometric edges of a filtered frame resolved from a sub-pixel G-buffer (MI355X,
 * gfx950). No reference counterpart: the reference shows the accumulator as it is.
 *
 * Every filter of this project (include/gpuart_denoise.h, include/gpuart_refine.h) treats a pixel as lying wholly on the surface its
 * centre ray hits, while the path tracer jitters every path over the pixel's footprint (reference shaders/path_tracing.glsl:144-170).
 * At a silhouette, a crease or a contact line the true pixel is a mix of two surfaces, the filters weight by the centre's surface
 * alone, and the error that leaves does not fall with the sample count. This library mends the filtered frame afterwards:
 * gpuart_edges_mark lists the pixels whose 8-neighbourhood holds another surface, gpuart_hip_trace_subpixel (include/gpuart_hip.h)
 * answers n_sub camera rays through each of them, and gpuart_edges_resolve gives every sub-sample the filtered light of the
 * neighbouring pixel whose centre lies on the sub-sample's surface, under the sub-sample's own albedo, and averages. Like the other
 * image libraries this one works on images alone.
 *
 * A record is a gpuart_ray_hit with its ordinal: of a pixel's centre ray (gpuart_hip_gbuffer) or of a sub-sample. Its class:
 *   sky      type < 0;
 *   sphere   ordinal -2 and userSphereFlags & (EM_NONZERO | SPECULAR) (1 | 2): the user sphere that is not filtered, the denoiser's rule;
 *   surface  everything else. a(type) is the reference's PRIMITIVE_COLOR of the type (include/gpuart_denoise.h).
 *
 * Every operation in fp32, in exactly this order (tests/edges_ref.py restates it in NumPy, bit for bit):
 *   match(a, b), a record a against a centre record b:
 *     a sky: b is sky. a sphere: b is sphere. a surface: b is surface, type_a == type_b, (ordinal_a == -2) == (ordinal_b == -2),
 *     dn = (n_a.x*n_b.x + n_a.y*n_b.y) + n_a.z*n_b.z > normal_min, and with d = p_a - p_b per component,
 *     |(n_b.x*d.x + n_b.y*d.y) + n_b.z*d.z| <= plane_tol * (pos_b > 1e-6f ? pos_b : 1e-6f).
 *   mark: tile pixel p is an edge pixel iff for some q = p + (dx, dy), (dx, dy) != (0, 0), -1 <= dx, dy <= 1, inside the tile,
 *     match(centre_q, centre_p) is false. The list holds the edge pixels' indices y*w + x in ascending order; *count their number.
 *   resolve: out = filtered; then for every listed pixel p = list[i] and k = 0 .. n_sub-1 in this order, with the sub-sample's record
 *     s = sub[k*n + i]: the candidates m = p + (dx, dy) are tried in the order (dy, dx) = (0,0), (0,1), (0,-1), (1,0), (-1,0), (1,1),
 *     (1,-1), (-1,1), (-1,-1), those outside the tile skipped, and the first with match(s, centre_m) wins.
 *       s surface:      c = (filtered_m.rgb / a(type_m)) * a(type_s) per channel;
 *       s sky or sphere: c = filtered_m.rgb;
 *       no candidate matches: c = filtered_p.rgb.
 *     sum += c per channel (sum starts at 0). out_p.rgb = sum / (float)n_sub; out_p.a = filtered_p.a.
 * Non-finite inputs are outside this contract; every index is still range-checked before use (a list entry >= w*h is skipped).
 *
 * The sub-pixel offsets are a rotated grid, fixed by the table GPUART_EDGES_ROTATION below: sub-sample k of n_sub takes
 * rand1 = ((float)k + 0.5f) / (float)n_sub and rand2 = ((float)perm(k) + 0.5f) / (float)n_sub with perm(k) = (k * GPUART_EDGES_ROTATION[n_sub])
 * mod n_sub, except for n_sub = 4, where perm = GPUART_EDGES_RGSS = {2, 0, 3, 1} (no multiplier mod 4 gives anything but a diagonal).
 * Every row and every column of the n_sub x n_sub grid then holds one sample. gpuart_edges_offsets writes them out; mark and resolve
 * never read them: they are what the callers hand gpuart_hip_trace_subpixel. Only n_sub 4, 8 and 16 have been measured.
 *
 * Defaults: n_sub 8, normal_min 0.95, plane_tol 0.02, and this table. Chosen on two scenes only, the box and scene P at 160 x 120, by
 * tools/edges_quality.py (profiles/edges.txt states the rule and the sweep).
 *
 * Conventions as include/gpuart_denoise.h: 0 on success or a negative gpuart_hip_status; the message of the last failure (per thread)
 * from gpuart_edges_last_error(). Images are tiles of w x h pixels, row-major, row 0 at the bottom. One handle per device; it owns its
 * HIP stream and the memory of mark's prefix (12 bytes per 64 pixels), kept for the next call of the same size or smaller.
 */
#ifndef GPUART_EDGES_H
#define GPUART_EDGES_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_edges gpuart_edges;

typedef struct gpuart_edges_params {
    uint32_t n_sub;   /* sub-samples per edge pixel, 1..GPUART_EDGES_MAX_SUB */
    float normal_min; /* a match needs dot(n_a, n_b) above this (-1..1) */
    float plane_tol;  /* ... and a's point within plane_tol * pos_b of b's tangent plane (finite, >= 0) */
} gpuart_edges_params;

#define GPUART_EDGES_MAX_SUB 16u /* = GPUART_HIP_MAX_SUBPIXEL */

/* perm(k) = (k * GPUART_EDGES_ROTATION[n_sub]) mod n_sub for n_sub = 0..16 (entry 0 unused); n_sub = 4: GPUART_EDGES_RGSS instead. */
static const uint8_t GPUART_EDGES_ROTATION[GPUART_EDGES_MAX_SUB + 1] = {0, 1, 1, 2, 0, 2, 5, 3, 3, 4, 3, 4, 5, 5, 5, 4, 7};
static const uint8_t GPUART_EDGES_RGSS[4] = {2, 0, 3, 1};
/* uv[2k], uv[2k + 1] = (rand1, rand2) of sub-sample k of n_sub, as stated above (host memory, 2 * n_sub floats). GPUART_HIP_ERR_ARG for
 * n_sub outside 1..GPUART_EDGES_MAX_SUB or uv NULL. */
int gpuart_edges_offsets(uint32_t n_sub, float *uv);

/* A handle on HIP device `device`. */
int gpuart_edges_create(int device, gpuart_edges **out);
int gpuart_edges_destroy(gpuart_edges *e);
/* n_sub 8, normal_min 0.95, plane_tol 0.02. */
int gpuart_edges_defaults(gpuart_edges_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_edges_finish before the outputs are used). The inputs must be complete
 * when the call is made. hits, prims: the G-buffer of the tile (gpuart_hip_gbuffer). list: room for w*h indices; count: one word.
 * hits 16-byte aligned, the others 4-byte aligned. p = NULL: the defaults (n_sub is not read). GPUART_HIP_ERR_ARG, with nothing
 * written, for NULL or misaligned pointers, w or h 0 or above 65536, or a parameter out of its range. */
int gpuart_edges_mark(gpuart_edges *e, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w, uint32_t h,
                      const gpuart_edges_params *p, uint32_t *list, uint32_t *count);
/* filtered: the frame to mend (w*h*4 floats); list: n pixel indices (mark's, or any: repeats write the same value twice); sub_hits,
 * sub_prims: p->n_sub * n records and ordinals, sub-sample k of list[i] at k*n + i, as gpuart_hip_trace_subpixel writes them; out:
 * w*h*4 floats, must not overlap filtered. filtered, hits, sub_hits and out 16-byte aligned, the others 4-byte aligned. n = 0 copies
 * the frame (list, sub_hits and sub_prims may then be NULL). GPUART_HIP_ERR_ARG, with nothing written, for NULL or misaligned
 * pointers, w or h 0 or above 65536, n * n_sub above GPUART_HIP_MAX_RAYS, a parameter out of its range, or out overlapping filtered. */
int gpuart_edges_resolve(gpuart_edges *e, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                         uint32_t w, uint32_t h, const uint32_t *list, size_t n, const gpuart_ray_hit *sub_hits, const int32_t *sub_prims,
                         const gpuart_edges_params *p, float *out);
/* Waits for the handle's stream. */
int gpuart_edges_finish(gpuart_edges *e);
const char *gpuart_edges_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_EDGES_H */
