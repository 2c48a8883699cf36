/* gpuart_upscale.h — C ABI of libgpuart_upscale.so: a filtered frame of w x h pixels upsampled to scale*w x scale*h under the guidance
 * of a G-buffer of the larger frame (MI355X, gfx950). No reference counterpart: the reference shows the accumulator at the size it
 * was rendered.
 *
 * The paths and every filter of this project cost in proportion to the pixel count, the primary-visibility rays of a G-buffer do not
 * by far. So a view is traced and filtered at w x h, gpuart_hip_gbuffer_scaled (include/gpuart_hip.h) answers the camera rays of the
 * scale times larger frame, and this library lets every output pixel take light only from the low-resolution neighbours whose centre
 * lies on the output pixel's own surface: silhouettes, creases and contact lines come out at the output resolution, only the lighting
 * is low resolution. It is the nearest relative of edge resolve (include/gpuart_edges.h), which asks for sub-pixel records at edge
 * pixels and averages them back into one pixel; this one asks for them everywhere, on the larger frame's own pixel grid, and keeps
 * them as pixels. Like the other image libraries this one works on images alone.
 *
 * A record is a gpuart_ray_hit with its ordinal: of a low pixel's centre ray (gpuart_hip_gbuffer) or of an output pixel's
 * (gpuart_hip_gbuffer_scaled). Its class, and match, are those of include/gpuart_edges.h with this library's normal_min and plane_tol:
 *   sky      type < 0;
 *   sphere   ordinal -2 and userSphereFlags & (EM_NONZERO | SPECULAR) (1 | 2): the user sphere that is not filtered, the denoiser's rule;
 *   surface  everything else.
 *
 * Every operation in fp32, in exactly this order (tests/upscale_ref.py restates it in NumPy, bit for bit):
 *   match(a, b), a record a against a centre record b:
 *     a sky: b is sky. a sphere: b is sphere. a surface: b is surface, type_a == type_b, (ordinal_a == -2) == (ordinal_b == -2),
 *     dn = (n_a.x*n_b.x + n_a.y*n_b.y) + n_a.z*n_b.z > normal_min, and with d = p_a - p_b per component,
 *     |(n_b.x*d.x + n_b.y*d.y) + n_b.z*d.z| <= plane_tol * (pos_b > 1e-6f ? pos_b : 1e-6f).
 *   For output pixel (X, Y) with record r, and s = (float)scale:
 *   1. fx = ((float)X + 0.5f)/s - 0.5f, x0 = floor(fx), ax = fx - x0; likewise fy, y0, ay. The containing low pixel is
 *      c = (X / scale, Y / scale) in integer division.
 *   2. The taps are the low pixels (x0 + ox, y0 + oy), oy = 0, 1 outer, ox = 0, 1 inner, with wx = (ox ? ax : 1.0f - ax),
 *      wy = (oy ? ay : 1.0f - ay), w = wy*wx. A tap counts iff it lies inside the w x h tile, w > 0 and match(r, centre_tap) holds.
 *      Over the counting taps in that order: Wsum += w, acc.rgb += w * filtered_tap.rgb (both start at 0).
 *   3. If Wsum > 0, out.rgb = acc.rgb / Wsum. Otherwise the candidates m = c + (dx, dy) are tried in edge resolve's order (dy, dx) =
 *      (0,0), (0,1), (0,-1), (1,0), (-1,0), (1,1), (1,-1), (-1,1), (-1,-1), those outside the tile skipped; the first with
 *      match(r, centre_m) gives out.rgb = filtered_m.rgb. If none matches, out.rgb = filtered_c.rgb.
 *   4. out.a = filtered_c.a.
 * No albedo enters: match demands equal types between surface records, and this project's albedo is a function of the type alone
 * (include/gpuart_denoise.h), so dividing one out and multiplying the other in would be the identity with rounding added.
 * Non-finite inputs are outside this contract; every index is still range-checked before use.
 *
 * Defaults: normal_min 0.95, plane_tol 0.02, edge resolve's (profiles/upscale.txt says what has been measured of them).
 *
 * Conventions as include/gpuart_denoise.h: 0 on success or a negative gpuart_hip_status; the message of the last failure (per thread)
 * from gpuart_upscale_last_error(). Images are tiles, row-major, row 0 at the bottom. One handle per device; it owns its HIP stream
 * and, for gpuart_upscale_run_host alone, a staging buffer (52 bytes per low pixel and 52 per output pixel), kept for the next call of
 * the same size or smaller. gpuart_upscale_run itself keeps nothing.
 */
#ifndef GPUART_UPSCALE_H
#define GPUART_UPSCALE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_upscale gpuart_upscale;

typedef struct gpuart_upscale_params {
    float normal_min; /* a match needs dot(n_a, n_b) above this (-1..1) */
    float plane_tol;  /* ... and a's point within plane_tol * pos_b of b's tangent plane (finite, >= 0) */
} gpuart_upscale_params;

#define GPUART_UPSCALE_MIN_SCALE 2u
#define GPUART_UPSCALE_MAX_SCALE 4u

/* A handle on HIP device `device`. */
int gpuart_upscale_create(int device, gpuart_upscale **out);
int gpuart_upscale_destroy(gpuart_upscale *u);
/* normal_min 0.95, plane_tol 0.02. */
int gpuart_upscale_defaults(gpuart_upscale_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_upscale_finish before the output is used). The inputs must be complete
 * when the call is made. filtered: the low frame (w*h*4 floats); hits, prims: its G-buffer (gpuart_hip_gbuffer); hi_hits, hi_prims: the
 * G-buffer of the scale*w x scale*h frame (gpuart_hip_gbuffer_scaled); out: scale*w * scale*h * 4 floats. filtered, hits, hi_hits and
 * out 16-byte aligned, prims and hi_prims 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with nothing written, for scale
 * outside 2..4, NULL or misaligned pointers, w or h 0, scale*w or scale*h above 65536, a parameter out of its range, or out
 * overlapping any input. */
int gpuart_upscale_run(gpuart_upscale *u, uint32_t scale, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims,
                       uint32_t w, uint32_t h, const gpuart_ray_hit *hi_hits, const int32_t *hi_prims, uint32_t userSphereFlags,
                       const gpuart_upscale_params *p, float *out);
/* The same in host memory, synchronous (staged through the handle's buffer); every pointer 4-byte aligned. */
int gpuart_upscale_run_host(gpuart_upscale *u, uint32_t scale, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims,
                            uint32_t w, uint32_t h, const gpuart_ray_hit *hi_hits, const int32_t *hi_prims, uint32_t userSphereFlags,
                            const gpuart_upscale_params *p, float *out);
/* Waits for the handle's stream. */
int gpuart_upscale_finish(gpuart_upscale *u);
const char *gpuart_upscale_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_UPSCALE_H */
