/* gpuart_moments.h — C ABI of libgpuart_moments.so: the luminance variance a temporal history has MEASURED, as the error map the
 * variance-guided filter takes (MI355X, gfx950). No reference counterpart: the reference keeps no history (include/gpuart_temporal.h).
 *
 * gpuart_temporal_accumulate is a weighted mean per channel, out = (nh*h + s*c)/(nh + s), whose taps and weights depend on the
 * G-buffer, the views and the parameters alone. So the moments of a pixel's luminance can ride through a SECOND gpuart_temporal handle
 * that is given, in place of the radiance, the image gpuart_moments_pack makes, {L, L*L, 1/s, a}, with the same G-buffers, views,
 * parameters and commits as the handle that carries the radiance. What that handle returns is m = {m1, m2, q, a}:
 * m1 = sum(b*y)/sum(b) and m2 = sum(b*y*y)/sum(b) over the views' luminances y with their weights b, and q = (number of views)/len.
 * These are the weighted batch means of include/gpuart_converge.h with one batch per view, B = len*q is the effective number of
 * batches, and (m2 - m1*m1)/(B - 1) is the variance of the blended mean luminance (E[sum b*(y - mean)^2] = (B - 1)*sigma^2, the
 * identity behind gpuart_converge_update). With one path per view q*len is the number of views exactly: both took the same roundings.
 * gpuart_moments_error turns the pair of blends into e, the standard error of the blended luminance relative to
 * max(luminance, lum_floor): the `error` of gpuart_refine_run. Where the history is too short to measure anything (a disoccluded
 * strip, the first views of a track) it falls back to the spatial guess of include/gpuart_denoise.h, the 7x7 window of the blend.
 * Like the other image libraries this one works on images alone and knows nothing of the scene or the tree.
 *
 * Every operation in fp32, in exactly this order (tests/moments_ref.py restates it in NumPy, bit for bit):
 *   L(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b; max(a, b) is (a > b ? a : b).
 *   A pixel is a surface pixel by the denoiser's rule: its record's type >= 0, unless its ordinal is -2 (the user sphere) and
 *   userSphereFlags has EM_NONZERO (1) or SPECULAR (2).
 *   pack, every pixel: l = L(c.rgb); out = {l, l*l, 1.0f/(float)spp, c.a}.
 *   error, per pixel, from the blended radiance x with its len and the blended moments m:
 *   1. Not a surface pixel: e = 0.
 *   2. B = len*m.b. If B >= min_batches: v = m.g - m.r*m.r; v = (v < 0 ? 0 : v) (a NaN stays a NaN);
 *      e = sqrt(v/(B - 1.0f)) / max(m.r, lum_floor).
 *   3. Otherwise, over q = p + (dx, dy) (dy outer, dx inner, -3..3, p included) that lie inside the tile and are surface pixels:
 *      cnt += 1, s1 += Lq, s2 += Lq*Lq with Lq = L(x_q.rgb); then mean = s1/cnt, var = max(s2/cnt - mean*mean, 0),
 *      e = (spatial_k*sqrt(var)) / max(L(x_p.rgb), lum_floor).
 * Every surface pixel gets a finite e for finite inputs; gpuart_refine_run copies a pixel whose e is not finite through. Non-finite
 * radiance is outside this contract.
 *
 * Defaults: min_batches 8, spatial_k 4. Chosen on two scenes only, the box and scene P at 160 x 120, one path per view, on two sideways
 * camera tracks, by tools/moments_quality.py (profiles/moments.txt, which states the rule). The history that feeds this map should be
 * long: the tool recommends max_history 32 for the guided preview, where the denoised preview does best with 4
 * (include/gpuart_temporal.h; gpuart_temporal_defaults stays 4).
 *
 * Conventions as include/gpuart_refine.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE); the
 * message of the last failure (per thread) from gpuart_moments_last_error(). Images are tiles of w x h pixels, row-major, in the local
 * row order of the tile that gpuart_hip_read uses (row 0 at the bottom). One handle per device; it owns its HIP stream and the staging
 * memory of the host entry points (76 bytes per pixel, kept for the next call of the same size or smaller).
 */
#ifndef GPUART_MOMENTS_H
#define GPUART_MOMENTS_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_moments gpuart_moments;

typedef struct gpuart_moments_params {
    float min_batches; /* least effective number of batches B at which the measured variance is used (finite, > 1) */
    float spatial_k;   /* the spatial fallback's e is this many window standard deviations (finite, >= 0) */
} gpuart_moments_params;

/* A handle on HIP device `device`. */
int gpuart_moments_create(int device, gpuart_moments **out);
int gpuart_moments_destroy(gpuart_moments *m);
/* min_batches 8, spatial_k 4. */
int gpuart_moments_defaults(gpuart_moments_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_moments_finish before `out` is used). rgba: w*h*4 floats, the mean of
 * spp >= 1 paths; out: w*h*4 floats, may be rgba itself; both 16-byte aligned. GPUART_HIP_ERR_ARG, with nothing written, for NULL or
 * misaligned pointers, w or h 0 or above 65536, spp 0, out overlapping rgba without being rgba. */
int gpuart_moments_pack(gpuart_moments *m, const float *rgba, uint32_t spp, uint32_t w, uint32_t h, float *out);
/* The same in host memory (every pointer 4-byte aligned), synchronous (staged through the handle's memory). */
int gpuart_moments_pack_host(gpuart_moments *m, const float *rgba, uint32_t spp, uint32_t w, uint32_t h, float *out);

/* Device memory, asynchronous on the handle's stream. The inputs must be complete when the call is made. rgba, len: the out_rgba
 * (w*h*4 floats) and out_len (w*h floats) of the gpuart_temporal_accumulate that blended the radiance; moments: the out_rgba of the
 * one that blended the packed image; hits, prims: the G-buffer of the tile (w*h records, w*h ordinals, -2: the user sphere); e: w*h
 * floats. rgba, moments and hits 16-byte aligned, len, prims and e 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with
 * nothing written, for NULL or misaligned pointers, w or h 0 or above 65536, lum_floor not finite or not above 0, min_batches not
 * finite or not above 1, spatial_k not finite or below 0, e overlapping an input. */
int gpuart_moments_error(gpuart_moments *m, const float *rgba, const float *len, const float *moments, const gpuart_ray_hit *hits,
                         const int32_t *prims, uint32_t userSphereFlags, float lum_floor, uint32_t w, uint32_t h,
                         const gpuart_moments_params *p, float *e);
/* The same in host memory (every pointer 4-byte aligned), synchronous (staged through the handle's memory). */
int gpuart_moments_error_host(gpuart_moments *m, const float *rgba, const float *len, const float *moments, const gpuart_ray_hit *hits,
                              const int32_t *prims, uint32_t userSphereFlags, float lum_floor, uint32_t w, uint32_t h,
                              const gpuart_moments_params *p, float *e);
/* Waits for the handle's stream. */
int gpuart_moments_finish(gpuart_moments *m);
const char *gpuart_moments_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_MOMENTS_H */
