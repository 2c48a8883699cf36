/* gpuart_denoise.h — C ABI of libgpuart_denoise.so: an edge-aware spatial denoiser for low-sample path-traced frames
 * (MI355X, gfx950). No reference counterpart: the reference shows the raw accumulator (shaders/pt_normalize.glsl).
 *
 * The filter works on images alone and knows nothing of the scene or the tree: its inputs are a tile of radiance and the
 * G-buffer gpuart_hip_gbuffer writes for the same tile (include/gpuart_hip.h: one gpuart_ray_hit and one primitive ordinal per
 * pixel). It is an à-trous wavelet filter guided by normal, hit distance and a luminance variance estimate, on radiance
 * demodulated by the primitive colour. It is for previews: at 1 to 4 paths per pixel it removes most of the noise, once the
 * accumulator has converged it blurs more than it removes (DESIGN.md "Denoiser"). The raw accumulator stays the exact result.
 *
 * The filter, every operation in fp32, in exactly this order (tests/denoise_ref.py restates it in NumPy, bit for bit):
 *   A pixel is a surface pixel if its record's type >= 0, unless its ordinal is -2 (the user sphere) and userSphereFlags has
 *   EM_NONZERO (1) or SPECULAR (2). Every other pixel (sky, emissive or mirror user sphere) is copied through and never serves as a
 *   neighbour. A surface pixel's albedo a is the reference's PRIMITIVE_COLOR[type] (shaders/path_tracing.glsl:123-126).
 *   1. x = c.rgb / a per channel; L(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b.
 *   2. Over the 7x7 window of surface pixels inside the tile (dy outer, dx inner, -3..3, the pixel itself included): cnt, m1 += L,
 *      m2 += L*L; mean = m1/cnt, var = max(m2/cnt - mean*mean, 0).
 *   3. Levels i = 0 .. iterations-1, step s = 2^i. For each surface pixel p, over the taps q = p + s*(dx, dy) (dy outer, dx inner,
 *      -2..2) that lie inside the tile and are surface pixels:
 *        h = H[dy+2]*H[dx+2], H = {1/16, 1/4, 3/8, 1/4, 1/16}
 *        sd = sqrt(var_p)*lum_k + 1e-4f, e = (L(x_q) - L(x_p))/sd, wl = 1/(1 + e*e)
 *        d = max((n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z, 0), wn = d squared normal_pow2 times
 *        dz = |pos_q - pos_p| / ((depth_sigma*max(pos_p, 1e-6f))*s), wz = 1/(1 + dz*dz)
 *        w = ((h*wl)*wn)*wz; num += w*x_q per channel, den += w, nv += (w*w)*var_q
 *      then x_p = num/den, var_p = nv/(den*den) for the next level; a pixel whose den is not > 0 keeps its values.
 *   4. The output is x*a for surface pixels and c for every other pixel; alpha is copied.
 *   With iterations = 0 the output is the input, bit for bit. max(a, b) is (a > b ? a : b).
 * Non-finite radiance, and radiance whose demodulated luminance squared overflows fp32, are outside this contract.
 *
 * Conventions as include/gpuart_hip.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE);
 * the message of the last failure (per thread) from gpuart_denoise_last_error(). Images are tiles of w x h RGBA32F pixels,
 * row-major, in the local row order of the tile that gpuart_hip_read uses (row 0 at the bottom). One handle per device; it owns
 * its HIP stream and its scratch (48 bytes per pixel, kept for the next call of the same size or smaller).
 */
#ifndef GPUART_DENOISE_H
#define GPUART_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_denoise gpuart_denoise;

typedef struct gpuart_denoise_params {
    uint32_t iterations;   /* à-trous levels, 0..GPUART_DENOISE_MAX_ITERATIONS (0: the output is the input) */
    float lum_k;           /* luminance edge: the tolerance in standard deviations of the local estimate (finite, >= 0) */
    uint32_t normal_pow2;  /* normal edge: the cosine is squared this many times (0..16) */
    float depth_sigma;     /* depth edge: relative hit-distance tolerance per unit of step (finite, > 0) */
} gpuart_denoise_params;
#define GPUART_DENOISE_MAX_ITERATIONS 8u

/* A handle on HIP device `device`. */
int gpuart_denoise_create(int device, gpuart_denoise **out);
int gpuart_denoise_destroy(gpuart_denoise *d);
/* iterations 5, lum_k 4, normal_pow2 5, depth_sigma 0.05. */
int gpuart_denoise_defaults(gpuart_denoise_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_denoise_finish before `out` is used). The inputs must be complete
 * when the call is made (e.g. gpuart_hip_finish after gpuart_hip_gbuffer / gpuart_hip_export). rgba: w*h*4 floats; hits: w*h
 * records; prims: w*h ordinals (-2: the user sphere); out: w*h*4 floats and may be rgba itself. rgba, hits and out 16-byte aligned,
 * prims 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG for NULL or misaligned pointers, w or h 0 or above 65536,
 * iterations above GPUART_DENOISE_MAX_ITERATIONS, or parameters out of range. */
int gpuart_denoise_run(gpuart_denoise *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                       uint32_t w, uint32_t h, const gpuart_denoise_params *p, float *out);
/* The same in host memory, synchronous (staged through the handle's scratch). */
int gpuart_denoise_run_host(gpuart_denoise *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims,
                            uint32_t userSphereFlags, uint32_t w, uint32_t h, const gpuart_denoise_params *p, float *out);
/* Waits for the handle's stream. */
int gpuart_denoise_finish(gpuart_denoise *d);
const char *gpuart_denoise_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_DENOISE_H */
