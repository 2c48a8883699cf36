/* gpuart_refine.h — C ABI of libgpuart_refine.so: a variance-guided filter for frames that carry a convergence estimate
 * (MI355X, gfx950). No reference counterpart: the reference shows the raw accumulator (shaders/pt_normalize.glsl).
 *
 * The denoiser of include/gpuart_denoise.h guesses a pixel's luminance variance from the 7x7 window of one frame, which is right at
 * 1 to 4 paths per pixel and blurs a converged frame. This filter is the same à-trous wavelet filter on radiance demodulated by the
 * primitive colour, guided by normal and hit distance, but its luminance variance is MEASURED: it comes from the error map of
 * include/gpuart_converge.h (gpuart_converge_measure), the standard error of each pixel's mean luminance. The luminance edge therefore
 * tightens by itself as the render converges, and the filter stays usable on the frame Renderer::RenderUntil leaves. Like the denoiser
 * it works on images alone and knows nothing of the scene or the tree; the raw accumulator stays the exact result.
 *
 * Inputs: a tile of radiance, the G-buffer gpuart_hip_gbuffer writes for the same tile (one gpuart_ray_hit and one primitive ordinal
 * per pixel), and `error`: per pixel the e that gpuart_converge_measure writes with the same lum_floor, the standard error of the
 * pixel's mean luminance relative to max(luminance, lum_floor).
 *
 * The filter, every operation in fp32, in exactly this order (tests/refine_ref.py restates it in NumPy, bit for bit):
 *   0. A pixel is VALID if it is a surface pixel by the denoiser's rule (its record's type >= 0, unless its ordinal is -2, the user
 *      sphere, and userSphereFlags has EM_NONZERO (1) or SPECULAR (2)) and its e is finite (neither NaN nor +-inf, whatever its sign).
 *      Every other pixel is copied through and never serves as a tap or as a prefilter neighbour. A valid pixel's albedo a is the
 *      reference's PRIMITIVE_COLOR[type] (shaders/path_tracing.glsl:123-126).
 *   1. x = c.rgb / a per channel; L(x) = (0.2126f*x.r + 0.7152f*x.g) + 0.0722f*x.b; sg = e * max(L, lum_floor); var = sg*sg.
 *   2. Levels i = 0 .. iterations-1, step s = 2^i. For each valid pixel p:
 *      a. The variance prefilter, never dilated: over q = p + (dx, dy) (dy outer, dx inner, -1..1) that lie inside the tile and are
 *         valid (p itself always is): g = G[dy+1]*G[dx+1], G = {1/4, 1/2, 1/4}; gn += g*var_q, gd += g; then gv = gn/gd.
 *      b. Over the taps q = p + s*(dx, dy) (dy outer, dx inner, -2..2) that lie inside the tile and are valid:
 *           h = H[dy+2]*H[dx+2], H = {1/16, 1/4, 3/8, 1/4, 1/16}
 *           sd = sqrt(gv)*lum_k + 1e-4f, e = (L(x_q) - L(x_p))/sd, wl = 1/(1 + e*e)
 *           d = max((n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z, 0), wn = d squared normal_pow2 times
 *           dz = |pos_q - pos_p| / ((depth_sigma*max(pos_p, 1e-6f))*s), wz = 1/(1 + dz*dz)
 *           w = ((h*wl)*wn)*wz; num += w*x_q per channel, den += w, nv += (w*w)*var_q    (the tap's own variance, not a prefiltered one)
 *      c. x_p = num/den, var_p = nv/(den*den) for the next level; a pixel whose den is not > 0 keeps both.
 *   3. The output is x*a for valid pixels and c for every other pixel; alpha is copied.
 *   With iterations = 0 the output is the input, bit for bit. max(a, b) is (a > b ? a : b).
 * Non-finite radiance, and radiance for which sg*sg overflows fp32, are outside this contract.
 *
 * The map must describe the radiance it comes with. Renderer::ReadRefined filters the current accumulator with the map of
 * RenderUntil's last batch: paths rendered by plain passes after that batch are in the image but not in e, so the map is then
 * slightly too large and the filter slightly too strong.
 *
 * Conventions as include/gpuart_hip.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE);
 * the message of the last failure (per thread) from gpuart_refine_last_error(). Images are tiles of w x h RGBA32F pixels,
 * row-major, in the local row order of the tile that gpuart_hip_read uses (row 0 at the bottom). One handle per device; it owns
 * its HIP stream and its scratch (48 bytes per pixel, kept for the next call of the same size or smaller).
 */
#ifndef GPUART_REFINE_H
#define GPUART_REFINE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_refine gpuart_refine;

typedef struct gpuart_refine_params {
    uint32_t iterations;   /* à-trous levels, 0..GPUART_REFINE_MAX_ITERATIONS (0: the output is the input) */
    float lum_k;           /* luminance edge: the tolerance in standard errors of the pixel's mean (finite, >= 0) */
    uint32_t normal_pow2;  /* normal edge: the cosine is squared this many times (0..16) */
    float depth_sigma;     /* depth edge: relative hit-distance tolerance per unit of step (finite, > 0) */
} gpuart_refine_params;
#define GPUART_REFINE_MAX_ITERATIONS 8u

/* A handle on HIP device `device`. */
int gpuart_refine_create(int device, gpuart_refine **out);
int gpuart_refine_destroy(gpuart_refine *r);
/* iterations 5, lum_k 1, normal_pow2 5, depth_sigma 0.05 (lum_k: the sweep of profiles/refine.txt). */
int gpuart_refine_defaults(gpuart_refine_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_refine_finish before `out` is used). The inputs must be complete when
 * the call is made. rgba: w*h*4 floats; hits: w*h records; prims: w*h ordinals (-2: the user sphere); error: w*h floats, the e of
 * gpuart_converge_measure for the same lum_floor; out: w*h*4 floats, may be rgba itself and must not overlap error. rgba, hits and
 * out 16-byte aligned, prims and error 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with nothing written, for NULL or
 * misaligned pointers, w or h 0 or above 65536, iterations above GPUART_REFINE_MAX_ITERATIONS, lum_k not finite or below 0,
 * depth_sigma not finite or not above 0, normal_pow2 above 16, lum_floor not finite or not above 0. */
int gpuart_refine_run(gpuart_refine *r, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                      const float *error, float lum_floor, uint32_t w, uint32_t h, const gpuart_refine_params *p, float *out);
/* The same in host memory (every pointer 4-byte aligned), synchronous (staged through the handle's scratch). */
int gpuart_refine_run_host(gpuart_refine *r, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                           const float *error, float lum_floor, uint32_t w, uint32_t h, const gpuart_refine_params *p, float *out);
/* Waits for the handle's stream. */
int gpuart_refine_finish(gpuart_refine *r);
const char *gpuart_refine_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_REFINE_H */
