/* gpuart_despeckle.h — C ABI of libgpuart_despeckle.so: the firefly clamp (MI355X, gfx950). A path reaches a small emissive user sphere
 * only by chance (there is no next-event estimate towards it), so at low path counts a few pixels carry tens of times their
 * neighbours' radiance. This stage caps a surface pixel's demodulated luminance at a multiple of a high order statistic of its
 * neighbourhood, before the filters and the temporal history take the pixel at face value. It is biased — it removes energy — and
 * therefore opt-in: the summary and the optional `scale` plane say how much was removed. Like the other image libraries this one
 * works on images alone and knows nothing of the scene or the tree.
 *
 * Every operation in fp32, in exactly this order (denormals kept, no contraction, IEEE '/'; tests/despeckle_ref.py restates it in NumPy,
 * bit for bit):
 *   L(v) = (0.2126f*v.r + 0.7152f*v.g) + 0.0722f*v.b.
 *
 * Per pixel p with colour c, G-buffer record and ordinal:
 *   1. p is a surface pixel iff its record's type >= 0 and it does not show an emissive or specular user sphere (ordinal -2 with
 *      userSphereFlags & 3): the denoiser's rule. Every other pixel is copied through bit for bit and is never a neighbour.
 *   2. a = PRIMITIVE_COLOR[type & 3] (0: {0.65, 0.4, 0.35}, 1: {0.1, 0.2, 0.1}, 2, 3: {0.3, 0.3, 0.3}), x = c.rgb / a, L = L(x).
 *      Lv = L for a surface pixel and NaN otherwise; a value is valid iff Lv == Lv, so a surface pixel whose L is NaN is no neighbour.
 *   3. The neighbours are the pixels q = p + (dx, dy), dy outer and dx inner, each from -radius to radius, p itself excluded, that lie
 *      inside the tile and are valid. cnt is their number; ref is the rank-th largest Lv among them, counted with multiplicity (only
 *      comparisons: ties cannot change the value).
 *   4. cap = k*ref + floor (a multiply, then an add). The pixel is clamped iff it is a surface pixel, cnt >= max(min_count, rank) and
 *      L > cap. Then s = cap / L and out.rgb = (x*s)*a; in every other case out.rgb = c.rgb bit for bit (not (c/a)*a). Alpha is c's.
 *      A NaN L fails L > cap and passes through: NaN or +-inf radiance is outside the contract but stays inside its pixel's output
 *      (an inf neighbour can still be a pixel's ref).
 *   5. scale (optional) holds s where the pixel was clamped and 1 elsewhere.
 * For non-negative radiance a clamped pixel has 0 <= s < 1, so no channel grows but for the rounding of (c/a*s)*a, which only shows
 * where s is within a few ulp of 1. With floor = 0, scaling every radiance by 2^n scales the output by exactly 2^n (no denormals or
 * overflow assumed). A rank of 3 in a 5x5 window (radius 2) leaves a one-pixel-wide lit line alone: such a line has four same-line
 * neighbours. In the default 3x3 window it has two, and a line more than k times brighter than what lies beside it is cut down.
 *
 * In place. out == rgba is allowed; any other overlap of out with rgba is an argument error. A block of the kernel derives the Lv of
 * its apron from rgba, which a neighbouring block of an in-place run may already have overwritten with a clamped value, and a clamped
 * neighbour can change a decision (it lowers ref). So an in-place run does not read the plane it writes: it first copies rgba into the
 * handle's own memory (16 bytes per pixel, device to device, on the handle's stream) and clamps from the copy. In place and separate
 * buffers therefore give identical bits.
 *
 * Conventions as include/gpuart_display.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE); the
 * message of the last failure (per thread) from gpuart_despeckle_last_error(), which begins "despeckle:". Images are tiles of w x h
 * pixels, row-major; the G-buffer is what gpuart_hip_gbuffer writes. One handle per device; it owns its HIP stream, the three counts
 * and the staging memory (kept for the next call of the same size or smaller).
 */
#ifndef GPUART_DESPECKLE_H
#define GPUART_DESPECKLE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_despeckle gpuart_despeckle;

typedef struct gpuart_despeckle_params {
    uint32_t radius;    /* the window is (2*radius + 1)^2: 1 or 2 */
    uint32_t rank;      /* ref is the rank-th largest valid neighbour: 1..4 */
    float k;            /* cap = k*ref + floor (finite, >= 1) */
    float floor;        /* (finite, >= 0) */
    uint32_t min_count; /* a pixel with fewer than max(min_count, rank) valid neighbours is left alone: 1..24 */
} gpuart_despeckle_params;

/* Exact counts of the last run. surface = clamped + too_few + the surface pixels that had enough neighbours and were not above
 * their cap. */
typedef struct gpuart_despeckle_summary {
    uint64_t surface; /* surface pixels */
    uint64_t clamped; /* of them, clamped */
    uint64_t too_few; /* of them, with cnt < max(min_count, rank) */
} gpuart_despeckle_summary;

/* A handle on HIP device `device`. */
int gpuart_despeckle_create(int device, gpuart_despeckle **out);
int gpuart_despeckle_destroy(gpuart_despeckle *d);
/* radius 1, rank 3, k 2, floor 1e-3, min_count 4 (profiles/despeckle.txt says how they were chosen). */
int gpuart_despeckle_defaults(gpuart_despeckle_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_despeckle_finish before out is used). The inputs must be complete when
 * the call is made. rgba, out: w*h*4 floats; hits: w*h records; all three 16-byte aligned. prims: w*h ordinals; scale: w*h floats or
 * NULL; both 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with nothing written, for a parameter out of its range
 * (checked first, so that the message names the field even without a device), NULL or misaligned pointers, w or h 0 or above 65536,
 * out overlapping rgba without being rgba, scale overlapping rgba or out, and, looked at last, a NULL handle. */
int gpuart_despeckle_run(gpuart_despeckle *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                         uint32_t w, uint32_t h, const gpuart_despeckle_params *p, float *out, float *scale);
/* The same in host memory (4-byte alignment), synchronous (staged through the handle's memory, 72 bytes per pixel). */
int gpuart_despeckle_run_host(gpuart_despeckle *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims,
                              uint32_t userSphereFlags, uint32_t w, uint32_t h, const gpuart_despeckle_params *p, float *out, float *scale);
/* Waits for the handle's stream and copies the counts of its last run out (zeros before the first). */
int gpuart_despeckle_read_summary(gpuart_despeckle *d, gpuart_despeckle_summary *out);
/* Waits for the handle's stream. */
int gpuart_despeckle_finish(gpuart_despeckle *d);
const char *gpuart_despeckle_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_DESPECKLE_H */
