/* gpuart_converge.h — C ABI of libgpuart_converge.so: a per-pixel standard error of the accumulated radiance, measured from the
 * render itself, and its reduction over the frame (MI355X, gfx950). No reference counterpart: the reference renders the path count
 * it is given (src/renderer.cpp:502-508) and its accumulator carries a sum and nothing about its spread.
 *
 * The estimator works on images alone and knows nothing of the scene: its only input is the raw path-tracing accumulator, the sum
 * over all paths so far (gpuart_hip_export with divide_by 1). The renderer never shows a single pass's colour, so the estimator uses
 * batch means: every time it is shown the accumulator it takes the luminance difference since last time, divided by the number of
 * paths in between, as one sample whose weight is that number of paths (West's weighted update).
 *   E[m2] = (batches - 1) * sigma^2 for a per-path luminance variance sigma^2, whatever the batch sizes;
 *   the variance of the mean is sigma^2 / total, so its standard error is sqrt(m2 / (batches - 1) / total).
 *
 * State: per pixel one float4 {mean, m2, prevL, 0}; per handle, on the host, total (paths seen), batches, w and h. After create or
 * reset the state is all zeros and total = 0: the first update is simply the first batch (a resumed checkpoint of P paths is one
 * batch of weight P).
 *
 * update, every operation in fp32, in exactly this order (tests/converge_ref.py restates it in NumPy, bit for bit):
 *   L(a)  = (0.2126f*a.r + 0.7152f*a.g) + 0.0722f*a.b
 *   b     = (float)(paths_total - total);  Wn = (float)paths_total;  r = b / Wn        (on the host, once per call)
 *   Lk    = L(accum);  y = (Lk - prevL) / b;  d = y - mean
 *   mean' = mean + r*d
 *   m2'   = m2 + (b*d)*(y - mean')
 *   prevL' = Lk
 * and then total = paths_total, batches += 1.
 *
 * measure (batches >= 2), per pixel:
 *   v  = (m2 < 0 ? 0 : m2) / (float)(batches - 1)          (rounding can leave m2 below 0; a NaN m2 stays NaN)
 *   se = sqrt(v / (float)total)
 *   e  = se / (mean > lum_floor ? mean : lum_floor)
 * e is the standard error of the pixel's mean luminance relative to that luminance (or to lum_floor where the pixel is darker).
 * NaN or infinite radiance leaves m2 NaN from its first update on and so e NaN; an m2 that overflowed gives e = +inf.
 * The summary counts the pixels for which !(e <= threshold) (`above`: a NaN counts), those whose e is NaN or +-inf (`non_finite`),
 * and holds the largest finite e (`max_error`, 0 if there is none). The three reductions are order-independent (integer counts, a
 * maximum over non-negative floats through their bit patterns): the summary is exact and the same in every run.
 *
 * The accumulator's floor. The estimator's own fp32 arithmetic is harmless: against a float64 two-pass estimate of the same luminances e
 * differs by at most 1.3e-8 over up to 4096 batches and 2^24 paths (tests/test_converge_range.py, profiles/convergence.txt section 4).
 * The fp32 accumulator it is shown is not: every luminance carries a rounding error relative to the whole sum, every batch mean is
 * the difference of two of them spread over the batch's paths, and the estimator cannot tell that noise from the paths' own. Against
 * the estimate on unrounded sums e changes by up to
 *   e_floor(total, b) = 2^-22 * sqrt(total / b),      b = the smallest batch after the first, in paths,
 * for a pixel at or above lum_floor (less below it), and a pixel without any spread reports up to that instead of 0 (measured: up to
 * 0.45 of it). A threshold below e_floor(total, b) is therefore not reliably reachable: with batches of 64 paths 1e-4 is out of reach
 * beyond 11.3 million paths and 1e-5 beyond 113 000; with batches of one path (a checkpoint of 2^23 paths continued path by path:
 * e_floor = 6.9e-4, steady pixels report up to 2.9e-4) 1e-4 is out of reach beyond 176 000 paths. The smallest threshold that can be
 * reached at the cap of 2^24 paths is 2^-10 / sqrt(b): 1.2e-4 for b = 64, 3.8e-6 for b = 65536. Larger batches lower the floor;
 * nothing reports that a threshold lies below it — RenderUntil then runs to its cap.
 *
 * Conventions as include/gpuart_hip.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE); the
 * message of the last failure (per thread) from gpuart_converge_last_error(). Images are tiles of w x h RGBA32F pixels, row-major,
 * in the local row order of the tile that gpuart_hip_read uses (row 0 at the bottom). One handle per device; it owns its HIP stream,
 * the state (16 bytes per pixel) and the staging memory of the host entry points.
 */
#ifndef GPUART_CONVERGE_H
#define GPUART_CONVERGE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_converge gpuart_converge;

typedef struct gpuart_converge_summary {
    uint64_t pixels;     /* w*h */
    uint64_t above;      /* pixels with !(e <= threshold) */
    uint64_t non_finite; /* pixels whose e is NaN or +-inf */
    float max_error;     /* the largest finite e; 0 if there is none */
    uint32_t batches;    /* updates since create / reset */
    uint32_t total;      /* paths per pixel the accumulator held at the last update */
} gpuart_converge_summary; /* 40 bytes */

/* Above this the path count is no longer exact in fp32: gpuart_converge_update rejects a larger paths_total. */
#define GPUART_CONVERGE_MAX_PATHS (1u << 24)
/* Paths per batch of Renderer::RenderUntil when the caller has no better idea (gpuart_cli --until-batch). A batch ends in an export
 * and a wait, which end the overlap of the render pipeline's runs: measured on cfg3 at 1080p (profiles/convergence.txt) a render in
 * batches of 8, 16, 32 and 64 paths takes 87 %, 40 %, 20 % and 12 % longer than the plain pass loop. None of the four is below 5 %;
 * 64 is the cheapest of them. Pass a larger batch for renders of thousands of paths. */
#define GPUART_CONVERGE_DEFAULT_BATCH 64u

/* A handle on HIP device `device`. */
int gpuart_converge_create(int device, gpuart_converge **out);
int gpuart_converge_destroy(gpuart_converge *c);
/* Forgets everything: the state is all zeros again, total = batches = 0, and the next update may have any size. Host work only. */
int gpuart_converge_reset(gpuart_converge *c);

/* Device memory, asynchronous on the handle's stream. accum: w*h*4 floats, 16-byte aligned, the raw accumulator after paths_total
 * paths per pixel; it must be complete when the call is made (e.g. gpuart_hip_finish after gpuart_hip_export) and stay untouched until
 * gpuart_converge_finish or a measure. GPUART_HIP_ERR_ARG, with nothing written and nothing counted, for paths_total <= total,
 * paths_total > GPUART_CONVERGE_MAX_PATHS, w or h different from the state's (unless the handle was reset), a NULL or misaligned
 * pointer, w or h 0 or above 65536. */
int gpuart_converge_update(gpuart_converge *c, const float *accum, uint32_t paths_total, uint32_t w, uint32_t h);
/* The same in host memory (4-byte aligned), synchronous (staged through the handle's memory). */
int gpuart_converge_update_host(gpuart_converge *c, const float *accum, uint32_t paths_total, uint32_t w, uint32_t h);

/* Synchronous: the summary comes back through pinned memory. error_map (may be NULL): w*h floats in device memory, 4-byte aligned,
 * receives e per pixel. GPUART_HIP_ERR_ARG, with nothing written, before the second update, for a threshold that is not finite and
 * >= 0, a lum_floor that is not finite and > 0, a misaligned error_map or a NULL summary. */
int gpuart_converge_measure(gpuart_converge *c, float threshold, float lum_floor, float *error_map, gpuart_converge_summary *summary);
/* The same with error_map (may be NULL) in host memory. */
int gpuart_converge_measure_host(gpuart_converge *c, float threshold, float lum_floor, float *error_map, gpuart_converge_summary *summary);

/* The state, w*h*4 floats {mean, m2, prevL, 0} to host memory; synchronous. GPUART_HIP_ERR_ARG before the first update. */
int gpuart_converge_read_state(gpuart_converge *c, float *state);
/* Waits for the handle's stream. */
int gpuart_converge_finish(gpuart_converge *c);
const char *gpuart_converge_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_CONVERGE_H */
