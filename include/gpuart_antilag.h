/* gpuart_antilag.h — C ABI of libgpuart_antilag.so: a fast history that overrides the long one where the lighting has changed
 * (MI355X, gfx950). No reference counterpart: the reference keeps no history (include/gpuart_temporal.h).
 *
 * include/gpuart_moments.h recommends a long window (max_history 32) for the guided preview, and include/gpuart_temporal.h says that
 * the window is the only bound on the lag when lighting changes behind the history's back (a moved diffuse user sphere changes shadows
 * elsewhere). gpuart_temporal_accumulate is a weighted mean whose taps and weights depend on the G-buffers, the views and the
 * parameters alone, so a THIRD gpuart_temporal handle that is given the same radiance, G-buffers, views and commits as the first, with
 * max_history = fast_history, holds the same light over a short window. The two blends differ only in how much old light they hold;
 * the measured moments say how large a difference noise alone explains. gpuart_antilag_mix compares the two over a 7x7 neighbourhood
 * and moves the long blend, and its len, towards the short one where they disagree by more than that: the fast/slow history pair of
 * real-time denoisers. The mixed len is what the next stage is given: gpuart_moments_error(out, out_len, moments, ...) sees
 * B = out_len*q, so where the history is distrusted its error map grows by itself, below min_batches it falls back to the spatial
 * estimate, and gpuart_refine_run filters more there. Like the other image libraries this one works on images alone.
 *
 * Every operation in fp32, in exactly this order (tests/antilag_ref.py restates it in NumPy, bit for bit):
 *   L(c), max(a, b) and the surface-pixel rule are those of include/gpuart_moments.h. s, f: the slow and the fast blend of the pixel,
 *   sl, fl their len, m the blended moments {m1, m2, q, a}.
 *   1. The statistic of a pixel. It VOTES iff it is a surface pixel, B = sl*m.b >= min_batches and fl < sl. For a voting pixel:
 *      v = m.g - m.r*m.r; v = (v < 0 ? 0 : v); sv = (v*B)/(B - 1.0f) (the sample variance of one view's luminance); Bf = fl*m.b;
 *      var = sv*(1.0f/Bf - 1.0f/B) (the variance of the difference of two nested means); r = L(f.rgb) - L(s.rgb). Where var > 0:
 *      lim = clip*sqrt(var); r = (r > lim ? lim : (r < -lim ? -lim : r)): one firefly must not speak for 49 pixels. Where var is not
 *      > 0, r stays as it is: a noise-free change is still a change.
 *   2. Not a surface pixel: out = s, out_len = sl, alpha = 0.
 *   3. A surface pixel p (voting or not): over q = p + (dx, dy) (dy outer, dx inner, -3..3, p included) that lie inside the tile and
 *      vote: cnt += 1, S1 += r_q, S2 += var_q. If cnt < min_votes: Z = 0. Otherwise, if S2 > 0: Z = |S1|/sqrt(S2); otherwise
 *      Z = (S1 == 0 ? 0 : +inf). t = (Z - z_lo)/(z_hi - z_lo); alpha = (t > 0 ? t : 0); alpha = (alpha > 1 ? 1 : alpha).
 *   4. alpha > 0: out.rgb = s + alpha*(f - s) per channel, out_len = sl + alpha*(fl - sl). alpha == 0: out and out_len are s and sl,
 *      bit for bit. out.a = s.a always.
 * Non-finite inputs are outside this contract; every index is still range-checked before use.
 *
 * The approximations. Bf uses the LONG history's q (the short one's moments are not carried): with one path per view q is 1 in both.
 * m1 and m2 still hold the light from before the change, so behind a change the error map of gpuart_moments_error is over-estimated
 * rather than under-estimated. Neighbouring pixels share bilinear taps of the history, so their r are correlated and Z under no change
 * is wider than N(0, 1): z_lo and z_hi are chosen by measurement (tools/antilag_quality.py, profiles/antilag.txt), not from a table.
 *
 * Defaults: fast_history 4, min_batches 8, min_votes 8, clip 3, z_lo 2, z_hi 4. Chosen on two scenes only, the box and scene P at
 * 160 x 120, one path per view, window 32, by tools/antilag_quality.py (profiles/antilag.txt states the rule and the sweep).
 *
 * Conventions as include/gpuart_moments.h: 0 on success or a negative gpuart_hip_status; the message of the last failure (per thread)
 * from gpuart_antilag_last_error(). Images are tiles of w x h pixels, row-major, row 0 at the bottom. One handle per device; it owns
 * its HIP stream, the copy of `slow` and `slow_len` an in-place call reads (20 bytes per pixel: a block's window reaches into pixels
 * another block writes) and the staging memory of the host entry point (116 bytes per pixel), kept for the next call of the same size
 * or smaller.
 */
#ifndef GPUART_ANTILAG_H
#define GPUART_ANTILAG_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_antilag gpuart_antilag;

typedef struct gpuart_antilag_params {
    float fast_history; /* max_history of the handle that carries the fast history (finite, >= 0); mix does not read it */
    float min_batches;  /* least effective number of batches B of the slow history at which a pixel votes (finite, > 1) */
    float min_votes;    /* least number of voting pixels in the window for a verdict (finite, >= 1) */
    float clip;         /* a vote is clipped to this many standard deviations (finite, > 0) */
    float z_lo;         /* Z at and below which the slow history is kept (finite, >= 0) */
    float z_hi;         /* Z at and above which the fast history replaces it (finite, > z_lo) */
} gpuart_antilag_params;

/* A handle on HIP device `device`. */
int gpuart_antilag_create(int device, gpuart_antilag **out);
int gpuart_antilag_destroy(gpuart_antilag *a);
/* fast_history 4, min_batches 8, min_votes 8, clip 3, z_lo 2, z_hi 4. */
int gpuart_antilag_defaults(gpuart_antilag_params *p);

/* Device memory, asynchronous on the handle's stream (gpuart_antilag_finish before the outputs are used). The inputs must be complete
 * when the call is made. slow, slow_len: the out_rgba (w*h*4 floats) and out_len (w*h floats) of the gpuart_temporal_accumulate that
 * blended the radiance with the long window; fast, fast_len: the same from a handle that saw the same commits with max_history =
 * fast_history; moments: the out_rgba of the long window's second handle (include/gpuart_moments.h); hits, prims: the G-buffer of the
 * tile. out: w*h*4 floats, may be slow itself; out_len: w*h floats, may be slow_len itself; alpha: w*h floats or NULL. slow, fast,
 * moments, hits and out 16-byte aligned, the others 4-byte aligned. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with nothing written,
 * for NULL (alpha excepted) or misaligned pointers, w or h 0 or above 65536, a parameter out of its range, an output overlapping an
 * input other than out == slow and out_len == slow_len, or another output. */
int gpuart_antilag_mix(gpuart_antilag *a, const float *slow, const float *slow_len, const float *fast, const float *fast_len,
                       const float *moments, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w,
                       uint32_t h, const gpuart_antilag_params *p, float *out, float *out_len, float *alpha);
/* The same in host memory (every pointer 4-byte aligned), synchronous (staged through the handle's memory). */
int gpuart_antilag_mix_host(gpuart_antilag *a, const float *slow, const float *slow_len, const float *fast, const float *fast_len,
                            const float *moments, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w,
                            uint32_t h, const gpuart_antilag_params *p, float *out, float *out_len, float *alpha);
/* Waits for the handle's stream. */
int gpuart_antilag_finish(gpuart_antilag *a);
const char *gpuart_antilag_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_ANTILAG_H */
