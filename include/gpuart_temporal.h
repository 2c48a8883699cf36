/* gpuart_temporal.h — C ABI of libgpuart_temporal.so: temporal accumulation by reprojection for the denoised preview
 * (MI355X, gfx950). No reference counterpart: the reference restarts its accumulation on every camera or user-sphere move
 * (src/main.cpp:549-599) and shows one path per pixel for as long as anything moves.
 *
 * The handle owns a HISTORY: per pixel of a tile a radiance, the number of paths it stands for ("length"), and the surface point it
 * was seen on, together with the view it was seen from. gpuart_temporal_accumulate re-samples that history into a new view through
 * the hit points of the new view's G-buffer (gpuart_hip_gbuffer, include/gpuart_hip.h), blends it with the new view's accumulator
 * by sample count, and — when asked to commit — makes the blend the next history. The scene is static apart from the user sphere.
 * The blend is meant to be handed to the spatial filter (include/gpuart_denoise.h) unchanged. Like that filter it works on images
 * alone and knows nothing of the scene or the tree.
 *
 * The algorithm, every operation in fp32, in exactly this order (tests/temporal_ref.py restates it in NumPy, bit for bit).
 *   dot(a, b)   = (a.x*b.x + a.y*b.y) + a.z*b.z
 *   cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 *   min(a, b)   = (a < b ? a : b)
 *   A pixel is a surface pixel if its record's type >= 0, unless its ordinal is -2 (the user sphere) and its view's userSphereFlags
 *   has EM_NONZERO (1) or SPECULAR (2) — the classes of include/gpuart_denoise.h. A surface pixel's class is (type & 3), plus 4 if
 *   its ordinal is -2. For a pixel of the current tile with colour c, hit point p and normal n (the record's p and n), s = (float)spp:
 *   1. Not a surface pixel: out = c, len = 0. It never serves as a tap.
 *   2. Surface pixel and the handle has no history, or no tap of step 4 carries weight: out = c, len = s.
 *   3. Back-projection into the history's view (pos', BL', DH', DV' = its pos, bottomLeft, deltaHorz, deltaVert; W' x H' its frame).
 *      A camera ray goes from pos' through BL' + u*DH' + v*DV', and frame pixel (x, y) has u = (x + 1/2)/W', v = (y + 1/2)/H'.
 *      Once per call: b = BL' - pos', N = cross(DH', DV'), A = cross(DV', b), B = cross(b, DH'), bN = dot(b, N).
 *      Per pixel: d = p - pos', dn = dot(d, N), k = bN/dn, u = dot(d, A)/dn, v = dot(d, B)/dn,
 *      fx = u*(float)W' - 0.5f, fy = v*(float)H' - 0.5f, x0 = floor(fx), y0 = floor(fy), ax = fx - x0, ay = fy - y0,
 *      tol = plane_tol*sqrt(dot(d, d)).
 *      The pixel has taps iff dn != 0 and k > 0 (p is in front of the old camera) and -1 <= x0 < W' and -1 <= y0 < H'.
 *   4. The taps are the frame pixels (x0 + ox, y0 + oy), oy = 0, 1 outer, ox = 0, 1 inner, with weight w = wy*wx,
 *      wx = (ox ? ax : 1.0f - ax), wy = (oy ? ay : 1.0f - ay). A tap is valid iff all of:
 *        it lies inside the old frame; its frame pixel belongs to the history's share (geom: column x0 <= x < x0 + tw, and the row is
 *        frame row y0 + (ly / band_rows)*band_stride + ly % band_rows of a local row ly < th);
 *        the history pixel there is a surface pixel of the same class; if that class is the user sphere's, the two views' userSphere
 *        are equal bit for bit; dot(n_tap, n) >= normal_min; |dot(p_tap - p, n)| <= tol.
 *      Over the valid taps in that order: Wsum += w, hr += w*hist.r (g, b alike), hl += w*hist_len.
 *      If Wsum > 0: h = hr/Wsum per channel, nh = min(hl/Wsum, max_history),
 *                   out = (nh*h + s*c)/(nh + s) per channel, len = nh + s. Otherwise step 2. Alpha is copied from c.
 *   5. commit: out.rgb, len, the pixel's class, n and p, and the view become the history (a pixel that is not a surface pixel is
 *      stored as such). The taps of a call read the history as it was before the call.
 * Weighting by sample count makes the blend the plain running mean where nothing moved; max_history turns it into an exponential
 * window, which bounds the lag when lighting changes behind the history's back (a moved diffuse user sphere changes shadows
 * elsewhere). What invalidates the history completely is the caller's business: gpuart_temporal_reset.
 * Non-finite radiance, hit points or camera vectors are outside this contract.
 * Step 3 is as accurate as fp32 allows, not more: against a float64 solve of the same camera equation fx and fy are off by up to about
 * 3 * W' * 2^-23 and 3 * H' * 2^-23 pixel (measured at 160 x 120 and 1920 x 1080: 6e-5 and 6e-4 pixel, tests/test_filter_edges.py). Frames
 * up to 65536 x 65536 are accepted, but for extreme aspect ratios the error is no longer a small share of a pixel: at 65536 x 16 fx is off
 * by more than a pixel (measured: up to 6.2), so the taps may be the neighbours of the right ones.
 *
 * Defaults: max_history 4, plane_tol 0.01, normal_min 0.8. They were chosen on two scenes only — the reference's box and the synthetic
 * scene P of gpuart_amd/synth_scenes.py, 160 x 120, eight views of a sideways camera track at one path each — by the sweep of
 * tools/temporal_quality.py (profiles/temporal.txt, which also states the rule). The error after the spatial filter is almost
 * insensitive to plane_tol and normal_min there, and a short window does better than a long one on the box: the filter sizes its
 * luminance edge by the variance of its input, so a cleaner input is also filtered less.
 *
 * Conventions as include/gpuart_denoise.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE);
 * the message of the last failure (per thread) from gpuart_temporal_last_error(). Images are tiles of w x h RGBA32F pixels,
 * row-major, in the local row order of the tile that gpuart_hip_read uses (row 0 at the bottom). One handle per device; it owns
 * its HIP stream, its history (two copies of 48 bytes per pixel: the taps read one, a commit writes the other) and the staging
 * memory of the host entry point (56 bytes per pixel).
 */
#ifndef GPUART_TEMPORAL_H
#define GPUART_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_temporal gpuart_temporal;

/* The view a tile was rendered from. */
typedef struct gpuart_temporal_view {
    float pos[3], bottomLeft[3], deltaHorz[3], deltaVert[3]; /* exactly as given to gpuart_hip_set_camera */
    gpuart_tile_geom geom;                                   /* the frame and the share the tile is (gpuart_hip_get_share) */
    float userSphere[4];                                     /* centre, radius: what gpuart_hip_gbuffer was given (zeros: none) */
    uint32_t userSphereFlags;                                /* 1 = EM_NONZERO, 2 = SPECULAR, 4 = FUZZY */
} gpuart_temporal_view;

typedef struct gpuart_temporal_params {
    float max_history; /* cap of the history's effective sample count (finite, >= 0; 0: the history never counts) */
    float plane_tol;   /* a tap's hit point may leave the pixel's tangent plane by this share of the distance to the old camera (finite, >= 0) */
    float normal_min;  /* least cosine between a tap's normal and the pixel's (-1..1) */
} gpuart_temporal_params;

/* A handle on HIP device `device`, without history. */
int gpuart_temporal_create(int device, gpuart_temporal **out);
int gpuart_temporal_destroy(gpuart_temporal *t);
/* max_history 4, plane_tol 0.01, normal_min 0.8. */
int gpuart_temporal_defaults(gpuart_temporal_params *p);
/* Drops the history (its memory is kept). */
int gpuart_temporal_reset(gpuart_temporal *t);

/* Device memory, asynchronous on the handle's stream (gpuart_temporal_finish before the outputs are used). The inputs must be
 * complete when the call is made. rgba: the normalised accumulator of the tile at `view`, w*h*4 floats, the mean of spp >= 1 paths;
 * hits, prims: the G-buffer of the same tile and view (w*h records, w*h ordinals, -2: the user sphere); out_rgba: w*h*4 floats, may
 * be rgba itself; out_len: w*h floats or NULL. rgba, hits and out_rgba 16-byte aligned, prims and out_len 4-byte aligned. p = NULL:
 * the defaults. commit != 0: the blend becomes the handle's history; commit = 0: the history is untouched, so a preview can be
 * taken any number of times while a view is still accumulating.
 * GPUART_HIP_ERR_ARG, and nothing written, for a NULL handle, view or pointer (out_len excepted), a misaligned pointer, w or h 0 or
 * above 65536, a geom that is not a w x h share of its frame (tw != w, th != h, W or H 0 or above 65536, x0 + tw > W, band_rows 0,
 * band_stride < band_rows, a last row beyond H), spp = 0, or parameters that are not finite or out of range. */
int gpuart_temporal_accumulate(gpuart_temporal *t, const float *rgba, uint32_t spp, const gpuart_ray_hit *hits, const int32_t *prims,
                               uint32_t w, uint32_t h, const gpuart_temporal_view *view, const gpuart_temporal_params *p, int commit,
                               float *out_rgba, float *out_len);
/* The same in host memory, synchronous (staged through the handle's memory); every pointer 4-byte aligned. */
int gpuart_temporal_accumulate_host(gpuart_temporal *t, const float *rgba, uint32_t spp, const gpuart_ray_hit *hits, const int32_t *prims,
                                    uint32_t w, uint32_t h, const gpuart_temporal_view *view, const gpuart_temporal_params *p, int commit,
                                    float *out_rgba, float *out_len);
/* Waits for the handle's stream. */
int gpuart_temporal_finish(gpuart_temporal *t);
const char *gpuart_temporal_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_TEMPORAL_H */
