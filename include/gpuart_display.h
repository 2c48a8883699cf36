/* gpuart_display.h — C ABI of libgpuart_display.so: the display stage (MI355X, gfx950). Linear float radiance in, 8-bit frames out:
 * exposure (fixed or adapted to the frame's luminance histogram), a tone curve, the display transfer function, an ordered dither
 * and the packing, all on the device, so that a frame leaves it as 4 bytes per pixel instead of 16. The reference shows the radiance
 * clamped to [0, 1] in its GL framebuffer; the defaults here are that (the bytes of gpuart_cli --ppm). Like the other image libraries
 * this one works on images alone and knows nothing of the scene or the tree.
 *
 * Every operation in fp32, in exactly this order, unless stated (tests/display_ref.py restates it in NumPy, bit for bit):
 *   L(c) = (0.2126f*c.r + 0.7152f*c.g) + 0.0722f*c.b.
 *
 * Exposure, only with auto_exposure; two kernels, nothing returns to the host in between.
 *   The histogram, per pixel: x = (c > 0 ? c : 0) per channel (a NaN and a negative become 0), L = L(x). A pixel whose L is not
 *   finite or not > 0 is counted in `skipped`; every other one in bin b = clamp((int)(bits(L) >> 21) - 380, 0, 255): four bins per
 *   octave from 2^-32 to 2^32, the float's exponent and its top two mantissa bits, a piecewise-linear log2. The counts are integers,
 *   so they do not depend on the order and are the same in every run.
 *   The gain, in integers and fp64:
 *   1. N = sum of h[b]. N = 0: the exposure word stays as it is.
 *   2. lo = floor((double)lo_share*N), hi = floor((double)hi_share*N).
 *   3. The window is the pixel ranks [lo, N - hi) in ascending bin order; t[b] is the part of bin b inside it.
 *   4. S = sum of t[b]*(2b + 1), Nw = sum of t[b] (64-bit integers).
 *   5. m = (double)S/(double)Nw/8 - 32.
 *   6. i = floor(m), f = m - i, Lavg = ldexp(1 + f, i): the inverse of the bins' piecewise-linear log.
 *   7. target = clamp((double)key/Lavg, min_gain, max_gain).
 *   8. g = valid ? g_prev + (target - g_prev)*adapt : target (fp64, g_prev the stored float), stored as float with valid = 1.
 *   The word holds g = 1, not valid, after create and after reset. The gain in force is G = gain*g (a float product) with
 *   auto_exposure and gain without. Scaling every radiance by 2^n moves every pixel by 4n bins, so wherever no clamp acts and S/Nw
 *   is exact (Nw a power of two, for one) target is scaled by exactly 2^-n.
 *
 * Encode, per pixel; alpha is ignored and written as 255.
 *   1. x = (c > 0 ? c : 0); x = x*G; x = (x < 65504 ? x : 65504) per channel: everything after is finite.
 *   2. curve 0: y = x.
 *      curve 1 (extended Reinhard on the luminance): L = L(x), Lo = (L*(1 + L/(white*white)))/(1 + L), s = (L > 0 ? Lo/L : 0), y = x*s.
 *      curve 2 (the ACES fit, per channel): y = (x*(2.51f*x + 0.03f))/(x*(2.43f*x + 0.59f) + 0.14f).
 *   3. y = (y < 1 ? y : 1).
 *   4. transfer 0 (linear): q = y*255, k = (int)q, frac = q - (float)k.
 *      transfer 1 (sRGB): a table E[0..255], E[j] the fp32 nearest to the float64 value of the inverse sRGB function at j/255
 *      (v/12.92 up to 0.04045, ((v + 0.055)/1.055)^2.4 above; gpuart_display_srgb_table). k is the largest index in 0..254 with
 *      E[k] <= y and frac = (y - E[k])/(E[k+1] - E[k]): linear inside one code step, at most 0.0084 of a code from the true curve.
 *   5. t = 0.5f without dither; with it t = ((float)B8[(origin_y + ly) & 7][(origin_x + lx) & 7] + 0.5f)/64 for the pixel (lx, ly) of
 *      the image, B8 the 8x8 Bayer index matrix (first row 0 32 8 40 2 34 10 42, second 48 16 56 24 50 18 58 26).
 *      code = k + (frac >= t).
 *   6. One little-endian word per pixel, r | g << 8 | b << 16 | 255 << 24.
 * With the defaults step 4 and 5 are std::lround(clamp(v, 0, 1)*255.0f) for every float v.
 *
 * Conventions as include/gpuart_moments.h: 0 on success or a negative gpuart_hip_status (GPUART_HIP_ERR_ARG, _DEVICE, _NO_DEVICE); the
 * message of the last failure (per thread) from gpuart_display_last_error(), which begins "display:". Images are tiles of w x h
 * pixels, row-major, in the local row order of the tile that gpuart_hip_read uses (row 0 at the bottom); the result has the input's
 * layout. The dither pattern follows the LOCAL rows: on an interleaved share (gpuart_hip_set_share) it does not follow frame rows. One
 * handle per device; it owns its HIP stream, the exposure word, the histogram and the staging memory of the host entry point (20
 * bytes per pixel, kept for the next call of the same size or smaller).
 */
#ifndef GPUART_DISPLAY_H
#define GPUART_DISPLAY_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_display gpuart_display;

enum { GPUART_DISPLAY_CLAMP = 0, GPUART_DISPLAY_REINHARD = 1, GPUART_DISPLAY_ACES = 2 };  /* curve */
enum { GPUART_DISPLAY_LINEAR = 0, GPUART_DISPLAY_SRGB = 1 };                              /* transfer */

/* Which of the Renderer's frames Renderer::ReadDisplay encodes (csrc/host/renderer.h); the library itself takes any image. */
typedef enum gpuart_display_source {
    GPUART_DISPLAY_RADIANCE = 0,       /* ReadRadiance(normalized) */
    GPUART_DISPLAY_DIRECT = 1,         /* ReadDirectLighting */
    GPUART_DISPLAY_DENOISED = 2,       /* ReadDenoised */
    GPUART_DISPLAY_PREVIEW = 3,        /* ReadPreview */
    GPUART_DISPLAY_GUIDED_PREVIEW = 4, /* ReadGuidedPreview */
    GPUART_DISPLAY_REFINED = 5         /* ReadRefined */
} gpuart_display_source;

typedef struct gpuart_display_params {
    float gain;             /* the fixed exposure: every channel is multiplied by it (finite, > 0) */
    uint32_t auto_exposure; /* 0/1: also multiply by the gain adapted to the frame's histogram */
    float key;              /* the luminance the window's log-average is brought to (finite, > 0) */
    float lo_share;         /* share of the counted pixels, the darkest, left out of the average (>= 0) */
    float hi_share;         /* share of the brightest left out (>= 0; lo_share + hi_share < 1) */
    float adapt;            /* how far a call moves the adapted gain towards its target (in (0, 1]) */
    float min_gain;         /* the target's bounds (finite, 0 < min_gain <= max_gain) */
    float max_gain;
    uint32_t curve;         /* GPUART_DISPLAY_CLAMP, _REINHARD, _ACES */
    float white;            /* the extended Reinhard curve's white point: the luminance that maps to 1 (finite, > 0) */
    uint32_t transfer;      /* GPUART_DISPLAY_LINEAR, _SRGB */
    uint32_t dither;        /* 0/1: the 8x8 ordered dither */
} gpuart_display_params;

/* What gpuart_display_read_state returns. The histogram is that of the last run with auto_exposure (zeros before the first). */
typedef struct gpuart_display_state {
    uint64_t histogram[256];
    uint64_t counted; /* the histogram's sum N */
    uint64_t skipped; /* pixels whose luminance was not finite or not above 0 */
    float gain;       /* g, the adapted gain in force: 1 until a run with auto_exposure counted a pixel */
    uint32_t valid;   /* 0 after create and reset: the next target is taken whole, whatever adapt is */
} gpuart_display_state;

/* A handle on HIP device `device`. */
int gpuart_display_create(int device, gpuart_display **out);
int gpuart_display_destroy(gpuart_display *d);
/* gain 1, auto_exposure 0, key 0.18, lo_share 0.5, hi_share 0.02, adapt 1, min_gain 2^-16, max_gain 2^16, curve clamp, white 4,
 * transfer linear, dither 0. */
int gpuart_display_defaults(gpuart_display_params *p);
/* Forgets the adapted exposure: g = 1, not valid. Asynchronous on the handle's stream. */
int gpuart_display_reset(gpuart_display *d);

/* Device memory, asynchronous on the handle's stream (gpuart_display_finish before rgba8 is used). The input must be complete when
 * the call is made. rgba: w*h*4 floats; rgba8: w*h*4 bytes; both 16-byte aligned. (origin_x, origin_y): where pixel (0, 0) of the
 * image lies in the dither pattern. p = NULL: the defaults. GPUART_HIP_ERR_ARG, with nothing written, for a parameter that is not
 * finite or out of its range (checked first, so that the message names the field), a NULL handle, NULL or misaligned pointers, w or
 * h 0 or above 65536, rgba8 overlapping rgba. */
int gpuart_display_run(gpuart_display *d, const float *rgba, uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t origin_x, uint32_t origin_y,
                       const gpuart_display_params *p);
/* The same in host memory (rgba 4-byte aligned), synchronous (staged through the handle's memory). */
int gpuart_display_run_host(gpuart_display *d, const float *rgba, uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t origin_x,
                            uint32_t origin_y, const gpuart_display_params *p);
/* Waits for the handle's stream and copies its state out. */
int gpuart_display_read_state(gpuart_display *d, gpuart_display_state *out);
/* The 256 floats of E. Host only: needs neither a handle nor a device. */
int gpuart_display_srgb_table(float *out256);
/* Waits for the handle's stream. */
int gpuart_display_finish(gpuart_display *d);
const char *gpuart_display_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_DISPLAY_H */
