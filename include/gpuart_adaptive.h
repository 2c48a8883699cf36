/* gpuart_adaptive.h — C ABI of libgpuart_adaptive.so: the convergence estimate of include/gpuart_converge.h kept per 8x8 pixel block,
 * the decision which blocks still need paths, and the normalisation of an accumulator whose blocks hold different numbers of paths
 * (MI355X, gfx950). No reference counterpart: the reference renders every pixel with the path count it is given.
 *
 * It serves adaptive sampling (gpuart_hip_set_active_blocks, Renderer::RenderAdaptive): a pass renders only the listed blocks, so the
 * blocks of one accumulator stop at different path counts. gpuart_converge keeps ONE path total for the frame; this library keeps one per
 * block. Blocks are the 8x8 blocks of include/gpuart_hip.h: ceil(w/8) x ceil(h/8) of them, row-major, ragged at the right and top edges.
 *
 * State: per pixel one float4 {mean, m2, prevL, 0}, as the convergence estimate; per block four words {seen, batches, active, 0}:
 * the paths per pixel at the block's last update, how many updates moved it, and whether it still needs paths. After create or reset
 * the pixel state is all zeros, seen = batches = 0 and active = 1 for every block.
 *
 * update, for every pixel of a block with paths[block] != seen[block], every operation in fp32 in exactly this order
 * (tests/adaptive_ref.py restates it in NumPy through tests/converge_ref.py, bit for bit):
 *   b     = (float)(paths[block] - seen[block]);  Wn = (float)paths[block];  r = b / Wn
 *   Lk    = L(accum);  y = (Lk - prevL) / b;  d = y - mean              (L as include/gpuart_converge.h)
 *   mean' = mean + r*d;  m2' = m2 + (b*d)*(y - mean');  prevL' = Lk
 * the convergence estimate's weighted update with the block's own batch weight and total. Pixels of a block whose count did not move
 * are not touched. Then, one thread per block and after every pixel has been written: seen = paths, batches += 1 for the blocks that
 * moved.
 *
 * e of a pixel, with its block's batches and seen (batches >= 2):
 *   v  = (m2 < 0 ? 0 : m2) / (float)(batches - 1);  se = sqrt(v / (float)seen);  e = se / (mean > lum_floor ? mean : lum_floor)
 * A pixel whose block has fewer than two batches has no estimate yet: its e is +inf (which gpuart_refine treats as invalid).
 *
 * select: a block stays active iff it is active now and (seen < min_paths, or batches < 2, or one of its pixels inside the image has
 * !(e <= threshold): a NaN counts). A block that was retired never comes back. The summary's reductions are integer counts and a
 * maximum over non-negative floats through their bit patterns: exact and the same in every run. `above` and `non_finite` count the
 * pixels of blocks without an estimate too (their e is +inf).
 *
 * normalize: out.rgb = accum.rgb / (float)(paths[block] ? paths[block] : 1) with IEEE division, what gpuart_hip_export's divide_by
 * does with one scalar; alpha is copied.
 *
 * Conventions as include/gpuart_converge.h: 0 or a negative gpuart_hip_status, the message of the last failure (per thread) from
 * gpuart_adaptive_last_error(); images are w x h RGBA32F, row-major, row 0 at the bottom; block counts are ceil(w/8)*ceil(h/8)
 * uint32 words, what gpuart_hip_export_block_paths / _read_block_paths give. One handle per device; it owns its HIP stream, the state
 * and the staging memory of the host entry points.
 */
#ifndef GPUART_ADAPTIVE_H
#define GPUART_ADAPTIVE_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_converge.h"
#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_adaptive gpuart_adaptive;

typedef struct gpuart_adaptive_summary {
    uint64_t pixels;        /* w*h */
    uint64_t above;         /* pixels with !(e <= threshold) */
    uint64_t non_finite;    /* pixels whose e is NaN or +-inf */
    uint64_t paths_sum;     /* sum over the image's pixels of their block's seen: the work actually spent */
    uint32_t blocks;        /* ceil(w/8)*ceil(h/8) */
    uint32_t active_blocks; /* blocks that stay active: the length of the list */
    uint32_t paths_min;     /* smallest and largest seen over the blocks */
    uint32_t paths_max;
    float max_error;        /* the largest finite e; 0 if there is none */
    uint32_t reserved;
} gpuart_adaptive_summary; /* 56 bytes */

/* Paths per pixel a block must hold before it may retire when the caller has no better idea (gpuart_cli --adaptive-min): the smallest of
 * 8, 16, 32 and 64 whose worst RMSE against a uniform render of the same work is within 2 % of the best one (profiles/adaptive.txt,
 * section 1, tools/adaptive_quality.py). */
#define GPUART_ADAPTIVE_DEFAULT_MIN_PATHS 8u

int gpuart_adaptive_create(int device, gpuart_adaptive **out);
int gpuart_adaptive_destroy(gpuart_adaptive *a);
/* Forgets everything: zero state, every block active, and the next update may have any size. Host work only. */
int gpuart_adaptive_reset(gpuart_adaptive *a);

/* accum (w*h*4 floats, 16-byte aligned) and block_paths (one word per block, 4-byte aligned) in device memory, complete when the call
 * is made. The counts are read back and checked first (the call waits for that copy; the kernels are asynchronous on the handle's
 * stream): GPUART_HIP_ERR_ARG, with nothing written, for a count above GPUART_CONVERGE_MAX_PATHS or below the block's seen, a size
 * other than the state's (unless reset), a NULL or misaligned pointer, w or h 0 or above 65536. */
int gpuart_adaptive_update(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, uint32_t w, uint32_t h);
/* The same in host memory (4-byte aligned), synchronous. */
int gpuart_adaptive_update_host(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, uint32_t w, uint32_t h);

/* Synchronous. error_map (may be NULL): w*h floats in device memory, receives e per pixel. blocks_host (may be NULL): room for one
 * word per block in host memory, receives the ascending list of the blocks that stay active, summary->active_blocks of them.
 * GPUART_HIP_ERR_ARG, with nothing written, before the first update, for a threshold that is not finite and >= 0 (1e9 is fine), a
 * lum_floor that is not finite and > 0, a misaligned error_map or a NULL summary. */
int gpuart_adaptive_select(gpuart_adaptive *a, float threshold, float lum_floor, uint32_t min_paths, float *error_map,
                           uint32_t *blocks_host, gpuart_adaptive_summary *summary);
/* e per pixel into device memory (w*h floats; w, h the state's), asynchronous on the handle's stream. Changes nothing. */
int gpuart_adaptive_error_map(gpuart_adaptive *a, float lum_floor, float *error_map, uint32_t w, uint32_t h);

/* out = accum / its block's count, device memory (16-byte aligned images; out may be accum), asynchronous on the handle's stream.
 * Needs no state: any size. */
int gpuart_adaptive_normalize(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, float *out, uint32_t w, uint32_t h);
/* The same in host memory, synchronous. */
int gpuart_adaptive_normalize_host(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, float *out, uint32_t w, uint32_t h);

/* To host memory, synchronous: state (may be NULL) w*h*4 floats {mean, m2, prevL, 0}; block_state (may be NULL) four words per block
 * {seen, batches, active, 0}. GPUART_HIP_ERR_ARG before the first update. */
int gpuart_adaptive_read_state(gpuart_adaptive *a, float *state, uint32_t *block_state);
/* Waits for the handle's stream. */
int gpuart_adaptive_finish(gpuart_adaptive *a);
const char *gpuart_adaptive_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_ADAPTIVE_H */
