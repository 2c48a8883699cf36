// converge.hip — libgpuart_converge.so (gfx950): the per-pixel standard error of the accumulated radiance by weighted batch means and
// its reduction over the frame, include/gpuart_converge.h, which states both operation by operation. Built like the denoiser — fp32
// denormals kept, IEEE '/' and sqrt, no contraction — so that every value is the one tests/converge_ref.py computes in NumPy float32.
// DESIGN.md "Convergence estimate" describes the kernels.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/estimate.h"
#include "gpuart_converge.h"

namespace {

const char LIB[] = "converge";

// The row block of image_lib.h: the accumulator and the state are coalesced 16-byte-per-lane accesses (1 KiB per wave instruction) and
// the error map 4-byte-per-lane ones.
// k_cv_measure walks the rows with a stride of the grid's, so that a wave ends in three atomics whatever the height: the most blocks it is given.
constexpr unsigned MEASURE_MAX_BLOCKS = 2048;

/// Pure streaming: 32 bytes in, 16 out per pixel.
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_cv_update(const float4 *accum, float4 *state, int w, int h, float b, float r) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    state[i] = estimate_step(accum[i], state[i], b, r);
}

/// What the frame's reduction ends in; zeroed on the stream before every k_cv_measure.
struct Words {
    unsigned long long above, non_finite;  ///< 64 bits: 65536 x 65536 pixels overflow 32
    unsigned int max_bits, pad;            ///< the largest finite e: non-negative floats order as their bit patterns do
};

/// 16 bytes in per pixel, 4 out with a map. Per wave: __ballot + __popcll for the two counts and a maximum over the lanes, kept in
/// wave-uniform registers across the rows the wave walks, then one atomic per word.
template <bool MAP>
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_cv_measure(const float4 *state, int w, int h, float nb1, float total, float threshold,
                                                               float lum_floor, float *map, Words *out) {
    const int x = blockIdx.x * ROW_X + threadIdx.x;
    unsigned long long above = 0, non_finite = 0;
    unsigned int mx = 0;
    for (int y = blockIdx.y * ROW_Y + threadIdx.y; y < h; y += gridDim.y * ROW_Y) {  // (wave-uniform: a wave is one row)
        bool ab = false, nf = false;
        if (x < w) {
            const size_t i = (size_t)y * w + x;
            const float e = estimate_error(state[i], nb1, total, lum_floor);
            if (MAP) map[i] = e;
            ab = !(e <= threshold);
            nf = !(fabsf(e) < INFINITY);  // NaN or +-inf
            if (!nf) {
                const unsigned int bits = __float_as_uint(e);  // (e >= +0 here: se >= +0 and the divisor > 0)
                mx = bits > mx ? bits : mx;
            }
        }
        above += __popcll(__ballot(ab));
        non_finite += __popcll(__ballot(nf));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if (threadIdx.x == 0) {
        if (above) atomicAdd(&out->above, above);
        if (non_finite) atomicAdd(&out->non_finite, non_finite);
        if (mx) atomicMax(&out->max_bits, mx);
    }
}

}  // namespace

struct gpuart_converge : ImageHandle {
    DeviceBuffer state;  ///< 16 bytes per pixel: {mean, m2, prevL, 0}
    DeviceBuffer stage;  ///< update_host: the accumulator (16 bytes per pixel); measure_host: the error map (4)
    Words *words = nullptr;   ///< device
    Words *pinned = nullptr;  ///< host, pinned: where a measure reads them
    uint32_t w = 0, h = 0;    ///< of the state; 0 after create and reset
    uint32_t total = 0, batches = 0;
};

namespace {

/// The checks both update entry points make; `align` is what accum must be aligned to. Nothing has been written when they fail.
int check_update(gpuart_converge *c, const void *accum, uint32_t paths_total, uint32_t w, uint32_t h, size_t align) {
    if (int r = check_handle(LIB, c)) return r;
    if (!accum) return fail(GPUART_HIP_ERR_ARG, "converge: accum is NULL");
    if (misaligned({accum}, align)) return fail(GPUART_HIP_ERR_ARG, "converge: misaligned pointer (accum needs " + std::to_string(align) + " bytes)");
    if (int r = check_size(LIB, w, h)) return r;
    if (c->w && (w != c->w || h != c->h))
        return fail(GPUART_HIP_ERR_ARG, "converge: size " + std::to_string(w) + " x " + std::to_string(h) + " is not the state's " + std::to_string(c->w) +
                                            " x " + std::to_string(c->h) + " (reset the handle first)");
    if (paths_total <= c->total)
        return fail(GPUART_HIP_ERR_ARG, "converge: paths_total " + std::to_string(paths_total) + " is not above the " + std::to_string(c->total) + " already seen");
    if (paths_total > GPUART_CONVERGE_MAX_PATHS)
        return fail(GPUART_HIP_ERR_ARG, "converge: paths_total " + std::to_string(paths_total) + " is above 2^24 (not exact in fp32)");
    return 0;
}

/// One update on device memory, on the handle's stream.
int launch_update(gpuart_converge *c, const float4 *accum, uint32_t paths_total, uint32_t w, uint32_t h) {
    const size_t n = (size_t)w * h;
    if (!c->w) {  // the first batch after create or reset: a state of zeros
        if (int r = ensure(c->stream, c->state, n * 16)) return r;
        HIP_TRY(hipMemsetAsync(c->state.mem, 0, n * 16, c->stream));
    }
    const float b = (float)(paths_total - c->total), Wn = (float)paths_total;
    const float r = b / Wn;
    k_cv_update<<<row_grid(w, h), row_block(), 0, c->stream>>>(accum, (float4 *)c->state.mem, (int)w, (int)h, b, r);
    HIP_TRY(hipGetLastError());
    c->w = w;
    c->h = h;
    c->total = paths_total;
    c->batches += 1;
    return 0;
}

int check_measure(gpuart_converge *c, float threshold, float lum_floor, const void *map, const gpuart_converge_summary *summary) {
    if (int r = check_handle(LIB, c)) return r;
    if (!summary) return fail(GPUART_HIP_ERR_ARG, "converge: summary is NULL");
    if (misaligned({map}, 4)) return fail(GPUART_HIP_ERR_ARG, "converge: misaligned pointer (error_map needs 4 bytes)");
    if (!std::isfinite(threshold) || !(threshold >= 0)) return fail(GPUART_HIP_ERR_ARG, "converge: threshold must be finite and >= 0");
    if (!std::isfinite(lum_floor) || !(lum_floor > 0)) return fail(GPUART_HIP_ERR_ARG, "converge: lum_floor must be finite and > 0");
    if (c->batches < 2)
        return fail(GPUART_HIP_ERR_ARG, "converge: a measure needs at least 2 batches (" + std::to_string(c->batches) + " so far)");
    return 0;
}

/// The reduction (and the map, in device memory) on the handle's stream; the words are in c->pinned when it returns 0.
int launch_measure(gpuart_converge *c, float threshold, float lum_floor, float *map) {
    HIP_TRY(hipMemsetAsync(c->words, 0, sizeof(Words), c->stream));
    dim3 grid = row_grid(c->w, c->h);
    const unsigned cap = MEASURE_MAX_BLOCKS / grid.x ? MEASURE_MAX_BLOCKS / grid.x : 1u;
    if (grid.y > cap) grid.y = cap;
    const dim3 block = row_block();
    const float nb1 = (float)(c->batches - 1), total = (float)c->total;
    if (map)
        k_cv_measure<true><<<grid, block, 0, c->stream>>>((const float4 *)c->state.mem, (int)c->w, (int)c->h, nb1, total, threshold, lum_floor, map, c->words);
    else
        k_cv_measure<false><<<grid, block, 0, c->stream>>>((const float4 *)c->state.mem, (int)c->w, (int)c->h, nb1, total, threshold, lum_floor, nullptr, c->words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->pinned, c->words, sizeof(Words), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

void fill(const gpuart_converge *c, gpuart_converge_summary *s) {
    s->pixels = (uint64_t)c->w * c->h;
    s->above = c->pinned->above;
    s->non_finite = c->pinned->non_finite;
    const uint32_t bits = c->pinned->max_bits;
    static_assert(sizeof(float) == sizeof(uint32_t), "fp32");
    __builtin_memcpy(&s->max_error, &bits, 4);
    s->batches = c->batches;
    s->total = c->total;
}

}  // namespace

extern "C" {

const char *gpuart_converge_last_error(void) { return g_last_error.c_str(); }

int gpuart_converge_create(int device, gpuart_converge **out) {
    if (int r = create_handle(LIB, device, out)) return r;
    gpuart_converge *c = *out;
    if (hipMalloc((void **)&c->words, sizeof(Words)) != hipSuccess || hipHostMalloc((void **)&c->pinned, sizeof(Words), hipHostMallocDefault) != hipSuccess) {
        gpuart_converge_destroy(c);
        *out = nullptr;
        return fail(GPUART_HIP_ERR_DEVICE, "converge: allocating the summary words failed");
    }
    return 0;
}

int gpuart_converge_destroy(gpuart_converge *c) {
    if (!c) return 0;
    destroy_handle(c, {c->state.mem, c->stage.mem, (void *)c->words});
    if (c->pinned) (void)hipHostFree(c->pinned);
    delete c;
    return 0;
}

int gpuart_converge_reset(gpuart_converge *c) {
    if (int r = check_handle(LIB, c)) return r;
    c->w = c->h = 0;  // the next update zeroes the state it then has
    c->total = c->batches = 0;
    return 0;
}

int gpuart_converge_finish(gpuart_converge *c) { return finish_handle(LIB, c); }

int gpuart_converge_update(gpuart_converge *c, const float *accum, uint32_t paths_total, uint32_t w, uint32_t h) {
    if (int r = check_update(c, accum, paths_total, w, h, 16)) return r;
    HIP_TRY(hipSetDevice(c->device));
    return launch_update(c, (const float4 *)accum, paths_total, w, h);
}

int gpuart_converge_update_host(gpuart_converge *c, const float *accum, uint32_t paths_total, uint32_t w, uint32_t h) {
    if (int r = check_update(c, accum, paths_total, w, h, 4)) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)w * h;
    if (int r = ensure(c->stream, c->stage, n * 16)) return r;
    HIP_TRY(hipMemcpyAsync(c->stage.mem, accum, n * 16, hipMemcpyHostToDevice, c->stream));
    if (int r = launch_update(c, (const float4 *)c->stage.mem, paths_total, w, h)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int gpuart_converge_measure(gpuart_converge *c, float threshold, float lum_floor, float *error_map, gpuart_converge_summary *summary) {
    if (int r = check_measure(c, threshold, lum_floor, error_map, summary)) return r;
    HIP_TRY(hipSetDevice(c->device));
    if (int r = launch_measure(c, threshold, lum_floor, error_map)) return r;
    HIP_TRY(hipStreamSynchronize(c->stream));
    fill(c, summary);
    return 0;
}

int gpuart_converge_measure_host(gpuart_converge *c, float threshold, float lum_floor, float *error_map, gpuart_converge_summary *summary) {
    if (int r = check_measure(c, threshold, lum_floor, error_map, summary)) return r;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)c->w * c->h;
    if (error_map)
        if (int r = ensure(c->stream, c->stage, n * 4)) return r;
    if (int r = launch_measure(c, threshold, lum_floor, error_map ? (float *)c->stage.mem : nullptr)) return r;
    if (error_map) HIP_TRY(hipMemcpyAsync(error_map, c->stage.mem, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    fill(c, summary);
    return 0;
}

int gpuart_converge_read_state(gpuart_converge *c, float *state) {
    if (int r = check_handle(LIB, c)) return r;
    if (!state || (uintptr_t)state % 4) return fail(GPUART_HIP_ERR_ARG, "converge: state is NULL or misaligned");
    if (!c->w) return fail(GPUART_HIP_ERR_ARG, "converge: no state before the first update");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(state, c->state.mem, (size_t)c->w * c->h * 16, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
