// display.hip — libgpuart_display.so (gfx950): exposure, tone curve, display transfer function, ordered dither and 8-bit packing, as
// include/gpuart_display.h states them operation by operation. Built without flushing fp32 denormals, with IEEE '/' and no
// contraction, so that every byte is the one tests/display_ref.py computes in NumPy. DESIGN.md "The display stage" describes the
// kernels.
#include <cmath>
#include <cstddef>

#include "../image/image_lib.h"
#include "gpuart_display.h"

namespace {

const char LIB[] = "display";

#define DP_FN __device__ __forceinline__

/// What the handle keeps on the device: the histogram of the last run with auto_exposure and the exposure word.
struct DevState {
    unsigned long long hist[256];  ///< 64 bits: 65536 x 65536 pixels in one bin overflow 32
    unsigned long long skipped;
    float g;
    uint32_t valid;
};

// ---- histogram ------------------------------------------------------------------------------------------------------------------
// The image as a flat array, walked with the grid's stride: 16 bytes in per pixel, four loads in flight per lane. A block counts into
// 256 words of LDS and ends in one global atomic per non-empty bin, and the grid is capped, so that a frame of any size ends in at
// most HIST_MAX_BLOCKS * 256 of them (about 10 ns each where they land on one cache line: DESIGN.md on k_cv_measure). A block of
// 1024 and one block per CU keep 16 waves per CU reading. Where every counted pixel of a wave falls into one bin — a flat frame, the
// LDS atomics' worst case — one lane adds the wave's count.
constexpr int HIST_THREADS = 1024, HIST_UNROLL = 4;
#ifndef DP_HIST_MAX_BLOCKS
#define DP_HIST_MAX_BLOCKS 256  // one per CU; profiles/display.txt has the measurement
#endif
constexpr unsigned HIST_MAX_BLOCKS = DP_HIST_MAX_BLOCKS;

DP_FN float pos(float c) { return c > 0.0f ? c : 0.0f; }  // (a NaN becomes 0)

DP_FN void count_pixel(const float4 c, unsigned int *s_hist, unsigned int &skipped) {
    const float L = lum(pos(c.x), pos(c.y), pos(c.z));
    if (L > 0.0f && L < INFINITY) {
        int b = (int)(__float_as_uint(L) >> 21) - 380;
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
        const int first = __builtin_amdgcn_readfirstlane(b);
        const unsigned long long same = __ballot(b == first);  // (among the lanes that count a pixel)
        if (b != first) atomicAdd(&s_hist[b], 1u);
        else if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1) atomicAdd(&s_hist[first], (unsigned int)__popcll(same));
    } else {
        skipped++;
    }
}

__global__ void __launch_bounds__(HIST_THREADS) k_dp_histogram(const float4 *rgba, unsigned long long n, DevState *st) {
    __shared__ unsigned int s_hist[256];
    __shared__ unsigned int s_skipped;
    if (threadIdx.x < 256) s_hist[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_skipped = 0;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * HIST_THREADS;
    unsigned long long i = (unsigned long long)blockIdx.x * HIST_THREADS + threadIdx.x;
    unsigned int skipped = 0;
    for (; i + (HIST_UNROLL - 1) * stride < n; i += HIST_UNROLL * stride) {
        float4 c[HIST_UNROLL];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) c[j] = rgba[i + j * stride];
#pragma unroll
        for (int j = 0; j < HIST_UNROLL; j++) count_pixel(c[j], s_hist, skipped);
    }
    for (; i < n; i += stride) count_pixel(rgba[i], s_hist, skipped);
    if (skipped) atomicAdd(&s_skipped, skipped);
    __syncthreads();
    if (threadIdx.x < 256 && s_hist[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], (unsigned long long)s_hist[threadIdx.x]);
    if (threadIdx.x == 0 && s_skipped) atomicAdd(&st->skipped, (unsigned long long)s_skipped);
}

// ---- exposure -------------------------------------------------------------------------------------------------------------------
// One wave: its lanes bring the 256 counts into LDS, its first lane walks them twice, in integers and fp64.
__global__ void __launch_bounds__(64) k_dp_exposure(DevState *st, float key, float lo_share, float hi_share, float adapt, float min_gain,
                                                    float max_gain) {
    __shared__ unsigned long long s_h[256];
    for (int b = threadIdx.x; b < 256; b += 64) s_h[b] = st->hist[b];
    __syncthreads();
    if (threadIdx.x != 0) return;
    unsigned long long N = 0;
    for (int b = 0; b < 256; b++) N += s_h[b];
    if (!N) return;
    const unsigned long long lo = (unsigned long long)floor((double)lo_share * (double)N), hi = (unsigned long long)floor((double)hi_share * (double)N);
    const unsigned long long end = hi < N ? N - hi : 0;
    unsigned long long at = 0, S = 0, Nw = 0;
    for (int b = 0; b < 256; b++) {
        const unsigned long long from = at > lo ? at : lo;
        at += s_h[b];
        const unsigned long long to = at < end ? at : end;
        if (to > from) {
            S += (to - from) * (unsigned long long)(2 * b + 1);
            Nw += to - from;
        }
    }
    if (!Nw) return;  // (the two floors' roundings left no rank: as N = 0)
    const double m = (double)S / (double)Nw / 8.0 - 32.0;
    const double i = floor(m), f = m - i;
    const double Lavg = ldexp(1.0 + f, (int)i);
    double target = (double)key / Lavg;
    target = target < (double)min_gain ? (double)min_gain : target;
    target = target > (double)max_gain ? (double)max_gain : target;
    const double prev = (double)st->g;
    const double g = st->valid ? prev + (target - prev) * (double)adapt : target;
    st->g = (float)g;
    st->valid = 1u;
}

// ---- encode ---------------------------------------------------------------------------------------------------------------------
// The image as a flat array; a thread takes four consecutive pixels: four 16-byte loads and one 16-byte store, aligned for any width
// (the last thread of an image whose size is no multiple of four stores its words one by one). The curve, the transfer and the dither
// are wave-uniform branches. The sRGB code is found by eight dependent steps through the table in LDS (1 KiB), three channels by four
// pixels of them independent of each other.
constexpr int ENC_THREADS = 256, ENC_PIXELS = 4;

DP_FN uint32_t bayer8(uint32_t x, uint32_t y) {  // B8[y & 7][x & 7]: the bits of x ^ y and of y, interleaved and reversed
    const uint32_t q = x ^ y;
    return (q & 1) << 5 | (y & 1) << 4 | (q & 2) << 2 | (y & 2) << 1 | (q & 4) >> 1 | (y & 4) >> 2;
}

DP_FN uint32_t quantize(float y, float t, bool srgb, const float *E) {
    int k;
    float frac;
    if (!srgb) {
        const float q = y * 255.0f;
        k = (int)q;
        frac = q - (float)k;
    } else {
        k = 0;
#pragma unroll
        for (int s = 128; s; s >>= 1) {
            const int j = k + s;
            if (j <= 254 && E[j] <= y) k = j;
        }
        const float e0 = E[k];
        frac = (y - e0) / (E[k + 1] - e0);
    }
    return (uint32_t)k + (frac >= t ? 1u : 0u);
}

__global__ void __launch_bounds__(ENC_THREADS) k_dp_encode(const float4 *rgba, uint32_t *out, unsigned long long n, uint32_t w, uint32_t ox,
                                                            uint32_t oy, float gain, const DevState *st, int curve, float white, int srgb,
                                                            int dither, const float *table) {
    __shared__ float s_E[256];
    if (srgb) {  // (uniform: every thread of the block is here)
        s_E[threadIdx.x] = table[threadIdx.x];
        __syncthreads();
    }
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * ENC_THREADS + threadIdx.x) * ENC_PIXELS;
    if (i0 >= n) return;
    const int cnt = n - i0 < ENC_PIXELS ? (int)(n - i0) : ENC_PIXELS;
    float4 c[ENC_PIXELS];
#pragma unroll
    for (int j = 0; j < ENC_PIXELS; j++) c[j] = j < cnt ? rgba[i0 + j] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float G = st ? gain * st->g : gain;
    uint32_t ly = (uint32_t)i0 / w, lx = (uint32_t)i0 - ly * w;  // (i0 < n <= 2^32)
    uint32_t word[ENC_PIXELS];
#pragma unroll
    for (int j = 0; j < ENC_PIXELS; j++) {
        float x[3] = {pos(c[j].x) * G, pos(c[j].y) * G, pos(c[j].z) * G};
        float y[3];
#pragma unroll
        for (int k = 0; k < 3; k++) x[k] = x[k] < 65504.0f ? x[k] : 65504.0f;
        if (curve == GPUART_DISPLAY_REINHARD) {
            const float L = lum(x[0], x[1], x[2]);
            const float Lo = (L * (1.0f + L / (white * white))) / (1.0f + L);
            const float s = L > 0.0f ? Lo / L : 0.0f;
#pragma unroll
            for (int k = 0; k < 3; k++) y[k] = x[k] * s;
        } else if (curve == GPUART_DISPLAY_ACES) {
#pragma unroll
            for (int k = 0; k < 3; k++) y[k] = (x[k] * (2.51f * x[k] + 0.03f)) / (x[k] * (2.43f * x[k] + 0.59f) + 0.14f);
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) y[k] = x[k];
        }
        const float t = dither ? ((float)bayer8(ox + lx, oy + ly) + 0.5f) / 64.0f : 0.5f;
        uint32_t code[3];
#pragma unroll
        for (int k = 0; k < 3; k++) code[k] = quantize(y[k] < 1.0f ? y[k] : 1.0f, t, srgb, s_E);
        word[j] = code[0] | code[1] << 8 | code[2] << 16 | 255u << 24;
        if (++lx == w) {
            lx = 0;
            ly++;
        }
    }
    if (cnt == ENC_PIXELS) {
        *(uint4 *)(out + i0) = make_uint4(word[0], word[1], word[2], word[3]);
    } else {
#pragma unroll
        for (int j = 0; j < ENC_PIXELS - 1; j++)
            if (j < cnt) out[i0 + j] = word[j];
    }
}

/// E of include/gpuart_display.h, made once.
const float *srgb_table() {
    static float E[256];
    static const bool made = [] {
        for (int j = 0; j < 256; j++) {
            const double v = (double)j / 255.0;
            E[j] = (float)(v <= 0.04045 ? v / 12.92 : std::pow((v + 0.055) / 1.055, 2.4));
        }
        return true;
    }();
    (void)made;
    return E;
}

}  // namespace

struct gpuart_display : ImageHandle {
    DevState *state = nullptr;  ///< device
    float *table = nullptr;     ///< device: E
    DeviceBuffer staging;       ///< run_host's: the radiance (16 bytes per pixel), then the words (4)
};

namespace {

int check_params(const gpuart_display_params *p) {
    if (!p) return 0;
    const auto bad = [](const char *what) { return fail(GPUART_HIP_ERR_ARG, std::string("display: ") + what); };
    if (!std::isfinite(p->gain) || !(p->gain > 0)) return bad("gain must be finite and > 0");
    if (p->auto_exposure > 1) return bad("auto_exposure must be 0 or 1");
    if (!std::isfinite(p->key) || !(p->key > 0)) return bad("key must be finite and > 0");
    if (!std::isfinite(p->lo_share) || !(p->lo_share >= 0)) return bad("lo_share must be finite and >= 0");
    if (!std::isfinite(p->hi_share) || !(p->hi_share >= 0)) return bad("hi_share must be finite and >= 0");
    if (!((double)p->lo_share + (double)p->hi_share < 1.0)) return bad("lo_share + hi_share must be < 1");
    if (!(p->adapt > 0) || !(p->adapt <= 1)) return bad("adapt must be in (0, 1]");
    if (!std::isfinite(p->min_gain) || !(p->min_gain > 0)) return bad("min_gain must be finite and > 0");
    if (!std::isfinite(p->max_gain) || !(p->max_gain >= p->min_gain)) return bad("max_gain must be finite and >= min_gain");
    if (p->curve > GPUART_DISPLAY_ACES) return bad("curve must be 0 (clamp), 1 (reinhard) or 2 (aces)");
    if (!std::isfinite(p->white) || !(p->white > 0)) return bad("white must be finite and > 0");
    if (p->transfer > GPUART_DISPLAY_SRGB) return bad("transfer must be 0 (linear) or 1 (sRGB)");
    if (p->dither > 1) return bad("dither must be 0 or 1");
    return 0;
}

/// The checks both run entry points make; `align` is what rgba and rgba8 must be aligned to (the host's words are bytes to the caller).
int check_run(gpuart_display *d, const void *rgba, const void *rgba8, uint32_t w, uint32_t h, const gpuart_display_params *p, size_t align,
              size_t align8) {
    if (int rc = check_params(p)) return rc;
    if (int rc = check_handle(LIB, d)) return rc;
    if (!rgba || !rgba8) return fail(GPUART_HIP_ERR_ARG, "display: rgba or rgba8 is NULL");
    if (misaligned({rgba}, align) || misaligned({rgba8}, align8))
        return fail(GPUART_HIP_ERR_ARG, "display: misaligned pointer (rgba needs " + std::to_string(align) + " bytes, rgba8 " + std::to_string(align8) + ")");
    if (int rc = check_size(LIB, w, h)) return rc;
    const size_t n = (size_t)w * h;
    if (overlaps(rgba8, n * 4, rgba, n * 16)) return fail(GPUART_HIP_ERR_ARG, "display: rgba8 overlaps rgba");
    return 0;
}

int launch(gpuart_display *d, const float4 *rgba, uint32_t *out, uint32_t w, uint32_t h, uint32_t ox, uint32_t oy, const gpuart_display_params &p) {
    const unsigned long long n = (unsigned long long)w * h;
    if (p.auto_exposure) {
        HIP_TRY(hipMemsetAsync(d->state, 0, offsetof(DevState, g), d->stream));
        const unsigned long long want = (n + HIST_THREADS - 1) / HIST_THREADS;
        k_dp_histogram<<<(unsigned)(want < HIST_MAX_BLOCKS ? want : HIST_MAX_BLOCKS), HIST_THREADS, 0, d->stream>>>(rgba, n, d->state);
        HIP_TRY(hipGetLastError());
        k_dp_exposure<<<1, 64, 0, d->stream>>>(d->state, p.key, p.lo_share, p.hi_share, p.adapt, p.min_gain, p.max_gain);
        HIP_TRY(hipGetLastError());
    }
    const unsigned long long threads = (n + ENC_PIXELS - 1) / ENC_PIXELS;
    k_dp_encode<<<(unsigned)((threads + ENC_THREADS - 1) / ENC_THREADS), ENC_THREADS, 0, d->stream>>>(
        rgba, out, n, w, ox, oy, p.gain, p.auto_exposure ? d->state : nullptr, (int)p.curve, p.white, (int)p.transfer, (int)p.dither, d->table);
    HIP_TRY(hipGetLastError());
    return 0;
}

/// g = 1, not valid, in the handle's stream order (the source is a constant, so nothing has to be waited for).
int reset_word(gpuart_display *d) {
    static const struct { float g; uint32_t valid; } word = {1.0f, 0u};
    HIP_TRY(hipMemcpyAsync(&d->state->g, &word, sizeof word, hipMemcpyHostToDevice, d->stream));
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_display_last_error(void) { return g_last_error.c_str(); }

int gpuart_display_defaults(gpuart_display_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "display: params is NULL");
    p->gain = 1.0f;
    p->auto_exposure = 0;
    p->key = 0.18f;
    p->lo_share = 0.5f;
    p->hi_share = 0.02f;
    p->adapt = 1.0f;
    p->min_gain = 1.0f / 65536.0f;
    p->max_gain = 65536.0f;
    p->curve = GPUART_DISPLAY_CLAMP;
    p->white = 4.0f;
    p->transfer = GPUART_DISPLAY_LINEAR;
    p->dither = 0;
    return 0;
}

int gpuart_display_srgb_table(float *out256) {
    if (!out256) return fail(GPUART_HIP_ERR_ARG, "display: out256 is NULL");
    const float *E = srgb_table();
    for (int j = 0; j < 256; j++) out256[j] = E[j];
    return 0;
}

int gpuart_display_create(int device, gpuart_display **out) {
    if (int rc = create_handle(LIB, device, out)) return rc;
    gpuart_display *d = *out;
    *out = nullptr;
    const auto undo = [&](hipError_t e, const char *what) {
        gpuart_display_destroy(d);
        return fail(GPUART_HIP_ERR_DEVICE, std::string("display: ") + what + ": " + hipGetErrorString(e));
    };
    hipError_t e;
    if ((e = hipMalloc((void **)&d->state, sizeof(DevState))) != hipSuccess) return undo(e, "allocating the state");
    if ((e = hipMalloc((void **)&d->table, 256 * sizeof(float))) != hipSuccess) return undo(e, "allocating the sRGB table");
    if ((e = hipMemset(d->state, 0, sizeof(DevState))) != hipSuccess) return undo(e, "clearing the state");
    if ((e = hipMemcpy(d->table, srgb_table(), 256 * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess) return undo(e, "uploading the sRGB table");
    if (int rc = reset_word(d)) {
        const std::string msg = g_last_error;
        gpuart_display_destroy(d);
        return fail(rc, msg);
    }
    *out = d;
    return 0;
}

int gpuart_display_destroy(gpuart_display *d) {
    if (!d) return 0;
    destroy_handle(d, {d->staging.mem, d->state, d->table});
    delete d;
    return 0;
}

int gpuart_display_finish(gpuart_display *d) { return finish_handle(LIB, d); }

int gpuart_display_reset(gpuart_display *d) {
    if (int rc = check_handle(LIB, d)) return rc;
    HIP_TRY(hipSetDevice(d->device));
    return reset_word(d);
}

int gpuart_display_run(gpuart_display *d, const float *rgba, uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t origin_x, uint32_t origin_y,
                       const gpuart_display_params *p) {
    if (int rc = check_run(d, rgba, rgba8, w, h, p, 16, 16)) return rc;
    HIP_TRY(hipSetDevice(d->device));
    return launch(d, (const float4 *)rgba, (uint32_t *)rgba8, w, h, origin_x, origin_y, params_or_defaults(p, gpuart_display_defaults));
}

int gpuart_display_run_host(gpuart_display *d, const float *rgba, uint8_t *rgba8, uint32_t w, uint32_t h, uint32_t origin_x,
                            uint32_t origin_y, const gpuart_display_params *p) {
    int rc = check_run(d, rgba, rgba8, w, h, p, 4, 1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)w * h;
    if ((rc = ensure(d->stream, d->staging, n * 20))) return rc;
    float4 *in = (float4 *)d->staging.mem;
    uint32_t *words = (uint32_t *)((char *)d->staging.mem + n * 16);
    HIP_TRY(hipMemcpyAsync(in, rgba, n * 16, hipMemcpyHostToDevice, d->stream));
    if ((rc = launch(d, in, words, w, h, origin_x, origin_y, params_or_defaults(p, gpuart_display_defaults)))) return rc;
    HIP_TRY(hipMemcpyAsync(rgba8, words, n * 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int gpuart_display_read_state(gpuart_display *d, gpuart_display_state *out) {
    if (int rc = check_handle(LIB, d)) return rc;
    if (!out) return fail(GPUART_HIP_ERR_ARG, "display: out is NULL");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    DevState s;
    HIP_TRY(hipMemcpy(&s, d->state, sizeof s, hipMemcpyDeviceToHost));
    out->counted = 0;
    for (int b = 0; b < 256; b++) out->counted += (out->histogram[b] = s.hist[b]);
    out->skipped = s.skipped;
    out->gain = s.g;
    out->valid = s.valid;
    return 0;
}

}  // extern "C"
