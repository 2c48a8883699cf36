// denoise.hip — libgpuart_denoise.so (gfx950): the edge-aware à-trous denoiser of include/gpuart_denoise.h, which states the
// filter operation by operation. Built without flushing fp32 denormals, with IEEE '/' and sqrt and no contraction, so that every
// value is the one tests/denoise_ref.py computes in NumPy float32. DESIGN.md "Denoiser" describes the kernels.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/atrous.h"
#include "gpuart_denoise.h"

namespace {

const char LIB[] = "denoise";

#define DN_FN __device__ __forceinline__

/// Pixel i's class: its primitive type when it is a surface pixel (image_lib.h), -1 otherwise.
DN_FN int surface_type(const float4 *hits, const int32_t *prims, uint32_t us_flags, size_t i) {
    const int type = __float_as_int(hits[2 * i + 1].w);
    if (type < 0) return -1;  // (prims is read only where something was hit)
    return is_surface(type, prims[i], us_flags) ? type & 3 : -1;
}

// ---- steps 1 and 2: demodulation, luminance and the 7x7 variance ---------------------------------------------------------------
// A 16 x 16 block classifies and demodulates its 22 x 22 window (the block and a 3-pixel apron) into LDS once; every pixel then sums
// its 49 neighbours from there. Output per surface pixel: the state {x.rgb, var} and the guide {n.xyz, pos}. A guide whose pos is NaN
// marks a pixel that is not a surface pixel (a closest hit's pos is never NaN: it won a comparison).
constexpr int PT = 16, PR = 3, PS = PT + 2 * PR;

__global__ void __launch_bounds__(PT * PT) k_dn_prepare(const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags,
                                                        int w, int h, float4 *state, float4 *guide) {
    __shared__ float s_lum[PS * PS];
    __shared__ int s_surf[PS * PS];
    const int bx = blockIdx.x * PT - PR, by = blockIdx.y * PT - PR;
    for (int k = threadIdx.y * PT + threadIdx.x; k < PS * PS; k += PT * PT) {
        const int gx = bx + k % PS, gy = by + k / PS;
        int type = -1;
        float L = 0.0f;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t i = (size_t)gy * w + gx;
            type = surface_type(hits, prims, us_flags, i);
            if (type >= 0) {
                const float4 c = rgba[i];
                const float3 a = albedo(type);
                L = lum(c.x / a.x, c.y / a.y, c.z / a.z);
            }
        }
        s_lum[k] = L;
        s_surf[k] = type >= 0;
    }
    __syncthreads();
    const int x = blockIdx.x * PT + threadIdx.x, y = blockIdx.y * PT + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const int type = surface_type(hits, prims, us_flags, i);
    if (type < 0) {
        guide[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
        return;
    }
    float cnt = 0.0f, m1 = 0.0f, m2 = 0.0f;
    for (int dy = 0; dy <= 2 * PR; dy++)
        for (int dx = 0; dx <= 2 * PR; dx++) {
            const int k = (threadIdx.y + dy) * PS + threadIdx.x + dx;
            if (!s_surf[k]) continue;  // (a pixel outside the tile is not a surface pixel)
            const float L = s_lum[k];
            cnt += 1.0f;
            m1 += L;
            m2 += L * L;
        }
    const float mean = m1 / cnt;
    const float var = gt_or(m2 / cnt - mean * mean, 0.0f);
    const float4 c = rgba[i];
    const float3 a = albedo(type);
    state[i] = make_float4(c.x / a.x, c.y / a.y, c.z / a.z, var);
    const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
    guide[i] = make_float4(h1.x, h1.y, h1.z, h0.x);
}

// ---- steps 3 and 4: one à-trous level; the last one remodulates ---------------------------------------------------------------
// The row block of image_lib.h: every tap of a wave reads 64 consecutive records (2 x 1 KiB).
template <bool LAST>
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_dn_atrous(const float4 *st_in, const float4 *guide, float4 *st_out, int w, int h, Level lv,
                                                             const float4 *rgba, const float4 *hits, float4 *out) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float4 gp = guide[i];
    if (!(gp.w == gp.w)) {  // not a surface pixel: copied through by the last level, never a tap
        if (LAST) out[i] = rgba[i];
        return;
    }
    const float4 xp = st_in[i];
    atrous_level<LAST>(x, y, i, gp, xp, xp.w, st_in, guide, st_out, w, h, lv, rgba, hits, out);
}

}  // namespace

struct gpuart_denoise : ImageHandle {
    DeviceBuffer scratch;  ///< 48 bytes per pixel: two states and the guide; then (run_host) the staged inputs and output
};

namespace {

/// The checks both entry points make; `align` is what rgba, hits and out must be aligned to.
int check_run(gpuart_denoise *d, const void *rgba, const void *hits, const void *prims, uint32_t w, uint32_t h,
              const gpuart_denoise_params *p, const void *out, size_t align) {
    if (int r = check_handle(LIB, d)) return r;
    if (!rgba || !hits || !prims || !out) return fail(GPUART_HIP_ERR_ARG, "denoise: rgba, hits, prims or out is NULL");
    if (misaligned({rgba, hits, out}, align) || misaligned({prims}, 4))
        return fail(GPUART_HIP_ERR_ARG, "denoise: misaligned pointer (rgba, hits and out need " + std::to_string(align) + " bytes, prims 4)");
    if (int r = check_size(LIB, w, h)) return r;
    return p ? check_params(LIB, *p, GPUART_DENOISE_MAX_ITERATIONS) : 0;
}

/// The filter on device memory, on the handle's stream; the states and the guide take the first 48 bytes per pixel of the scratch.
int launch(gpuart_denoise *d, const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags, int w, int h,
           const gpuart_denoise_params &p, float4 *out) {
    const size_t n = (size_t)w * h;
    if (p.iterations == 0) {
        if (out != rgba) HIP_TRY(hipMemcpyAsync(out, rgba, n * sizeof(float4), hipMemcpyDeviceToDevice, d->stream));
        return 0;
    }
    float4 *st[2] = {(float4 *)d->scratch.mem, (float4 *)d->scratch.mem + n};
    float4 *guide = (float4 *)d->scratch.mem + 2 * n;
    k_dn_prepare<<<dim3((w + PT - 1) / PT, (h + PT - 1) / PT), dim3(PT, PT), 0, d->stream>>>(rgba, hits, prims, us_flags, w, h, st[0], guide);
    HIP_TRY(hipGetLastError());
    const dim3 grid = row_grid(w, h), block = row_block();
    for (uint32_t it = 0; it < p.iterations; it++) {
        const Level lv = make_level(p, it);
        if (it + 1 == p.iterations)
            k_dn_atrous<true><<<grid, block, 0, d->stream>>>(st[it & 1], guide, nullptr, w, h, lv, rgba, hits, out);
        else
            k_dn_atrous<false><<<grid, block, 0, d->stream>>>(st[it & 1], guide, st[(it + 1) & 1], w, h, lv, rgba, hits, out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_denoise_last_error(void) { return g_last_error.c_str(); }

int gpuart_denoise_defaults(gpuart_denoise_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "denoise: params is NULL");
    p->iterations = 5;
    p->lum_k = 4.0f;
    p->normal_pow2 = 5;
    p->depth_sigma = 0.05f;
    return 0;
}

int gpuart_denoise_create(int device, gpuart_denoise **out) { return create_handle(LIB, device, out); }

int gpuart_denoise_destroy(gpuart_denoise *d) {
    if (!d) return 0;
    destroy_handle(d, {d->scratch.mem});
    delete d;
    return 0;
}

int gpuart_denoise_finish(gpuart_denoise *d) { return finish_handle(LIB, d); }

int gpuart_denoise_run(gpuart_denoise *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                       uint32_t w, uint32_t h, const gpuart_denoise_params *p, float *out) {
    int r = check_run(d, rgba, hits, prims, w, h, p, out, 16);
    if (r) return r;
    const gpuart_denoise_params dp = params_or(p, gpuart_denoise_defaults);
    HIP_TRY(hipSetDevice(d->device));
    if ((r = ensure(d->stream, d->scratch, (size_t)w * h * 48))) return r;
    return launch(d, (const float4 *)rgba, (const float4 *)hits, prims, userSphereFlags, (int)w, (int)h, dp, (float4 *)out);
}

int gpuart_denoise_run_host(gpuart_denoise *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims,
                            uint32_t userSphereFlags, uint32_t w, uint32_t h, const gpuart_denoise_params *p, float *out) {
    int r = check_run(d, rgba, hits, prims, w, h, p, out, 4);
    if (r) return r;
    const gpuart_denoise_params dp = params_or(p, gpuart_denoise_defaults);
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)w * h;
    // the filter's 48 bytes per pixel, then the staged inputs; the staged radiance is also the output
    if ((r = ensure(d->stream, d->scratch, n * (48 + STAGED_BYTES)))) return r;
    Staged in;
    if ((r = stage_gbuffer(d->stream, (char *)d->scratch.mem + n * 48, n, rgba, hits, prims, in))) return r;
    if ((r = launch(d, in.rgba, in.hits, in.prims, userSphereFlags, (int)w, (int)h, dp, in.rgba))) return r;
    HIP_TRY(hipMemcpyAsync(out, in.rgba, n * 16, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

}  // extern "C"
