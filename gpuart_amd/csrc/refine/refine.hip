// refine.hip — libgpuart_refine.so (gfx950): the variance-guided filter of include/gpuart_refine.h, which states it operation by
// operation. Built without flushing fp32 denormals, with IEEE '/' and sqrt and no contraction, so that every value is the one
// tests/refine_ref.py computes in NumPy float32. DESIGN.md "Variance-guided filter" describes the kernels.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/atrous.h"
#include "gpuart_refine.h"

namespace {

const char LIB[] = "refine";

#define RF_FN __device__ __forceinline__

/// neither NaN nor +-inf, whatever the sign: the exponent is not all ones
RF_FN bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// ---- steps 0 and 1: validity, demodulation and the variance from the error map ----------------------------------------------------
// Pure streaming on the row block of image_lib.h: 56 bytes in (radiance, record, ordinal, e) and 32 out per pixel, the state
// {x.rgb, var} and the guide {n.xyz, pos}. A guide whose pos is NaN marks a pixel that is not valid (a closest hit's pos is never NaN:
// it won a comparison); its state is not written.
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_rf_prepare(const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags,
                                                              const float *error, float lum_floor, int w, int h, float4 *state, float4 *guide) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
    const int type = __float_as_int(h1.w);
    const float e = error[i];
    // (prims is read only where something was hit)
    if (type < 0 || !is_surface(type, prims[i], us_flags) || !finite_bits(e)) {
        guide[i] = make_float4(0.0f, 0.0f, 0.0f, __builtin_nanf(""));
        return;
    }
    const float4 c = rgba[i];
    const float3 a = albedo(type & 3);
    const float xr = c.x / a.x, xg = c.y / a.y, xb = c.z / a.z;
    const float sg = e * gt_or(lum(xr, xg, xb), lum_floor);
    state[i] = make_float4(xr, xg, xb, sg * sg);
    guide[i] = make_float4(h1.x, h1.y, h1.z, h0.x);
}

// ---- step 2: one level; the last one remodulates (step 3) --------------------------------------------------------------------------
// The row block of image_lib.h: every tap of a wave reads 64 consecutive records (2 x 1 KiB). The nine values of the variance
// prefilter come from an LDS tile of the block's variances and a one-pixel apron, 66 x 6, filled once per block: the block's own
// pixels from the registers that hold their state anyway, the 140 apron pixels by the first 140 threads (4 bytes of the guide and 4 of
// the state each).
constexpr int VT_X = ROW_X + 2, VT_Y = ROW_Y + 2, APRON = 2 * VT_X + 2 * ROW_Y;

template <bool LAST>
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_rf_level(const float4 *st_in, const float4 *guide, float4 *st_out, int w, int h, Level lv,
                                                            const float4 *rgba, const float4 *hits, float4 *out) {
    __shared__ float s_var[VT_X * VT_Y];
    __shared__ int s_valid[VT_X * VT_Y];
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    const bool inside = x < w && y < h;
    const size_t i = (size_t)y * w + x;
    float4 gp = make_float4(0.0f, 0.0f, 0.0f, 0.0f), xp = gp;
    bool valid = false;
    if (inside) {
        gp = guide[i];
        valid = gp.w == gp.w;
        if (valid) xp = st_in[i];
    }
    const int own = (threadIdx.y + 1) * VT_X + threadIdx.x + 1;
    s_var[own] = xp.w;
    s_valid[own] = valid;
    const int k = threadIdx.y * ROW_X + threadIdx.x;
    if (k < APRON) {
        int row, col;
        if (k < VT_X) { row = 0; col = k; }
        else if (k < 2 * VT_X) { row = VT_Y - 1; col = k - VT_X; }
        else { row = 1 + (k - 2 * VT_X) / 2; col = (k & 1) ? VT_X - 1 : 0; }  // (2 * VT_X is even: k's parity is the side)
        const int qx = (int)(blockIdx.x * ROW_X) - 1 + col, qy = (int)(blockIdx.y * ROW_Y) - 1 + row;
        float v = 0.0f;
        bool ok = false;
        if (qx >= 0 && qx < w && qy >= 0 && qy < h) {
            const size_t q = (size_t)qy * w + qx;
            const float pq = guide[q].w;
            ok = pq == pq;
            if (ok) v = st_in[q].w;
        }
        s_var[row * VT_X + col] = v;
        s_valid[row * VT_X + col] = ok;
    }
    __syncthreads();
    if (!inside) return;
    if (!valid) {  // copied through by the last level, never a tap
        if (LAST) out[i] = rgba[i];
        return;
    }
    // a. the 3x3 variance prefilter
    const float G[3] = {0.25f, 0.5f, 0.25f};
    float gn = 0.0f, gd = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int t = own + dy * VT_X + dx;
            if (!s_valid[t]) continue;  // (a pixel outside the tile is not valid)
            const float g = G[dy + 1] * G[dx + 1];
            gn += g * s_var[t];
            gd += g;
        }
    const float gv = gn / gd;
    // b. the taps, c. the update
    atrous_level<LAST>(x, y, i, gp, xp, gv, st_in, guide, st_out, w, h, lv, rgba, hits, out);
}

}  // namespace

struct gpuart_refine : ImageHandle {
    DeviceBuffer scratch;  ///< 48 bytes per pixel: two states and the guide; then (run_host) the staged inputs, the error map and the output
};

namespace {

/// The checks both entry points make; `align` is what rgba, hits and out must be aligned to.
int check_run(gpuart_refine *r, const void *rgba, const void *hits, const void *prims, const void *error, float lum_floor, uint32_t w,
              uint32_t h, const gpuart_refine_params *p, const void *out, size_t align) {
    if (int rc = check_handle(LIB, r)) return rc;
    if (!rgba || !hits || !prims || !error || !out) return fail(GPUART_HIP_ERR_ARG, "refine: rgba, hits, prims, error or out is NULL");
    if (misaligned({rgba, hits, out}, align) || misaligned({prims, error}, 4))
        return fail(GPUART_HIP_ERR_ARG, "refine: misaligned pointer (rgba, hits and out need " + std::to_string(align) + " bytes, prims and error 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (!std::isfinite(lum_floor) || !(lum_floor > 0)) return fail(GPUART_HIP_ERR_ARG, "refine: lum_floor must be finite and > 0");
    return p ? check_params(LIB, *p, GPUART_REFINE_MAX_ITERATIONS) : 0;
}

/// The filter on device memory, on the handle's stream; the states and the guide take the first 48 bytes per pixel of the scratch.
int launch(gpuart_refine *r, const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags, const float *error,
           float lum_floor, int w, int h, const gpuart_refine_params &p, float4 *out) {
    const size_t n = (size_t)w * h;
    if (p.iterations == 0) {
        if (out != rgba) HIP_TRY(hipMemcpyAsync(out, rgba, n * sizeof(float4), hipMemcpyDeviceToDevice, r->stream));
        return 0;
    }
    float4 *st[2] = {(float4 *)r->scratch.mem, (float4 *)r->scratch.mem + n};
    float4 *guide = (float4 *)r->scratch.mem + 2 * n;
    const dim3 grid = row_grid(w, h), block = row_block();
    k_rf_prepare<<<grid, block, 0, r->stream>>>(rgba, hits, prims, us_flags, error, lum_floor, w, h, st[0], guide);
    HIP_TRY(hipGetLastError());
    for (uint32_t it = 0; it < p.iterations; it++) {
        const Level lv = make_level(p, it);
        if (it + 1 == p.iterations)
            k_rf_level<true><<<grid, block, 0, r->stream>>>(st[it & 1], guide, nullptr, w, h, lv, rgba, hits, out);
        else
            k_rf_level<false><<<grid, block, 0, r->stream>>>(st[it & 1], guide, st[(it + 1) & 1], w, h, lv, rgba, hits, out);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_refine_last_error(void) { return g_last_error.c_str(); }

int gpuart_refine_defaults(gpuart_refine_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "refine: params is NULL");
    p->iterations = 5;
    p->lum_k = 1.0f;
    p->normal_pow2 = 5;
    p->depth_sigma = 0.05f;
    return 0;
}

int gpuart_refine_create(int device, gpuart_refine **out) { return create_handle(LIB, device, out); }

int gpuart_refine_destroy(gpuart_refine *r) {
    if (!r) return 0;
    destroy_handle(r, {r->scratch.mem});
    delete r;
    return 0;
}

int gpuart_refine_finish(gpuart_refine *r) { return finish_handle(LIB, r); }

int gpuart_refine_run(gpuart_refine *r, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                      const float *error, float lum_floor, uint32_t w, uint32_t h, const gpuart_refine_params *p, float *out) {
    int rc = check_run(r, rgba, hits, prims, error, lum_floor, w, h, p, out, 16);
    if (rc) return rc;
    const gpuart_refine_params rp = params_or(p, gpuart_refine_defaults);
    HIP_TRY(hipSetDevice(r->device));
    if ((rc = ensure(r->stream, r->scratch, (size_t)w * h * 48))) return rc;
    return launch(r, (const float4 *)rgba, (const float4 *)hits, prims, userSphereFlags, error, lum_floor, (int)w, (int)h, rp, (float4 *)out);
}

int gpuart_refine_run_host(gpuart_refine *r, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                           const float *error, float lum_floor, uint32_t w, uint32_t h, const gpuart_refine_params *p, float *out) {
    int rc = check_run(r, rgba, hits, prims, error, lum_floor, w, h, p, out, 4);
    if (rc) return rc;
    const gpuart_refine_params rp = params_or(p, gpuart_refine_defaults);
    HIP_TRY(hipSetDevice(r->device));
    const size_t n = (size_t)w * h;
    // the filter's 48 bytes per pixel, then the staged inputs and the error map; the staged radiance is also the output
    if ((rc = ensure(r->stream, r->scratch, n * (48 + STAGED_BYTES + 4)))) return rc;
    Staged in;
    if ((rc = stage_gbuffer(r->stream, (char *)r->scratch.mem + n * 48, n, rgba, hits, prims, in))) return rc;
    float *err = (float *)((char *)r->scratch.mem + n * (48 + STAGED_BYTES));
    HIP_TRY(hipMemcpyAsync(err, error, n * 4, hipMemcpyHostToDevice, r->stream));
    if ((rc = launch(r, in.rgba, in.hits, in.prims, userSphereFlags, err, lum_floor, (int)w, (int)h, rp, in.rgba))) return rc;
    HIP_TRY(hipMemcpyAsync(out, in.rgba, n * 16, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return 0;
}

}  // extern "C"
