// upscale.hip — libgpuart_upscale.so (gfx950): a filtered frame upsampled under the guidance of a G-buffer of the larger frame, as
// include/gpuart_upscale.h states it operation by operation. Built without flushing fp32 denormals, with IEEE '/' and no contraction,
// so that every value is the one tests/upscale_ref.py computes in NumPy float32. DESIGN.md "The upscaler" describes the kernel.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/atrous.h"
#include "gpuart_upscale.h"

namespace {

const char LIB[] = "upscale";

#define UP_FN __device__ __forceinline__

enum { C_SKY = 0, C_SPHERE = 1, C_SURFACE = 2 };

/// A record as match() reads it.
struct Rec {
    float pos;
    float3 p, n;
    int type, cls;
    bool us;  ///< ordinal -2
};

UP_FN Rec load_rec(const float4 *hits, const int32_t *prims, size_t i, uint32_t us_flags) {
    const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
    Rec r;
    r.pos = h0.x;
    r.p = make_float3(h0.y, h0.z, h0.w);
    r.n = make_float3(h1.x, h1.y, h1.z);
    r.type = __float_as_int(h1.w);
    r.us = false;
    r.cls = C_SKY;
    if (r.type >= 0) {  // (prims is read only where something was hit)
        r.us = prims[i] == -2;
        r.cls = r.us && (us_flags & (US_EM_NONZERO | US_SPECULAR)) ? C_SPHERE : C_SURFACE;
    }
    return r;
}

/// match(a, b) of the header: a record against a centre record.
UP_FN bool match(const Rec &a, const Rec &b, float normal_min, float plane_tol) {
    if (a.cls != b.cls) return false;
    if (a.cls != C_SURFACE) return true;
    if (a.type != b.type || a.us != b.us) return false;
    const float dn = (a.n.x * b.n.x + a.n.y * b.n.y) + a.n.z * b.n.z;
    if (!(dn > normal_min)) return false;
    const float dx = a.p.x - b.p.x, dy = a.p.y - b.p.y, dz = a.p.z - b.p.z;
    const float dist = fabsf((b.n.x * dx + b.n.y * dy) + b.n.z * dz);
    return dist <= plane_tol * gt_or(b.pos, 1e-6f);
}

/// Step 3's second half, for the output pixels none of whose taps counted: the first of the nine candidates around the containing
/// low pixel (cx, cy) that lies on the surface of output record o, or the containing pixel itself. Rare, and kept out of the kernel's
/// straight path: a call that loads the record again, so that nothing of it has to live across the call.
__device__ __noinline__ float4 fallback(const float4 *hi_hits, const int32_t *hi_prims, size_t o, const float4 *filtered, const float4 *hits,
                                        const int32_t *prims, uint32_t us_flags, int w, int h, int cx, int cy, float normal_min,
                                        float plane_tol) {
    const Rec r = load_rec(hi_hits, hi_prims, o, us_flags);
    const int DY[9] = {0, 0, 0, 1, -1, 1, 1, -1, -1}, DX[9] = {0, 1, -1, 0, 0, 1, -1, 1, -1};
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const int qx = cx + DX[k], qy = cy + DY[k];
        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
        const size_t q = (size_t)qy * w + qx;
        if (match(r, load_rec(hits, prims, q, us_flags), normal_min, plane_tol)) return filtered[q];
    }
    return filtered[(size_t)cy * w + cx];
}

// One thread per output pixel on the 64 x 4 row block: a wave is 64 consecutive output pixels of one row, so its record, ordinal and
// result are one request per 16-byte plane, and its taps are 64/scale + 1 neighbouring low pixels of two rows, which the cache serves.
__global__ void __launch_bounds__(ROW_X *ROW_Y) k_up_joint(const float4 *filtered, const float4 *hits, const int32_t *prims, int w, int h,
                                                           const float4 *hi_hits, const int32_t *hi_prims, uint32_t us_flags, int scale,
                                                           float normal_min, float plane_tol, float4 *out) {
    const int X = blockIdx.x * ROW_X + threadIdx.x, Y = blockIdx.y * ROW_Y + threadIdx.y;
    const int W = w * scale, H = h * scale;
    if (X >= W || Y >= H) return;
    const size_t o = (size_t)Y * W + X;
    const Rec r = load_rec(hi_hits, hi_prims, o, us_flags);
    const float s = (float)scale;
    const float fx = ((float)X + 0.5f) / s - 0.5f, fy = ((float)Y + 0.5f) / s - 0.5f;
    const float flx = floorf(fx), fly = floorf(fy);
    const float ax = fx - flx, ay = fy - fly;
    const int x0 = (int)flx, y0 = (int)fly;
    const int cx = X / scale, cy = Y / scale;  // inside the tile: X < w * scale
    float wsum = 0.0f, ar = 0.0f, ag = 0.0f, ab = 0.0f;
#pragma unroll
    for (int oy = 0; oy < 2; oy++) {
        const int ty = y0 + oy;
        const float wy = oy ? ay : 1.0f - ay;
#pragma unroll
        for (int ox = 0; ox < 2; ox++) {
            const int tx = x0 + ox;
            const float wx = ox ? ax : 1.0f - ax;
            const float wt = wy * wx;
            if (tx < 0 || tx >= w || ty < 0 || ty >= h || !(wt > 0.0f)) continue;
            const size_t q = (size_t)ty * w + tx;
            if (!match(r, load_rec(hits, prims, q, us_flags), normal_min, plane_tol)) continue;
            const float4 f = filtered[q];  // (after the verdict: loading all four taps' light up front measured 10 % slower)
            wsum += wt;
            ar += wt * f.x;
            ag += wt * f.y;
            ab += wt * f.z;
        }
    }
    const float alpha = filtered[(size_t)cy * w + cx].w;
    if (wsum > 0.0f) {
        out[o] = make_float4(ar / wsum, ag / wsum, ab / wsum, alpha);
        return;
    }
    const float4 f = fallback(hi_hits, hi_prims, o, filtered, hits, prims, us_flags, w, h, cx, cy, normal_min, plane_tol);
    out[o] = make_float4(f.x, f.y, f.z, alpha);
}

}  // namespace

struct gpuart_upscale : ImageHandle {
    DeviceBuffer staging;  ///< run_host's: the high G-buffer (36 bytes per output pixel), out (16) and the low tile's planes (52 per pixel)
};

namespace {

int check_params(const gpuart_upscale_params *p) {
    if (!p) return 0;
    if (!(p->normal_min >= -1) || !(p->normal_min <= 1)) return fail(GPUART_HIP_ERR_ARG, "upscale: normal_min must be in -1..1");
    if (!std::isfinite(p->plane_tol) || !(p->plane_tol >= 0)) return fail(GPUART_HIP_ERR_ARG, "upscale: plane_tol must be finite and >= 0");
    return 0;
}

/// The checks both run entry points make; `align` is what the float4 planes and the records must be aligned to. The handle comes
/// last: every other message can be had without a device.
int check_run(gpuart_upscale *u, uint32_t scale, const void *filtered, const void *hits, const void *prims, uint32_t w, uint32_t h,
              const void *hi_hits, const void *hi_prims, const gpuart_upscale_params *p, const void *out, size_t align) {
    if (scale < GPUART_UPSCALE_MIN_SCALE || scale > GPUART_UPSCALE_MAX_SCALE)
        return fail(GPUART_HIP_ERR_ARG, "upscale: scale = " + std::to_string(scale) + " is not in 2..4");
    if (int rc = check_params(p)) return rc;
    if (!filtered || !hits || !prims || !hi_hits || !hi_prims || !out)
        return fail(GPUART_HIP_ERR_ARG, "upscale: filtered, hits, prims, hi_hits, hi_prims or out is NULL");
    if (misaligned({filtered, hits, hi_hits, out}, align) || misaligned({prims, hi_prims}, 4))
        return fail(GPUART_HIP_ERR_ARG, "upscale: misaligned pointer (filtered, hits, hi_hits and out need " + std::to_string(align) +
                                            " bytes, prims and hi_prims 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if ((uint64_t)w * scale > 65536 || (uint64_t)h * scale > 65536)
        return fail(GPUART_HIP_ERR_ARG, "upscale: the output of " + std::to_string((uint64_t)w * scale) + " x " + std::to_string((uint64_t)h * scale) +
                                            " pixels has a side above 65536");
    const size_t n = (size_t)w * h, N = n * scale * scale;
    if (overlaps(out, N * 16, filtered, n * 16) || overlaps(out, N * 16, hits, n * 32) || overlaps(out, N * 16, prims, n * 4) ||
        overlaps(out, N * 16, hi_hits, N * 32) || overlaps(out, N * 16, hi_prims, N * 4))
        return fail(GPUART_HIP_ERR_ARG, "upscale: out overlaps an input");
    return check_handle(LIB, u);
}

int launch(gpuart_upscale *u, uint32_t scale, const float4 *filtered, const float4 *hits, const int32_t *prims, uint32_t w, uint32_t h,
           const float4 *hi_hits, const int32_t *hi_prims, uint32_t us_flags, const gpuart_upscale_params &p, float4 *out) {
    k_up_joint<<<row_grid(w * scale, h * scale), row_block(), 0, u->stream>>>(filtered, hits, prims, (int)w, (int)h, hi_hits, hi_prims, us_flags,
                                                                               (int)scale, p.normal_min, p.plane_tol, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_upscale_last_error(void) { return g_last_error.c_str(); }

int gpuart_upscale_defaults(gpuart_upscale_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "upscale: params is NULL");
    p->normal_min = 0.95f;
    p->plane_tol = 0.02f;
    return 0;
}

int gpuart_upscale_create(int device, gpuart_upscale **out) { return create_handle(LIB, device, out); }

int gpuart_upscale_destroy(gpuart_upscale *u) {
    if (!u) return 0;
    destroy_handle(u, {u->staging.mem});
    delete u;
    return 0;
}

int gpuart_upscale_finish(gpuart_upscale *u) { return finish_handle(LIB, u); }

int gpuart_upscale_run(gpuart_upscale *u, uint32_t scale, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t w,
                       uint32_t h, const gpuart_ray_hit *hi_hits, const int32_t *hi_prims, uint32_t userSphereFlags,
                       const gpuart_upscale_params *p, float *out) {
    if (int rc = check_run(u, scale, filtered, hits, prims, w, h, hi_hits, hi_prims, p, out, 16)) return rc;
    HIP_TRY(hipSetDevice(u->device));
    return launch(u, scale, (const float4 *)filtered, (const float4 *)hits, prims, w, h, (const float4 *)hi_hits, hi_prims, userSphereFlags,
                  params_or_defaults(p, gpuart_upscale_defaults), (float4 *)out);
}

int gpuart_upscale_run_host(gpuart_upscale *u, uint32_t scale, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims,
                            uint32_t w, uint32_t h, const gpuart_ray_hit *hi_hits, const int32_t *hi_prims, uint32_t userSphereFlags,
                            const gpuart_upscale_params *p, float *out) {
    int rc = check_run(u, scale, filtered, hits, prims, w, h, hi_hits, hi_prims, p, out, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(u->device));
    const size_t n = (size_t)w * h, N = n * scale * scale;
    if ((rc = ensure(u->stream, u->staging, (n + N) * STAGED_BYTES))) return rc;
    // the 16-byte planes first, so that each is aligned: the high records, out, the low tile's planes, and the high ordinals last
    char *base = (char *)u->staging.mem;
    float4 *d_hi_hits = (float4 *)base, *d_out = (float4 *)(base + N * 32);
    Staged lo;
    if ((rc = stage_gbuffer(u->stream, base + N * 48, n, filtered, hits, prims, lo))) return rc;
    int32_t *d_hi_prims = (int32_t *)(base + N * 48 + n * STAGED_BYTES);
    HIP_TRY(hipMemcpyAsync(d_hi_hits, hi_hits, N * 32, hipMemcpyHostToDevice, u->stream));
    HIP_TRY(hipMemcpyAsync(d_hi_prims, hi_prims, N * 4, hipMemcpyHostToDevice, u->stream));
    if ((rc = launch(u, scale, lo.rgba, lo.hits, lo.prims, w, h, d_hi_hits, d_hi_prims, userSphereFlags, params_or_defaults(p, gpuart_upscale_defaults),
                     d_out)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, N * 16, hipMemcpyDeviceToHost, u->stream));
    HIP_TRY(hipStreamSynchronize(u->stream));
    return 0;
}

}  // extern "C"
