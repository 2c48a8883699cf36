// moments.hip — libgpuart_moments.so (gfx950): the error map of a temporal history's measured luminance variance, as
// include/gpuart_moments.h states it operation by operation. Built without flushing fp32 denormals, with IEEE '/' and sqrt and no
// contraction, so that every value is the one tests/moments_ref.py computes in NumPy float32. DESIGN.md "History variance" describes
// the kernels.
#include <cmath>

#include "../image/image_lib.h"
#include "gpuart_moments.h"

namespace {

const char LIB[] = "moments";

#define MO_FN __device__ __forceinline__

MO_FN float gt_or(float a, float b) { return a > b ? a : b; }

// ---- pack: {L, L*L, 1/s, a} ---------------------------------------------------------------------------------------------------------
// Pure streaming on the row block of image_lib.h: 16 bytes in and 16 out per pixel. inv_s is 1.0f/(float)spp, an IEEE division
// wherever it is made: the host makes it once.
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_mo_pack(const float4 *rgba, float inv_s, int w, int h, float4 *out) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float4 c = rgba[i];
    const float l = lum(c.x, c.y, c.z);
    out[i] = make_float4(l, l * l, inv_s, c.w);
}

// ---- error ----------------------------------------------------------------------------------------------------------------------
// The row block of image_lib.h. Every pixel first takes the measured branch from its own 16 bytes of moments, its length and the
// second half of its record (the type; the ordinal where something was hit). Only a pixel whose history is too short needs the 7x7
// window, and in a steady preview those are the disoccluded strips: the block votes, and only a block with such a pixel classifies
// its 70 x 10 window (the block and a 3-pixel apron) and stages its luminance and surface flag through LDS, as k_dn_prepare does for
// its 22 x 22 window. 700 entries, three rounds of the 256 threads; rows of 70 floats, read by a wave at consecutive addresses.
constexpr int WR = 3, WT_X = ROW_X + 2 * WR, WT_Y = ROW_Y + 2 * WR;

__global__ void __launch_bounds__(ROW_X * ROW_Y) k_mo_error(const float4 *rgba, const float *len, const float4 *mom, const float4 *hits,
                                                            const int32_t *prims, uint32_t us_flags, float lum_floor, float min_batches,
                                                            float spatial_k, int w, int h, float *e) {
    __shared__ float s_lum[WT_X * WT_Y];
    __shared__ int s_surf[WT_X * WT_Y];
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    const bool inside = x < w && y < h;
    const size_t i = (size_t)y * w + x;
    float out = 0.0f;
    bool fallback = false;
    if (inside) {
        const int type = __float_as_int(hits[2 * i + 1].w);
        // (prims is read only where something was hit)
        if (type >= 0 && is_surface(type, prims[i], us_flags)) {
            const float4 m = mom[i];
            const float B = len[i] * m.z;
            if (B >= min_batches) {
                float v = m.y - m.x * m.x;
                v = v < 0.0f ? 0.0f : v;  // (keeps a NaN)
                out = sqrtf(v / (B - 1.0f)) / gt_or(m.x, lum_floor);
            } else {
                fallback = true;
            }
        }
    }
    if (__syncthreads_or(fallback)) {  // (every thread of the block is here: none has returned)
        const int bx = blockIdx.x * ROW_X - WR, by = blockIdx.y * ROW_Y - WR;
        for (int k = threadIdx.y * ROW_X + threadIdx.x; k < WT_X * WT_Y; k += ROW_X * ROW_Y) {
            const int gx = bx + k % WT_X, gy = by + k / WT_X;
            bool surf = false;
            float L = 0.0f;
            if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
                const size_t q = (size_t)gy * w + gx;
                const int type = __float_as_int(hits[2 * q + 1].w);
                surf = type >= 0 && is_surface(type, prims[q], us_flags);
                if (surf) {
                    const float4 c = rgba[q];
                    L = lum(c.x, c.y, c.z);
                }
            }
            s_lum[k] = L;
            s_surf[k] = surf;
        }
        __syncthreads();
        if (fallback) {
            float cnt = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = 0; dy <= 2 * WR; dy++)
                for (int dx = 0; dx <= 2 * WR; dx++) {
                    const int k = (threadIdx.y + dy) * WT_X + threadIdx.x + dx;
                    if (!s_surf[k]) continue;  // (a pixel outside the tile is not a surface pixel)
                    const float L = s_lum[k];
                    cnt += 1.0f;
                    s1 += L;
                    s2 += L * L;
                }
            const float mean = s1 / cnt;
            const float var = gt_or(s2 / cnt - mean * mean, 0.0f);
            out = (spatial_k * sqrtf(var)) / gt_or(s_lum[(threadIdx.y + WR) * WT_X + threadIdx.x + WR], lum_floor);
        }
    }
    if (inside) e[i] = out;
}

}  // namespace

struct gpuart_moments : ImageHandle {
    DeviceBuffer staging;  ///< the host entry points': pack_host 16 bytes per pixel; error_host the staged radiance and G-buffer, moments, len and e
};

namespace {

int check_pack(gpuart_moments *m, const void *rgba, uint32_t spp, uint32_t w, uint32_t h, const void *out, size_t align) {
    if (int rc = check_handle(LIB, m)) return rc;
    if (!rgba || !out) return fail(GPUART_HIP_ERR_ARG, "moments: rgba or out is NULL");
    if (misaligned({rgba, out}, align)) return fail(GPUART_HIP_ERR_ARG, "moments: misaligned pointer (rgba and out need " + std::to_string(align) + " bytes)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (spp == 0) return fail(GPUART_HIP_ERR_ARG, "moments: spp is 0");
    const size_t bytes = (size_t)w * h * 16;
    if (out != rgba && overlaps(out, bytes, rgba, bytes)) return fail(GPUART_HIP_ERR_ARG, "moments: out overlaps rgba without being rgba");
    return 0;
}

/// The checks both error entry points make; `align` is what rgba, moments and hits must be aligned to.
int check_error(gpuart_moments *m, const void *rgba, const void *len, const void *mom, const void *hits, const void *prims, float lum_floor,
                uint32_t w, uint32_t h, const gpuart_moments_params *p, const void *e, size_t align) {
    if (int rc = check_handle(LIB, m)) return rc;
    if (!rgba || !len || !mom || !hits || !prims || !e) return fail(GPUART_HIP_ERR_ARG, "moments: rgba, len, moments, hits, prims or e is NULL");
    if (misaligned({rgba, mom, hits}, align) || misaligned({len, prims, e}, 4))
        return fail(GPUART_HIP_ERR_ARG, "moments: misaligned pointer (rgba, moments and hits need " + std::to_string(align) + " bytes, len, prims and e 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (!std::isfinite(lum_floor) || !(lum_floor > 0)) return fail(GPUART_HIP_ERR_ARG, "moments: lum_floor must be finite and > 0");
    if (p) {
        if (!std::isfinite(p->min_batches) || !(p->min_batches > 1)) return fail(GPUART_HIP_ERR_ARG, "moments: min_batches must be finite and > 1");
        if (!std::isfinite(p->spatial_k) || !(p->spatial_k >= 0)) return fail(GPUART_HIP_ERR_ARG, "moments: spatial_k must be finite and >= 0");
    }
    const size_t n = (size_t)w * h;
    if (overlaps(e, n * 4, rgba, n * 16) || overlaps(e, n * 4, len, n * 4) || overlaps(e, n * 4, mom, n * 16) || overlaps(e, n * 4, hits, n * 32) ||
        overlaps(e, n * 4, prims, n * 4))
        return fail(GPUART_HIP_ERR_ARG, "moments: e overlaps an input");
    return 0;
}

int launch_pack(gpuart_moments *m, const float4 *rgba, uint32_t spp, int w, int h, float4 *out) {
    k_mo_pack<<<row_grid(w, h), row_block(), 0, m->stream>>>(rgba, 1.0f / (float)spp, w, h, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_error(gpuart_moments *m, const float4 *rgba, const float *len, const float4 *mom, const float4 *hits, const int32_t *prims,
                 uint32_t us_flags, float lum_floor, int w, int h, const gpuart_moments_params &p, float *e) {
    k_mo_error<<<row_grid(w, h), row_block(), 0, m->stream>>>(rgba, len, mom, hits, prims, us_flags, lum_floor, p.min_batches, p.spatial_k, w, h, e);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_moments_last_error(void) { return g_last_error.c_str(); }

int gpuart_moments_defaults(gpuart_moments_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "moments: params is NULL");
    p->min_batches = 8.0f;
    p->spatial_k = 4.0f;
    return 0;
}

int gpuart_moments_create(int device, gpuart_moments **out) { return create_handle(LIB, device, out); }

int gpuart_moments_destroy(gpuart_moments *m) {
    if (!m) return 0;
    destroy_handle(m, {m->staging.mem});
    delete m;
    return 0;
}

int gpuart_moments_finish(gpuart_moments *m) { return finish_handle(LIB, m); }

int gpuart_moments_pack(gpuart_moments *m, const float *rgba, uint32_t spp, uint32_t w, uint32_t h, float *out) {
    if (int rc = check_pack(m, rgba, spp, w, h, out, 16)) return rc;
    HIP_TRY(hipSetDevice(m->device));
    return launch_pack(m, (const float4 *)rgba, spp, (int)w, (int)h, (float4 *)out);
}

int gpuart_moments_pack_host(gpuart_moments *m, const float *rgba, uint32_t spp, uint32_t w, uint32_t h, float *out) {
    int rc = check_pack(m, rgba, spp, w, h, out, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const size_t n = (size_t)w * h;
    if ((rc = ensure(m->stream, m->staging, n * 16))) return rc;
    float4 *img = (float4 *)m->staging.mem;  // packed in place
    HIP_TRY(hipMemcpyAsync(img, rgba, n * 16, hipMemcpyHostToDevice, m->stream));
    if ((rc = launch_pack(m, img, spp, (int)w, (int)h, img))) return rc;
    HIP_TRY(hipMemcpyAsync(out, img, n * 16, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return 0;
}

int gpuart_moments_error(gpuart_moments *m, const float *rgba, const float *len, const float *moments, const gpuart_ray_hit *hits,
                         const int32_t *prims, uint32_t userSphereFlags, float lum_floor, uint32_t w, uint32_t h,
                         const gpuart_moments_params *p, float *e) {
    if (int rc = check_error(m, rgba, len, moments, hits, prims, lum_floor, w, h, p, e, 16)) return rc;
    HIP_TRY(hipSetDevice(m->device));
    return launch_error(m, (const float4 *)rgba, len, (const float4 *)moments, (const float4 *)hits, prims, userSphereFlags, lum_floor, (int)w,
                        (int)h, params_or_defaults(p, gpuart_moments_defaults), e);
}

int gpuart_moments_error_host(gpuart_moments *m, const float *rgba, const float *len, const float *moments, const gpuart_ray_hit *hits,
                              const int32_t *prims, uint32_t userSphereFlags, float lum_floor, uint32_t w, uint32_t h,
                              const gpuart_moments_params *p, float *e) {
    int rc = check_error(m, rgba, len, moments, hits, prims, lum_floor, w, h, p, e, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(m->device));
    const size_t n = (size_t)w * h;
    // the moments (16 bytes per pixel), the staged radiance and G-buffer, then len and e (4 each): the 16-byte planes come first
    if ((rc = ensure(m->stream, m->staging, n * (16 + STAGED_BYTES + 4 + 4)))) return rc;
    float4 *mom = (float4 *)m->staging.mem;
    Staged in;
    if ((rc = stage_gbuffer(m->stream, (char *)m->staging.mem + n * 16, n, rgba, hits, prims, in))) return rc;
    float *ln = (float *)((char *)m->staging.mem + n * (16 + STAGED_BYTES));
    float *err = ln + n;
    HIP_TRY(hipMemcpyAsync(mom, moments, n * 16, hipMemcpyHostToDevice, m->stream));
    HIP_TRY(hipMemcpyAsync(ln, len, n * 4, hipMemcpyHostToDevice, m->stream));
    if ((rc = launch_error(m, in.rgba, ln, mom, in.hits, in.prims, userSphereFlags, lum_floor, (int)w, (int)h, params_or_defaults(p, gpuart_moments_defaults), err))) return rc;
    HIP_TRY(hipMemcpyAsync(e, err, n * 4, hipMemcpyDeviceToHost, m->stream));
    HIP_TRY(hipStreamSynchronize(m->stream));
    return 0;
}

}  // extern "C"
