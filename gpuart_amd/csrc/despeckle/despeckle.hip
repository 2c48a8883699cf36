// despeckle.hip — libgpuart_despeckle.so (gfx950): the firefly clamp of include/gpuart_despeckle.h, which states it operation by
// operation. Built without flushing fp32 denormals, with IEEE '/' and no contraction, so that every value is the one
// tests/despeckle_ref.py computes in NumPy float32. DESIGN.md "Firefly clamp" describes the kernel.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/atrous.h"
#include "gpuart_despeckle.h"

namespace {

const char LIB[] = "despeckle";

#define DS_FN __device__ __forceinline__

/// Pixel i's class: its primitive type when it is a surface pixel (image_lib.h), -1 otherwise.
DS_FN int surface_type(const float4 *hits, const int32_t *prims, uint32_t us_flags, size_t i) {
    const int type = __float_as_int(hits[2 * i + 1].w);
    if (type < 0) return -1;  // (prims is read only where something was hit)
    return is_surface(type, prims[i], us_flags) ? type & 3 : -1;
}

/// The counts of a run, in device memory.
struct Counts {
    unsigned long long surface, clamped, too_few;
};

// A 16 x 16 block classifies and demodulates its 20 x 20 window (the block and a 2-pixel apron, whatever the radius) into LDS once,
// as k_dn_prepare does: Lv, NaN for everything that is no valid neighbour (outside the tile, not a surface pixel, a NaN luminance).
// Every thread then keeps the four largest valid neighbours of its window in four registers, by insertion with '>', and takes entry
// rank - 1. `rgba` is never the plane `out` names (the entry points stage an in-place run), so no block reads what another wrote.
// The three counts are ballots per wave, summed over the block's four waves in LDS, and end in at most one atomic per count and block.
constexpr int DT = 16, DR = 2, DS = DT + 2 * DR;

__global__ void __launch_bounds__(DT * DT) k_ds_clamp(const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags, int w, int h,
                                                      int radius, int rank, float k, float floor, int need, float4 *out, float *scale,
                                                      Counts *counts) {
    __shared__ float s_lv[DS * DS];
    __shared__ unsigned s_cnt[DT * DT / 64][3];
    const int tid = threadIdx.y * DT + threadIdx.x;
    const int bx = blockIdx.x * DT - DR, by = blockIdx.y * DT - DR;
    for (int j = tid; j < DS * DS; j += DT * DT) {
        const int gx = bx + j % DS, gy = by + j / DS;
        float lv = __builtin_nanf("");
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t i = (size_t)gy * w + gx;
            const int type = surface_type(hits, prims, us_flags, i);
            if (type >= 0) {
                const float4 c = rgba[i];
                const float3 a = albedo(type);
                lv = lum(c.x / a.x, c.y / a.y, c.z / a.z);
            }
        }
        s_lv[j] = lv;
    }
    __syncthreads();
    const int x = blockIdx.x * DT + threadIdx.x, y = blockIdx.y * DT + threadIdx.y;
    const bool inside = x < w && y < h;
    bool surf = false, clamped = false, few = false;
    if (inside) {
        const size_t i = (size_t)y * w + x;
        const int type = surface_type(hits, prims, us_flags, i);
        const float4 c = rgba[i];
        float4 o = c;
        float s = 1.0f;
        if (type >= 0) {
            surf = true;
            const float ninf = -__builtin_inff();
            float m0 = ninf, m1 = ninf, m2 = ninf, m3 = ninf;
            int cnt = 0;
            for (int dy = -radius; dy <= radius; dy++)
                for (int dx = -radius; dx <= radius; dx++) {
                    if (dx == 0 && dy == 0) continue;
                    const float v = s_lv[(threadIdx.y + DR + dy) * DS + threadIdx.x + DR + dx];
                    if (!(v == v)) continue;  // (a pixel outside the tile is NaN too)
                    cnt++;
                    if (v > m0) {
                        m3 = m2; m2 = m1; m1 = m0; m0 = v;
                    } else if (v > m1) {
                        m3 = m2; m2 = m1; m1 = v;
                    } else if (v > m2) {
                        m3 = m2; m2 = v;
                    } else if (v > m3) {
                        m3 = v;
                    }
                }
            few = cnt < need;
            if (!few) {  // (need >= rank: entry rank - 1 is a neighbour's value)
                const float ref = rank == 1 ? m0 : rank == 2 ? m1 : rank == 3 ? m2 : m3;
                const float cap = k * ref + floor;
                const float3 a = albedo(type);
                const float xr = c.x / a.x, xg = c.y / a.y, xb = c.z / a.z;
                const float L = lum(xr, xg, xb);
                if (L > cap) {
                    clamped = true;
                    s = cap / L;
                    o = make_float4((xr * s) * a.x, (xg * s) * a.y, (xb * s) * a.z, c.w);
                }
            }
        }
        out[i] = o;
        if (scale) scale[i] = s;
    }
    const unsigned long long b0 = __ballot(surf), b1 = __ballot(clamped), b2 = __ballot(few);
    if ((tid & 63) == 0) {
        s_cnt[tid >> 6][0] = (unsigned)__popcll(b0);
        s_cnt[tid >> 6][1] = (unsigned)__popcll(b1);
        s_cnt[tid >> 6][2] = (unsigned)__popcll(b2);
    }
    __syncthreads();
    if (tid < 3) {
        unsigned long long sum = 0;
        for (int v = 0; v < DT * DT / 64; v++) sum += s_cnt[v][tid];
        if (sum) atomicAdd(&counts->surface + tid, sum);
    }
}

}  // namespace

struct gpuart_despeckle : ImageHandle {
    Counts *counts = nullptr;  ///< device
    DeviceBuffer staging;      ///< run in place: the copy of rgba (16 bytes per pixel); run_host: the staged inputs (52), out (16), scale (4)
};

namespace {

int check_params(const gpuart_despeckle_params *p) {
    if (!p) return 0;
    const auto bad = [](const char *what) { return fail(GPUART_HIP_ERR_ARG, std::string("despeckle: ") + what); };
    if (p->radius < 1 || p->radius > 2) return bad("radius must be 1 or 2");
    if (p->rank < 1 || p->rank > 4) return bad("rank must be in 1..4");
    if (!std::isfinite(p->k) || !(p->k >= 1)) return bad("k must be finite and >= 1");
    if (!std::isfinite(p->floor) || !(p->floor >= 0)) return bad("floor must be finite and >= 0");
    if (p->min_count < 1 || p->min_count > 24) return bad("min_count must be in 1..24");
    return 0;
}

/// The checks both run entry points make; `align` is what rgba, hits and out must be aligned to. The handle comes last: every other
/// message can be had without a device.
int check_run(gpuart_despeckle *d, const void *rgba, const void *hits, const void *prims, uint32_t w, uint32_t h, const gpuart_despeckle_params *p,
              const void *out, const void *scale, size_t align) {
    if (int rc = check_params(p)) return rc;
    if (!rgba || !hits || !prims || !out) return fail(GPUART_HIP_ERR_ARG, "despeckle: rgba, hits, prims or out is NULL");
    if (misaligned({rgba, hits, out}, align) || misaligned({prims, scale}, 4))
        return fail(GPUART_HIP_ERR_ARG, "despeckle: misaligned pointer (rgba, hits and out need " + std::to_string(align) + " bytes, prims and scale 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    const size_t n = (size_t)w * h;
    if (out != rgba && overlaps(out, n * 16, rgba, n * 16)) return fail(GPUART_HIP_ERR_ARG, "despeckle: out overlaps rgba without being rgba");
    if (scale && (overlaps(scale, n * 4, rgba, n * 16) || overlaps(scale, n * 4, out, n * 16)))
        return fail(GPUART_HIP_ERR_ARG, "despeckle: scale overlaps rgba or out");
    return check_handle(LIB, d);
}

/// The clamp on device memory, on the handle's stream; rgba is not out. The counts start from zero.
int launch(gpuart_despeckle *d, const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags, int w, int h,
           const gpuart_despeckle_params &p, float4 *out, float *scale) {
    HIP_TRY(hipMemsetAsync(d->counts, 0, sizeof(Counts), d->stream));
    const int need = (int)(p.min_count > p.rank ? p.min_count : p.rank);
    k_ds_clamp<<<dim3((w + DT - 1) / DT, (h + DT - 1) / DT), dim3(DT, DT), 0, d->stream>>>(rgba, hits, prims, us_flags, w, h, (int)p.radius,
                                                                                           (int)p.rank, p.k, p.floor, need, out, scale, d->counts);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_despeckle_last_error(void) { return g_last_error.c_str(); }

int gpuart_despeckle_defaults(gpuart_despeckle_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "despeckle: params is NULL");
    p->radius = 1;
    p->rank = 3;
    p->k = 2.0f;
    p->floor = 1e-3f;
    p->min_count = 4;
    return 0;
}

int gpuart_despeckle_create(int device, gpuart_despeckle **out) {
    if (int rc = create_handle(LIB, device, out)) return rc;
    gpuart_despeckle *d = *out;
    *out = nullptr;
    hipError_t e = hipMalloc((void **)&d->counts, sizeof(Counts));
    if (e == hipSuccess) e = hipMemset(d->counts, 0, sizeof(Counts));
    if (e != hipSuccess) {
        gpuart_despeckle_destroy(d);
        return fail(GPUART_HIP_ERR_DEVICE, std::string("despeckle: allocating the counts: ") + hipGetErrorString(e));
    }
    *out = d;
    return 0;
}

int gpuart_despeckle_destroy(gpuart_despeckle *d) {
    if (!d) return 0;
    destroy_handle(d, {d->staging.mem, d->counts});
    delete d;
    return 0;
}

int gpuart_despeckle_finish(gpuart_despeckle *d) { return finish_handle(LIB, d); }

int gpuart_despeckle_run(gpuart_despeckle *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                         uint32_t w, uint32_t h, const gpuart_despeckle_params *p, float *out, float *scale) {
    if (int rc = check_run(d, rgba, hits, prims, w, h, p, out, scale, 16)) return rc;
    HIP_TRY(hipSetDevice(d->device));
    const float4 *in = (const float4 *)rgba;
    if (out == rgba) {  // in place: clamp from a copy (the header says why)
        const size_t bytes = (size_t)w * h * 16;
        if (int rc = ensure(d->stream, d->staging, bytes)) return rc;
        HIP_TRY(hipMemcpyAsync(d->staging.mem, rgba, bytes, hipMemcpyDeviceToDevice, d->stream));
        in = (const float4 *)d->staging.mem;
    }
    return launch(d, in, (const float4 *)hits, prims, userSphereFlags, (int)w, (int)h, params_or_defaults(p, gpuart_despeckle_defaults), (float4 *)out, scale);
}

int gpuart_despeckle_run_host(gpuart_despeckle *d, const float *rgba, const gpuart_ray_hit *hits, const int32_t *prims,
                              uint32_t userSphereFlags, uint32_t w, uint32_t h, const gpuart_despeckle_params *p, float *out, float *scale) {
    int rc = check_run(d, rgba, hits, prims, w, h, p, out, scale, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(d->device));
    const size_t n = (size_t)w * h;
    if ((rc = ensure(d->stream, d->staging, n * (STAGED_BYTES + 16 + 4)))) return rc;
    Staged in;
    if ((rc = stage_gbuffer(d->stream, d->staging.mem, n, rgba, hits, prims, in))) return rc;
    float4 *dout = (float4 *)((char *)d->staging.mem + n * STAGED_BYTES);
    float *dscale = (float *)((char *)d->staging.mem + n * (STAGED_BYTES + 16));
    if ((rc = launch(d, in.rgba, in.hits, in.prims, userSphereFlags, (int)w, (int)h, params_or_defaults(p, gpuart_despeckle_defaults), dout, scale ? dscale : nullptr))) return rc;
    HIP_TRY(hipMemcpyAsync(out, dout, n * 16, hipMemcpyDeviceToHost, d->stream));
    if (scale) HIP_TRY(hipMemcpyAsync(scale, dscale, n * 4, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int gpuart_despeckle_read_summary(gpuart_despeckle *d, gpuart_despeckle_summary *out) {
    if (int rc = check_handle(LIB, d)) return rc;
    if (!out) return fail(GPUART_HIP_ERR_ARG, "despeckle: out is NULL");
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipStreamSynchronize(d->stream));
    Counts c;
    HIP_TRY(hipMemcpy(&c, d->counts, sizeof c, hipMemcpyDeviceToHost));
    out->surface = c.surface;
    out->clamped = c.clamped;
    out->too_few = c.too_few;
    return 0;
}

}  // extern "C"
