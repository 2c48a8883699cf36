// temporal.hip — libgpuart_temporal.so (gfx950): temporal accumulation by reprojection, include/gpuart_temporal.h, which states the
// algorithm operation by operation. Built like the denoiser — fp32 denormals kept, IEEE '/' and sqrt, no contraction — so that every
// value is the one tests/temporal_ref.py computes in NumPy float32. DESIGN.md "Temporal accumulation" describes the kernel.
#include <cmath>
#include <cstring>

#include "../image/image_lib.h"
#include "gpuart_temporal.h"

namespace {

const char LIB[] = "temporal";

#define TP_FN __host__ __device__ __forceinline__

struct V3 {
    float x, y, z;
};
TP_FN V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
TP_FN float dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
TP_FN V3 cross(V3 a, V3 b) { return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

// The history of one tile: three planes of 16 bytes per pixel, so that a tap is at most three 16-byte requests and the taps of a wave
// (neighbouring lanes, neighbouring history pixels) fall into the same lines.
//   col   {r, g, b, len}
//   guide {n.xyz, class}   class as int bits: -1 not a surface pixel (image_lib.h), else (type & 3) | (user sphere ? 4 : 0)
//   point {p.xyz, 0}
struct History {
    float4 *col, *guide, *point;
};

/// What the kernel needs of the history's view (step 3's per-call values) and of its share.
struct Reproject {
    V3 pos, N, A, B;
    float bN, Wf, Hf;
    int W, H, x0, y0, tw, th, band_rows, band_stride;
    int sphere_same;  ///< the two views' userSphere are bit-equal
    int have;         ///< the handle has a history
};

// The row block of image_lib.h. The pixel's colour, record and ordinal are coalesced 16-byte-per-lane loads; the four taps of
// neighbouring lanes are neighbouring history pixels.

template <bool COMMIT>
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_tp_accumulate(const float4 *rgba, const float4 *hits, const int32_t *prims, uint32_t us_flags,
                                                                 float s, int w, int h, Reproject rp, History old, float max_history,
                                                                 float plane_tol, float normal_min, float4 *out, float *out_len, History next) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const float4 c = rgba[i];
    const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
    const int32_t prim = prims[i];
    const int type = __float_as_int(h1.w);
    int cls = -1;  // is_surface(type, prim, us_flags) of image_lib.h, written out (see there), and the temporal library's own | 4
    if (type >= 0 && !(prim == -2 && (us_flags & (US_EM_NONZERO | US_SPECULAR)))) cls = (type & 3) | (prim == -2 ? 4 : 0);
    const V3 p{h0.y, h0.z, h0.w}, n{h1.x, h1.y, h1.z};
    float4 o = c;
    float len = 0.0f;
    if (cls >= 0) {
        len = s;
        if (rp.have) {
            const V3 d = sub(p, rp.pos);
            const float dn = dot(d, rp.N);
            const float k = rp.bN / dn;
            const float u = dot(d, rp.A) / dn, v = dot(d, rp.B) / dn;
            const float fx = u * rp.Wf - 0.5f, fy = v * rp.Hf - 0.5f;
            const float x0 = floorf(fx), y0 = floorf(fy);
            const float ax = fx - x0, ay = fy - y0;
            const float tol = plane_tol * sqrtf(dot(d, d));
            if (dn != 0.0f && k > 0.0f && x0 >= -1.0f && x0 < rp.Wf && y0 >= -1.0f && y0 < rp.Hf) {
                const int ix = (int)x0, iy = (int)y0;
                float Wsum = 0.0f, hr = 0.0f, hg = 0.0f, hb = 0.0f, hl = 0.0f;
#pragma unroll
                for (int oy = 0; oy < 2; oy++) {
                    const int ty = iy + oy;
                    const float wy = oy ? ay : 1.0f - ay;
#pragma unroll
                    for (int ox = 0; ox < 2; ox++) {
                        const int tx = ix + ox;
                        const float wt = wy * (ox ? ax : 1.0f - ax);
                        if (tx < 0 || tx >= rp.W || ty < 0 || ty >= rp.H) continue;
                        const int lx = tx - rp.x0, ry = ty - rp.y0;
                        if (lx < 0 || lx >= rp.tw || ry < 0) continue;
                        const int r = ry % rp.band_stride;
                        if (r >= rp.band_rows) continue;
                        const int ly = (ry / rp.band_stride) * rp.band_rows + r;
                        if (ly >= rp.th) continue;
                        const size_t q = (size_t)ly * rp.tw + lx;
                        const float4 g = old.guide[q];
                        if (__float_as_int(g.w) != cls) continue;
                        if ((cls & 4) && !rp.sphere_same) continue;
                        if (!(dot(V3{g.x, g.y, g.z}, n) >= normal_min)) continue;
                        const float4 pt = old.point[q];
                        if (!(fabsf(dot(sub(V3{pt.x, pt.y, pt.z}, p), n)) <= tol)) continue;
                        const float4 hc = old.col[q];
                        Wsum += wt;
                        hr += wt * hc.x;
                        hg += wt * hc.y;
                        hb += wt * hc.z;
                        hl += wt * hc.w;
                    }
                }
                if (Wsum > 0.0f) {
                    float nh = hl / Wsum;
                    nh = nh < max_history ? nh : max_history;
                    const float den = nh + s;
                    o.x = (nh * (hr / Wsum) + s * c.x) / den;
                    o.y = (nh * (hg / Wsum) + s * c.y) / den;
                    o.z = (nh * (hb / Wsum) + s * c.z) / den;
                    len = den;
                }
            }
        }
    }
    out[i] = o;
    if (out_len) out_len[i] = len;
    if (COMMIT) {
        next.col[i] = make_float4(o.x, o.y, o.z, len);
        next.guide[i] = make_float4(n.x, n.y, n.z, __int_as_float(cls));
        next.point[i] = make_float4(p.x, p.y, p.z, 0.0f);
    }
}

}  // namespace

struct gpuart_temporal : ImageHandle {
    DeviceBuffer hist[2];  ///< 48 bytes per pixel each: the planes of History
    int cur = 0;        ///< hist[cur] is the history when `have`
    bool have = false;
    gpuart_temporal_view view{};  ///< the history's view
    DeviceBuffer stage;  ///< accumulate_host: the staged inputs (the radiance is also the blend), then the lengths (4 B per pixel)
};

namespace {

History planes(void *mem, size_t n) {
    float4 *b = (float4 *)mem;
    return History{b, b + n, b + 2 * n};
}

int check_params(const gpuart_temporal_params &p) {
    if (!std::isfinite(p.max_history) || !(p.max_history >= 0)) return fail(GPUART_HIP_ERR_ARG, "temporal: max_history must be finite and >= 0");
    if (!std::isfinite(p.plane_tol) || !(p.plane_tol >= 0)) return fail(GPUART_HIP_ERR_ARG, "temporal: plane_tol must be finite and >= 0");
    if (!(p.normal_min >= -1) || !(p.normal_min <= 1)) return fail(GPUART_HIP_ERR_ARG, "temporal: normal_min must lie in -1..1");
    return 0;
}

int check_geom(const gpuart_tile_geom &g, uint32_t w, uint32_t h) {
    bool ok = g.tw == w && g.th == h && g.W >= 1 && g.W <= 65536 && g.H >= 1 && g.H <= 65536 && (uint64_t)g.x0 + g.tw <= g.W &&
              g.band_rows >= 1 && g.band_stride >= g.band_rows;
    if (ok) {
        const uint64_t last = (uint64_t)g.y0 + (uint64_t)((g.th - 1) / g.band_rows) * g.band_stride + (g.th - 1) % g.band_rows;
        ok = last < g.H;
    }
    if (!ok)
        return fail(GPUART_HIP_ERR_ARG, "temporal: geom is not a " + std::to_string(w) + " x " + std::to_string(h) + " share of its frame (frame " +
                                            std::to_string(g.W) + " x " + std::to_string(g.H) + ", share " + std::to_string(g.tw) + " x " +
                                            std::to_string(g.th) + " at " + std::to_string(g.x0) + ", " + std::to_string(g.y0) + ", bands " +
                                            std::to_string(g.band_rows) + " / " + std::to_string(g.band_stride) + ")");
    return 0;
}

/// The checks both entry points make; `align` is what rgba, hits and out_rgba must be aligned to.
int check_call(gpuart_temporal *t, const void *rgba, uint32_t spp, const void *hits, const void *prims, uint32_t w, uint32_t h,
               const gpuart_temporal_view *view, const gpuart_temporal_params *p, const void *out, const void *out_len, size_t align) {
    if (int r = check_handle(LIB, t)) return r;
    if (!rgba || !hits || !prims || !out || !view) return fail(GPUART_HIP_ERR_ARG, "temporal: rgba, hits, prims, view or out_rgba is NULL");
    if (misaligned({rgba, hits, out}, align) || misaligned({prims, out_len}, 4))
        return fail(GPUART_HIP_ERR_ARG, "temporal: misaligned pointer (rgba, hits and out_rgba need " + std::to_string(align) + " bytes, prims and out_len 4)");
    if (int r = check_size(LIB, w, h)) return r;
    if (int r = check_geom(view->geom, w, h)) return r;
    if (spp == 0) return fail(GPUART_HIP_ERR_ARG, "temporal: spp is 0 (the accumulator must hold at least one path)");
    return p ? check_params(*p) : 0;
}

V3 v3(const float a[3]) { return V3{a[0], a[1], a[2]}; }

/// One accumulation on device memory, on the handle's stream; with `commit` the other copy of the history is written and becomes the history.
int launch(gpuart_temporal *t, const float4 *rgba, uint32_t spp, const float4 *hits, const int32_t *prims, int w, int h,
           const gpuart_temporal_view &view, const gpuart_temporal_params &p, bool commit, float4 *out, float *out_len) {
    const size_t n = (size_t)w * h;
    Reproject rp{};
    History old{nullptr, nullptr, nullptr}, next{nullptr, nullptr, nullptr};
    if (t->have) {
        const gpuart_temporal_view &hv = t->view;
        const V3 b = sub(v3(hv.bottomLeft), v3(hv.pos));
        rp.pos = v3(hv.pos);
        rp.N = cross(v3(hv.deltaHorz), v3(hv.deltaVert));
        rp.A = cross(v3(hv.deltaVert), b);
        rp.B = cross(b, v3(hv.deltaHorz));
        rp.bN = dot(b, rp.N);
        rp.W = (int)hv.geom.W; rp.H = (int)hv.geom.H;
        rp.Wf = (float)hv.geom.W; rp.Hf = (float)hv.geom.H;
        rp.x0 = (int)hv.geom.x0; rp.y0 = (int)hv.geom.y0; rp.tw = (int)hv.geom.tw; rp.th = (int)hv.geom.th;
        rp.band_rows = (int)hv.geom.band_rows; rp.band_stride = (int)hv.geom.band_stride;
        rp.sphere_same = memcmp(hv.userSphere, view.userSphere, sizeof view.userSphere) == 0;
        rp.have = 1;
        old = planes(t->hist[t->cur].mem, (size_t)hv.geom.tw * hv.geom.th);
    }
    const int nxt = t->cur ^ (t->have ? 1 : 0);
    if (commit) {
        if (int r = ensure(t->stream, t->hist[nxt], n * 48)) return r;
        next = planes(t->hist[nxt].mem, n);
    }
    const dim3 grid = row_grid(w, h), block = row_block();
    if (commit)
        k_tp_accumulate<true><<<grid, block, 0, t->stream>>>(rgba, hits, prims, view.userSphereFlags, (float)spp, w, h, rp, old, p.max_history,
                                                              p.plane_tol, p.normal_min, out, out_len, next);
    else
        k_tp_accumulate<false><<<grid, block, 0, t->stream>>>(rgba, hits, prims, view.userSphereFlags, (float)spp, w, h, rp, old, p.max_history,
                                                               p.plane_tol, p.normal_min, out, out_len, next);
    HIP_TRY(hipGetLastError());
    if (commit) {
        t->cur = nxt;
        t->have = true;
        t->view = view;
    }
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_temporal_last_error(void) { return g_last_error.c_str(); }

int gpuart_temporal_defaults(gpuart_temporal_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "temporal: params is NULL");
    p->max_history = 4.0f;
    p->plane_tol = 0.01f;
    p->normal_min = 0.8f;
    return 0;
}

int gpuart_temporal_create(int device, gpuart_temporal **out) { return create_handle(LIB, device, out); }

int gpuart_temporal_destroy(gpuart_temporal *t) {
    if (!t) return 0;
    destroy_handle(t, {t->hist[0].mem, t->hist[1].mem, t->stage.mem});
    delete t;
    return 0;
}

int gpuart_temporal_reset(gpuart_temporal *t) {
    if (int r = check_handle(LIB, t)) return r;
    t->have = false;
    return 0;
}

int gpuart_temporal_finish(gpuart_temporal *t) { return finish_handle(LIB, t); }

int gpuart_temporal_accumulate(gpuart_temporal *t, const float *rgba, uint32_t spp, const gpuart_ray_hit *hits, const int32_t *prims,
                               uint32_t w, uint32_t h, const gpuart_temporal_view *view, const gpuart_temporal_params *p, int commit,
                               float *out_rgba, float *out_len) {
    int r = check_call(t, rgba, spp, hits, prims, w, h, view, p, out_rgba, out_len, 16);
    if (r) return r;
    gpuart_temporal_params tp;
    if (p) tp = *p;
    else gpuart_temporal_defaults(&tp);
    HIP_TRY(hipSetDevice(t->device));
    return launch(t, (const float4 *)rgba, spp, (const float4 *)hits, prims, (int)w, (int)h, *view, tp, commit != 0, (float4 *)out_rgba, out_len);
}

int gpuart_temporal_accumulate_host(gpuart_temporal *t, const float *rgba, uint32_t spp, const gpuart_ray_hit *hits, const int32_t *prims,
                                    uint32_t w, uint32_t h, const gpuart_temporal_view *view, const gpuart_temporal_params *p, int commit,
                                    float *out_rgba, float *out_len) {
    int r = check_call(t, rgba, spp, hits, prims, w, h, view, p, out_rgba, out_len, 4);
    if (r) return r;
    gpuart_temporal_params tp;
    if (p) tp = *p;
    else gpuart_temporal_defaults(&tp);
    HIP_TRY(hipSetDevice(t->device));
    const size_t n = (size_t)w * h;
    // the staged inputs (the staged radiance is also the blend), then the lengths (4 bytes per pixel)
    if ((r = ensure(t->stream, t->stage, n * (STAGED_BYTES + 4)))) return r;
    Staged in;
    if ((r = stage_gbuffer(t->stream, t->stage.mem, n, rgba, hits, prims, in))) return r;
    float *d_len = (float *)((char *)t->stage.mem + n * STAGED_BYTES);
    if ((r = launch(t, in.rgba, spp, in.hits, in.prims, (int)w, (int)h, *view, tp, commit != 0, in.rgba, d_len))) return r;
    HIP_TRY(hipMemcpyAsync(out_rgba, in.rgba, n * 16, hipMemcpyDeviceToHost, t->stream));
    if (out_len) HIP_TRY(hipMemcpyAsync(out_len, d_len, n * 4, hipMemcpyDeviceToHost, t->stream));
    HIP_TRY(hipStreamSynchronize(t->stream));
    return 0;
}

}  // extern "C"
