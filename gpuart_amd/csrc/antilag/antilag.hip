// antilag.hip — libgpuart_antilag.so (gfx950): the mix of a slow and a fast temporal history where they disagree by more than the
// measured variance explains, as include/gpuart_antilag.h states it operation by operation. Built without flushing fp32 denormals,
// with IEEE '/' and sqrt and no contraction, so that every value is the one tests/antilag_ref.py computes in NumPy float32. DESIGN.md
// "History anti-lag" describes the kernel.
#include <cmath>

#include "../image/image_lib.h"
#include "gpuart_antilag.h"

namespace {

const char LIB[] = "antilag";

#define AL_FN __device__ __forceinline__

struct AlParams {
    float min_batches, min_votes, clip, z_lo, z_hi;
};

// ---- the statistic of one pixel -------------------------------------------------------------------------------------------------
// Step 1 of the header from the pixel's record, ordinal, moments and the two len: does it vote? The two radiances are loaded only
// for a pixel that does (`r_var`).
AL_FN bool votes(const float4 &m, float sl, float fl, float min_batches, float &B) {
    B = sl * m.z;
    return B >= min_batches && fl < sl;
}

AL_FN void r_var(const float4 &m, float B, float fl, const float4 &s, const float4 &f, float clip, float &r, float &var) {
    float v = m.y - m.x * m.x;
    v = v < 0.0f ? 0.0f : v;
    const float sv = (v * B) / (B - 1.0f);
    const float Bf = fl * m.z;
    var = sv * (1.0f / Bf - 1.0f / B);
    r = lum(f.x, f.y, f.z) - lum(s.x, s.y, s.z);
    if (var > 0.0f) {
        const float lim = clip * sqrtf(var);
        r = r > lim ? lim : (r < -lim ? -lim : r);
    }
}

// ---- mix ------------------------------------------------------------------------------------------------------------------------
// The row block of image_lib.h. Every thread first makes the statistic of its own pixel from 16-byte loads (the record's second half,
// the moments, the two radiances) and 4-byte loads (the ordinal, the two len) and keeps what its output needs in registers; the
// block's 3-pixel apron, 444 of the 70 x 10 window's 700 entries, is staged by the 256 threads in two rounds. LDS holds {clipped r,
// var} and the voting mark: rows of 70 words, read by a wave at consecutive addresses. A block whose window holds no voter (the first
// views of a track, a disoccluded strip, a static len) writes `slow` through without the sums; otherwise every surface pixel sums its
// 49 entries in the header's order. An in-place call reads `slow` and `slow_len` from the handle's copy: the apron reaches into
// pixels other blocks write.
constexpr int WR = 3, WT_X = ROW_X + 2 * WR, WT_Y = ROW_Y + 2 * WR;
constexpr int APRON = WT_X * WT_Y - ROW_X * ROW_Y;  // the top and bottom WR rows, then WR columns on either side of the ROW_Y rows between

__global__ void __launch_bounds__(ROW_X * ROW_Y) k_al_mix(const float4 *slow, const float *slow_len, const float4 *fast, const float *fast_len,
                                                          const float4 *mom, const float4 *hits, const int32_t *prims, uint32_t us_flags,
                                                          AlParams P, int w, int h, float4 *out, float *out_len, float *alpha) {
    __shared__ float s_r[WT_X * WT_Y];
    __shared__ float s_var[WT_X * WT_Y];
    __shared__ int s_vote[WT_X * WT_Y];
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    const bool inside = x < w && y < h;
    const size_t i = (size_t)y * w + x;
    float4 s = make_float4(0, 0, 0, 0), f = s;
    float sl = 0.0f, fl = 0.0f;
    bool surf = false, any = false;
    {
        bool vote = false;
        float r = 0.0f, var = 0.0f;
        if (inside) {
            s = slow[i];
            sl = slow_len[i];
            const int type = __float_as_int(hits[2 * i + 1].w);
            // (prims is read only where something was hit)
            if (type >= 0 && is_surface(type, prims[i], us_flags)) {
                surf = true;
                f = fast[i];
                fl = fast_len[i];
                const float4 m = mom[i];
                float B;
                if ((vote = votes(m, sl, fl, P.min_batches, B))) r_var(m, B, fl, s, f, P.clip, r, var);
            }
        }
        const int k = (threadIdx.y + WR) * WT_X + threadIdx.x + WR;
        s_r[k] = r;
        s_var[k] = var;
        s_vote[k] = vote;
        any = vote;
    }
    const int bx = blockIdx.x * ROW_X - WR, by = blockIdx.y * ROW_Y - WR;
    for (int a = threadIdx.y * ROW_X + threadIdx.x; a < APRON; a += ROW_X * ROW_Y) {
        int row, col;
        if (a < 2 * WR * WT_X) {
            row = a / WT_X;
            col = a - row * WT_X;
            if (row >= WR) row += ROW_Y;
        } else {
            const int b = a - 2 * WR * WT_X;
            row = WR + b / (2 * WR);
            col = b % (2 * WR);
            if (col >= WR) col += ROW_X;
        }
        const int gx = bx + col, gy = by + row;
        bool vote = false;
        float r = 0.0f, var = 0.0f;
        if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
            const size_t q = (size_t)gy * w + gx;
            const int type = __float_as_int(hits[2 * q + 1].w);
            if (type >= 0 && is_surface(type, prims[q], us_flags)) {
                const float4 m = mom[q];
                const float ql = slow_len[q], qf = fast_len[q];
                float B;
                if ((vote = votes(m, ql, qf, P.min_batches, B))) r_var(m, B, qf, slow[q], fast[q], P.clip, r, var);
            }
        }
        const int k = row * WT_X + col;
        s_r[k] = r;
        s_var[k] = var;
        s_vote[k] = vote;
        any = any || vote;
    }
    float al = 0.0f;
    if (__syncthreads_or(any)) {  // (every thread of the block is here: none has returned; the barrier also completes the staging)
        if (surf) {
            float cnt = 0.0f, s1 = 0.0f, s2 = 0.0f;
            for (int dy = 0; dy <= 2 * WR; dy++)
                for (int dx = 0; dx <= 2 * WR; dx++) {
                    const int k = (threadIdx.y + dy) * WT_X + threadIdx.x + dx;
                    if (!s_vote[k]) continue;  // (a pixel outside the tile does not vote)
                    cnt += 1.0f;
                    s1 += s_r[k];
                    s2 += s_var[k];
                }
            float Z = 0.0f;
            if (!(cnt < P.min_votes)) {
                if (s2 > 0.0f) Z = fabsf(s1) / sqrtf(s2);
                else Z = s1 == 0.0f ? 0.0f : INFINITY;
            }
            const float t = (Z - P.z_lo) / (P.z_hi - P.z_lo);
            al = t > 0.0f ? t : 0.0f;
            al = al > 1.0f ? 1.0f : al;
        }
    }
    if (!inside) return;
    float4 o = s;
    float ol = sl;
    if (al > 0.0f) {
        o.x = s.x + al * (f.x - s.x);
        o.y = s.y + al * (f.y - s.y);
        o.z = s.z + al * (f.z - s.z);
        ol = sl + al * (fl - sl);
    }
    out[i] = o;
    out_len[i] = ol;
    if (alpha) alpha[i] = al;
}

}  // namespace

struct gpuart_antilag : ImageHandle {
    DeviceBuffer copy;     ///< an in-place call's slow (16 bytes per pixel) and slow_len (4)
    DeviceBuffer staging;  ///< mix_host's planes
};

namespace {

int check_params(const gpuart_antilag_params *p) {
    if (!p) return 0;
    if (!std::isfinite(p->fast_history) || !(p->fast_history >= 0)) return fail(GPUART_HIP_ERR_ARG, "antilag: fast_history must be finite and >= 0");
    if (!std::isfinite(p->min_batches) || !(p->min_batches > 1)) return fail(GPUART_HIP_ERR_ARG, "antilag: min_batches must be finite and > 1");
    if (!std::isfinite(p->min_votes) || !(p->min_votes >= 1)) return fail(GPUART_HIP_ERR_ARG, "antilag: min_votes must be finite and >= 1");
    if (!std::isfinite(p->clip) || !(p->clip > 0)) return fail(GPUART_HIP_ERR_ARG, "antilag: clip must be finite and > 0");
    if (!std::isfinite(p->z_lo) || !(p->z_lo >= 0)) return fail(GPUART_HIP_ERR_ARG, "antilag: z_lo must be finite and >= 0");
    if (!std::isfinite(p->z_hi) || !(p->z_hi > p->z_lo)) return fail(GPUART_HIP_ERR_ARG, "antilag: z_hi must be finite and > z_lo");
    return 0;
}

/// The checks both entry points make; `align` is what the 16-byte planes must be aligned to.
int check_mix(gpuart_antilag *a, const void *slow, const void *slow_len, const void *fast, const void *fast_len, const void *mom, const void *hits,
              const void *prims, uint32_t w, uint32_t h, const gpuart_antilag_params *p, const void *out, const void *out_len, const void *alpha,
              size_t align) {
    if (int rc = check_handle(LIB, a)) return rc;
    if (!slow || !slow_len || !fast || !fast_len || !mom || !hits || !prims || !out || !out_len)
        return fail(GPUART_HIP_ERR_ARG, "antilag: slow, slow_len, fast, fast_len, moments, hits, prims, out or out_len is NULL");
    if (misaligned({slow, fast, mom, hits, out}, align) || misaligned({slow_len, fast_len, prims, out_len, alpha}, 4))
        return fail(GPUART_HIP_ERR_ARG, "antilag: misaligned pointer (slow, fast, moments, hits and out need " + std::to_string(align) +
                                            " bytes, slow_len, fast_len, prims, out_len and alpha 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (int rc = check_params(p)) return rc;
    const size_t n = (size_t)w * h;
    struct Plane { const void *p; size_t bytes; };
    const Plane in[] = {{slow, n * 16}, {slow_len, n * 4}, {fast, n * 16}, {fast_len, n * 4}, {mom, n * 16}, {hits, n * 32}, {prims, n * 4}};
    const Plane outs[] = {{out, n * 16}, {out_len, n * 4}, {alpha, n * 4}};
    for (int o = 0; o < 3; o++) {
        if (!outs[o].p) continue;
        for (int k = 0; k < 7; k++) {
            if (o == k && o < 2 && outs[o].p == in[k].p) continue;  // out == slow, out_len == slow_len
            if (overlaps(outs[o].p, outs[o].bytes, in[k].p, in[k].bytes))
                return fail(GPUART_HIP_ERR_ARG, "antilag: an output overlaps an input (only out == slow and out_len == slow_len may)");
        }
        for (int k = o + 1; k < 3; k++)
            if (outs[k].p && overlaps(outs[o].p, outs[o].bytes, outs[k].p, outs[k].bytes))
                return fail(GPUART_HIP_ERR_ARG, "antilag: an output overlaps another output");
    }
    return 0;
}

/// The launch; where an output is its input, that input is first copied into the handle's memory and read from there.
int launch_mix(gpuart_antilag *a, const float4 *slow, const float *slow_len, const float4 *fast, const float *fast_len, const float4 *mom,
               const float4 *hits, const int32_t *prims, uint32_t us_flags, int w, int h, const gpuart_antilag_params &p, float4 *out, float *out_len,
               float *alpha) {
    const size_t n = (size_t)w * h;
    if (out == slow || out_len == slow_len) {
        if (int rc = ensure(a->stream, a->copy, n * 20)) return rc;
        if (out == slow) {
            HIP_TRY(hipMemcpyAsync(a->copy.mem, slow, n * 16, hipMemcpyDeviceToDevice, a->stream));
            slow = (const float4 *)a->copy.mem;
        }
        if (out_len == slow_len) {
            float *c = (float *)((char *)a->copy.mem + n * 16);
            HIP_TRY(hipMemcpyAsync(c, slow_len, n * 4, hipMemcpyDeviceToDevice, a->stream));
            slow_len = c;
        }
    }
    const AlParams P{p.min_batches, p.min_votes, p.clip, p.z_lo, p.z_hi};
    k_al_mix<<<row_grid(w, h), row_block(), 0, a->stream>>>(slow, slow_len, fast, fast_len, mom, hits, prims, us_flags, P, w, h, out, out_len, alpha);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_antilag_last_error(void) { return g_last_error.c_str(); }

int gpuart_antilag_defaults(gpuart_antilag_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "antilag: params is NULL");
    p->fast_history = 4.0f;
    p->min_batches = 8.0f;
    p->min_votes = 8.0f;
    p->clip = 3.0f;
    p->z_lo = 2.0f;
    p->z_hi = 4.0f;
    return 0;
}

int gpuart_antilag_create(int device, gpuart_antilag **out) { return create_handle(LIB, device, out); }

int gpuart_antilag_destroy(gpuart_antilag *a) {
    if (!a) return 0;
    destroy_handle(a, {a->copy.mem, a->staging.mem});
    delete a;
    return 0;
}

int gpuart_antilag_finish(gpuart_antilag *a) { return finish_handle(LIB, a); }

int gpuart_antilag_mix(gpuart_antilag *a, const float *slow, const float *slow_len, const float *fast, const float *fast_len,
                       const float *moments, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w,
                       uint32_t h, const gpuart_antilag_params *p, float *out, float *out_len, float *alpha) {
    if (int rc = check_mix(a, slow, slow_len, fast, fast_len, moments, hits, prims, w, h, p, out, out_len, alpha, 16)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    return launch_mix(a, (const float4 *)slow, slow_len, (const float4 *)fast, fast_len, (const float4 *)moments, (const float4 *)hits, prims,
                      userSphereFlags, (int)w, (int)h, params_or_defaults(p, gpuart_antilag_defaults), (float4 *)out, out_len, alpha);
}

int gpuart_antilag_mix_host(gpuart_antilag *a, const float *slow, const float *slow_len, const float *fast, const float *fast_len,
                            const float *moments, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w,
                            uint32_t h, const gpuart_antilag_params *p, float *out, float *out_len, float *alpha) {
    int rc = check_mix(a, slow, slow_len, fast, fast_len, moments, hits, prims, w, h, p, out, out_len, alpha, 4);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(a->device));
    const size_t n = (size_t)w * h;
    // the 16-byte planes first: fast, moments and out, the staged slow and G-buffer, then the 4-byte planes slow_len, fast_len, out_len, alpha
    if ((rc = ensure(a->stream, a->staging, n * (16 + 16 + 16 + STAGED_BYTES + 4 + 4 + 4 + 4)))) return rc;
    char *base = (char *)a->staging.mem;
    float4 *d_fast = (float4 *)base, *d_mom = (float4 *)(base + n * 16), *d_out = (float4 *)(base + n * 32);
    Staged in;
    if ((rc = stage_gbuffer(a->stream, base + n * 48, n, slow, hits, prims, in))) return rc;
    float *d_sl = (float *)(base + n * (48 + STAGED_BYTES)), *d_fl = d_sl + n, *d_ol = d_fl + n, *d_al = d_ol + n;
    HIP_TRY(hipMemcpyAsync(d_fast, fast, n * 16, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(d_mom, moments, n * 16, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(d_sl, slow_len, n * 4, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(d_fl, fast_len, n * 4, hipMemcpyHostToDevice, a->stream));
    if ((rc = launch_mix(a, in.rgba, d_sl, d_fast, d_fl, d_mom, in.hits, in.prims, userSphereFlags, (int)w, (int)h, params_or_defaults(p, gpuart_antilag_defaults), d_out, d_ol,
                         alpha ? d_al : nullptr)))
        return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, n * 16, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipMemcpyAsync(out_len, d_ol, n * 4, hipMemcpyDeviceToHost, a->stream));
    if (alpha) HIP_TRY(hipMemcpyAsync(alpha, d_al, n * 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return 0;
}

}  // extern "C"
