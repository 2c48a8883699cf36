// atrous.h — the one à-trous level of the two edge-aware filters (denoise/denoise.hip, refine/refine.hip), private to them and included
// after image_lib.h: the helpers both state, the level's parameters, the body of a level for one valid pixel, and the check of the
// parameter record both public headers declare under two names. The filters differ in one value, the variance the luminance edge is
// sized by, and that value is an argument. The operation order below is the contract: tests/denoise_ref.py `level` restates it, and
// both kernels are held to that restatement bit for bit. In an anonymous namespace, like image_lib.h: Level is part of the level
// kernels' mangled names.
#pragma once
#include <cmath>

namespace {

#define AT_FN __device__ __forceinline__

/// max(a, b) as the headers state it: a > b ? a : b
AT_FN float gt_or(float a, float b) { return a > b ? a : b; }

/// the reference's PRIMITIVE_COLOR (shaders/path_tracing.glsl:123-126); the user sphere has type 0
AT_FN float3 albedo(int type) {
    if (type == 0) return make_float3(0.65f, 0.4f, 0.35f);
    if (type == 1) return make_float3(0.1f, 0.2f, 0.1f);
    return make_float3(0.3f, 0.3f, 0.3f);
}

struct Level {
    float lum_k, depth_sigma, step;
    int s;
    uint32_t normal_pow2;
};

/// Level `it` of a filter with the parameter record p (gpuart_denoise_params or gpuart_refine_params): a dilation of 2^it.
template <class P>
Level make_level(const P &p, uint32_t it) {
    Level lv;
    lv.lum_k = p.lum_k;
    lv.depth_sigma = p.depth_sigma;
    lv.s = 1 << it;
    lv.step = (float)lv.s;
    lv.normal_pow2 = p.normal_pow2;
    return lv;
}

/// One level for the valid pixel i = (x, y) with guide gp and state xp: the 25 taps, the update, and the state store or (LAST) the
/// remodulation. `var` sizes the luminance edge: the pixel's own variance in the denoiser, the prefiltered one in the variance-guided
/// filter. A tap outside the frame or on a pixel whose guide is NaN (not valid) does not count.
template <bool LAST>
AT_FN void atrous_level(int x, int y, size_t i, const float4 &gp, const float4 &xp, float var, const float4 *st_in, const float4 *guide, float4 *st_out,
                        int w, int h, const Level &lv, const float4 *rgba, const float4 *hits, float4 *out) {
    const float H[5] = {1.0f / 16, 1.0f / 4, 3.0f / 8, 1.0f / 4, 1.0f / 16};
    const float Lp = lum(xp.x, xp.y, xp.z);
    const float sd = sqrtf(var) * lv.lum_k + 1e-4f;
    const float zs = (lv.depth_sigma * gt_or(gp.w, 1e-6f)) * lv.step;
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f, nv = 0.0f;
    for (int dy = -2; dy <= 2; dy++) {
        const int qy = y + lv.s * dy;
        if (qy < 0 || qy >= h) continue;
        for (int dx = -2; dx <= 2; dx++) {
            const int qx = x + lv.s * dx;
            if (qx < 0 || qx >= w) continue;
            const size_t q = (size_t)qy * w + qx;
            const float4 gq = guide[q];
            if (!(gq.w == gq.w)) continue;
            const float4 xq = st_in[q];
            const float hk = H[dy + 2] * H[dx + 2];
            const float e = (lum(xq.x, xq.y, xq.z) - Lp) / sd;
            const float wl = 1.0f / (1.0f + e * e);
            float wn = gt_or((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.0f);
            for (uint32_t k = 0; k < lv.normal_pow2; k++) wn = wn * wn;
            const float dz = fabsf(gq.w - gp.w) / zs;
            const float wz = 1.0f / (1.0f + dz * dz);
            const float wt = ((hk * wl) * wn) * wz;
            nr += wt * xq.x;
            ng += wt * xq.y;
            nb += wt * xq.z;
            den += wt;
            nv += (wt * wt) * xq.w;
        }
    }
    float4 xo = xp;
    if (den > 0.0f) xo = make_float4(nr / den, ng / den, nb / den, nv / (den * den));
    if (LAST) {
        const float3 a = albedo(__float_as_int(hits[2 * i + 1].w) & 3);
        out[i] = make_float4(xo.x * a.x, xo.y * a.y, xo.z * a.z, rgba[i].w);
    } else {
        st_out[i] = xo;
    }
}

/// The rules of the parameter record, the same in both headers but for the cap on iterations (GPUART_<LIB>_MAX_ITERATIONS).
template <class P>
int check_params(const char *lib, const P &p, uint32_t max_iterations) {
    const std::string l(lib);
    if (p.iterations > max_iterations)
        return fail(GPUART_HIP_ERR_ARG, l + ": iterations = " + std::to_string(p.iterations) + " exceeds " + std::to_string(max_iterations));
    if (!std::isfinite(p.lum_k) || !(p.lum_k >= 0)) return fail(GPUART_HIP_ERR_ARG, l + ": lum_k must be finite and >= 0");
    if (!std::isfinite(p.depth_sigma) || !(p.depth_sigma > 0)) return fail(GPUART_HIP_ERR_ARG, l + ": depth_sigma must be finite and > 0");
    if (p.normal_pow2 > 16) return fail(GPUART_HIP_ERR_ARG, l + ": normal_pow2 exceeds 16");
    return 0;
}

/// The record an entry point runs with: the caller's, or the library's defaults where it gave none.
template <class P>
P params_or(const P *p, int (*defaults)(P *)) {
    P v;
    if (p) v = *p;
    else defaults(&v);
    return v;
}

}  // namespace
