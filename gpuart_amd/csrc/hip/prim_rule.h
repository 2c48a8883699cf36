// prim_rule.h — what a primitive's canonical data quads (Primitive::StoreDataIntoBVH, host/core.cpp) must satisfy before a box can be
// said to bound the primitive, and the box itself: stated once for the uploader (converter.h: Converter::prim_in_box), the device refit
// (refit/refit.hip: the validation of an update and the box of an updated primitive) and the host refit (host/bvh.cpp). Host and device,
// plain fp32 with no contraction; nothing here is called by a kernel of libgpuart_hip.so.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PR_FN __host__ __device__ static inline
#else
#define PR_FN static inline
#endif

namespace prim_rule {

enum { SPHERE = 0, DISC = 1, TRIANGLE = 2, CONE = 3 };
constexpr int PAYLOAD = 16;  ///< floats of a zero-padded payload: the longest primitive's four data quads

/// Data quads of a primitive of `type` (StoreDataIntoBVH).
PR_FN int data_quads(uint32_t type) { return (int)(type & 3) + 1; }

/// The box's starting value and its running minimum / maximum (host/bvh.cpp PrepareNode): `<` and `>` keep the first of equal values
/// and skip a NaN.
PR_FN void box_start(float lo[3], float hi[3]) {
    for (int k = 0; k < 3; k++) { lo[k] = 99.0e+29f; hi[k] = -99.0e+29f; }
}
PR_FN void box_fold(float lo[3], float hi[3], const float clo[3], const float chi[3]) {
    for (int k = 0; k < 3; k++) {
        if (clo[k] < lo[k]) lo[k] = clo[k];
        if (chi[k] > hi[k]) hi[k] = chi[k];
    }
}

/// The preconditions. Coordinates beyond 2^20 (the hostile classes use 1e10 ... 1e30): the intersectors' own arithmetic cancels there — a
/// vertex at -1e30 swallows the ray origin in `origin - v0` — and a hit parameter that is off by more than the band says nothing about
/// the box it came from. (ulp(2^20) = 0.06: no scene a float path tracer renders sensibly is excluded.) A cone's derived constants
/// 12..14 — width coefficient, cosB, dotAxC1 — are included; pads are excluded: word 7 of a disc, word 15 of a cone, every fourth word of
/// a triangle — the device never reads them (tests/test_converter.py). Radii and a cone's length are >= 0; a NaN fails everything.
PR_FN bool prim_ok(uint32_t type, const float *d) {
    const int len = type == SPHERE ? 4 : type == DISC ? 7 : type == TRIANGLE ? 12 : 15;
    if (type > 3) return false;
    for (int k = 0; k < len; k++)
        if (!(fabsf(d[k]) <= 1048576.0f) && !(type == TRIANGLE && (k & 3) == 3)) return false;
    if (type == SPHERE || type == DISC) return d[3] >= 0;  // (the reference bounds a disc by the sphere of its radius)
    if (type == TRIANGLE) return true;
    const float r1 = d[3], r2 = d[7], length = d[11], wc = d[12];
    if (!(r1 >= 0) || !(r2 >= 0) || !(length >= 0)) return false;
    // the intersector works from (centre 1, radius 1, axis, length, width coefficient): they must describe the same frustum
    const float tol = 1.0e-4f * (length + r1 + r2) + 1.0e-30f;
    for (int k = 0; k < 3; k++)
        if (!(fabsf(d[k] + length * d[8 + k] - d[4 + k]) <= tol)) return false;
    if (!(fabsf(r1 + wc * length - r2) <= tol)) return false;
    // ... and so must the constants that POSITION the surface for cone_hit (device_scene.h; reference shaders/cone.glsl:30-135 with
    // the host's src/core.cpp:191-226): a unit axis, dotAxC1 = axis . centre 1 (the F and H terms), cosB from the radii and the
    // length (the normal only — but a record that lies about one derived constant is hand-made: no benefit of the doubt)
    const float ax2 = d[8] * d[8] + d[9] * d[9] + d[10] * d[10];
    if (length > 0 && !(fabsf(ax2 - 1.0f) <= 1.0e-4f)) return false;
    const float dot_c1 = d[8] * d[0] + d[9] * d[1] + d[10] * d[2];
    if (!(fabsf(d[14] - dot_c1) <= 1.0e-4f * (fabsf(d[0]) + fabsf(d[1]) + fabsf(d[2]) + 1.0f))) return false;
    float cosb = 0.0f;
    if (fabsf(r1 - r2) >= 1.0e-7f && length > 0) {
        const float rr = r1 > r2 ? r1 : r2, h = rr * length / fabsf(r1 - r2);
        cosb = (r1 > r2 ? rr : -rr) / sqrtf(h * h + rr * rr);
    }
    return fabsf(d[13] - cosb) <= 1.0e-3f;
}

/// The box the primitive's constructor gives it (host/core.cpp; reference src/core.cpp:36-65,80-90,136-150,217-225), from its data quads.
PR_FN void prim_box(uint32_t type, const float *d, float lo[3], float hi[3]) {
    if (type == TRIANGLE) {
        for (int k = 0; k < 3; k++) { lo[k] = 9e+19f; hi[k] = -9e+19f; }
        for (int v = 0; v < 3; v++)
            for (int k = 0; k < 3; k++) {
                const float x = d[4 * v + k];
                if (x < lo[k]) lo[k] = x;
                if (x > hi[k]) hi[k] = x;
            }
    } else if (type == CONE) {
        for (int k = 0; k < 3; k++) {
            const float a = d[k] - d[3], b = d[4 + k] - d[7], A = d[k] + d[3], B = d[4 + k] + d[7];
            lo[k] = b < a ? b : a;  // std::min(a, b)
            hi[k] = A < B ? B : A;  // std::max(A, B)
        }
    } else {
        for (int k = 0; k < 3; k++) { lo[k] = d[k] - d[3]; hi[k] = d[k] + d[3]; }
    }
}

}  // namespace prim_rule
