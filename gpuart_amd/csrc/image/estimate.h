// estimate.h — the convergence estimate's two formulas, private to the two libraries that keep one (converge/converge.hip for the frame,
// adaptive/adaptive.hip per 8x8 block) and included by them after image_lib.h: the weighted batch-means step and the relative error,
// include/gpuart_converge.h, which states both operation by operation. tests/converge_ref.py `Estimator` is the one restatement both
// libraries are compared with (tests/adaptive_ref.py calls it). The kernels' instructions are held to what they were with the bodies
// written out (profiles/estimate.txt).
#pragma once

namespace {

/// One batch: the raw accumulator's pixel `a` and the pixel's state {mean, m2, prevL, 0} to the new state, for a batch of b paths that is
/// the share r = b / total of all the paths so far.
__device__ __forceinline__ float4 estimate_step(const float4 a, const float4 s, float b, float r) {
    const float Lk = lum(a.x, a.y, a.z);
    const float yk = (Lk - s.z) / b;
    const float d = yk - s.x;
    const float mean = s.x + r * d;
    const float m2 = s.y + (b * d) * (yk - mean);
    return make_float4(mean, m2, Lk, 0.0f);
}

/// e of a state after nb1 + 1 batches and `total` paths: the standard error of the mean luminance over max(that luminance, lum_floor).
__device__ __forceinline__ float estimate_error(const float4 s, float nb1, float total, float lum_floor) {
    const float v = (s.y < 0.0f ? 0.0f : s.y) / nb1;  // (a NaN m2 stays NaN: such a pixel has not converged)
    const float se = sqrtf(v / total);
    return se / (s.x > lum_floor ? s.x : lum_floor);
}

}  // namespace
