// prim_pack.h — the 48-byte device record of a primitive from its canonical data quads, by the uploader's arithmetic
// (hip/converter.h: Converter::pack_prim), stated once for the device: refit/refit.hip (an updated primitive) and edit/edit.hip (an added
// one) include this. Plain fp32 with no contraction: a triangle's edges are subtracted, everything else is copied. `T` is word 3 of the
// first quad as the caller wants it: the type, and on a leaf's first primitive the leaf's count above it.
#pragma once
#include "../hip/prim_rule.h"

namespace {

__device__ __forceinline__ void pack_prim(uint32_t type, const float *d, float T, float4 rec[3]) {
    rec[0] = make_float4(d[0], d[1], d[2], T);
    rec[2] = make_float4(0, 0, 0, 0);
    if (type == prim_rule::SPHERE) rec[1] = make_float4(d[3], 0, 0, 0);
    else if (type == prim_rule::DISC) rec[1] = make_float4(d[4], d[5], d[6], d[3]);
    else if (type == prim_rule::TRIANGLE) {
        rec[1] = make_float4(d[4] - d[0], d[5] - d[1], d[6] - d[2], 0);   // edge1 = v1 - v0
        rec[2] = make_float4(d[8] - d[0], d[9] - d[1], d[10] - d[2], 0);  // edge2 = v2 - v0
    } else {
        rec[1] = make_float4(d[8], d[9], d[10], d[11]);
        rec[2] = make_float4(d[3], d[12], d[13], d[14]);
    }
}

/// The 16 floats of payload `i` (four float4, 16-byte aligned).
__device__ __forceinline__ void load_payload(const float4 *payload, size_t i, float d[prim_rule::PAYLOAD]) {
    for (int k = 0; k < 4; k++) {
        const float4 v = payload[4 * i + k];
        d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
}

}  // namespace
