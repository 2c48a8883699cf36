// CPU-only: csrc/hip/nearest_rule.h in a stand-alone program under AddressSanitizer + UBSan (tools/sanitize_nearest.sh). Honest and
// degenerate primitives of the four types against ordinary, coincident, huge, tiny and non-finite points: closest_on_prim must return a
// point of the primitive's box and a d2 that is no NaN for every finite point, and the lemma — box_d2 of the primitive's box and of every
// box around it is <= d2 — must hold with no exception.   nearest_sanitize [rounds]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "nearest_rule.h"
#include "prim_rule.h"

namespace nr = nearest_rule;

static std::mt19937 rng(7);
static float uni(float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); }

/// The 48-byte record of a primitive from its 16 data floats (the uploader's arithmetic: hip/converter.h pack_prim).
static void pack(uint32_t type, const float *d, float rec[12]) {
    memset(rec, 0, 48);
    rec[0] = d[0]; rec[1] = d[1]; rec[2] = d[2];
    memcpy(rec + 3, &type, 4);
    if (type == 0) rec[4] = d[3];
    else if (type == 1) { rec[4] = d[4]; rec[5] = d[5]; rec[6] = d[6]; rec[7] = d[3]; }
    else if (type == 2) for (int k = 0; k < 3; k++) { rec[4 + k] = d[4 + k] - d[k]; rec[8 + k] = d[8 + k] - d[k]; }
    else { rec[4] = d[8]; rec[5] = d[9]; rec[6] = d[10]; rec[7] = d[11]; rec[8] = d[3]; rec[9] = d[12]; rec[10] = d[13]; rec[11] = d[14]; }
}

static void make(uint32_t type, int degenerate, float scale, float d[16]) {
    memset(d, 0, 64);
    for (int k = 0; k < 3; k++) d[k] = uni(-scale, scale);
    const float r = degenerate == 1 ? 0.0f : uni(0.01f, 0.5f) * scale;
    if (type == 0) d[3] = r;
    else if (type == 1) {
        d[3] = r;
        float n[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        const float l = sqrtf(nr::dot3(n, n));
        for (int k = 0; k < 3; k++) d[4 + k] = degenerate == 2 || !(l > 0) ? 0.0f : n[k] / l;
    } else if (type == 2) {
        for (int v = 1; v < 3; v++)
            for (int k = 0; k < 3; k++) d[4 * v + k] = degenerate == 1 ? d[k] : degenerate == 2 ? d[k] + v * 0.25f * scale : d[k] + uni(-0.5f, 0.5f) * scale;
    } else {
        float a[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
        float l = sqrtf(nr::dot3(a, a));
        const float len = degenerate == 2 ? 0.0f : uni(0.05f, 1.0f) * scale;
        for (int k = 0; k < 3; k++) { a[k] = len > 0 && l > 0 ? a[k] / l : 0.0f; d[4 + k] = d[k] + a[k] * len; d[8 + k] = a[k]; }
        d[3] = r; d[7] = degenerate == 1 ? 0.0f : uni(0.0f, 0.5f) * scale; d[11] = len;
        d[12] = len > 0 ? (d[7] - d[3]) / len : 0.0f;
        d[14] = nr::dot3(a, d);
    }
}

int main(int argc, char **argv) {
    const long rounds = argc > 1 ? atol(argv[1]) : 200000;
    long tested = 0, equal = 0;
    const float scales[4] = {1.0f, 1048576.0f / 4, 1e-30f, 1e-3f};
    for (long i = 0; i < rounds; i++) {
        const uint32_t type = (uint32_t)(i & 3);
        const float scale = scales[(i >> 2) & 3];
        float d[16], rec[12], box[6];
        make(type, (int)((i >> 4) % 3), scale, d);
        pack(type, d, rec);
        prim_rule::prim_box(type, d, box, box + 3);
        float outer[6];
        for (int k = 0; k < 3; k++) { outer[k] = box[k] - uni(0, 1) * scale; outer[3 + k] = box[3 + k] + uni(0, 1) * scale; }
        for (int j = 0; j < 8; j++) {
            float p[3];
            for (int k = 0; k < 3; k++)
                p[k] = j == 0 ? d[k] : j == 1 ? box[k + 3 * (int)(i & 1)] : j == 2 ? 3e38f * (k == 1 ? -1 : 1) : j == 3 ? 0.0f : d[k] + uni(-2, 2) * scale;
            if (j == 4 && type == 3) for (int k = 0; k < 3; k++) p[k] = d[k] + d[8 + k] * uni(-1, 2) * d[11];  // on a cone's axis
            float q[3];
            const float d2 = nr::closest_on_prim(type, rec, box, p, q);
            for (int k = 0; k < 3; k++)
                if (!(q[k] >= box[k] && q[k] <= box[3 + k])) { printf("FAIL: q outside its box (round %ld, point %d)\n", i, j); return 1; }
            if (d2 != d2) { printf("FAIL: d2 is NaN (round %ld, point %d)\n", i, j); return 1; }
            const float b = nr::box_d2(box, box + 3, p), o = nr::box_d2(outer, outer + 3, p);
            if (!(b <= d2) || !(o <= b)) { printf("FAIL: the lemma (round %ld, point %d): outer %g box %g d2 %g\n", i, j, o, b, d2); return 1; }
            equal += b == d2;
            tested++;
        }
        const float bad[3] = {NAN, INFINITY, 0.0f};
        float q[3];
        (void)nr::closest_on_prim(type, rec, box, bad, q);  // (not a query: query_ok refuses it; it must still raise nothing)
        if (nr::query_ok(bad, 1.0f) || nr::query_ok(d, NAN) || nr::query_ok(d, -1.0f) || !nr::query_ok(d, INFINITY)) { printf("FAIL: query_ok\n"); return 1; }
    }
    printf("nearest_rule.h: %ld (primitive, point) pairs, every q in its box, no NaN, the lemma without exception (%ld equalities)\n", tested, equal);
    return 0;
}
