// tree_rule.h — what everything that reads or writes the device tree must agree on, stated once: the ref word of a record
// (device_scene.h walks it; converter.h, the box pass of refit/box_pass.h and treebuild/build.hip write it), the two conditions a tree's
// boxes are classified by, and the Morton rule of include/gpuart_build.h, which treebuild/build.hip applies on the device and
// host/bvh.cpp (RebuildMorton) on the host. Host and device, plain C++ like prim_rule.h: fp32 with no contraction and IEEE division
// (every includer is built so). The tests' restatements (tests/build_ref.py, tests/refit_ref.py, tests/converter_ref.py) do not read it.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TR_FN __host__ __device__ static inline
#else
#define TR_FN static inline
#endif

namespace tree_rule {

// ---- the ref word: an interior child's record index, or REF_LEAF | flags | the leaf's first primitive -----------------------------
constexpr uint32_t REF_LEAF = 0x80000000u;
constexpr uint32_t REF_TRIS = 0x40000000u;   ///< with REF_LEAF: the leaf holds only triangles, one or two of them
constexpr uint32_t REF_TWO = 0x20000000u;    ///< with REF_TRIS or REF_SMALL: two of them (both records are fetched at once)
constexpr uint32_t REF_SMALL = 0x10000000u;  ///< with REF_LEAF, without REF_TRIS: one or two primitives, not all of them triangles
constexpr uint32_t REF_INDEX = 0x0fffffffu;  ///< the first primitive; also the most records and primitives a tree can have

/// The ref of the leaf of `count` primitives from `first` on; all_tris: every one of them is a triangle. (A leaf of the reference's
/// builder may hold none, the empty scene, or more than two: it carries no flag and is walked primitive by primitive.)
/// treebuild/build.hip (leaf_ref) writes the line out for its leaves of one or two: through the call k_bd_emit and k_bd_root_leaf
/// compile to other instructions, and the kernels are held to what they were (profiles/tree_rule.txt).
TR_FN uint32_t leaf_ref(uint32_t first, uint32_t count, bool all_tris) {
    if (count != 1 && count != 2) return REF_LEAF | first;
    return REF_LEAF | first | (all_tris ? REF_TRIS : REF_SMALL) | (count == 2 ? REF_TWO : 0u);
}

/// The root's ref: record 0 of a tree with records, else a leaf inside the primitives.
TR_FN bool root_ref_ok(uint32_t root_ref, uint64_t n_recs, uint64_t n_prims) {
    return n_recs ? root_ref == 0 : (root_ref & REF_LEAF) && (root_ref & REF_INDEX) < n_prims;
}

// ---- boxes ------------------------------------------------------------------------------------------------------------------------
/// A plane the quick box answers accept (box_quick.h): zero, or at least 2^-60 in magnitude. False for NaN and for a subnormal number.
TR_FN bool plane_ok(float p) { return p == 0.0f || (p >= 8.6736173798840355e-19f || p <= -8.6736173798840355e-19f); }

/// A box that is finite and ordered — regular: the fast box test (med3) assumes min <= max and a finite plane. A NaN fails <=.
TR_FN bool box_ok(const float lo[3], const float hi[3]) {
    for (int k = 0; k < 3; k++)
        if (!(lo[k] <= hi[k]) || std::isinf(lo[k]) || std::isinf(hi[k])) return false;
    return true;
}

// ---- the Morton rule (include/gpuart_build.h) ---------------------------------------------------------------------------------------
/// Bits of a 21-bit number spread to every third bit.
TR_FN uint64_t spread3(uint32_t q) {
    uint64_t x = q & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

/// The 63-bit key of the box [lo, hi] in the root box: per axis the box's centre, as a fraction of the root's extent, in 21 bits.
TR_FN uint64_t morton_key(const float lo[3], const float hi[3], const float root_lo[3], const float root_hi[3]) {
    uint64_t key = 0;
    for (int k = 0; k < 3; k++) {
        const float c = lo[k] * 0.5f + hi[k] * 0.5f;
        const float e = root_hi[k] - root_lo[k];
        const float t = (c - root_lo[k]) / e;
        uint32_t q = 0;
        if (e > 0.0f && t > 0.0f) {
            const float s = t * 2097152.0f;
            q = s >= 2097151.0f ? 2097151u : (uint32_t)s;
        }
        key |= spread3(q) << (2 - k);
    }
    return key;
}

/// delta(i, j) of the sorted leaves i and j with keys ki and kj: the length of their keys' common prefix, or past 64 that of their
/// indices. Precondition i != j (the count of leading zeros of 0 is not defined): Karras' search never compares a leaf with itself, nor
/// does the host's bisection.
TR_FN int key_delta(uint64_t ki, uint64_t kj, uint32_t i, uint32_t j) {
    const uint64_t x = ki ^ kj;
    return x ? __builtin_clzll(x) : 64 + __builtin_clz(i ^ j);
}

}  // namespace tree_rule
