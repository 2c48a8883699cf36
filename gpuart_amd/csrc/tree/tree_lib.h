// tree_lib.h — the scaffold of the four libraries that change an uploaded scene's tree (refit/refit.hip, treebuild/build.hip,
// ploc/ploc.hip, edit/edit.hip), private to them and included after image/image_lib.h, whose last error, HIP_TRY, handle, checks and
// grow-only buffer it builds on: the checks of a scene descriptor and of a build's arguments, the step timer, the shared part of create,
// the staged run of a build's _host entry point, the refusal word, the Morton front end (for the two builds, which define
// TREE_LIB_MORTON before they include this: it needs rocPRIM's sort) and the device functions more than one library states. Each
// library is one translation unit that includes this once, so everything sits in an anonymous namespace. DESIGN.md "The tree
// libraries' scaffold" says what stays in each library.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>

#ifdef TREE_LIB_MORTON
#include <rocprim/device/device_radix_sort.hpp>
#endif

#include "../hip/prim_rule.h"
#include "../hip/tree_rule.h"

namespace {

using tree_rule::REF_INDEX;
using tree_rule::REF_LEAF;

constexpr uint32_t PARENT_LOWER = 0x80000000u;  ///< a parent link: this bit when the node is its parent's lower child

/// GPUART_HIP_TOP_DEPTH as the uploader reads it: records above this depth carry the mark. Read once per run.
inline uint32_t top_depth() {
    const char *e = getenv("GPUART_HIP_TOP_DEPTH");
    return e ? (uint32_t)atoi(e) : 0u;
}

/// Workgroups of 256 for one thread per item.
inline uint32_t blocks(size_t items) { return (uint32_t)((items + 255) / 256); }

// ---- argument checks -------------------------------------------------------------------------------------------------------------
/// The checks of a scene descriptor whose tree is to be refitted, rebuilt or edited (`done`: "refitted", "rebuilt", "edited"). Every
/// message starts with `lib`, and names the argument where the library takes more than one descriptor (`arg`, else ""). An edit reads
/// no record: `records` = false leaves them unchecked.
inline int check_descriptor(const gpuart_hip_scene *s, const char *lib, const char *arg, const char *done, bool records) {
    const std::string w = std::string(lib) + ": " + (*arg ? std::string(arg) + ": " : "");
    if (s->layout != 1) return fail(GPUART_HIP_ERR_ARG, w + "unknown layout " + std::to_string(s->layout));
    if (s->exact_boxes) return fail(GPUART_HIP_ERR_ARG, w + "a tree with irregular boxes (or boxes that do not bound their contents) is not " + done);
    if (!s->prims || !s->prim_boxes || !s->n_prims || s->n_prims > REF_INDEX || (records && ((s->n_recs && !s->recs) || s->n_recs > REF_INDEX)))
        return fail(GPUART_HIP_ERR_ARG, w + "the scene's arrays or counts are empty or out of range");
    return 0;
}

/// What a build (gpuart_<lib>_run) asks of its arguments, in the order its messages are promised in: the handle, src, dst with room for
/// `room(n)` records and n primitives, new_to_old, nothing of dst sharing a byte with src or with itself, and a scene that is not the
/// empty one. Makes the handle's device current. `word` receives word 3 of the first min(n, 2) primitives' first quads (the types) where
/// n <= 2: what the root's ref is made of when the root is a leaf.
inline int check_build(const char *lib, const ImageHandle *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, const uint32_t *new_to_old,
                       size_t (*room)(size_t n), uint32_t word[2]) {
    const std::string w = std::string(lib) + ": ";
    if (int rc = check_handle(lib, h)) return rc;
    if (!src) return fail(GPUART_HIP_ERR_ARG, w + "src is NULL");
    if (int rc = check_descriptor(src, lib, "src", "rebuilt", true)) return rc;
    if (misaligned({src->recs, src->prims}, 16) || misaligned({src->prim_boxes}, 4)) return fail(GPUART_HIP_ERR_ARG, w + "src: misaligned arrays");
    if (!dst) return fail(GPUART_HIP_ERR_ARG, w + "dst is NULL");
    if (dst->layout != 1) return fail(GPUART_HIP_ERR_ARG, w + "dst: unknown layout " + std::to_string(dst->layout));
    const size_t n = src->n_prims, n_recs = room(n);
    if (!tree_rule::box_ok(src->root_min, src->root_max)) return fail(GPUART_HIP_ERR_ARG, w + "the root box is not finite and ordered");
    if (!new_to_old || misaligned({new_to_old}, 4)) return fail(GPUART_HIP_ERR_ARG, w + "new_to_old is NULL or misaligned");
    if (!dst->prims || !dst->prim_boxes || (n_recs && !dst->recs) || misaligned({dst->recs, dst->prims}, 16) || misaligned({dst->prim_boxes}, 4))
        return fail(GPUART_HIP_ERR_ARG, w + "dst's arrays are NULL or misaligned");
    if (dst->n_prims < n || dst->n_recs < n_recs)
        return fail(GPUART_HIP_ERR_ARG, w + "dst is too small: " + std::to_string(dst->n_recs) + " records and " + std::to_string(dst->n_prims) +
                                            " primitives for " + std::to_string(n_recs) + " and " + std::to_string(n));
    const struct { const void *p; size_t bytes; } S[3] = {{src->recs, src->n_recs * 64}, {src->prims, n * 48}, {src->prim_boxes, n * 24}},
                                                  D[4] = {{dst->recs, n_recs * 64}, {dst->prims, n * 48}, {dst->prim_boxes, n * 24}, {new_to_old, n * 4}};
    for (const auto &s : S)
        for (const auto &d : D)
            if (s.bytes && d.bytes && overlaps(s.p, s.bytes, d.p, d.bytes)) return fail(GPUART_HIP_ERR_ARG, w + "dst's arrays alias src's");
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
            if (D[a].bytes && D[b].bytes && overlaps(D[a].p, D[a].bytes, D[b].p, D[b].bytes)) return fail(GPUART_HIP_ERR_ARG, w + "dst's arrays overlap");
    HIP_TRY(hipSetDevice(h->device));
    word[0] = word[1] = 0;
    if (n <= 2) {  // an empty scene keeps one dummy record, whose count is 0 (converter.h)
        for (size_t k = 0; k < n; k++) HIP_TRY(hipMemcpy(&word[k], (const char *)src->prims + 48 * k + 12, 4, hipMemcpyDeviceToHost));
        if (n == 1 && (word[0] >> 2) == 0) return fail(GPUART_HIP_ERR_ARG, w + "src: an empty scene is not rebuilt");
    }
    return 0;
}

// ---- the step timer --------------------------------------------------------------------------------------------------------------
/// The device time of a run's `steps` steps: steps + 1 events, recorded in order by mark(); step k is what lies between event from[k]
/// and the one after it (from = NULL: between event k and k + 1), so a library may report its steps in another order than it runs them.
/// The events live as long as the handle.
struct StepTimer {
    static constexpr int MAX_STEPS = 7;
    hipEvent_t ev[MAX_STEPS + 1] = {};
    double ms[MAX_STEPS] = {};
    int steps = 0, at = 0;
    hipStream_t stream = nullptr;  ///< of the run being timed

    hipError_t create(int n) {
        steps = n;
        hipError_t e = hipSuccess;
        for (int k = 0; k <= n && e == hipSuccess; k++) e = hipEventCreate(&ev[k]);
        return e;
    }
    void destroy() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    void start(hipStream_t s) { stream = s; at = 0; }
    hipError_t mark() { return hipEventRecord(ev[at++], stream); }
    /// After the stream was waited for.
    int read(const int *from = nullptr) {
        for (int k = 0; k < steps; k++) {
            const int a = from ? from[k] : k;
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, ev[a], ev[a + 1]));
            ms[k] = t;
        }
        return 0;
    }
};

/// gpuart_<lib>_step_ms of a handle with a `timer`.
template <class H>
int step_ms(const char *lib, H *h, double *ms) {
    if (int rc = check_handle(lib, h)) return rc;
    if (!ms) return fail(GPUART_HIP_ERR_ARG, std::string(lib) + ": ms is NULL");
    memcpy(ms, h->timer.ms, h->timer.steps * sizeof(double));
    return 0;
}

// ---- create, and a build's _host entry point ---------------------------------------------------------------------------------------
/// create: the handle, then `alloc(h)` — the library's status and its kin in device memory, its timer's events —; a failure there
/// destroys what was made, and *out stays NULL.
template <class H, class A>
int create_tree_handle(const char *lib, int device, H **out, int (*destroy)(H *), A alloc) {
    if (int rc = create_handle(lib, device, out)) return rc;
    H *h = *out;
    *out = nullptr;
    const hipError_t e = alloc(h);
    if (e != hipSuccess) {
        destroy(h);
        return fail(GPUART_HIP_ERR_DEVICE, std::string(lib) + ": allocating the status: " + hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

/// gpuart_<lib>_run_host of a build: `run` into the handle's `staging`, then the permutation copied to the host's new_to_old.
template <class H, class R>
int run_staged(const char *lib, H *h, int (*run)(H *, const gpuart_hip_scene *, const gpuart_hip_scene *, uint32_t *, R *), const gpuart_hip_scene *src,
               const gpuart_hip_scene *dst, uint32_t *new_to_old, R *result) {
    if (int rc = check_handle(lib, h)) return rc;
    if (!src || !new_to_old || !src->n_prims) return fail(GPUART_HIP_ERR_ARG, std::string(lib) + ": src or new_to_old is NULL, or the scene is empty");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure(h->stream, h->staging, src->n_prims * sizeof(uint32_t))) return rc;
    if (int rc = run(h, src, dst, (uint32_t *)h->staging.mem, result)) return rc;
    HIP_TRY(hipMemcpyAsync(new_to_old, h->staging.mem, src->n_prims * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- the refusal word ------------------------------------------------------------------------------------------------------------
// A status' `refused` = ~(4 x index + why) of the first offending item of a list — the largest over the items (atomicMax) —, 0 while
// nothing is refused.
enum { WHY_ORDER = 1, WHY_RANGE = 2, WHY_RULE = 3 };

__device__ __forceinline__ void refuse(uint32_t *refused, uint32_t i, uint32_t why) { atomicMax(refused, ~(4u * i + why)); }

inline uint32_t refused_index(uint32_t refused) { return ~refused >> 2; }

/// Why: the two texts every list shares, and for WHY_RULE the library's own (`rule`).
inline const char *refused_why(uint32_t refused, const char *rule) {
    const char *const why[4] = {"", "its ordinal does not exceed the one before it (ordinals are strictly ascending)",
                                "its ordinal is not below the number of primitives", rule};
    return why[~refused & 3u];
}

// ---- device functions ------------------------------------------------------------------------------------------------------------
/// One primitive moved: its three quads from `s` to `d`, word 3 of the first made of its type and `cnt` (the leaf's count on a leaf's
/// first primitive, else 0), and its six box floats from `sb` to `db`. k_bd_permute, k_pl_permute and k_ed_compact move theirs by this.
__device__ __forceinline__ void move_prim(const float4 *src, const float *src_box, uint32_t from, uint32_t cnt, float4 *dst, float *dst_box, uint32_t to) {
    const float4 *s = src + 3 * (size_t)from;
    float4 r0 = s[0];
    r0.w = __uint_as_float((__float_as_uint(r0.w) & 3u) | cnt << 2);
    float4 *d = dst + 3 * (size_t)to;
    d[0] = r0; d[1] = s[1]; d[2] = s[2];
    const float *sb = src_box + 6 * (size_t)from;
    float *db = dst_box + 6 * (size_t)to;
    for (int k = 0; k < 6; k++) db[k] = sb[k];
}

// "Are the one or two primitives at `first` all triangles" (build's leaf_ref, ploc's child_ref: three lines on the records' type words)
// is NOT stated here: every form of a shared function that was tried moved instructions in k_bd_emit, k_bd_root_leaf and k_pl_emit, and
// those kernels are held to what they were (profiles/tree_libs.txt). Both libraries keep the lines written out.

// ---- the Morton front end ----------------------------------------------------------------------------------------------------------
#ifdef TREE_LIB_MORTON
struct Box3 { float lo[3], hi[3]; };

// One thread per primitive: its 63-bit key from its box and the root box, and its ordinal as the sort's value.
__global__ void __launch_bounds__(256) k_tr_keys(const float *pbox, uint32_t n, Box3 root, uint64_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *b = pbox + 6 * (size_t)i;
    keys[i] = tree_rule::morton_key(b, b + 3, root.lo, root.hi);
    vals[i] = i;
}

/// The keys of src's primitives, then rocPRIM's sort of (key, ordinal) from keys_in / vals_in into keys / sorted, on the started timer's
/// stream. `temp` grows to what the sort asks for, or to `at_least` where that is more (the caller's own use of it). The timer is marked
/// before the keys, between the two and after the sort.
inline int morton_sort(StepTimer &timer, DeviceBuffer &temp, size_t at_least, const gpuart_hip_scene *src, uint64_t *keys_in, uint64_t *keys,
                       uint32_t *vals_in, uint32_t *sorted) {
    const hipStream_t stream = timer.stream;
    const size_t n = src->n_prims;
    size_t sort_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, sort_bytes, keys_in, keys, vals_in, sorted, n, 0, 63, stream));
    if (int rc = ensure(stream, temp, std::max(sort_bytes, at_least) + 16)) return rc;
    Box3 root;
    memcpy(root.lo, src->root_min, 12); memcpy(root.hi, src->root_max, 12);
    HIP_TRY(timer.mark());
    k_tr_keys<<<blocks(n), 256, 0, stream>>>((const float *)src->prim_boxes, (uint32_t)n, root, keys_in, vals_in);
    HIP_TRY(hipGetLastError());
    HIP_TRY(timer.mark());
    HIP_TRY(rocprim::radix_sort_pairs(temp.mem, sort_bytes, keys_in, keys, vals_in, sorted, n, 0, 63, stream));
    HIP_TRY(timer.mark());
    return 0;
}
#endif

}  // namespace
