// refit.hip — libgpuart_refit.so (gfx950): listed primitives of an uploaded scene replaced and its tree's boxes refitted in place, as
// include/gpuart_refit.h states it. Built without flushing fp32 denormals and without contraction: a box plane is copied, a triangle's
// edge subtracted, exactly as the host uploader does (csrc/hip/converter.h) and tests/refit_ref.py restates in NumPy float32.
// DESIGN.md "Refit" describes the launches and why nothing is handed between workgroups inside one. The box pass (k_rf_level, k_rf_root)
// is in box_pass.h, which treebuild/build.hip shares; the descriptor's checks and the refusal word are the tree libraries' (tree/tree_lib.h).
#include <cmath>
#include <cstring>
#include <vector>

#include "../image/image_lib.h"
#include "../tree/tree_lib.h"
#include "box_pass.h"
#include "prim_pack.h"
#include "gpuart_refit.h"

namespace {

const char LIB[] = "refit";

constexpr uint32_t NONE = GPUART_REFIT_NO_UPDATE;

// 1. One thread per update: ordinals ascending and in range, the payload inside the rule for the type the primitive has.
__global__ void __launch_bounds__(256) k_rf_validate(const uint32_t *ord, const float4 *payload, uint32_t n, const float4 *prims, uint32_t n_prims,
                                                     Status *st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = ord[i];
    uint32_t why = 0;
    if (i > 0 && !(ord[i - 1] < p)) why = WHY_ORDER;
    else if (p >= n_prims) why = WHY_RANGE;
    else {
        float d[prim_rule::PAYLOAD];
        load_payload(payload, i, d);
        const uint32_t type = __float_as_uint(prims[3 * (size_t)p].w) & 3u;
        if (!prim_rule::prim_ok(type, d)) why = WHY_RULE;
    }
    if (why) refuse(&st->refused, i, why);
}

// 2. One thread per update: the three float4 of the record by the uploader's arithmetic (prim_pack.h), word 3 of the first —
// the type and the leaf's count — kept, and the primitive's own box. Nothing is written once an update is refused: the status word was
// written by the launch before this one.
__global__ void __launch_bounds__(256) k_rf_update(const uint32_t *ord, const float4 *payload, uint32_t n, float4 *prims, float *pbox, const Status *st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || st->refused) return;
    const uint32_t p = ord[i];
    float d[prim_rule::PAYLOAD];
    load_payload(payload, i, d);
    float4 *rec = prims + 3 * (size_t)p;
    const float T = rec[0].w;
    const uint32_t type = __float_as_uint(T) & 3u;
    float4 r[3];
    pack_prim(type, d, T, r);
    rec[0] = r[0]; rec[1] = r[1]; rec[2] = r[2];
    float lo[3], hi[3];
    prim_rule::prim_box(type, d, lo, hi);
    float *b = pbox + 6 * (size_t)p;
    for (int k = 0; k < 3; k++) { b[k] = lo[k]; b[3 + k] = hi[k]; }
}

/// Word 3 of every primitive's first quad (the type, and on a leaf's first primitive its count), gathered for the host's bind.
__global__ void __launch_bounds__(256) k_rf_type_words(const float4 *prims, uint32_t n_prims, uint32_t *out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_prims) out[i] = __float_as_uint(prims[3 * (size_t)i].w);
}

}  // namespace

struct gpuart_refit : ImageHandle {
    Status *status = nullptr;    ///< device
    DeviceBuffer order;          ///< record indices sorted by level, deepest level last
    std::vector<uint32_t> level; ///< level l's records are order[level[l] .. level[l + 1])
    DeviceBuffer staging;        ///< run_host: the ordinals, then the payload
    bool bound = false;
    gpuart_hip_scene scene{};    ///< what the handle is bound to
};

namespace {

inline uint32_t ubits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

int check_scene(const gpuart_refit *h, const gpuart_hip_scene *s) {
    if (!s) return fail(GPUART_HIP_ERR_ARG, "refit: scene is NULL");
    if (!h->bound) return fail(GPUART_HIP_ERR_ARG, "refit: the handle is not bound to a scene");
    if (s->generation != h->scene.generation || s->recs != h->scene.recs || s->prims != h->scene.prims || s->prim_boxes != h->scene.prim_boxes ||
        s->n_recs != h->scene.n_recs || s->n_prims != h->scene.n_prims || s->root_ref != h->scene.root_ref)
        return fail(GPUART_HIP_ERR_ARG, "refit: the handle was bound to another upload (generation " + std::to_string(h->scene.generation) + ", the scene's is " +
                                            std::to_string(s->generation) + "): bind again");
    return 0;
}

/// The device sequence on ordinals and payload in device memory, and the read-back.
int run_device(gpuart_refit *h, const uint32_t *ord, const float4 *payload, uint32_t n, gpuart_refit_result *result) {
    const gpuart_hip_scene &s = h->scene;
    float4 *recs = (float4 *)s.recs, *prims = (float4 *)s.prims;
    float *pbox = (float *)s.prim_boxes;
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(Status), h->stream));
    if (n) {
        k_rf_validate<<<blocks(n), 256, 0, h->stream>>>(ord, payload, n, prims, (uint32_t)s.n_prims, h->status);
        HIP_TRY(hipGetLastError());
        k_rf_update<<<blocks(n), 256, 0, h->stream>>>(ord, payload, n, prims, pbox, h->status);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t *order = (const uint32_t *)h->order.mem;
    for (size_t l = h->level.size() - 1; l-- > 0;) {  // deepest level first
        const uint32_t count = h->level[l + 1] - h->level[l];
        k_rf_level<<<(2u * count + 255u) / 256u, 256, 0, h->stream>>>(order + h->level[l], count, recs, prims, pbox, h->status);
        HIP_TRY(hipGetLastError());
    }
    k_rf_root<<<1, 64, 0, h->stream>>>(recs, prims, pbox, s.root_ref, h->status);
    HIP_TRY(hipGetLastError());
    Status st;
    HIP_TRY(hipMemcpyAsync(&st, h->status, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (result) {
        result->status = st.refused ? GPUART_HIP_ERR_ARG : 0;
        result->first_bad = st.refused ? refused_index(st.refused) : NONE;
        result->subnormal = st.subnormal;
        memcpy(result->root_min, st.refused ? s.root_min : st.root_min, 12);
        memcpy(result->root_max, st.refused ? s.root_max : st.root_max, 12);
    }
    if (st.refused) {
        const char *why = refused_why(st.refused, "its payload is outside the primitive rule (a word that is not finite or beyond 2^20, a negative radius or length, "
                                                  "or a cone's derived constants that contradict its centres and radii)");
        return fail(GPUART_HIP_ERR_ARG, "refit: update " + std::to_string(refused_index(st.refused)) + " refused: " + why + "; nothing was written");
    }
    memcpy(h->scene.root_min, st.root_min, 12);
    memcpy(h->scene.root_max, st.root_max, 12);
    return 0;
}

int check_run(gpuart_refit *h, const gpuart_hip_scene *scene, const void *ordinals, const void *payload, size_t n, size_t align) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (int rc = check_scene(h, scene)) return rc;
    if (n > h->scene.n_prims) return fail(GPUART_HIP_ERR_ARG, "refit: more updates (" + std::to_string(n) + ") than primitives (" + std::to_string(h->scene.n_prims) + ")");
    if (n && (!ordinals || !payload)) return fail(GPUART_HIP_ERR_ARG, "refit: ordinals or payload is NULL");
    if (n && (misaligned({ordinals}, 4) || misaligned({payload}, align)))
        return fail(GPUART_HIP_ERR_ARG, "refit: misaligned pointer (ordinals need 4 bytes, payload " + std::to_string(align) + ")");
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_refit_last_error(void) { return g_last_error.c_str(); }

int gpuart_refit_create(int device, gpuart_refit **out) {
    return create_tree_handle(LIB, device, out, gpuart_refit_destroy, [](gpuart_refit *h) { return hipMalloc((void **)&h->status, sizeof(Status)); });
}

int gpuart_refit_destroy(gpuart_refit *h) {
    if (!h) return 0;
    destroy_handle(h, {h->status, h->order.mem, h->staging.mem});
    delete h;
    return 0;
}

int gpuart_refit_finish(gpuart_refit *h) { return finish_handle(LIB, h); }

int gpuart_refit_bind(gpuart_refit *h, const gpuart_hip_scene *s) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!s) return fail(GPUART_HIP_ERR_ARG, "refit: scene is NULL");
    h->bound = false;
    if (int rc = check_descriptor(s, LIB, "", "refitted", true)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const size_t n_recs = s->n_recs, n_prims = s->n_prims;
    // every leaf's count, which its first primitive carries, and the records
    std::vector<float> recs(16 * n_recs);
    std::vector<uint32_t> tw(n_prims);
    if (n_recs) HIP_TRY(hipMemcpy(recs.data(), s->recs, recs.size() * 4, hipMemcpyDeviceToHost));
    if (int rc = ensure(h->stream, h->staging, n_prims * 4)) return rc;
    k_rf_type_words<<<blocks(n_prims), 256, 0, h->stream>>>((const float4 *)s->prims, (uint32_t)n_prims, (uint32_t *)h->staging.mem);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(tw.data(), h->staging.mem, n_prims * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const auto leaf_ok = [&](uint32_t ref) {
        const size_t first = ref & REF_INDEX;
        if (first >= n_prims) return false;
        const size_t cnt = tw[first] >> 2;
        return cnt >= 1 && cnt <= n_prims - first;
    };
    // Records lie in pre-order: a child's record comes after its parent's, and every record but the root's is some record's child once.
    std::vector<uint32_t> depth(n_recs, 0);
    std::vector<char> seen(n_recs, 0);
    uint32_t deepest = 0;
    const auto bad_tree = [] { return fail(GPUART_HIP_ERR_ARG, "refit: the records' refs do not form the tree the counts describe"); };
    if (!tree_rule::root_ref_ok(s->root_ref, n_recs, n_prims) || (!n_recs && !leaf_ok(s->root_ref))) return bad_tree();
    for (size_t r = 0; r < n_recs; r++) {
        if (r && !seen[r]) return bad_tree();
        for (int c = 0; c < 2; c++) {
            const uint32_t ref = ubits(recs[16 * r + 4 * c + 3]);
            if (ref & REF_LEAF) {
                if (!leaf_ok(ref)) return bad_tree();
            } else {
                if (ref <= r || ref >= n_recs || seen[ref]) return bad_tree();
                seen[ref] = 1;
                depth[ref] = depth[r] + 1;
                if (depth[ref] > deepest) deepest = depth[ref];
            }
        }
    }
    // a counting sort by level
    const size_t levels = n_recs ? (size_t)deepest + 1 : 0;
    h->level.assign(levels + 1, 0);
    for (size_t r = 0; r < n_recs; r++) h->level[depth[r] + 1]++;
    for (size_t l = 0; l < levels; l++) h->level[l + 1] += h->level[l];
    std::vector<uint32_t> order(n_recs), at(h->level.begin(), h->level.end() - 1);
    for (size_t r = 0; r < n_recs; r++) order[at[depth[r]]++] = (uint32_t)r;
    if (n_recs) {
        if (int rc = ensure(h->stream, h->order, n_recs * 4)) return rc;
        HIP_TRY(hipMemcpy(h->order.mem, order.data(), n_recs * 4, hipMemcpyHostToDevice));
    }
    h->scene = *s;
    h->bound = true;
    return 0;
}

int gpuart_refit_levels(gpuart_refit *h, uint32_t *levels) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!levels) return fail(GPUART_HIP_ERR_ARG, "refit: levels is NULL");
    if (!h->bound) return fail(GPUART_HIP_ERR_ARG, "refit: the handle is not bound to a scene");
    *levels = (uint32_t)(h->level.size() - 1);
    return 0;
}

int gpuart_refit_run(gpuart_refit *h, const gpuart_hip_scene *scene, const uint32_t *ordinals, const float *payload, size_t n,
                     gpuart_refit_result *result) {
    if (int rc = check_run(h, scene, ordinals, payload, n, 16)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return run_device(h, ordinals, (const float4 *)payload, (uint32_t)n, result);
}

int gpuart_refit_run_host(gpuart_refit *h, const gpuart_hip_scene *scene, const uint32_t *ordinals, const float *payload, size_t n,
                          gpuart_refit_result *result) {
    if (int rc = check_run(h, scene, ordinals, payload, n, 4)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    if (!n) return run_device(h, nullptr, nullptr, 0, result);
    // the payload first: it is read as float4
    if (int rc = ensure(h->stream, h->staging, n * (64 + 4))) return rc;
    float4 *dpay = (float4 *)h->staging.mem;
    uint32_t *dord = (uint32_t *)((char *)h->staging.mem + n * 64);
    HIP_TRY(hipMemcpyAsync(dpay, payload, n * 64, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(dord, ordinals, n * 4, hipMemcpyHostToDevice, h->stream));
    return run_device(h, dord, dpay, (uint32_t)n, result);
}

}  // extern "C"
