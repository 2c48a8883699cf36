// edit.hip — libgpuart_edit.so (gfx950): primitives of an uploaded scene removed and new ones appended on the device, as
// include/gpuart_edit.h states it. Built without flushing fp32 denormals and without contraction: an added triangle's edges are
// subtracted exactly as the host uploader does (csrc/hip/converter.h; refit/prim_pack.h restates it for the device) and
// tests/edit_ref.py restates in NumPy float32. DESIGN.md "Edit" describes the launches; nothing is handed between workgroups inside
// one, and the only atomic sets the status word.
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "../image/image_lib.h"
#include "../tree/tree_lib.h"
#include "../refit/prim_pack.h"
#include "gpuart_edit.h"

namespace {

const char LIB[] = "edit";

constexpr uint32_t ITEMS = 8;  ///< boxes per thread of the reduction's first launch

/// What the device sequence leaves for the host, in device memory; zero before a run. `refused`: tree_lib.h's refusal word.
struct Status {
    uint32_t refused;
    uint32_t type_mask;
    float root_min[3], root_max[3];
};

/// A workgroup's share of the reduction.
struct Partial {
    float lo[3], hi[3];
    uint32_t mask, pad;
};

// The reduction's order: per plane a total order on the numbers (no NaN reaches it), -0 below +0, so that any grouping gives the same bits.
__device__ __forceinline__ float min_plane(float a, float b) { return (b < a || (b == a && __float_as_uint(b) >> 31)) ? b : a; }
__device__ __forceinline__ float max_plane(float a, float b) { return (b > a || (b == a && !(__float_as_uint(b) >> 31))) ? b : a; }

__device__ __forceinline__ void merge(Partial &a, const Partial &b) {
    for (int k = 0; k < 3; k++) { a.lo[k] = min_plane(a.lo[k], b.lo[k]); a.hi[k] = max_plane(a.hi[k], b.hi[k]); }
    a.mask |= b.mask;
}

__device__ __forceinline__ Partial nothing() {
    Partial p;
    prim_rule::box_start(p.lo, p.hi);
    p.mask = 0; p.pad = 0;
    return p;
}

// 1. One thread per removal, then one per addition: ordinals strictly ascending and below n_old; a type within 3 and a payload inside
// the rule for it.
__global__ void __launch_bounds__(256) k_ed_validate(const uint32_t *remove, uint32_t n_remove, const uint32_t *types, const float4 *payload, uint32_t n_add,
                                                     uint32_t n_old, Status *st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_remove + n_add) return;
    uint32_t why = 0;
    if (i < n_remove) {
        const uint32_t p = remove[i];
        if (i > 0 && !(remove[i - 1] < p)) why = WHY_ORDER;
        else if (p >= n_old) why = WHY_RANGE;
    } else {
        const uint32_t k = i - n_remove, type = types[k];
        float d[prim_rule::PAYLOAD];
        load_payload(payload, k, d);
        if (type > 3u || !prim_rule::prim_ok(type, d)) why = WHY_RULE;
    }
    if (why) refuse(&st->refused, i, why);
}

// 2. One thread per removal: its primitive's keep flag cleared (the flags were set to 1 by a fill before this launch). An ordinal out
// of range writes nothing; validation has refused it.
__global__ void __launch_bounds__(256) k_ed_flags(const uint32_t *remove, uint32_t n_remove, uint32_t n_old, uint32_t *keep) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_remove) return;
    const uint32_t p = remove[i];
    if (p < n_old) keep[p] = 0;
}

// 4. One thread per old primitive, after the exclusive scan of the flags: a survivor's record (word 3 of the first quad: the bare type,
// `count` above it) and box go to its place in the edited list, and source says where it came from.
__global__ void __launch_bounds__(256) k_ed_compact(const float4 *src, const float *src_box, const uint32_t *keep, const uint32_t *pos, uint32_t n_old,
                                                    uint32_t n_keep, uint32_t count, float4 *dst, float *dst_box, int32_t *source, const Status *st) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_old || st->refused || !keep[i]) return;
    const uint32_t q = pos[i];
    if (q >= n_keep) return;  // (cannot happen once validation passed: the removals are distinct and in range)
    move_prim(src, src_box, i, count, dst, dst_box, q);
    source[q] = (int32_t)i;
}

// 5. One thread per addition: its record by the uploader's arithmetic and its constructor's box, behind the survivors.
__global__ void __launch_bounds__(256) k_ed_append(const uint32_t *types, const float4 *payload, uint32_t n_add, uint32_t n_old, uint32_t n_keep, uint32_t count,
                                                   float4 *dst, float *dst_box, int32_t *source, const Status *st) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n_add || st->refused) return;
    const uint32_t type = types[k] & 3u;
    float d[prim_rule::PAYLOAD];
    load_payload(payload, k, d);
    float4 r[3];
    pack_prim(type, d, __uint_as_float(type | count << 2), r);
    const size_t q = (size_t)n_keep + k;
    float4 *rec = dst + 3 * q;
    rec[0] = r[0]; rec[1] = r[1]; rec[2] = r[2];
    float lo[3], hi[3];
    prim_rule::prim_box(type, d, lo, hi);
    float *b = dst_box + 6 * q;
    for (int a = 0; a < 3; a++) { b[a] = lo[a]; b[3 + a] = hi[a]; }
    source[q] = (int32_t)(n_old + k);
}

/// The workgroup's 256 partial results folded into thread 0's.
__device__ __forceinline__ Partial block_fold(Partial mine) {
    __shared__ Partial sh[256];
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            Partial a = sh[threadIdx.x];
            merge(a, sh[threadIdx.x + w]);
            sh[threadIdx.x] = a;
        }
        __syncthreads();
    }
    return sh[0];
}

// 6a. A workgroup folds 256 x ITEMS boxes and types of the edited list into one partial result.
__global__ void __launch_bounds__(256) k_ed_reduce(const float4 *prims, const float *pbox, uint32_t n, Partial *partial, const Status *st) {
    if (st->refused) return;
    Partial mine = nothing();
    const size_t first = (size_t)blockIdx.x * 256u * ITEMS;
    for (uint32_t t = 0; t < ITEMS; t++) {
        const size_t q = first + (size_t)t * 256u + threadIdx.x;
        if (q < n) {
            Partial p;
            const float *b = pbox + 6 * q;
            for (int k = 0; k < 3; k++) { p.lo[k] = b[k]; p.hi[k] = b[3 + k]; }
            p.mask = 1u << (__float_as_uint(prims[3 * q].w) & 3u);
            merge(mine, p);
        }
    }
    const Partial all = block_fold(mine);
    if (threadIdx.x == 0) partial[blockIdx.x] = all;
}

// 6b. One workgroup folds the partial results into the status.
__global__ void __launch_bounds__(256) k_ed_root(const Partial *partial, uint32_t count, Status *st) {
    if (st->refused) return;
    Partial mine = nothing();
    for (uint32_t q = threadIdx.x; q < count; q += 256u) merge(mine, partial[q]);
    const Partial all = block_fold(mine);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 3; k++) { st->root_min[k] = all.lo[k]; st->root_max[k] = all.hi[k]; }
        st->type_mask = all.mask;
    }
}

__global__ void __launch_bounds__(256) k_ed_compose(const int32_t *source, const uint32_t *perm, uint32_t n, int32_t *out) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t q = perm[p];
    out[p] = q < n ? source[q] : -1;
}

}  // namespace

struct gpuart_edit : ImageHandle {
    Status *status = nullptr;  ///< device
    DeviceBuffer prims, boxes; ///< the edited list: what `edited` describes
    DeviceBuffer scratch;      ///< keep flags, their scan, the partial results
    DeviceBuffer temp;         ///< the scan's
    DeviceBuffer staging;      ///< run_host: payload, removals, types, source
    StepTimer timer;           ///< validate and flags, scan, compact and append, reduce
};

namespace {

int check_run(gpuart_edit *h, const gpuart_hip_scene *src, const void *remove, size_t n_remove, const void *types, const void *payload, size_t n_add,
              const void *source, const gpuart_hip_scene *edited, size_t payload_align) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!src || !edited) return fail(GPUART_HIP_ERR_ARG, "edit: src or edited is NULL");
    if (int rc = check_descriptor(src, LIB, "src", "edited", false)) return rc;
    if (misaligned({src->prims}, 16) || misaligned({src->prim_boxes}, 4)) return fail(GPUART_HIP_ERR_ARG, "edit: src: misaligned arrays");
    if (n_remove > src->n_prims) return fail(GPUART_HIP_ERR_ARG, "edit: more removals (" + std::to_string(n_remove) + ") than primitives (" + std::to_string(src->n_prims) + ")");
    if (n_add >= GPUART_EDIT_MAX_PRIMS) return fail(GPUART_HIP_ERR_ARG, "edit: too many additions");
    const size_t n_new = src->n_prims - n_remove + n_add;
    if (!n_new) return fail(GPUART_HIP_ERR_ARG, "edit: the edit leaves no primitive (an empty scene is uploaded, not edited)");
    if (n_new >= GPUART_EDIT_MAX_PRIMS) return fail(GPUART_HIP_ERR_ARG, "edit: too many primitives: " + std::to_string(n_new));
    if ((n_remove && !remove) || (n_add && (!types || !payload)) || !source) return fail(GPUART_HIP_ERR_ARG, "edit: remove, add_types, add_payload or source is NULL");
    if (misaligned({remove, types, source}, 4) || misaligned({payload}, payload_align))
        return fail(GPUART_HIP_ERR_ARG, "edit: misaligned pointer (remove, add_types and source need 4 bytes, add_payload " + std::to_string(payload_align) + ")");
    return 0;
}

/// The device sequence on lists in device memory, and the read-back.
int run_device(gpuart_edit *h, const gpuart_hip_scene *src, const uint32_t *remove, uint32_t n_remove, const uint32_t *types, const float4 *payload,
               uint32_t n_add, int32_t *source, gpuart_hip_scene *edited, gpuart_edit_result *result) {
    const uint32_t n_old = (uint32_t)src->n_prims, n_keep = n_old - n_remove, n_new = n_keep + n_add;
    const struct { const void *p; size_t bytes; } S[2] = {{src->prims, (size_t)n_old * 48}, {src->prim_boxes, (size_t)n_old * 24}};
    for (const auto &s : S)
        if (overlaps(s.p, s.bytes, source, (size_t)n_new * 4)) return fail(GPUART_HIP_ERR_ARG, "edit: source aliases src's arrays");
    // (the same slack past the end as an upload's arrays)
    if (int rc = ensure(h->stream, h->prims, ((size_t)n_new * 3 + 4) * sizeof(float4))) return rc;
    if (int rc = ensure(h->stream, h->boxes, (size_t)n_new * 24 + 16)) return rc;
    const uint32_t parts = (n_new + 256u * ITEMS - 1) / (256u * ITEMS);
    const size_t N = ((size_t)n_old + 3) & ~(size_t)3;
    if (int rc = ensure(h->stream, h->scratch, 2 * 4 * N + (size_t)parts * sizeof(Partial))) return rc;
    uint32_t *keep = (uint32_t *)h->scratch.mem, *pos = keep + N;
    Partial *partial = (Partial *)(pos + N);
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, keep, pos, 0u, (size_t)n_old, rocprim::plus<uint32_t>(), h->stream));
    if (int rc = ensure(h->stream, h->temp, scan_bytes + 16)) return rc;
    for (const DeviceBuffer *b : {&h->prims, &h->boxes})
        for (const auto &s : S)
            if (overlaps(s.p, s.bytes, b->mem, b->bytes)) return fail(GPUART_HIP_ERR_ARG, "edit: src's arrays are the handle's own staging arrays");

    const uint32_t count = n_new == 1 ? 1u : 0u;  // a list of one primitive is a leaf of one
    float4 *dprims = (float4 *)h->prims.mem;
    float *dbox = (float *)h->boxes.mem;
    h->timer.start(h->stream);

    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(Status), h->stream));
    HIP_TRY(h->timer.mark());
    if (n_remove + n_add) {
        k_ed_validate<<<blocks((size_t)n_remove + n_add), 256, 0, h->stream>>>(remove, n_remove, types, payload, n_add, n_old, h->status);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)keep, 1, n_old, h->stream));
    if (n_remove) {
        k_ed_flags<<<blocks(n_remove), 256, 0, h->stream>>>(remove, n_remove, n_old, keep);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(h->timer.mark());
    HIP_TRY(rocprim::exclusive_scan(h->temp.mem, scan_bytes, keep, pos, 0u, (size_t)n_old, rocprim::plus<uint32_t>(), h->stream));
    HIP_TRY(h->timer.mark());
    k_ed_compact<<<blocks(n_old), 256, 0, h->stream>>>((const float4 *)src->prims, (const float *)src->prim_boxes, keep, pos, n_old, n_keep, count, dprims, dbox,
                                                       source, h->status);
    HIP_TRY(hipGetLastError());
    if (n_add) {
        k_ed_append<<<blocks(n_add), 256, 0, h->stream>>>(types, payload, n_add, n_old, n_keep, count, dprims, dbox, source, h->status);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(h->timer.mark());
    k_ed_reduce<<<parts, 256, 0, h->stream>>>(dprims, dbox, n_new, partial, h->status);
    HIP_TRY(hipGetLastError());
    k_ed_root<<<1, 256, 0, h->stream>>>(partial, parts, h->status);
    HIP_TRY(hipGetLastError());
    // the slack behind the list ends in zeros, as behind an upload's
    HIP_TRY(hipMemsetAsync((char *)dprims + (size_t)n_new * 48, 0, 4 * sizeof(float4), h->stream));
    HIP_TRY(hipMemsetAsync((char *)dbox + (size_t)n_new * 24, 0, 16, h->stream));
    HIP_TRY(h->timer.mark());
    Status st;
    HIP_TRY(hipMemcpyAsync(&st, h->status, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (int rc = h->timer.read()) return rc;
    if (result) {
        memset(result, 0, sizeof *result);
        result->status = st.refused ? GPUART_HIP_ERR_ARG : 0;
        result->first_bad = st.refused ? refused_index(st.refused) : GPUART_EDIT_NONE;
        result->n_prims = st.refused ? 0 : n_new;
        result->type_mask = st.refused ? 0 : st.type_mask;
        if (!st.refused) { memcpy(result->root_min, st.root_min, 12); memcpy(result->root_max, st.root_max, 12); }
    }
    if (st.refused) {
        const char *why = refused_why(st.refused, "its type is above 3 or its payload is outside the primitive rule (a word that is not finite or beyond 2^20, a "
                                                  "negative radius or length, or a cone's derived constants that contradict its centres and radii)");
        const uint32_t i = refused_index(st.refused);
        return fail(GPUART_HIP_ERR_ARG, std::string("edit: ") + (i < n_remove ? "removal " + std::to_string(i) : "addition " + std::to_string(i - n_remove)) +
                                            " refused: " + why + "; nothing was edited");
    }
    memset(edited, 0, sizeof *edited);
    edited->layout = 1;
    edited->prims = dprims;
    edited->prim_boxes = dbox;
    edited->n_prims = n_new;
    edited->generation = src->generation;
    memcpy(edited->root_min, st.root_min, 12);
    memcpy(edited->root_max, st.root_max, 12);
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_edit_last_error(void) { return g_last_error.c_str(); }

int gpuart_edit_create(int device, gpuart_edit **out) {
    return create_tree_handle(LIB, device, out, gpuart_edit_destroy, [](gpuart_edit *h) {
        const hipError_t e = hipMalloc((void **)&h->status, sizeof(Status));
        return e == hipSuccess ? h->timer.create(4) : e;
    });
}

int gpuart_edit_destroy(gpuart_edit *h) {
    if (!h) return 0;
    destroy_handle(h, {h->status, h->prims.mem, h->boxes.mem, h->scratch.mem, h->temp.mem, h->staging.mem});
    h->timer.destroy();
    delete h;
    return 0;
}

int gpuart_edit_finish(gpuart_edit *h) { return finish_handle(LIB, h); }

int gpuart_edit_step_ms(gpuart_edit *h, double ms[4]) { return step_ms(LIB, h, ms); }

int gpuart_edit_run(gpuart_edit *h, const gpuart_hip_scene *src, const uint32_t *remove, size_t n_remove, const uint32_t *add_types,
                    const float *add_payload, size_t n_add, int32_t *source, gpuart_hip_scene *edited, gpuart_edit_result *result) {
    if (int rc = check_run(h, src, remove, n_remove, add_types, add_payload, n_add, source, edited, 16)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    return run_device(h, src, remove, (uint32_t)n_remove, add_types, (const float4 *)add_payload, (uint32_t)n_add, source, edited, result);
}

int gpuart_edit_run_host(gpuart_edit *h, const gpuart_hip_scene *src, const uint32_t *remove, size_t n_remove, const uint32_t *add_types,
                         const float *add_payload, size_t n_add, int32_t *source, gpuart_hip_scene *edited, gpuart_edit_result *result) {
    if (int rc = check_run(h, src, remove, n_remove, add_types, add_payload, n_add, source, edited, 4)) return rc;
    HIP_TRY(hipSetDevice(h->device));
    const size_t n_new = src->n_prims - n_remove + n_add;
    // the payload first: it is read as float4
    if (int rc = ensure(h->stream, h->staging, n_add * (64 + 4) + n_remove * 4 + n_new * 4 + 16)) return rc;
    float4 *dpay = (float4 *)h->staging.mem;
    uint32_t *dtypes = (uint32_t *)((char *)h->staging.mem + n_add * 64), *drem = dtypes + n_add;
    int32_t *dsource = (int32_t *)(drem + n_remove);
    if (n_add) {
        HIP_TRY(hipMemcpyAsync(dpay, add_payload, n_add * 64, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(dtypes, add_types, n_add * 4, hipMemcpyHostToDevice, h->stream));
    }
    if (n_remove) HIP_TRY(hipMemcpyAsync(drem, remove, n_remove * 4, hipMemcpyHostToDevice, h->stream));
    if (int rc = run_device(h, src, drem, (uint32_t)n_remove, dtypes, dpay, (uint32_t)n_add, dsource, edited, result)) return rc;
    HIP_TRY(hipMemcpyAsync(source, dsource, n_new * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int gpuart_edit_compose(gpuart_edit *h, const int32_t *source, const uint32_t *perm, size_t n, int32_t *out) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!n) return 0;
    if (!source || !perm || !out || misaligned({source, perm, out}, 4)) return fail(GPUART_HIP_ERR_ARG, "edit: source, perm or out is NULL or misaligned");
    if (n >= GPUART_EDIT_MAX_PRIMS) return fail(GPUART_HIP_ERR_ARG, "edit: too many primitives: " + std::to_string(n));
    if (overlaps(out, n * 4, source, n * 4) || overlaps(out, n * 4, perm, n * 4)) return fail(GPUART_HIP_ERR_ARG, "edit: out overlaps source or perm");
    HIP_TRY(hipSetDevice(h->device));
    k_ed_compose<<<blocks(n), 256, 0, h->stream>>>(source, perm, (uint32_t)n, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

}  // extern "C"
