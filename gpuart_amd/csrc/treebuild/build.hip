// build.hip — libgpuart_build.so (gfx950): the tree of an uploaded scene rebuilt on the device in Morton order, as include/gpuart_build.h
// states it, and the cost measure of a tree. Built without flushing fp32 denormals and without contraction, so that NumPy float32
// (tests/build_ref.py) restates the keys and the boxes exactly. The topology is Karras' parallel construction (every interior node
// finds its range and split from the sorted keys alone); the box pass is the refit's (refit/box_pass.h). DESIGN.md "Rebuild" describes
// the launches; nothing is handed between workgroups inside a hand-written launch.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "../image/image_lib.h"
#include "../refit/box_pass.h"
#include "gpuart_build.h"

namespace {

const char LIB[] = "build";

constexpr uint32_t MAX_LEVELS = GPUART_BUILD_MAX_LEVELS;
constexpr uint32_t CHILD_LEAF = 0x80000000u;  ///< a child code: this bit | leaf index, or an interior node's index
constexpr uint32_t PARENT_LOWER = 0x80000000u;  ///< a parent link: this bit when the node is its parent's lower child
constexpr uint32_t COST_ITEMS = 8;  ///< records per thread of the cost kernel

/// What the build leaves for the host beside the refit's Status.
struct Extra {
    uint32_t root_ref;            ///< when the root is a leaf
    uint32_t too_deep;            ///< a node below MAX_LEVELS (cannot happen: 63 + 32 bits of key)
    uint32_t hist[MAX_LEVELS];    ///< records per level
    uint32_t cursor[MAX_LEVELS];  ///< where the next record of a level goes in the per-level lists
};

// 1. One thread per primitive: its 63-bit key from its box and the root box, and its ordinal as the sort's value.
struct Box3 { float lo[3], hi[3]; };

__global__ void __launch_bounds__(256) k_bd_keys(const float *pbox, uint32_t n, Box3 root, uint64_t *keys, uint32_t *vals) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *b = pbox + 6 * (size_t)i;
    keys[i] = tree_rule::morton_key(b, b + 3, root.lo, root.hi);
    vals[i] = i;
}

// 3. One thread per new position: the primitive's record and box moved there; word 3 of the first quad says the type and, on a leaf's
// first primitive, the leaf's count.
__global__ void __launch_bounds__(256) k_bd_permute(const float4 *src, const float *src_box, const uint32_t *new_to_old, uint32_t n, float4 *dst,
                                                    float *dst_box) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t old = new_to_old[p];
    const float4 *s = src + 3 * (size_t)old;
    float4 r0 = s[0];
    const uint32_t type = __float_as_uint(r0.w) & 3u;
    const uint32_t cnt = (p & 1u) ? 0u : (p + 1u < n ? 2u : 1u);
    r0.w = __uint_as_float(type | cnt << 2);
    float4 *d = dst + 3 * (size_t)p;
    d[0] = r0; d[1] = s[1]; d[2] = s[2];
    const float *sb = src_box + 6 * (size_t)old;
    float *db = dst_box + 6 * (size_t)p;
    for (int k = 0; k < 6; k++) db[k] = sb[k];
}

/// delta(i, j) over the m leaf keys (leaf j's key is that of position 2j); -1 outside. Never asked for j == i (k_bd_hierarchy).
RF_FN int delta(const uint64_t *keys, uint32_t m, uint32_t i, int64_t j) {
    if (j < 0 || j >= (int64_t)m) return -1;
    return tree_rule::key_delta(keys[2 * (size_t)i], keys[2 * (size_t)j], i, (uint32_t)j);
}

// 4. One thread per interior node i (the node whose range begins or ends at leaf i; the root is node 0): its range, split and children,
// and the parent link of each interior child — slots no other thread writes. Every j that delta is asked for differs from i: the
// neighbours i +- 1, i + (a step >= 1) x d while searching the far end and the split, and the far end itself, l >= 1 steps away
// (delta(i, i + d) > dmin by the choice of d).
__global__ void __launch_bounds__(256) k_bd_hierarchy(const uint64_t *keys, uint32_t m, uint32_t *lower, uint32_t *upper, uint32_t *first, uint32_t *parent) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i + 1 >= m) return;
    const int d = delta(keys, m, i, (int64_t)i + 1) > delta(keys, m, i, (int64_t)i - 1) ? 1 : -1;
    const int dmin = delta(keys, m, i, (int64_t)i - d);
    int64_t lmax = 2;
    while (delta(keys, m, i, (int64_t)i + lmax * d) > dmin) lmax *= 2;
    int64_t l = 0;
    for (int64_t t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, m, i, (int64_t)i + (l + t) * d) > dmin) l += t;
    const int64_t j = (int64_t)i + l * d;
    const int dnode = delta(keys, m, i, j);
    int64_t s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, m, i, (int64_t)i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int64_t g = (int64_t)i + s * d + (d < 0 ? -1 : 0);
    const int64_t a = d > 0 ? (int64_t)i : j, b = d > 0 ? j : (int64_t)i;
    const bool lo_leaf = a == g, hi_leaf = b == g + 1;
    lower[i] = (uint32_t)g | (lo_leaf ? CHILD_LEAF : 0u);
    upper[i] = (uint32_t)(g + 1) | (hi_leaf ? CHILD_LEAF : 0u);
    first[i] = (uint32_t)a;
    if (!lo_leaf) parent[g] = i | PARENT_LOWER;
    if (!hi_leaf) parent[g + 1] = i;
    if (i == 0) parent[0] = 0;
}

// 5. One thread per interior node: up its parent links to the root, counting its depth and the descents that went to a lower child.
// Its pre-order record index is the first leaf of its range + those descents: before it in pre-order lie its ancestors and the subtrees
// hanging off its path on the lower side, which hold all the leaves before its range and one record fewer than leaves each.
// The per-level histogram is counted in LDS first: a workgroup adds to each level's global counter once, not once per node (a few
// dozen addresses would take every node's atomic in turn: 1.8 of the 4.1 ms of an 871 k build, profiles/build.txt).
__global__ void __launch_bounds__(256) k_bd_number(const uint32_t *parent, const uint32_t *first, uint32_t m, uint32_t *rec, uint32_t *depth, Extra *ex) {
    __shared__ uint32_t hist[MAX_LEVELS];
    if (threadIdx.x < MAX_LEVELS) hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i + 1 < m) {
        uint32_t d = 0, low = 0;
        for (uint32_t c = i; c != 0 && d <= MAX_LEVELS; d++) {
            const uint32_t p = parent[c];
            low += p >> 31;
            c = p & ~PARENT_LOWER;
        }
        rec[i] = first[i] + low;
        depth[i] = d;
        if (d >= MAX_LEVELS) atomicOr(&ex->too_deep, 1u);
        else atomicAdd(&hist[d], 1u);
    }
    __syncthreads();
    if (threadIdx.x < MAX_LEVELS && hist[threadIdx.x]) atomicAdd(&ex->hist[threadIdx.x], hist[threadIdx.x]);
}

/// The per-level lists' starts, from the histogram (one thread: at most MAX_LEVELS additions).
__global__ void k_bd_offsets(Extra *ex) {
    if (blockIdx.x || threadIdx.x) return;
    uint32_t at = 0;
    for (uint32_t l = 0; l < MAX_LEVELS; l++) { ex->cursor[l] = at; at += ex->hist[l]; }
}

/// The ref of leaf j: one or two primitives, all triangles or not. The last line is tree_rule::leaf_ref(p, two ? 2 : 1, tris) written
/// out with its constants (see there).
RF_FN uint32_t leaf_ref(const float4 *prims, uint32_t n, uint32_t j) {
    const uint32_t p = 2u * j;
    const bool two = p + 1u < n;
    bool tris = (__float_as_uint(prims[3 * (size_t)p].w) & 3u) == (uint32_t)prim_rule::TRIANGLE;
    if (two) tris = tris && (__float_as_uint(prims[3 * (size_t)p + 3].w) & 3u) == (uint32_t)prim_rule::TRIANGLE;
    return REF_LEAF | p | (tris ? tree_rule::REF_TRIS : tree_rule::REF_SMALL) | (two ? tree_rule::REF_TWO : 0u);
}

// 6. One thread per interior node: the fourth words of its record — the two refs, the mark and the pad (the box pass writes the other
// twelve) — and its record index into its level's list. A workgroup takes its share of each level's list with one atomic per level
// (its nodes rank themselves in LDS first); the order within a level is whatever the atomics make it, and nothing depends on it.
__global__ void __launch_bounds__(256) k_bd_emit(const uint32_t *lower, const uint32_t *upper, const uint32_t *rec, const uint32_t *depth, uint32_t m,
                                                 const float4 *prims, uint32_t n, uint32_t top_depth, float4 *recs, uint32_t *order, Extra *ex) {
    __shared__ uint32_t count[MAX_LEVELS], base[MAX_LEVELS];
    if (threadIdx.x < MAX_LEVELS) count[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i + 1 < m && !ex->too_deep;  // (too_deep was written by the launch before this one: the same for every thread)
    uint32_t r = 0, d = 0, rank = 0;
    if (live) {
        const uint32_t lo = lower[i], hi = upper[i];
        r = rec[i];
        d = depth[i];
        float *q = (float *)(recs + 4 * (size_t)r);
        q[3] = __uint_as_float(lo & CHILD_LEAF ? leaf_ref(prims, n, lo & ~CHILD_LEAF) : rec[lo]);
        q[7] = __uint_as_float(hi & CHILD_LEAF ? leaf_ref(prims, n, hi & ~CHILD_LEAF) : rec[hi]);
        q[11] = __uint_as_float(d < top_depth ? 1u : 0u);
        q[15] = 0.0f;
        rank = atomicAdd(&count[d], 1u);
    }
    __syncthreads();
    if (threadIdx.x < MAX_LEVELS && count[threadIdx.x]) base[threadIdx.x] = atomicAdd(&ex->cursor[threadIdx.x], count[threadIdx.x]);
    __syncthreads();
    if (live) order[base[d] + rank] = r;
}

__global__ void k_bd_root_leaf(const float4 *prims, uint32_t n, Extra *ex) {
    if (blockIdx.x || threadIdx.x) return;
    ex->root_ref = leaf_ref(prims, n, 0);
}

/// Half the area of a box, in fp64 from its fp32 planes.
RF_FN double half_area(float4 lo, float4 hi) {
    const double x = (double)hi.x - (double)lo.x, y = (double)hi.y - (double)lo.y, z = (double)hi.z - (double)lo.z;
    return x * y + y * z + z * x;
}

/// Block b sums records [b * 256 * COST_ITEMS, ...): every thread its COST_ITEMS consecutive records in order, then a tree over the
/// block's 256 sums in LDS — a fixed order, so partial[b] depends on nothing but the records.
__global__ void __launch_bounds__(256) k_bd_cost(const float4 *recs, uint32_t n_recs, double *partial) {
    __shared__ double sum[256];
    const size_t base = ((size_t)blockIdx.x * 256u + threadIdx.x) * COST_ITEMS;
    double s = 0.0;
    for (uint32_t k = 0; k < COST_ITEMS; k++) {
        const size_t r = base + k;
        if (r < n_recs) {
            const float4 *q = recs + 4 * r;
            s += half_area(q[0], q[1]) + half_area(q[2], q[3]);
        }
    }
    sum[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t w = 128; w >= 1; w >>= 1) {
        if (threadIdx.x < w) sum[threadIdx.x] += sum[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = sum[0];
}

}  // namespace

struct gpuart_build : ImageHandle {
    Status *status = nullptr;  ///< device: the box pass's
    Extra *extra = nullptr;    ///< device
    DeviceBuffer scratch;      ///< keys in and out, ordinals, the hierarchy's arrays, the per-level lists
    DeviceBuffer temp;         ///< the sort's
    DeviceBuffer partial;      ///< the cost's partial sums
    DeviceBuffer staging;      ///< run_host: the permutation
    hipEvent_t ev[8] = {};
    double step_ms[7] = {0, 0, 0, 0, 0, 0, 0};
};

extern "C" {

const char *gpuart_build_last_error(void) { return g_last_error.c_str(); }

int gpuart_build_create(int device, gpuart_build **out) {
    if (int rc = create_handle(LIB, device, out)) return rc;
    gpuart_build *h = *out;
    *out = nullptr;
    hipError_t e = hipMalloc((void **)&h->status, sizeof(Status));
    if (e == hipSuccess) e = hipMalloc((void **)&h->extra, sizeof(Extra));
    for (int k = 0; k < 8 && e == hipSuccess; k++) e = hipEventCreate(&h->ev[k]);
    if (e != hipSuccess) {
        gpuart_build_destroy(h);
        return fail(GPUART_HIP_ERR_DEVICE, std::string("build: allocating the status: ") + hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

int gpuart_build_destroy(gpuart_build *h) {
    if (!h) return 0;
    destroy_handle(h, {h->status, h->extra, h->scratch.mem, h->temp.mem, h->partial.mem, h->staging.mem});
    for (hipEvent_t e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

int gpuart_build_finish(gpuart_build *h) { return finish_handle(LIB, h); }

int gpuart_build_step_ms(gpuart_build *h, double ms[7]) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!ms) return fail(GPUART_HIP_ERR_ARG, "build: ms is NULL");
    memcpy(ms, h->step_ms, sizeof h->step_ms);
    return 0;
}

int gpuart_build_run(gpuart_build *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_build_result *result) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!src) return fail(GPUART_HIP_ERR_ARG, "build: src is NULL");
    if (int rc = check_descriptor(src, LIB, "src", "rebuilt")) return rc;
    if (misaligned({src->recs, src->prims}, 16) || misaligned({src->prim_boxes}, 4)) return fail(GPUART_HIP_ERR_ARG, "build: src: misaligned arrays");
    if (!dst) return fail(GPUART_HIP_ERR_ARG, "build: dst is NULL");
    if (dst->layout != 1) return fail(GPUART_HIP_ERR_ARG, "build: dst: unknown layout " + std::to_string(dst->layout));
    const size_t n = src->n_prims, m = (n + 1) / 2, n_recs = m - 1;
    if (!tree_rule::box_ok(src->root_min, src->root_max)) return fail(GPUART_HIP_ERR_ARG, "build: the root box is not finite and ordered");
    if (!new_to_old || misaligned({new_to_old}, 4)) return fail(GPUART_HIP_ERR_ARG, "build: new_to_old is NULL or misaligned");
    if (!dst->prims || !dst->prim_boxes || (n_recs && !dst->recs) || misaligned({dst->recs, dst->prims}, 16) || misaligned({dst->prim_boxes}, 4))
        return fail(GPUART_HIP_ERR_ARG, "build: dst's arrays are NULL or misaligned");
    if (dst->n_prims < n || dst->n_recs < n_recs)
        return fail(GPUART_HIP_ERR_ARG, "build: dst is too small: " + std::to_string(dst->n_recs) + " records and " + std::to_string(dst->n_prims) +
                                            " primitives for " + std::to_string(n_recs) + " and " + std::to_string(n));
    const struct { const void *p; size_t bytes; } S[3] = {{src->recs, src->n_recs * 64}, {src->prims, n * 48}, {src->prim_boxes, n * 24}},
                                                  D[4] = {{dst->recs, n_recs * 64}, {dst->prims, n * 48}, {dst->prim_boxes, n * 24}, {new_to_old, n * 4}};
    for (const auto &s : S)
        for (const auto &d : D)
            if (s.bytes && d.bytes && overlaps(s.p, s.bytes, d.p, d.bytes)) return fail(GPUART_HIP_ERR_ARG, "build: dst's arrays alias src's");
    for (int a = 0; a < 4; a++)
        for (int b = a + 1; b < 4; b++)
            if (D[a].bytes && D[b].bytes && overlaps(D[a].p, D[a].bytes, D[b].p, D[b].bytes)) return fail(GPUART_HIP_ERR_ARG, "build: dst's arrays overlap");
    HIP_TRY(hipSetDevice(h->device));
    if (n == 1) {  // an empty scene keeps one dummy record, whose count is 0 (converter.h)
        uint32_t word = 0;
        HIP_TRY(hipMemcpy(&word, (const char *)src->prims + 12, 4, hipMemcpyDeviceToHost));
        if ((word >> 2) == 0) return fail(GPUART_HIP_ERR_ARG, "build: src: an empty scene is not rebuilt");
    }

    // scratch: keys in, keys out (8 bytes each), then the 4-byte arrays
    const size_t N8 = (n + 1) & ~(size_t)1, M4 = (m + 3) & ~(size_t)3;
    if (int rc = ensure(h->stream, h->scratch, 16 * N8 + 4 * N8 + 7 * 4 * M4)) return rc;
    uint64_t *keys_in = (uint64_t *)h->scratch.mem, *keys = keys_in + N8;
    uint32_t *vals_in = (uint32_t *)(keys + N8);
    uint32_t *lower = vals_in + N8, *upper = lower + M4, *first = upper + M4, *parent = first + M4, *rec = parent + M4, *depth = rec + M4, *order = depth + M4;
    size_t temp_bytes = 0;
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, keys_in, keys, vals_in, new_to_old, n, 0, 63, h->stream));
    if (int rc = ensure(h->stream, h->temp, temp_bytes + 16)) return rc;

    const float4 *sprims = (const float4 *)src->prims;
    float4 *drecs = (float4 *)dst->recs, *dprims = (float4 *)dst->prims;
    float *dbox = (float *)dst->prim_boxes;
    uint32_t top_depth = 0;
    if (const char *e = getenv("GPUART_HIP_TOP_DEPTH")) top_depth = (uint32_t)atoi(e);
    Box3 root;
    memcpy(root.lo, src->root_min, 12); memcpy(root.hi, src->root_max, 12);
    const uint32_t nb = (uint32_t)((n + 255) / 256), mb = (uint32_t)((m - 1 + 255) / 256);
    int at = 0;
    const auto mark = [&] { return hipEventRecord(h->ev[at++], h->stream); };

    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(Status), h->stream));
    HIP_TRY(hipMemsetAsync(h->extra, 0, sizeof(Extra), h->stream));
    HIP_TRY(mark());
    k_bd_keys<<<nb, 256, 0, h->stream>>>((const float *)src->prim_boxes, (uint32_t)n, root, keys_in, vals_in);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark());
    HIP_TRY(rocprim::radix_sort_pairs(h->temp.mem, temp_bytes, keys_in, keys, vals_in, new_to_old, n, 0, 63, h->stream));
    HIP_TRY(mark());
    k_bd_permute<<<nb, 256, 0, h->stream>>>(sprims, (const float *)src->prim_boxes, new_to_old, (uint32_t)n, dprims, dbox);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark());
    if (n_recs) {
        k_bd_hierarchy<<<mb, 256, 0, h->stream>>>(keys, (uint32_t)m, lower, upper, first, parent);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(mark());
    if (n_recs) {
        k_bd_number<<<mb, 256, 0, h->stream>>>(parent, first, (uint32_t)m, rec, depth, h->extra);
        HIP_TRY(hipGetLastError());
        k_bd_offsets<<<1, 64, 0, h->stream>>>(h->extra);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(mark());
    if (n_recs) {
        k_bd_emit<<<mb, 256, 0, h->stream>>>(lower, upper, rec, depth, (uint32_t)m, dprims, (uint32_t)n, top_depth, drecs, order, h->extra);
    } else {
        k_bd_root_leaf<<<1, 64, 0, h->stream>>>(dprims, (uint32_t)n, h->extra);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark());
    // the per-level counts, once: they size the level launches
    Extra ex;
    HIP_TRY(hipMemcpyAsync(&ex, h->extra, sizeof ex, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (ex.too_deep) return fail(GPUART_HIP_ERR_DEVICE, "build: a node below level " + std::to_string(MAX_LEVELS));
    uint32_t levels = 0;
    std::vector<uint32_t> start(MAX_LEVELS + 1, 0);
    for (uint32_t l = 0; l < MAX_LEVELS; l++) {
        start[l + 1] = start[l] + ex.hist[l];
        if (ex.hist[l]) levels = l + 1;
    }
    if (start[MAX_LEVELS] != n_recs) return fail(GPUART_HIP_ERR_DEVICE, "build: the levels hold " + std::to_string(start[MAX_LEVELS]) + " records of " + std::to_string(n_recs));
    for (uint32_t l = levels; l-- > 0;) {  // deepest level first
        const uint32_t count = ex.hist[l];
        if (!count) return fail(GPUART_HIP_ERR_DEVICE, "build: an empty level above a filled one");
        k_rf_level<<<(2u * count + 255u) / 256u, 256, 0, h->stream>>>(order + start[l], count, drecs, dprims, dbox, h->status);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t root_ref = n_recs ? 0u : ex.root_ref;
    k_rf_root<<<1, 64, 0, h->stream>>>(drecs, dprims, dbox, root_ref, h->status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(mark());
    Status st;
    HIP_TRY(hipMemcpyAsync(&st, h->status, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < 7; k++) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[k], h->ev[k + 1]));
        h->step_ms[k] = ms;
    }
    if (result) {
        result->n_recs = n_recs;
        result->root_ref = root_ref;
        result->max_depth = n_recs ? levels : 0;  // the deepest node is a leaf, one below the deepest record
        result->subnormal = st.subnormal;
        result->levels = levels;
        memcpy(result->root_min, st.root_min, 12);
        memcpy(result->root_max, st.root_max, 12);
    }
    return 0;
}

int gpuart_build_run_host(gpuart_build *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_build_result *result) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!src || !new_to_old || !src->n_prims) return fail(GPUART_HIP_ERR_ARG, "build: src or new_to_old is NULL, or the scene is empty");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = ensure(h->stream, h->staging, src->n_prims * sizeof(uint32_t))) return rc;
    if (int rc = gpuart_build_run(h, src, dst, (uint32_t *)h->staging.mem, result)) return rc;
    HIP_TRY(hipMemcpyAsync(new_to_old, h->staging.mem, src->n_prims * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int gpuart_build_cost(gpuart_build *h, const gpuart_hip_scene *scene, double *cost) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!cost) return fail(GPUART_HIP_ERR_ARG, "build: cost is NULL");
    if (!scene || scene->layout != 1 || (scene->n_recs && !scene->recs) || scene->n_recs > REF_INDEX || misaligned({scene->recs}, 16))
        return fail(GPUART_HIP_ERR_ARG, "build: scene is NULL, of an unknown layout or its records are out of range");
    *cost = 0.0;
    const double x = (double)scene->root_max[0] - (double)scene->root_min[0], y = (double)scene->root_max[1] - (double)scene->root_min[1],
                 z = (double)scene->root_max[2] - (double)scene->root_min[2];
    const double root = x * y + y * z + z * x;
    if (!scene->n_recs || !(root > 0.0)) return 0;
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t blocks = (uint32_t)((scene->n_recs + 256 * COST_ITEMS - 1) / (256 * COST_ITEMS));
    if (int rc = ensure(h->stream, h->partial, blocks * sizeof(double))) return rc;
    k_bd_cost<<<blocks, 256, 0, h->stream>>>((const float4 *)scene->recs, (uint32_t)scene->n_recs, (double *)h->partial.mem);
    HIP_TRY(hipGetLastError());
    std::vector<double> part(blocks);
    HIP_TRY(hipMemcpyAsync(part.data(), h->partial.mem, blocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    double sum = 0.0;
    for (double p : part) sum += p;
    *cost = sum / root;
    return 0;
}

}  // extern "C"
