// build.hip — libgpuart_build.so (gfx950): the tree of an uploaded scene rebuilt on the device in Morton order, as include/gpuart_build.h
// states it, and the cost measure of a tree. Built without flushing fp32 denormals and without contraction, so that NumPy float32
// (tests/build_ref.py) restates the keys and the boxes exactly. The topology is Karras' parallel construction (every interior node
// finds its range and split from the sorted keys alone); the box pass is the refit's (refit/box_pass.h), the argument checks, the keys and
// their sort the tree libraries' (tree/tree_lib.h). DESIGN.md "Rebuild" describes the launches; nothing is handed between workgroups
// inside a hand-written launch.
#include <cmath>
#include <vector>

#include "../image/image_lib.h"
#define TREE_LIB_MORTON
#include "../tree/tree_lib.h"
#include "../refit/box_pass.h"
#include "gpuart_build.h"

namespace {

const char LIB[] = "build";

constexpr uint32_t MAX_LEVELS = GPUART_BUILD_MAX_LEVELS;
constexpr uint32_t CHILD_LEAF = 0x80000000u;  ///< a child code: this bit | leaf index, or an interior node's index
constexpr uint32_t COST_ITEMS = 8;  ///< records per thread of the cost kernel

/// What the build leaves for the host beside the refit's Status.
struct Extra {
    uint32_t root_ref;            ///< when the root is a leaf
    uint32_t too_deep;            ///< a node below MAX_LEVELS (cannot happen: 63 + 32 bits of key)
    uint32_t hist[MAX_LEVELS];    ///< records per level
    uint32_t cursor[MAX_LEVELS];  ///< where the next record of a level goes in the per-level lists
};

// 1, 2. The keys and their sort: tree_lib.h's morton_sort.
// 3. One thread per new position: the primitive's record and box moved there; word 3 of the first quad says the type and, on a leaf's
// first primitive, the leaf's count.
__global__ void __launch_bounds__(256) k_bd_permute(const float4 *src, const float *src_box, const uint32_t *new_to_old, uint32_t n, float4 *dst,
                                                    float *dst_box) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t old = new_to_old[p];
    const uint32_t cnt = (p & 1u) ? 0u : (p + 1u < n ? 2u : 1u);
    move_prim(src, src_box, old, cnt, dst, dst_box, p);
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
    StepTimer timer;           ///< keys, sort, permute, hierarchy, number, emit, boxes
};

extern "C" {

const char *gpuart_build_last_error(void) { return g_last_error.c_str(); }

int gpuart_build_create(int device, gpuart_build **out) {
    return create_tree_handle(LIB, device, out, gpuart_build_destroy, [](gpuart_build *h) {
        hipError_t e = hipMalloc((void **)&h->status, sizeof(Status));
        if (e == hipSuccess) e = hipMalloc((void **)&h->extra, sizeof(Extra));
        return e == hipSuccess ? h->timer.create(7) : e;
    });
}

int gpuart_build_destroy(gpuart_build *h) {
    if (!h) return 0;
    destroy_handle(h, {h->status, h->extra, h->scratch.mem, h->temp.mem, h->partial.mem, h->staging.mem});
    h->timer.destroy();
    delete h;
    return 0;
}

int gpuart_build_finish(gpuart_build *h) { return finish_handle(LIB, h); }

int gpuart_build_step_ms(gpuart_build *h, double ms[7]) { return step_ms(LIB, h, ms); }

int gpuart_build_run(gpuart_build *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_build_result *result) {
    uint32_t word[2];  // (of a root that is a leaf: the refs come from the permuted records here)
    if (int rc = check_build(LIB, h, src, dst, new_to_old, [](size_t n) { return (n + 1) / 2 - 1; }, word)) return rc;
    const size_t n = src->n_prims, m = (n + 1) / 2, n_recs = m - 1;

    // scratch: keys in, keys out (8 bytes each), then the 4-byte arrays
    const size_t N8 = (n + 1) & ~(size_t)1, M4 = (m + 3) & ~(size_t)3;
    if (int rc = ensure(h->stream, h->scratch, 16 * N8 + 4 * N8 + 7 * 4 * M4)) return rc;
    uint64_t *keys_in = (uint64_t *)h->scratch.mem, *keys = keys_in + N8;
    uint32_t *vals_in = (uint32_t *)(keys + N8);
    uint32_t *lower = vals_in + N8, *upper = lower + M4, *first = upper + M4, *parent = first + M4, *rec = parent + M4, *depth = rec + M4, *order = depth + M4;

    const float4 *sprims = (const float4 *)src->prims;
    float4 *drecs = (float4 *)dst->recs, *dprims = (float4 *)dst->prims;
    float *dbox = (float *)dst->prim_boxes;
    const uint32_t mb = blocks(m - 1);
    h->timer.start(h->stream);

    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(Status), h->stream));
    HIP_TRY(hipMemsetAsync(h->extra, 0, sizeof(Extra), h->stream));
    if (int rc = morton_sort(h->timer, h->temp, 0, src, keys_in, keys, vals_in, new_to_old)) return rc;
    k_bd_permute<<<blocks(n), 256, 0, h->stream>>>(sprims, (const float *)src->prim_boxes, new_to_old, (uint32_t)n, dprims, dbox);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->timer.mark());
    if (n_recs) {
        k_bd_hierarchy<<<mb, 256, 0, h->stream>>>(keys, (uint32_t)m, lower, upper, first, parent);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(h->timer.mark());
    if (n_recs) {
        k_bd_number<<<mb, 256, 0, h->stream>>>(parent, first, (uint32_t)m, rec, depth, h->extra);
        HIP_TRY(hipGetLastError());
        k_bd_offsets<<<1, 64, 0, h->stream>>>(h->extra);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(h->timer.mark());
    if (n_recs) {
        k_bd_emit<<<mb, 256, 0, h->stream>>>(lower, upper, rec, depth, (uint32_t)m, dprims, (uint32_t)n, top_depth(), drecs, order, h->extra);
    } else {
        k_bd_root_leaf<<<1, 64, 0, h->stream>>>(dprims, (uint32_t)n, h->extra);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->timer.mark());
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
    HIP_TRY(h->timer.mark());
    Status st;
    HIP_TRY(hipMemcpyAsync(&st, h->status, sizeof st, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (int rc = h->timer.read()) return rc;
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
    return run_staged(LIB, h, gpuart_build_run, src, dst, new_to_old, result);
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
