// ploc.hip — libgpuart_ploc.so (gfx950): the tree of an uploaded scene rebuilt on the device by locally-ordered clustering, as
// include/gpuart_ploc.h states it. Built without flushing fp32 denormals and without contraction, so that NumPy float32
// (tests/ploc_ref.py) restates the distances and the boxes exactly. The keys are the Morton rule's (hip/tree_rule.h); the argument checks,
// the keys' kernel and their sort the tree libraries' (tree/tree_lib.h); the Status and the root's box the refit's (refit/box_pass.h). DESIGN.md "Clustered rebuild" describes the launches; nothing
// is handed between workgroups inside a launch, and atomics only count.
//
// A node has an id: the initial cluster of sorted position p is node p (one primitive), the k-th merge of the whole build makes node
// n + k (k from a scan of the iteration's new-node flags, on top of the merges of the iterations before). Per id: its box, its parent
// (with PARENT_LOWER when it is the lower child), the records and the primitives of its subtree; per merged node its two children.
#include <vector>

#include <rocprim/device/device_scan.hpp>

#include "../image/image_lib.h"
#define TREE_LIB_MORTON
#include "../tree/tree_lib.h"
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"  // box_pass.h's level kernel is not launched here: every box is computed when its node is made
#include "../refit/box_pass.h"
#pragma clang diagnostic pop
#include "gpuart_ploc.h"

namespace {

const char LIB[] = "ploc";

constexpr uint32_t RADIUS = GPUART_PLOC_RADIUS, MAX_ITERATIONS = GPUART_PLOC_MAX_ITERATIONS;
constexpr uint32_t BOX_STRIDE = 7;              ///< floats per staged box in LDS (6 and one of padding: an odd stride has no bank conflicts)

/// After an iteration: the clusters left and the merged nodes made so far. Iteration t reads state[t & 1] and writes state[(t + 1) & 1].
struct State { uint32_t c, nodes; };

/// What the build leaves for the host: the refit's Status (subnormal, the root's box) and the build's own.
struct Extra {
    Status st;
    State state[2];
    uint32_t depth;   ///< level of the deepest node
    uint32_t n_recs;  ///< records of the root's subtree
    uint32_t broken;  ///< a parent link that leads nowhere, or a position out of range (cannot happen)
};

// 1. The keys and their sort: tree_lib.h's morton_sort.
// 2. One thread per sorted position p: initial cluster p = node p, one primitive with that primitive's box.
__global__ void __launch_bounds__(256) k_pl_init(const float *pbox, const uint32_t *sorted, uint32_t n, float *nbox, uint32_t *parent, uint32_t *nrec,
                                                 uint32_t *npr, uint32_t *cnode, Extra *ex) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const float *s = pbox + 6 * (size_t)sorted[p];
    float *d = nbox + 6 * (size_t)p;
    for (int k = 0; k < 6; k++) d[k] = s[k];
    parent[p] = 0; nrec[p] = 0; npr[p] = 1; cnode[p] = p;
    if (p == 0) { ex->state[0].c = n; ex->state[0].nodes = 0; }
}

/// d(lower, upper): the half-area of the box of the cluster at the lower position folded with the other's.
RF_FN float distance(const float *a, const float *b) {
    float lo[3] = {a[0], a[1], a[2]}, hi[3] = {a[3], a[4], a[5]};
    prim_rule::box_fold(lo, hi, b, b + 3);
    const float x = hi[0] - lo[0], y = hi[1] - lo[1], z = hi[2] - lo[2];
    return (x * y + y * z) + z * x;
}

// 3. The hot kernel. A workgroup of 256 clusters stages their boxes and those of the RADIUS clusters on either side in LDS once; every
// thread then evaluates its <= 2 RADIUS distances from LDS and writes nn[i], the j that minimises (d(i, j), i xor j).
__global__ void __launch_bounds__(256) k_pl_nearest(const uint32_t *cnode, uint32_t c, const float *nbox, uint32_t *nn) {
    __shared__ float sb[(256 + 2 * RADIUS) * BOX_STRIDE];
    const int64_t first = (int64_t)blockIdx.x * 256 - (int64_t)RADIUS;  // the position staged in slot 0
    for (uint32_t s = threadIdx.x; s < 256 + 2 * RADIUS; s += 256) {
        const int64_t q = first + s;
        if (q >= 0 && q < (int64_t)c) {
            const float *b = nbox + 6 * (size_t)cnode[q];
            for (int k = 0; k < 6; k++) sb[s * BOX_STRIDE + k] = b[k];
        }
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c) return;
    const float *mine = sb + (threadIdx.x + RADIUS) * BOX_STRIDE;
    float best = __builtin_inff();
    uint32_t best_x = ~0u, best_j = i;
    for (int o = -(int)RADIUS; o <= (int)RADIUS; o++) {
        const int64_t j = (int64_t)i + o;
        if (o == 0 || j < 0 || j >= (int64_t)c) continue;
        const float *other = sb + (int)(threadIdx.x + RADIUS + o) * (int)BOX_STRIDE;
        const float d = o < 0 ? distance(other, mine) : distance(mine, other);
        const uint32_t x = i ^ (uint32_t)j;
        if (d < best || (d == best && x < best_x)) { best = d; best_x = x; best_j = (uint32_t)j; }
    }
    nn[i] = best_j;
}

// 4. One thread per cluster: is its nearest neighbour's nearest neighbour itself? The lower partner of a mutual pair makes a node (bit
// 32: counted by the scan's upper half), the upper partner leaves the array (bit 0 clear: the lower half counts the survivors).
__global__ void __launch_bounds__(256) k_pl_merge(const uint32_t *nn, uint32_t c, uint64_t *flags) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c) return;
    const uint32_t j = nn[i];
    const bool mutual = j < c && j != i && nn[j] == i;
    flags[i] = (mutual && j < i ? 0ull : 1ull) | (mutual && i < j ? 1ull << 32 : 0ull);
}

// 5. One thread per cluster, after the exclusive scan of the flags: a survivor goes to its place in the next array; the lower partner
// of a mutual pair first makes the merged node — children, box (the distance's fold), counts, and the children's parent links. The
// children's counts were written by earlier launches; nobody reads this launch's nodes before the next one.
__global__ void __launch_bounds__(256) k_pl_scatter(const uint32_t *cnode, const uint32_t *nn, const uint64_t *flags, const uint64_t *scan, uint32_t c,
                                                    uint32_t n, const State *was, State *now, float *nbox, uint32_t *lower, uint32_t *upper,
                                                    uint32_t *parent, uint32_t *nrec, uint32_t *npr, uint32_t *cnode_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= c) return;
    const uint64_t f = flags[i], s = scan[i];
    const uint32_t keep = (uint32_t)f & 1u, made = (uint32_t)(f >> 32), at = (uint32_t)s, k = was->nodes + (uint32_t)(s >> 32);
    if (i == c - 1) { now->c = at + keep; now->nodes = k + made; }
    if (!keep) return;
    uint32_t id = cnode[i];
    if (made && k + 1 < n) {  // (a tree of n primitives has at most n - 1 merged nodes: ids stay below 2n - 1)
        const uint32_t a = id, b = cnode[nn[i]];
        id = n + k;
        const float *ba = nbox + 6 * (size_t)a, *bb = nbox + 6 * (size_t)b;
        float lo[3] = {ba[0], ba[1], ba[2]}, hi[3] = {ba[3], ba[4], ba[5]};
        prim_rule::box_fold(lo, hi, bb, bb + 3);
        float *d = nbox + 6 * (size_t)id;
        for (int q = 0; q < 3; q++) { d[q] = lo[q]; d[3 + q] = hi[q]; }
        lower[k] = a; upper[k] = b;
        parent[a] = id | PARENT_LOWER; parent[b] = id; parent[id] = 0;
        const uint32_t prims = npr[a] + npr[b];
        npr[id] = prims;
        nrec[id] = prims == 2 ? 0u : 1u + nrec[a] + nrec[b];  // two single primitives make a leaf of two: no record
    }
    cnode_out[at] = id;
}

// 6. One thread per node (initial clusters and merged nodes): up its parent links to the root. Its pre-order record index is the sum
// over its ancestors of 1 + [it went to the upper child] x the records of the lower sibling's subtree; the position of its first
// primitive the sum of [went upper] x the primitives of the lower sibling's subtree; its depth the number of links. The deepest level
// is counted per workgroup in LDS first, then once per workgroup.
__global__ void __launch_bounds__(256) k_pl_number(uint32_t n, uint32_t total, uint32_t root, const uint32_t *parent, const uint32_t *lower, const uint32_t *nrec,
                                                   const uint32_t *npr, uint32_t *rec_of, uint32_t *first_of, uint32_t *depth_of, Extra *ex) {
    __shared__ uint32_t deepest;
    if (threadIdx.x == 0) deepest = 0;
    __syncthreads();
    const uint32_t id = blockIdx.x * 256u + threadIdx.x;
    if (id < n + total) {
        uint32_t rec = 0, first = 0, d = 0, cur = id;
        bool is_node = id >= n || n == 1;  // an initial cluster is a node of the tree (a leaf of one) unless its parent is a leaf of two
        while (cur != root) {
            const uint32_t p = parent[cur], par = p & ~PARENT_LOWER;
            if (par < n || par >= n + total || d > MAX_ITERATIONS) { atomicOr(&ex->broken, 1u); break; }
            if (cur == id && id < n) is_node = npr[par] > 2;
            if (!(p >> 31)) {
                const uint32_t sib = lower[par - n];
                rec += nrec[sib];
                first += npr[sib];
            }
            rec++; d++;
            cur = par;
        }
        rec_of[id] = rec; first_of[id] = first; depth_of[id] = d;
        if (is_node) atomicMax(&deepest, d);
        if (id == root) ex->n_recs = nrec[root];
    }
    __syncthreads();
    if (threadIdx.x == 0 && deepest) atomicMax(&ex->depth, deepest);
}

// 7. One thread per sorted position: the primitive's record and box moved to its place among the leaves in pre-order; word 3 of the
// first quad says the type and, on a leaf's first primitive, the leaf's count; new_to_old composed with the sort's.
__global__ void __launch_bounds__(256) k_pl_permute(const float4 *src, const float *src_box, const uint32_t *sorted, uint32_t n, const uint32_t *parent,
                                                    const uint32_t *npr, const uint32_t *first_of, float4 *dst, float *dst_box, uint32_t *new_to_old, Extra *ex) {
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const uint32_t at = first_of[p], old = sorted[p];
    if (at >= n) { atomicOr(&ex->broken, 1u); return; }
    uint32_t cnt = 1;
    if (n > 1) {
        const uint32_t link = parent[p];
        if (npr[link & ~PARENT_LOWER] == 2) cnt = link >> 31 ? 2u : 0u;
    }
    move_prim(src, src_box, old, cnt, dst, dst_box, at);
    new_to_old[at] = old;
}

/// The ref of child `c`: its record, or its leaf of one or two primitives (whose types the permuted records say).
RF_FN uint32_t child_ref(uint32_t c, const uint32_t *npr, const uint32_t *rec_of, const uint32_t *first_of, const float4 *prims) {
    const uint32_t cnt = npr[c];
    if (cnt > 2) return rec_of[c];
    const uint32_t first = first_of[c];
    bool tris = (__float_as_uint(prims[3 * (size_t)first].w) & 3u) == (uint32_t)prim_rule::TRIANGLE;
    if (cnt == 2) tris = tris && (__float_as_uint(prims[3 * (size_t)first + 3].w) & 3u) == (uint32_t)prim_rule::TRIANGLE;
    return tree_rule::leaf_ref(first, cnt, tris);
}

// 8. One thread per merged node that is no leaf of two: the sixteen words of its record — both children's boxes as the clustering
// carried them, their refs, the GPUART_HIP_TOP_DEPTH mark and the pad — and the planes' verdict into the status.
__global__ void __launch_bounds__(256) k_pl_emit(uint32_t n, uint32_t total, uint32_t room, const uint32_t *lower, const uint32_t *upper, const uint32_t *npr,
                                                 const uint32_t *rec_of, const uint32_t *first_of, const uint32_t *depth_of, const float *nbox, const float4 *prims,
                                                 uint32_t top_depth, float4 *recs, Extra *ex) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= total || npr[n + k] <= 2) return;
    const uint32_t r = rec_of[n + k], a = lower[k], b = upper[k];
    if (r >= room) { atomicOr(&ex->broken, 1u); return; }
    const float *ba = nbox + 6 * (size_t)a, *bb = nbox + 6 * (size_t)b;
    float4 *q = recs + 4 * (size_t)r;
    q[0] = make_float4(ba[0], ba[1], ba[2], __uint_as_float(child_ref(a, npr, rec_of, first_of, prims)));
    q[1] = make_float4(ba[3], ba[4], ba[5], __uint_as_float(child_ref(b, npr, rec_of, first_of, prims)));
    q[2] = make_float4(bb[0], bb[1], bb[2], __uint_as_float(depth_of[n + k] < top_depth ? 1u : 0u));
    q[3] = make_float4(bb[3], bb[4], bb[5], 0.0f);
    if (!planes_ok(ba, ba + 3) || !planes_ok(bb, bb + 3)) atomicOr(&ex->st.subnormal, 1u);
}

}  // namespace

struct gpuart_ploc : ImageHandle {
    Extra *extra = nullptr;  ///< device
    DeviceBuffer scratch;    ///< keys in and out, ordinals, the nodes' arrays, the cluster arrays, flags and their scan
    DeviceBuffer temp;       ///< the sort's and the scan's
    DeviceBuffer staging;    ///< run_host: the permutation
    StepTimer timer;         ///< reported as keys, sort, iterations (with the initial clusters), number, emit, permute
};

extern "C" {

const char *gpuart_ploc_last_error(void) { return g_last_error.c_str(); }

int gpuart_ploc_create(int device, gpuart_ploc **out) {
    return create_tree_handle(LIB, device, out, gpuart_ploc_destroy, [](gpuart_ploc *h) {
        const hipError_t e = hipMalloc((void **)&h->extra, sizeof(Extra));
        return e == hipSuccess ? h->timer.create(6) : e;
    });
}

int gpuart_ploc_destroy(gpuart_ploc *h) {
    if (!h) return 0;
    destroy_handle(h, {h->extra, h->scratch.mem, h->temp.mem, h->staging.mem});
    h->timer.destroy();
    delete h;
    return 0;
}

int gpuart_ploc_finish(gpuart_ploc *h) { return finish_handle(LIB, h); }

int gpuart_ploc_step_ms(gpuart_ploc *h, double ms[6]) { return step_ms(LIB, h, ms); }

int gpuart_ploc_run(gpuart_ploc *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_ploc_result *result) {
    uint32_t word[2];
    if (int rc = check_build(LIB, h, src, dst, new_to_old, [](size_t n) { return n - 1; }, word)) return rc;
    const size_t n = src->n_prims, room = n - 1;
    uint32_t root_ref = 0;
    if (n <= 2) {  // the root is a leaf: its ref from the primitives' type words
        const uint32_t tri = (uint32_t)prim_rule::TRIANGLE;
        root_ref = tree_rule::leaf_ref(0, (uint32_t)n, (word[0] & 3u) == tri && (n == 1 || (word[1] & 3u) == tri));
    }

    // scratch: the 8-byte arrays (keys in, keys out, flags, scan), the boxes of 2n nodes, then the 4-byte arrays
    const size_t N = (n + 3) & ~(size_t)3;
    if (int rc = ensure(h->stream, h->scratch, 4 * 8 * N + 24 * 2 * N + 4 * N * 19)) return rc;
    uint64_t *keys_in = (uint64_t *)h->scratch.mem, *keys = keys_in + N, *flags = keys + N, *scan = flags + N;
    float *nbox = (float *)(scan + N);
    uint32_t *vals_in = (uint32_t *)(nbox + 12 * N), *sorted = vals_in + N;
    uint32_t *parent = sorted + N, *nrec = parent + 2 * N, *npr = nrec + 2 * N, *rec_of = npr + 2 * N;
    uint32_t *lower = rec_of + 2 * N, *upper = lower + N;
    uint32_t *cnode[2] = {upper + N, upper + 2 * N};
    uint32_t *nn = cnode[1] + N, *first_of = nn + N, *depth_of = first_of + 2 * N;
    size_t scan_bytes = 0;  // (the scan shares the sort's temporary storage)
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, flags, scan, (uint64_t)0, n, rocprim::plus<uint64_t>(), h->stream));
    h->timer.start(h->stream);

    HIP_TRY(hipMemsetAsync(h->extra, 0, sizeof(Extra), h->stream));
    if (int rc = morton_sort(h->timer, h->temp, scan_bytes, src, keys_in, keys, vals_in, sorted)) return rc;
    k_pl_init<<<blocks(n), 256, 0, h->stream>>>((const float *)src->prim_boxes, sorted, (uint32_t)n, nbox, parent, nrec, npr, cnode[0], h->extra);
    HIP_TRY(hipGetLastError());
    State state = {(uint32_t)n, 0};
    uint32_t iterations = 0;
    while (state.c > 1) {
        if (iterations == MAX_ITERATIONS) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            return fail(GPUART_HIP_ERR_ARG, "ploc: the scene needs more than " + std::to_string(MAX_ITERATIONS) + " iterations");
        }
        const uint32_t c = state.c, t = iterations & 1u, g = blocks(c);
        k_pl_nearest<<<g, 256, 0, h->stream>>>(cnode[t], c, nbox, nn);
        HIP_TRY(hipGetLastError());
        k_pl_merge<<<g, 256, 0, h->stream>>>(nn, c, flags);
        HIP_TRY(hipGetLastError());
        size_t bytes = scan_bytes;
        HIP_TRY(rocprim::exclusive_scan(h->temp.mem, bytes, flags, scan, (uint64_t)0, c, rocprim::plus<uint64_t>(), h->stream));
        k_pl_scatter<<<g, 256, 0, h->stream>>>(cnode[t], nn, flags, scan, c, (uint32_t)n, &h->extra->state[t], &h->extra->state[t ^ 1u], nbox, lower, upper,
                                                 parent, nrec, npr, cnode[t ^ 1u]);
        HIP_TRY(hipGetLastError());
        // the new c sizes the next launches and ends the loop
        HIP_TRY(hipMemcpyAsync(&state, &h->extra->state[t ^ 1u], sizeof state, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        iterations++;
        if (state.c == 0 || state.c >= c || state.nodes >= n)
            return fail(GPUART_HIP_ERR_DEVICE, "ploc: an iteration left " + std::to_string(state.c) + " clusters of " + std::to_string(c));
    }
    HIP_TRY(h->timer.mark());
    const uint32_t total = state.nodes, root_id = n > 1 ? (uint32_t)n + total - 1 : 0u;  // the last iteration merges the last two clusters
    float4 *drecs = (float4 *)dst->recs, *dprims = (float4 *)dst->prims;
    float *dbox = (float *)dst->prim_boxes;
    k_pl_number<<<blocks(n + total), 256, 0, h->stream>>>((uint32_t)n, total, root_id, parent, lower, nrec, npr, rec_of, first_of, depth_of, h->extra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->timer.mark());
    k_pl_permute<<<blocks(n), 256, 0, h->stream>>>((const float4 *)src->prims, (const float *)src->prim_boxes, sorted, (uint32_t)n, parent, npr, first_of, dprims,
                                                    dbox, new_to_old, h->extra);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->timer.mark());
    if (total) {
        k_pl_emit<<<blocks(total), 256, 0, h->stream>>>((uint32_t)n, total, (uint32_t)room, lower, upper, npr, rec_of, first_of, depth_of, nbox, dprims, top_depth(),
                                                        drecs, h->extra);
        HIP_TRY(hipGetLastError());
    }
    k_rf_root<<<1, 64, 0, h->stream>>>(drecs, dprims, dbox, root_ref, &h->extra->st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(h->timer.mark());
    Extra ex;
    HIP_TRY(hipMemcpyAsync(&ex, h->extra, sizeof ex, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (ex.broken || ex.n_recs > room || (n > 2) != (ex.n_recs > 0)) return fail(GPUART_HIP_ERR_DEVICE, "ploc: the clustering left an inconsistent tree");
    if (ex.n_recs < room) {  // room was asked for n - 1 records: what lies beyond the tree's ends in zeros, as behind an upload's
        HIP_TRY(hipMemsetAsync((char *)dst->recs + (size_t)ex.n_recs * 64, 0, (room - ex.n_recs) * 64, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    const int from[6] = {0, 1, 2, 3, 5, 4};  // keys, sort, iterations (with the initial clusters), number, emit, permute
    if (int rc = h->timer.read(from)) return rc;
    if (result) {
        result->n_recs = ex.n_recs;
        result->root_ref = root_ref;
        result->max_depth = ex.depth;
        result->subnormal = ex.st.subnormal;
        result->iterations = iterations;
        memcpy(result->root_min, ex.st.root_min, 12);
        memcpy(result->root_max, ex.st.root_max, 12);
    }
    return 0;
}

int gpuart_ploc_run_host(gpuart_ploc *h, const gpuart_hip_scene *src, const gpuart_hip_scene *dst, uint32_t *new_to_old, gpuart_ploc_result *result) {
    return run_staged(LIB, h, gpuart_ploc_run, src, dst, new_to_old, result);
}

}  // extern "C"
