// nearest.hip — libgpuart_nearest.so (gfx950): closest-point queries over an uploaded scene's tree, as include/gpuart_nearest.h states
// them. Built without flushing fp32 denormals and without contraction: the rule (csrc/hip/nearest_rule.h) is restated in NumPy float32
// (tests/nearest_ref.py) and every answer is compared bit for bit. DESIGN.md "Closest points" describes the kernel. The library reads
// the scene's arrays and writes none of them. Behind k_nearest, the neighbour lists of the same header — every primitive within r, as CSR:
// k_within_count, rocPRIM's scan, k_within_fill. The three kernels differ in what a candidate does, in how a record's children are ordered
// and in what ends a query; a lane's state, its stack, the leaf walk, the user sphere, a query's prologue and the persistent-lane loop are
// stated once ("the walk: what the three kernels share") and compile to the kernels the written-out copies gave (profiles/nearest_walk.txt).
// Behind them the k nearest of the same header: k_knn, a fourth lane type of that walk, whose best so far is a list of k in LDS (DESIGN.md
// "k nearest", profiles/knn.txt). Behind them box overlap: k_overlap_count and k_overlap_fill, a fifth lane type whose query is a box and whose
// candidates are the primitives' boxes — box queries and, with the scene's own boxes as the queries, overlapping pairs (DESIGN.md "Box
// overlap", profiles/overlap.txt). What two lane types share is stated once beside what all share: the ordered record step of k_nearest and
// k_knn (k_knn keeps its record branch written out: as a call it costs two VGPRs) and the list lane — at, end, sum, begin, finish, next
// node, body — of k_within and k_overlap, whose lower-first record steps stay in place; on the host one timed launch, one count and one fill launch, one staged CSR run, one fill
// check and one check of caller-given offsets for the three kinds of list, one launch and one chunk loop for k_nearest and k_knn
// (profiles/nearest_lists.txt).
//
// Compile-time switches (tools/nearest_time.py builds the variants; the shipped library sets none):
//   NEAREST_PLAIN   the kernels as one thread per query with a grid stride and no refill: the A/B partner of the persistent-lane form
//   NEAREST_COUNT   box steps and primitive tests counted per query and summed (gpuart_nearest_counts, _within_counts, _knn_counts, _overlap_counts): a
//                   counting build, not a timed one
//   NEAREST_REFILL  idle lanes of a wave at which it takes new queries (default 16)
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <vector>

#include "../image/image_lib.h"
#include "../tree/tree_lib.h"
#include "../hip/nearest_rule.h"
#include "gpuart_nearest.h"

#ifndef NEAREST_REFILL
#define NEAREST_REFILL 16
#endif

namespace {

namespace nr = nearest_rule;
using tree_rule::REF_TWO;
using tree_rule::REF_TRIS;
using tree_rule::REF_SMALL;

const char LIB[] = "nearest";

constexpr uint32_t BLOCK = 256;                      ///< four waves
constexpr uint32_t WAVES = BLOCK / 64;
constexpr uint32_t CHUNK = GPUART_NEAREST_CHUNK;     ///< queries a wave takes from the cursor at a time
constexpr uint32_t RING = GPUART_NEAREST_RING;       ///< stack entries a lane keeps in LDS; older ones go to its global column
constexpr uint32_t NONE = 0xffffffffu;               ///< no query
constexpr size_t HOST_CHUNK = (size_t)1 << 20;       ///< queries per staged launch of run_host
constexpr size_t SPILL_BUDGET = (size_t)512 << 20;   ///< most bytes of global stack columns: the grid shrinks for deep trees

/// What the launches leave for the host, in device memory.
struct Status {
    uint32_t refused;   ///< the nesting check: tree_lib.h's refusal word
    uint32_t overflow;  ///< a walk met a full stack column (a descriptor whose max_depth is below the tree's depth): its answer is void
    unsigned long long box_steps, prim_tests;  ///< NEAREST_COUNT
    // the neighbour lists (k_within), behind what k_nearest knows
    uint32_t mismatch;  ///< a fill met a list that is longer or shorter than its offsets say, or an index at or beyond the capacity
    uint32_t pad;
    unsigned long long total;                      ///< of the last count: the items of all lists
    unsigned long long w_box_steps, w_prim_tests;  ///< NEAREST_COUNT
    unsigned long long k_box_steps, k_prim_tests;  ///< NEAREST_COUNT: the k nearest (k_knn)
    unsigned long long o_box_steps, o_prim_tests;  ///< NEAREST_COUNT: box overlap (k_overlap), both passes, box queries and pairs
};

struct SceneView {
    const float4 *recs, *prims;
    const float *pbox;
    uint32_t n_recs, n_prims, root_ref;
    float root_lo[3], root_hi[3];
};

__device__ __forceinline__ void xyz(const float4 &v, float o[3]) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }

// ---- the nesting check ----------------------------------------------------------------------------------------------------------------
enum { WHY_BOX = 1, WHY_REF = 2, WHY_NEST = 3 };

__device__ __forceinline__ bool inside(const float lo[3], const float hi[3], const float plo[3], const float phi[3]) {
    bool ok = true;
    for (int k = 0; k < 3; k++) ok = ok && lo[k] >= plo[k] && hi[k] <= phi[k] && lo[k] <= hi[k];  // (a NaN fails)
    return ok;
}

/// The child `ref` with box [lo, hi] that record `r` holds (r = n_recs: the descriptor's root): 0, or why the tree is refused.
__device__ uint32_t check_child(const SceneView &sc, uint32_t r, const float lo[3], const float hi[3], uint32_t ref) {
    if (!tree_rule::box_ok(lo, hi)) return WHY_BOX;
    if (!(ref & REF_LEAF)) {
        if (ref >= sc.n_recs || (r < sc.n_recs && ref <= r)) return WHY_REF;
        const float4 *c = sc.recs + 4 * (size_t)ref;
        float l0[3], h0[3], l1[3], h1[3];
        xyz(c[0], l0); xyz(c[1], h0); xyz(c[2], l1); xyz(c[3], h1);
        return inside(l0, h0, lo, hi) && inside(l1, h1, lo, hi) ? 0u : (uint32_t)WHY_NEST;
    }
    const uint32_t first = ref & REF_INDEX;
    if (first >= sc.n_prims) return WHY_REF;
    const uint32_t count = (ref & (REF_TRIS | REF_SMALL)) ? ((ref & REF_TWO) ? 2u : 1u) : __float_as_uint(sc.prims[3 * (size_t)first].w) >> 2;
    if (count > sc.n_prims - first) return WHY_REF;
    for (uint32_t k = 0; k < count; k++) {
        const float *b = sc.pbox + 6 * (size_t)(first + k);
        const float pl[3] = {b[0], b[1], b[2]}, ph[3] = {b[3], b[4], b[5]};
        if (!inside(pl, ph, lo, hi)) return WHY_NEST;
    }
    return 0;
}

// One thread per record, and one more for the descriptor's root box and root ref.
__global__ void __launch_bounds__(256) k_nr_nesting(SceneView sc, Status *st) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r > sc.n_recs) return;
    uint32_t why;
    if (r == sc.n_recs) {
        why = check_child(sc, r, sc.root_lo, sc.root_hi, sc.root_ref);
    } else {
        const float4 *c = sc.recs + 4 * (size_t)r;
        const float4 a = c[0], b = c[1], e = c[2], f = c[3];
        float l0[3], h0[3], l1[3], h1[3];
        xyz(a, l0); xyz(b, h0); xyz(e, l1); xyz(f, h1);
        why = check_child(sc, r, l0, h0, __float_as_uint(a.w));
        if (!why) why = check_child(sc, r, l1, h1, __float_as_uint(b.w));
    }
    if (why) refuse(&st->refused, r, why);
}

// ---- the walk: what the three kernels share ---------------------------------------------------------------------------------------------
/// A lane's query and its walk, whatever the query asks for.
struct Walk {
    uint32_t qi;           ///< the query, or NONE
    uint32_t node;         ///< the ref to visit next
    uint32_t sp, spilled;  ///< stack entries in all, and how many of them (the oldest) are in the global column
    float p[3], r2;
#ifdef NEAREST_COUNT
    uint32_t boxes, tests;
#endif
};

/// The stack of a lane, of entries E (k_nearest: a ref and its box's distance; the lists: a ref): the newest RING entries in a column of LDS
/// (entry i at ring[(i % RING) * BLOCK + thread]: a wave's lanes are neighbours, no bank is shared), the older ones in the lane's column
/// of `columns` (entry i at spill[i * lanes + lane]).
template <class E>
struct Stack {
    E *ring;       ///< LDS, this thread's column
    E *spill;      ///< global, this lane's column
    size_t lanes;
    uint32_t cap;  ///< entries of the global column
    uint32_t *overflow;

    __device__ __forceinline__ Stack(E *lds, E *columns, uint32_t cap_, Status *status)
        : ring(lds + threadIdx.x), spill(columns + ((size_t)blockIdx.x * BLOCK + threadIdx.x)), lanes((size_t)gridDim.x * BLOCK), cap(cap_),
          overflow(&status->overflow) {}

    __device__ __forceinline__ void push(Walk &L, const E &e) const {
        if (L.sp - L.spilled == RING) {
            if (L.spilled >= cap) {  // (no tree the descriptor describes gets here: the entry is dropped and the run is reported void)
                *overflow = 1u;
                return;
            }
            spill[L.spilled * lanes] = ring[(L.spilled % RING) * BLOCK];
            L.spilled++;
        }
        ring[(L.sp % RING) * BLOCK] = e;
        L.sp++;
    }

    __device__ __forceinline__ E pop(Walk &L) const {
        L.sp--;
        if (L.sp >= L.spilled) return ring[(L.sp % RING) * BLOCK];
        L.spilled = L.sp;
        return spill[L.sp * lanes];
    }
};

struct PrimData { float rec[12], box[6]; };

/// The user sphere (centre x, y, z; radius r) as a primitive's record and box: the first candidate of a query, on the device and in the
/// brute-force host functions.
__host__ __device__ inline void user_sphere_prim(float x, float y, float z, float r, PrimData &d) {
    for (int k = 0; k < 12; k++) d.rec[k] = 0.0f;
    d.rec[0] = x; d.rec[1] = y; d.rec[2] = z; d.rec[4] = r;
    d.box[0] = x - r; d.box[1] = y - r; d.box[2] = z - r;
    d.box[3] = x + r; d.box[4] = y + r; d.box[5] = z + r;
}

__device__ __forceinline__ void load_prim(const SceneView &sc, uint32_t i, PrimData &d) {
    const float4 a = sc.prims[3u * i], b = sc.prims[3u * i + 1u], c = sc.prims[3u * i + 2u];
    const float *bx = sc.pbox + 6u * i;
    d.rec[0] = a.x; d.rec[1] = a.y; d.rec[2] = a.z; d.rec[3] = a.w;
    d.rec[4] = b.x; d.rec[5] = b.y; d.rec[6] = b.z; d.rec[7] = b.w;
    d.rec[8] = c.x; d.rec[9] = c.y; d.rec[10] = c.z; d.rec[11] = c.w;
    for (int k = 0; k < 6; k++) d.box[k] = bx[k];
}

/// The leaf `ref`: candidate(type, record and box, ordinal) for each of its primitives. A flagged leaf holds one or two primitives (REF_TWO:
/// both records and boxes are in flight at once); an unflagged one says its count in its first record's word and is walked primitive by
/// primitive, the next one's loads ahead of this one's test.
template <class Candidate>
__device__ __forceinline__ void walk_leaf(const SceneView &sc, uint32_t ref, Candidate candidate) {
    const uint32_t first = ref & REF_INDEX;
    const bool flagged = (ref & (REF_TRIS | REF_SMALL)) != 0;
    PrimData cur, nxt;
    load_prim(sc, first, cur);
    nxt = cur;
    if (flagged && (ref & REF_TWO)) load_prim(sc, first + 1u, nxt);
    const uint32_t count = flagged ? ((ref & REF_TWO) ? 2u : 1u) : __float_as_uint(cur.rec[3]) >> 2;
    for (uint32_t k = 0; k < count; k++) {
        if (!flagged && k + 1u < count) load_prim(sc, first + k + 1u, nxt);
        candidate(__float_as_uint(cur.rec[3]) & 3u, cur, first + k);
        cur = nxt;
    }
}

/// Query i enters the lane: an empty stack, counters at zero.
__device__ __forceinline__ void reset_walk(Walk &L, uint32_t i) {
    L.qi = i;
    L.sp = L.spilled = 0;
#ifdef NEAREST_COUNT
    L.boxes = L.tests = 0;
#endif
}

/// Query i, a point and a radius, enters the lane. Returns the radius as the caller gave it.
__device__ __forceinline__ float take_query(Walk &L, const float4 *points, uint32_t i) {
    const float4 pt = points[i];
    reset_walk(L, i);
    L.p[0] = pt.x; L.p[1] = pt.y; L.p[2] = pt.z;
    L.r2 = pt.w * pt.w;
    return pt.w;
}

#ifndef NEAREST_PLAIN
__device__ __forceinline__ uint32_t wave_value(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t least(uint64_t a, uint64_t b) { return a < b ? a : b; }
#endif

/// The queries of a launch (a.points, a.n) through the lanes of the grid. A kernel says what a query is by the type of its lane:
/// begin(L, st, a, i) starts query i in lane L — or ends it at once —, step(L, st, a) takes its walk one record or one leaf further, and
/// whichever of the two finds the walk at its end stores the answer and sets L.qi = NONE.
/// Persistent lanes: a wave takes chunks of CHUNK queries — its first by its place in the grid, later ones from the cursor — and a lane
/// whose walk has ended is idle; once NEAREST_REFILL lanes are idle (or all) the idle lanes take the next queries of the chunk. Queries
/// differ in length by orders of magnitude: a point on the surface ends after one descent, a point far outside walks much of the tree.
/// Returns the lane as its last query left it (the count's sum rides in it).
/// The lane is a local of this function and begin and step are found by the lane's type, on purpose: with the caller's lane passed in by
/// reference the compiler arranges the loop while the lane is still memory, and k_nearest came out at 104 VGPRs, 4 waves per SIMD where
/// it has 5 (profiles/nearest_walk.txt lists the forms that were compiled and what each cost).
template <class L_, class E, class A>
__device__ __forceinline__ L_ walk_queries(const Stack<E> &st, const A &a) {
    L_ L;
    L.qi = NONE;
#ifdef NEAREST_PLAIN
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < a.n; i += st.lanes) {
        begin(L, st, a, (uint32_t)i);
        while (L.qi != NONE) step(L, st, a);
    }
#else
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = wave_value(blockIdx.x * WAVES + threadIdx.x / 64u), waves = gridDim.x * WAVES;
    // the cursor (wave-uniform): [next, end) is what is left of the wave's chunk; chunks behind the static ones come from the counter
    const uint64_t static_end = (uint64_t)waves * CHUNK;
    uint32_t next = (uint32_t)least((uint64_t)wave * CHUNK, a.n), end = (uint32_t)least(((uint64_t)wave + 1) * CHUNK, a.n);
    bool dry = false;
    for (;;) {
        unsigned long long idle = __ballot(L.qi == NONE);
        if (idle && !dry && ((uint32_t)__popcll(idle) >= NEAREST_REFILL || idle == ~0ull)) {
            while (idle && !dry) {
                if (next == end) {
                    uint32_t got = 0;
                    if (static_end < a.n) {
                        if (lane == 0) got = atomicAdd(a.cursor, CHUNK);
                        got = wave_value(got);
                    }
                    const uint64_t base = static_end + got;
                    if (static_end >= a.n || base >= a.n) { dry = true; break; }
                    next = (uint32_t)base;
                    end = (uint32_t)least(base + CHUNK, a.n);
                }
                const uint32_t want = (uint32_t)__popcll(idle), got = min(want, end - next);
                const uint32_t rank = (uint32_t)__popcll(idle & ((1ull << lane) - 1ull));
                if (L.qi == NONE && rank < got) begin(L, st, a, next + rank);
                next += got;
                idle = __ballot(L.qi == NONE);  // (a query that was answered at once has left its lane idle)
            }
            idle = __ballot(L.qi == NONE);
        }
        if (idle == ~0ull) {
            if (dry) break;
            continue;
        }
        if (L.qi != NONE) step(L, st, a);
    }
#endif
    return L;
}

/// The record `ref`, read whole: both children's boxes and refs.
struct Record {
    float l0[3], h0[3], l1[3], h1[3];
    uint32_t rlo, rhi;

    __device__ __forceinline__ Record(const SceneView &sc, uint32_t ref) {
        const float4 *rec = sc.recs + 4u * ref;  // (base + 32-bit offset: 4 * n_recs <= 2^30)
        const float4 ra = rec[0], rb = rec[1], rc = rec[2], rd = rec[3];
        xyz(ra, l0); xyz(rb, h0); xyz(rc, l1); xyz(rd, h1);
        rlo = __float_as_uint(ra.w);
        rhi = __float_as_uint(rb.w);
    }
};

/// The ordered record step (k_nearest; of k_knn, whose record branch stays written out, the pop). Like begin and step it finds what differs
/// by the lane's type: skip(L, a, d2) — a box at d2 cannot hold anything the query still wants — and walk_ended(L, a). The lower-first step
/// of the lists stays in their steps: with the box test behind a hook, a member or a callable the four kernels' instructions move
/// (profiles/nearest_lists.txt).
/// The next node off the stack that is not skipped by now, or the end of the walk.
template <class L_, class A>
__device__ __forceinline__ void next_ordered(L_ &L, const Stack<uint2> &st, const A &a) {
    for (;;) {
        if (L.sp == 0) { walk_ended(L, a); return; }
        const uint2 e = st.pop(L);
        if (!skip(L, a, __uint_as_float(e.y))) { L.node = e.x; return; }
    }
}

/// The ordered step (k_nearest, k_knn): the nearer child is entered, the farther stacked with its distance, each unless it is skipped.
template <class L_, class A>
__device__ __forceinline__ void ordered_record(L_ &L, const Stack<uint2> &st, const A &a, uint32_t ref) {
    const Record r(a.sc, ref);
    const float dlo = nr::box_d2(r.l0, r.h0, L.p), dhi = nr::box_d2(r.l1, r.h1, L.p);
    const bool klo = !skip(L, a, dlo), khi = !skip(L, a, dhi);
#ifdef NEAREST_COUNT
    L.boxes++;
#endif
    if (klo && khi) {
        const bool upper_first = dhi < dlo;
        st.push(L, make_uint2(upper_first ? r.rlo : r.rhi, __float_as_uint(upper_first ? dlo : dhi)));
        L.node = upper_first ? r.rhi : r.rlo;
    } else if (klo) L.node = r.rlo;
    else if (khi) L.node = r.rhi;
    else next_ordered(L, st, a);
}

/// A lane of the lists (k_within, k_overlap): nothing that is found prunes anything, so a stack entry is the ref alone, a record's children
/// are entered lower first — the contract's order of a list — and what comes off the stack is not tested again. The count leaves each
/// list's length at offsets[qi] and sums the lengths of the lane's queries; the fill writes list qi from offsets[qi] on, in the walk's order.
/// Q: what the kind's query holds beyond a point and a radius, ahead of the list's own members (behind them k_overlap's instructions move).
struct PointQuery {};
template <class Q>
struct ListLane : Walk, Q {
    uint32_t at, end;            ///< count: the items so far, unused; fill: where the next item goes, and where the list ends
    unsigned long long sum = 0;  ///< count: the items of all lists this lane has finished
};

/// Query i's list begins: empty for the count, between its two offsets for the fill.
template <class L_, class A>
__device__ __forceinline__ void list_begin(L_ &L, const A &a, uint32_t i) {
    L.at = L.end = 0;
    if (L_::FILLS) { L.at = a.offsets[i]; L.end = a.offsets[i + 1u]; }
}

/// The walk has ended: the count stores the list's length, the fill holds the list to its offsets; the lane is idle. counters(L): the
/// first of the lane kind's two NEAREST_COUNT members of the status.
template <class L_, class A>
__device__ __forceinline__ void list_finish(L_ &L, const A &a) {
    if (L_::FILLS) {
        if (L.at != L.end) a.status->mismatch = 1u;
    } else {
        a.offsets[L.qi] = L.at;
        L.sum += L.at;
    }
#ifdef NEAREST_COUNT
    unsigned long long *c = &(a.status->*counters(L));
    atomicAdd(c, (unsigned long long)L.boxes);
    atomicAdd(c + 1, (unsigned long long)L.tests);
#endif
    L.qi = NONE;
}

template <class L_, class A>
__device__ __forceinline__ void list_next(L_ &L, const Stack<uint32_t> &st, const A &a) {
    if (L.sp == 0) { list_finish(L, a); return; }
    L.node = st.pop(L);  // (what was stacked was not pruned, and nothing has changed since: there is no best so far)
}

/// A list kernel's body: the lengths of a wave's queries, summed in 64 bits lane by lane and then across the wave, go to the status' total
/// with one atomic per wave at the end of its life.
template <class L_, class A>
__device__ __forceinline__ void list_body(const A &a, uint32_t *ring) {
    const Stack<uint32_t> st(ring, a.spill, a.cap, a.status);
    const L_ L = walk_queries<L_>(st, a);
    if (!L_::FILLS) {
        unsigned long long sum = L.sum;
        for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
        if ((threadIdx.x & 63u) == 0 && sum) atomicAdd(&a.status->total, sum);
    }
}

// ---- closest points: k_nearest ----------------------------------------------------------------------------------------------------------
struct Launch {
    SceneView sc;
    const float4 *points;
    uint32_t n;
    float4 us;
    uint32_t use_us;
    gpuart_nearest_hit *hits;
    uint2 *spill;
    uint32_t cap;
    uint32_t *cursor;
    Status *status;
};

struct Lane : Walk {
    float best, q[3];    ///< the best so far: d2 (+inf: none) and the point
    uint32_t ord, type;  ///< its ordinal (NO_PRIM: none) and type
};

/// One candidate: primitive `ord` of `type` with record and box `d`.
__device__ __forceinline__ void candidate(Lane &L, uint32_t type, const PrimData &d, uint32_t ord) {
    float q[3];
    const float d2 = nr::closest_on_prim(type, d.rec, d.box, L.p, q);
    if (nr::better(d2, ord, L.r2, L.best, L.ord)) {
        L.best = d2; L.ord = ord; L.type = type & 3u;
        L.q[0] = q[0]; L.q[1] = q[1]; L.q[2] = q[2];
    }
#ifdef NEAREST_COUNT
    L.tests++;
#endif
}

__device__ __forceinline__ void store_hit(gpuart_nearest_hit *hits, uint32_t i, const Lane &L) {
    float4 *o = (float4 *)(hits + i);
    if (L.ord == nr::NO_PRIM) {
        o[0] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
        o[1] = make_float4(0.0f, __int_as_float(-1), __int_as_float(-1), 0.0f);
    } else {
        o[0] = make_float4(sqrtf(L.best), L.q[0], L.q[1], L.q[2]);
        o[1] = make_float4(L.best, __uint_as_float(L.ord), __uint_as_float(L.type), 0.0f);
    }
}

/// The query is answered: its record is stored and the lane is idle.
__device__ __forceinline__ void finish(Lane &L, const Launch &a) {
    store_hit(a.hits, L.qi, L);
#ifdef NEAREST_COUNT
    atomicAdd(&a.status->box_steps, (unsigned long long)L.boxes);
    atomicAdd(&a.status->prim_tests, (unsigned long long)L.tests);
#endif
    L.qi = NONE;
}

__device__ __forceinline__ bool skip(const Lane &L, const Launch &, float d2) { return nr::pruned(d2, L.r2, L.best); }
__device__ __forceinline__ void walk_ended(Lane &L, const Launch &a) { finish(L, a); }

/// Query i begins: a miss at once, or the user sphere as the first candidate and the root.
__device__ __forceinline__ void begin(Lane &L, const Stack<uint2> &, const Launch &a, uint32_t i) {
    const float r = take_query(L, a.points, i);
    L.best = __builtin_inff(); L.ord = nr::NO_PRIM; L.type = 0;
    L.q[0] = L.q[1] = L.q[2] = 0.0f;
    if (!nr::query_ok(L.p, r)) { finish(L, a); return; }
    if (a.use_us) {
        PrimData d;
        user_sphere_prim(a.us.x, a.us.y, a.us.z, a.us.w, d);
        candidate(L, nr::SPHERE, d, nr::USER_SPHERE);
    }
    if (nr::pruned(nr::box_d2(a.sc.root_lo, a.sc.root_hi, L.p), L.r2, L.best)) { finish(L, a); return; }
    L.node = a.sc.root_ref;
}

/// One step of a lane's walk: a record (the ordered step) or a leaf.
__device__ __forceinline__ void step(Lane &L, const Stack<uint2> &st, const Launch &a) {
    const uint32_t ref = L.node;
    if (!(ref & REF_LEAF)) { ordered_record(L, st, a, ref); return; }
    walk_leaf(a.sc, ref, [&](uint32_t type, const PrimData &d, uint32_t ord) { candidate(L, type, d, ord); });
    next_ordered(L, st, a);
}

// k_nearest. Types are branched on at run time (closest_on_prim): the descriptor does not carry the type mask, and one launch per mask would
// need a reduction over the records in bind for a gain that only the leaf step could show (a probe with the leaf's type fixed to
// "triangle" compiled to the same 96 VGPRs and occupancy: DESIGN.md).
__global__ void __launch_bounds__(BLOCK) k_nearest(Launch a) {
    __shared__ uint2 ring[RING * BLOCK];
    const Stack<uint2> st(ring, a.spill, a.cap, a.status);
    walk_queries<Lane>(st, a);
}

// ---- the neighbour lists: k_within_count and k_within_fill ------------------------------------------------------------------------------
// The walk of k_nearest without a best so far, as a list lane: an item is the 32-byte record of a primitive within r.
struct WLaunch {
    SceneView sc;
    const float4 *points;
    uint32_t n;
    float4 us;
    uint32_t use_us;
    uint32_t *offsets;          ///< count: written; fill: read
    gpuart_nearest_hit *items;  ///< fill
    uint32_t capacity;          ///< fill: records of items
    uint32_t *spill;
    uint32_t cap;
    uint32_t *cursor;
    Status *status;
};

template <bool FILL>
struct WLane : ListLane<PointQuery> {
    static constexpr bool FILLS = FILL;
};
template <bool FILL>
__device__ __forceinline__ unsigned long long Status::*counters(const WLane<FILL> &) { return &Status::w_box_steps; }

/// One candidate: an item of the list if it is accepted. The fill stores it where the offsets put it, and nowhere else: an index at or
/// beyond the list's end or the capacity is not written and marks the run.
template <bool FILL>
__device__ __forceinline__ void candidate(WLane<FILL> &L, const WLaunch &a, uint32_t type, const PrimData &d, uint32_t ord) {
    float q[3];
    const float d2 = nr::closest_on_prim(type, d.rec, d.box, L.p, q);
    if (nr::within_accept(d2, L.r2)) {
        if (FILL) {
            if (L.at < L.end && L.at < a.capacity) {
                float4 *o = (float4 *)(a.items + L.at);
                o[0] = make_float4(sqrtf(d2), q[0], q[1], q[2]);
                o[1] = make_float4(d2, __uint_as_float(ord), __uint_as_float(type & 3u), 0.0f);
            } else {
                a.status->mismatch = 1u;
            }
        }
        L.at++;
    }
#ifdef NEAREST_COUNT
    L.tests++;
#endif
}

/// Query i begins: an empty list at once, or the user sphere as the first candidate and the root.
template <bool FILL>
__device__ __forceinline__ void begin(WLane<FILL> &L, const Stack<uint32_t> &, const WLaunch &a, uint32_t i) {
    const float r = take_query(L, a.points, i);
    list_begin(L, a, i);
    if (!nr::query_ok(L.p, r)) { list_finish(L, a); return; }
    if (a.use_us) {
        PrimData d;
        user_sphere_prim(a.us.x, a.us.y, a.us.z, a.us.w, d);
        candidate(L, a, nr::SPHERE, d, nr::USER_SPHERE);
    }
    if (nr::within_pruned(nr::box_d2(a.sc.root_lo, a.sc.root_hi, L.p), L.r2)) { list_finish(L, a); return; }
    L.node = a.sc.root_ref;
}

/// One step of a lane's walk: a record (both boxes, lower child first) or a leaf.
template <bool FILL>
__device__ __forceinline__ void step(WLane<FILL> &L, const Stack<uint32_t> &st, const WLaunch &a) {
    const uint32_t ref = L.node;
    if (!(ref & REF_LEAF)) {  // the lower child is entered, the upper stacked, each unless pruned
        const Record r(a.sc, ref);
        const bool klo = !nr::within_pruned(nr::box_d2(r.l0, r.h0, L.p), L.r2), khi = !nr::within_pruned(nr::box_d2(r.l1, r.h1, L.p), L.r2);
#ifdef NEAREST_COUNT
        L.boxes++;
#endif
        if (klo && khi) {
            st.push(L, r.rhi);
            L.node = r.rlo;
        } else if (klo) L.node = r.rlo;
        else if (khi) L.node = r.rhi;
        else list_next(L, st, a);
        return;
    }
    walk_leaf(a.sc, ref, [&](uint32_t type, const PrimData &d, uint32_t ord) { candidate(L, a, type, d, ord); });
    list_next(L, st, a);
}

// k_within_count (FILL = false) and k_within_fill (FILL = true).
__global__ void __launch_bounds__(BLOCK) k_within_count(WLaunch a) {
    __shared__ uint32_t ring[RING * BLOCK];
    list_body<WLane<false>>(a, ring);
}

__global__ void __launch_bounds__(BLOCK) k_within_fill(WLaunch a) {
    __shared__ uint32_t ring[RING * BLOCK];
    list_body<WLane<true>>(a, ring);
}

// ---- the k nearest: k_knn -----------------------------------------------------------------------------------------------------------------
// The walk of k_nearest with the best so far replaced by the k best so far: the bound that prunes is the d2 of the worst of them, and only
// once k are kept (nearest_rule.h: knn_pruned). What is kept is {d2, ordinal}, 8 bytes, in a column of LDS (entry j of a thread at
// list[j * BLOCK + thread]: the bank is the thread's alone, whatever j) as a binary max-heap on the contract's order, the worst at the root
// and its key in registers: a candidate is one compare against registers unless it is kept. At the end of a walk the heap is sorted in place
// and each kept ordinal's point is computed a second time for its record — closest_on_prim is a function of its operands, so the record is
// the one k_within_fill writes — which keeps 8 bytes per entry instead of 32.
struct KnnLaunch {
    SceneView sc;
    const float4 *points;
    uint32_t n;
    float4 us;
    uint32_t use_us;
    uint32_t k;                ///< 1 .. the kernel's capacity
    gpuart_nearest_hit *hits;  ///< n * k
    uint2 *spill;
    uint32_t cap;
    uint32_t *cursor;
    Status *status;
};

/// This thread's column of the kept lists of a kernel of capacity CAP: entry j at [j * BLOCK].
template <uint32_t CAP>
__device__ __forceinline__ uint2 *knn_list() {
    __shared__ uint2 list[CAP * BLOCK];
    return list + threadIdx.x;
}

/// A member of the launch's arguments, read from the kernel's argument segment where it is used (k_knn's only argument is the KnnLaunch, at
/// offset 0 of the segment; the read is volatile, so it stays where it is written). The root box, the user sphere, points and hits are
/// needed once or twice per query, in steps with registers to spare; as plain members of `a` the compiler loads them ahead of the lane
/// loop and holds their fourteen words in scalar registers through the leaf step, where the kernel then has thirteen too few and spills.
template <class T>
__device__ __forceinline__ T launch_value(size_t offset) {
    typedef const char __attribute__((address_space(4))) *Segment;
    return *(const volatile T __attribute__((address_space(4))) *)((Segment)__builtin_amdgcn_kernarg_segment_ptr() + offset);
}
__device__ __forceinline__ float launch_word(size_t offset) { return launch_value<float>(offset); }
/// A pointer member, with what the compiler knows of a kernel argument and cannot of a word it has read: that it points to global memory.
template <class T>
__device__ __forceinline__ T *launch_pointer(size_t offset) {
    typedef T __attribute__((address_space(1))) *Global;
    return (T *)(Global)launch_value<uintptr_t>(offset);
}

/// What a lane's `node` says before its walk and once it has ended — no tree's ref: leaves that begin at REF_INDEX, beyond every primitive.
/// SPHERE_FIRST: the next step tests the user sphere and enters the root; WALKED: the next step sorts the kept and writes the misses behind
/// them; WRITING: each further step writes one record, the lane's `sp` (the stack is empty) counting them. So the sort is stated once in
/// the kernel and not at each of the four places where a walk can end, a record's point is computed where a candidate's is, by the same
/// instructions — the kernel holds one closest_on_prim over the four types, as k_nearest does —, and the user sphere has one place.
constexpr uint32_t WALKED = REF_LEAF | REF_INDEX, WRITING = REF_LEAF | REF_TWO | REF_INDEX, SPHERE_FIRST = REF_LEAF | REF_SMALL | REF_INDEX;

template <uint32_t CAP>
struct KLane : Walk {
    uint32_t kept;       ///< entries of the list
    float worst;         ///< the heap's root (the worst kept) while the list is full; else +inf and NO_PRIM
    uint32_t worst_ord;
};

__device__ __forceinline__ bool before(const uint2 &x, const uint2 &y) { return nr::knn_before(__uint_as_float(x.x), x.y, __uint_as_float(y.x), y.y); }

/// `e` takes the root's place in the heap of m entries and sinks to where both its children come before it. (An only child is read
/// twice, as its own sibling: one loop with one way out, where a branch for it would nest another.)
__device__ __forceinline__ void sift_down(uint2 *list, uint32_t m, uint2 e) {
    uint32_t i = 0;
    for (uint32_t c = 1u; c < m; c = 2u * i + 1u) {
        const uint32_t c1 = min(c + 1u, m - 1u);
        const uint2 h0 = list[c * BLOCK], h1 = list[c1 * BLOCK];
        const bool second = before(h0, h1);
        const uint2 hc = second ? h1 : h0;
        if (!before(e, hc)) break;
        list[i * BLOCK] = hc;
        i = second ? c1 : c;
    }
    list[i * BLOCK] = e;
}

/// One candidate (d2, ord): kept if it is accepted and the list has room (it rises from the end: parents that come before it move down),
/// or if it comes before the worst kept, which then leaves (it sinks from the root).
template <uint32_t CAP>
__device__ __forceinline__ void keep(KLane<CAP> &L, const KnnLaunch &a, float d2, uint32_t ord) {
    uint2 *list = knn_list<CAP>();
    const uint2 e = make_uint2(__float_as_uint(d2), ord);
    const bool accepted = nr::within_accept(d2, L.r2), room = L.kept < a.k;
    const bool rises = accepted && room, sinks = accepted && !room && nr::knn_before(d2, ord, L.worst, L.worst_ord);
    if (rises) {
        uint32_t i = L.kept++;
        while (i) {
            const uint32_t parent = (i - 1u) >> 1;
            const uint2 hp = list[parent * BLOCK];
            if (!before(hp, e)) break;
            list[i * BLOCK] = hp;
            i = parent;
        }
        list[i * BLOCK] = e;
    }
    if (sinks) sift_down(list, a.k, e);
    if ((rises || sinks) && L.kept == a.k) {
        const uint2 root = list[0];
        L.worst = __uint_as_float(root.x);
        L.worst_ord = root.y;
    }
}

template <uint32_t CAP>
__device__ __forceinline__ bool skip(const KLane<CAP> &L, const KnnLaunch &a, float d2) { return nr::knn_pruned(d2, L.r2, L.kept == a.k, L.worst); }
/// The walk has ended; the next step sorts the kept.
template <uint32_t CAP>
__device__ __forceinline__ void walk_ended(KLane<CAP> &L, const KnnLaunch &) { L.node = WALKED; }

/// The walk has ended: the heap is sorted in place (the root goes behind the heap, which shrinks by one) and the miss record fills the
/// slots behind the kept. With nothing kept the query is answered and the lane is idle; else the records follow, one a step.
template <uint32_t CAP>
__device__ __forceinline__ void sort_kept(KLane<CAP> &L, const KnnLaunch &a) {
    uint2 *list = knn_list<CAP>();
    for (uint32_t m = L.kept; m > 1u; m--) {
        const uint2 root = list[0], last = list[(m - 1u) * BLOCK];
        list[(m - 1u) * BLOCK] = root;
        sift_down(list, m - 1u, last);
    }
    float4 *o = (float4 *)(launch_pointer<gpuart_nearest_hit>(offsetof(KnnLaunch, hits)) + (size_t)L.qi * a.k);
    for (uint32_t j = L.kept; j < a.k; j++) {
        o[2u * j] = make_float4(-1.0f, 0.0f, 0.0f, 0.0f);
        o[2u * j + 1u] = make_float4(0.0f, __int_as_float(-1), __int_as_float(-1), 0.0f);
    }
#ifdef NEAREST_COUNT
    atomicAdd(&a.status->k_box_steps, (unsigned long long)L.boxes);
    atomicAdd(&a.status->k_prim_tests, (unsigned long long)L.tests);
#endif
    L.sp = 0;
    if (L.kept) L.node = WRITING;
    else L.qi = NONE;
}

/// The record of the kept entry L.sp, whose point and distance have just been computed again; behind the last one the lane is idle.
template <uint32_t CAP>
__device__ __forceinline__ void write_kept(KLane<CAP> &L, const KnnLaunch &a, uint32_t type, const float q[3], float d2, uint32_t ord) {
    float4 *o = (float4 *)(launch_pointer<gpuart_nearest_hit>(offsetof(KnnLaunch, hits)) + ((size_t)L.qi * a.k + L.sp));
    o[0] = make_float4(sqrtf(d2), q[0], q[1], q[2]);
    o[1] = make_float4(d2, __uint_as_float(ord), __uint_as_float(type & 3u), 0.0f);
    if (++L.sp == L.kept) {
        L.sp = 0;
        L.qi = NONE;
    }
}

/// The walk begins at the root, unless the root is pruned already.
template <uint32_t CAP>
__device__ __forceinline__ void enter_root(KLane<CAP> &L, const KnnLaunch &a) {
    float lo[3], hi[3];
    for (int c = 0; c < 3; c++) {
        lo[c] = launch_word(offsetof(KnnLaunch, sc.root_lo) + 4 * c);
        hi[c] = launch_word(offsetof(KnnLaunch, sc.root_hi) + 4 * c);
    }
    L.node = skip(L, a, nr::box_d2(lo, hi, L.p)) ? WALKED : a.sc.root_ref;
}

/// Query i begins: its walk has ended at once, or its first node is the user sphere, or the root.
template <uint32_t CAP>
__device__ __forceinline__ void begin(KLane<CAP> &L, const Stack<uint2> &, const KnnLaunch &a, uint32_t i) {
    const float r = take_query(L, launch_pointer<const float4>(offsetof(KnnLaunch, points)), i);
    L.kept = 0; L.worst = __builtin_inff(); L.worst_ord = nr::NO_PRIM;
    if (!nr::query_ok(L.p, r)) L.node = WALKED;
    else if (a.use_us) L.node = SPHERE_FIRST;
    else enter_root(L, a);
}

/// One step of a lane: of its walk, as k_nearest's — a record (both boxes, the nearer child entered, the farther stacked with its distance)
/// or a leaf —, or of its answer: the sort, or one record. A kept primitive's record goes through the leaf's code as a leaf of that one
/// primitive; the user sphere's, which is no primitive of the scene, is written here.
template <uint32_t CAP>
__device__ __forceinline__ void step(KLane<CAP> &L, const Stack<uint2> &st, const KnnLaunch &a) {
    uint32_t ref = L.node;
    if (ref == WALKED) { sort_kept(L, a); return; }
    const bool writing = ref == WRITING;
    bool sphere = ref == SPHERE_FIRST;
    if (writing) {
        const uint32_t ord = knn_list<CAP>()[L.sp * BLOCK].y;
        sphere = ord == nr::USER_SPHERE;
        ref = REF_LEAF | REF_SMALL | ord;
    }
    if (sphere) {
        PrimData d;
        float q[3];
        user_sphere_prim(launch_word(offsetof(KnnLaunch, us.x)), launch_word(offsetof(KnnLaunch, us.y)), launch_word(offsetof(KnnLaunch, us.z)),
                         launch_word(offsetof(KnnLaunch, us.w)), d);
        const float d2 = nr::closest_on_prim(nr::SPHERE, d.rec, d.box, L.p, q);
        if (writing) {
            write_kept(L, a, nr::SPHERE, q, d2, nr::USER_SPHERE);
        } else {
            keep(L, a, d2, nr::USER_SPHERE);
#ifdef NEAREST_COUNT
            L.tests++;
#endif
            enter_root(L, a);
        }
        return;
    }
    if (!(ref & REF_LEAF)) {  // ordered_record, written out: as a call of it this kernel takes 96 VGPRs for 94 (profiles/nearest_lists.txt)
        const float4 *rec = a.sc.recs + 4u * ref;
        const float4 ra = rec[0], rb = rec[1], rc = rec[2], rd = rec[3];
        float l0[3], h0[3], l1[3], h1[3];
        xyz(ra, l0); xyz(rb, h0); xyz(rc, l1); xyz(rd, h1);
        const float dlo = nr::box_d2(l0, h0, L.p), dhi = nr::box_d2(l1, h1, L.p);
        const uint32_t rlo = __float_as_uint(ra.w), rhi = __float_as_uint(rb.w);
        const bool klo = !skip(L, a, dlo), khi = !skip(L, a, dhi);
#ifdef NEAREST_COUNT
        L.boxes++;
#endif
        if (klo && khi) {
            const bool upper_first = dhi < dlo;
            st.push(L, make_uint2(upper_first ? rlo : rhi, __float_as_uint(upper_first ? dlo : dhi)));
            L.node = upper_first ? rhi : rlo;
        } else if (klo) L.node = rlo;
        else if (khi) L.node = rhi;
        else next_ordered(L, st, a);
        return;
    }
    walk_leaf(a.sc, ref, [&](uint32_t type, const PrimData &d, uint32_t ord) {
        float q[3];
        const float d2 = nr::closest_on_prim(type, d.rec, d.box, L.p, q);
        if (writing) {
            write_kept(L, a, type, q, d2, ord);
        } else {
            keep(L, a, d2, ord);
#ifdef NEAREST_COUNT
            L.tests++;
#endif
        }
    });
    if (!writing) next_ordered(L, st, a);
}

// k_knn<CAP>: lists of up to CAP entries, CAP * 2 KiB of LDS per workgroup beside the ring's 16 KiB. The occupancy is the LDS's: the host
// picks the smallest capacity that holds the call's k (knn_capacity) and sizes the grid per capacity.
template <uint32_t CAP>
__global__ void __launch_bounds__(BLOCK) k_knn(KnnLaunch a) {
    __shared__ uint2 ring[RING * BLOCK];
    const Stack<uint2> st(ring, a.spill, a.cap, a.status);
    walk_queries<KLane<CAP>>(st, a);
}

constexpr uint32_t KNN_SIZES = 4;
constexpr uint32_t KNN_CAPS[KNN_SIZES] = {4, 8, 16, GPUART_NEAREST_KNN_MAX};
void (*const KNN_KERNELS[KNN_SIZES])(KnnLaunch) = {k_knn<4>, k_knn<8>, k_knn<16>, k_knn<GPUART_NEAREST_KNN_MAX>};

/// The smallest capacity that holds lists of k entries (1 <= k <= GPUART_NEAREST_KNN_MAX), as an index of the two arrays above.
uint32_t knn_capacity(uint32_t k) {
    uint32_t s = 0;
    while (KNN_CAPS[s] < k) s++;
    return s;
}

// ---- box overlap: k_overlap_count and k_overlap_fill -------------------------------------------------------------------------------------
// A fifth lane type of the walk: the query is a box, inflated once by the call's margin, and both the item test and the prune are
// nearest_rule.h's overlap_test — comparisons of stored numbers. As in k_within nothing that is found prunes anything: a stack entry is the
// ref, the lower child is entered first, what comes off the stack is not tested again. An item is the ordinal, 4 bytes. The leaf step reads
// the primitives' boxes and, of an unflagged leaf, the count word of its first record — not the 48-byte records walk_leaf loads.
// Pairs are the same kernels under a launch flag: the host points `boxes` at the scene's own prim_boxes from the launch's first ordinal on,
// query i's own ordinal is self0 + i, and an item is kept only strictly above it (pairs_keep). The flag is wave-uniform; the one compare it
// adds to a box query's item is not worth a second pair of kernels.
struct OLaunch {
    SceneView sc;
    const float *boxes;  ///< query i's six words {lo.xyz, hi.xyz} at boxes + 6 i
    uint32_t n;
    uint32_t self0;      ///< pairs: the ordinal of query 0
    uint32_t pairs;
    float margin;
    float4 us;
    uint32_t use_us;
    uint32_t *offsets;   ///< count: written; fill: read
    int32_t *items;      ///< fill
    uint32_t capacity;   ///< fill: ordinals of items
    uint32_t *spill;
    uint32_t cap;
    uint32_t *cursor;
    Status *status;
};

struct BoxQuery {
    float qlo[3], qhi[3];  ///< the inflated query
    uint32_t self;         ///< pairs: the query's own ordinal
};
template <bool FILL>
struct OLane : ListLane<BoxQuery> {
    static constexpr bool FILLS = FILL;
};
template <bool FILL>
__device__ __forceinline__ unsigned long long Status::*counters(const OLane<FILL> &) { return &Status::o_box_steps; }

/// One candidate: the box [blo, bhi] of ordinal `ord`. The fill stores an item where the offsets put it, and nowhere else.
template <bool FILL>
__device__ __forceinline__ void offer(OLane<FILL> &L, const OLaunch &a, uint32_t ord, const float blo[3], const float bhi[3]) {
    if (nr::overlap_test(L.qlo, L.qhi, blo, bhi) && (!a.pairs || nr::pairs_keep(L.self, ord))) {
        if (FILL) {
            if (L.at < L.end && L.at < a.capacity) a.items[L.at] = (int32_t)ord;
            else a.status->mismatch = 1u;
        }
        L.at++;
    }
#ifdef NEAREST_COUNT
    L.tests++;
#endif
}

__device__ __forceinline__ void load_box(const SceneView &sc, uint32_t i, float b[6]) {
    const float *bx = sc.pbox + 6u * i;
    for (int k = 0; k < 6; k++) b[k] = bx[k];
}

/// The leaf `ref`: candidate(box, ordinal) for each of its primitives, in walk_leaf's order and with its loads ahead, of the boxes alone.
template <class Candidate>
__device__ __forceinline__ void walk_leaf_boxes(const SceneView &sc, uint32_t ref, Candidate candidate) {
    const uint32_t first = ref & REF_INDEX;
    const bool flagged = (ref & (REF_TRIS | REF_SMALL)) != 0;
    float cur[6], nxt[6];
    load_box(sc, first, cur);
    for (int k = 0; k < 6; k++) nxt[k] = cur[k];
    if (flagged && (ref & REF_TWO)) load_box(sc, first + 1u, nxt);
    uint32_t count = (ref & REF_TWO) ? 2u : 1u;
    if (!flagged) count = __float_as_uint(((const float *)sc.prims)[12u * first + 3u]) >> 2;
    for (uint32_t k = 0; k < count; k++) {
        if (!flagged && k + 1u < count) load_box(sc, first + k + 1u, nxt);
        candidate(cur, first + k);
        for (int c = 0; c < 6; c++) cur[c] = nxt[c];
    }
}

/// Query i begins: an empty list at once (no box, or one that misses the root), or the user sphere's box as the first candidate and the root.
template <bool FILL>
__device__ __forceinline__ void begin(OLane<FILL> &L, const Stack<uint32_t> &, const OLaunch &a, uint32_t i) {
    const float *b = a.boxes + 6 * (size_t)i;
    const float box[6] = {b[0], b[1], b[2], b[3], b[4], b[5]};
    reset_walk(L, i);
    L.self = a.self0 + i;
    list_begin(L, a, i);
    nr::overlap_inflate(box, a.margin, L.qlo, L.qhi);
    if (!nr::overlap_query_ok(box)) { list_finish(L, a); return; }
    if (a.use_us) {
        PrimData d;
        user_sphere_prim(a.us.x, a.us.y, a.us.z, a.us.w, d);
        offer(L, a, nr::USER_SPHERE, d.box, d.box + 3);
    }
    if (!nr::overlap_test(L.qlo, L.qhi, a.sc.root_lo, a.sc.root_hi)) { list_finish(L, a); return; }
    L.node = a.sc.root_ref;
}

/// One step of a lane's walk: a record (both boxes, lower child first) or a leaf.
template <bool FILL>
__device__ __forceinline__ void step(OLane<FILL> &L, const Stack<uint32_t> &st, const OLaunch &a) {
    const uint32_t ref = L.node;
    if (!(ref & REF_LEAF)) {  // the lower child is entered, the upper stacked, each unless it misses the query
        const Record r(a.sc, ref);
        const bool klo = nr::overlap_test(L.qlo, L.qhi, r.l0, r.h0), khi = nr::overlap_test(L.qlo, L.qhi, r.l1, r.h1);
#ifdef NEAREST_COUNT
        L.boxes++;
#endif
        if (klo && khi) {
            st.push(L, r.rhi);
            L.node = r.rlo;
        } else if (klo) L.node = r.rlo;
        else if (khi) L.node = r.rhi;
        else list_next(L, st, a);
        return;
    }
    walk_leaf_boxes(a.sc, ref, [&](const float *bx, uint32_t ord) { offer(L, a, ord, bx, bx + 3); });
    list_next(L, st, a);
}

// k_overlap_count (FILL = false) and k_overlap_fill (FILL = true).
__global__ void __launch_bounds__(BLOCK) k_overlap_count(OLaunch a) {
    __shared__ uint32_t ring[RING * BLOCK];
    list_body<OLane<false>>(a, ring);
}

__global__ void __launch_bounds__(BLOCK) k_overlap_fill(OLaunch a) {
    __shared__ uint32_t ring[RING * BLOCK];
    list_body<OLane<true>>(a, ring);
}

/// Whose the last count was: the three kinds of lists share the handle's bookkeeping of it, and a fill of another kind is refused.
enum { COUNT_WITHIN = 1, COUNT_OVERLAP = 2, COUNT_PAIRS = 3 };
const char *const COUNT_NAMES[4] = {"nothing", "neighbour lists (within)", "box queries (overlap)", "pairs"};

/// The walk kernels as slots of the handle's occupancy figures (a fill's is its count's + 1), and the timed steps (likewise).
enum { K_NEAREST, K_WCOUNT, K_WFILL, K_OCOUNT, K_OFILL, K_KNN, KERNELS = K_KNN + KNN_SIZES };
enum { T_CHECK, T_WALK, T_KWALK, T_WCOUNT, T_WFILL, T_OCOUNT, T_OFILL, TIMERS };
constexpr int TIMER_STEPS[TIMERS] = {1, 1, 1, 2, 1, 2, 1};  ///< a count is its kernel and the scan

/// What tells the two kinds of list launch apart on the host.
template <class A>
struct ListKernels {
    void (*count)(A);
    void (*fill)(A);
    uint32_t slot;  ///< of the count
    int timer;      ///< of the count
};
const ListKernels<WLaunch> WITHIN_KERNELS = {k_within_count, k_within_fill, K_WCOUNT, T_WCOUNT};
const ListKernels<OLaunch> OVERLAP_KERNELS = {k_overlap_count, k_overlap_fill, K_OCOUNT, T_OCOUNT};
const ListKernels<WLaunch> &kernels_of(const WLaunch &) { return WITHIN_KERNELS; }
const ListKernels<OLaunch> &kernels_of(const OLaunch &) { return OVERLAP_KERNELS; }

}  // namespace

struct gpuart_nearest : ImageHandle {
    Status *status = nullptr;    ///< device
    uint32_t *cursor = nullptr;  ///< device
    gpuart_hip_scene scene{};    ///< what the handle is bound to
    bool bound = false;
    DeviceBuffer spill;          ///< the lanes' global stack columns
    DeviceBuffer staging;        ///< the runs through host memory: a chunk's queries and what comes back
    uint32_t blocks[KERNELS] = {};  ///< per kernel: the workgroups the device holds at once
    uint32_t max_blocks = 0;     ///< the most a launch takes: k_nearest's figure, or what gpuart_nearest_set_limits says
    size_t spill_budget = SPILL_BUDGET, host_chunk = HOST_CHUNK;  ///< likewise
    uint32_t last_blocks = 0, last_launches = 0;  ///< the last launch's grid; the launches of the last run
    StepTimer timers[TIMERS];
    bool recorded[TIMERS] = {};  ///< the timer's events have been recorded
    // the lists: the three kinds share the bookkeeping of "the last count", which therefore says whose it is
    DeviceBuffer scan_temp;      ///< rocPRIM's
    uint64_t max_items = GPUART_NEAREST_WITHIN_MAX_ITEMS;
    bool fill_pending = false;   ///< a fill was launched since the last finish looked at the mismatch word
    bool total_read = false;     ///< last_total is the last count's
    uint64_t last_total = 0;
    size_t counted_n = 0;        ///< the queries of the last count
    int counted_kind = 0;        ///< COUNT_WITHIN, COUNT_OVERLAP or COUNT_PAIRS: what the last count counted (0: nothing yet)
    std::vector<uint32_t> host_offsets;  ///< a staged chunk's
};

namespace {

SceneView view_of(const gpuart_hip_scene *s) {
    SceneView v;
    v.recs = (const float4 *)s->recs;
    v.prims = (const float4 *)s->prims;
    v.pbox = (const float *)s->prim_boxes;
    v.n_recs = (uint32_t)s->n_recs;
    v.n_prims = (uint32_t)s->n_prims;
    v.root_ref = s->root_ref;
    memcpy(v.root_lo, s->root_min, 12);
    memcpy(v.root_hi, s->root_max, 12);
    return v;
}

int check_user_sphere(const float us[4]) {
    if (!us) return 0;
    for (int k = 0; k < 4; k++)
        if (!(fabsf(us[k]) < INFINITY)) return fail(GPUART_HIP_ERR_ARG, "nearest: the user sphere has a word that is not finite");
    if (!(us[3] >= 0)) return fail(GPUART_HIP_ERR_ARG, "nearest: the user sphere's radius is negative");
    return 0;
}

int check_bound(const gpuart_nearest *h, const gpuart_hip_scene *s) {
    if (!s) return fail(GPUART_HIP_ERR_ARG, "nearest: scene is NULL");
    if (!h->bound) return fail(GPUART_HIP_ERR_ARG, "nearest: the handle is not bound to a scene: gpuart_nearest_bind first");
    if (s->generation != h->scene.generation || s->recs != h->scene.recs || s->prims != h->scene.prims || s->prim_boxes != h->scene.prim_boxes ||
        s->n_recs != h->scene.n_recs || s->n_prims != h->scene.n_prims || s->root_ref != h->scene.root_ref)
        return fail(GPUART_HIP_ERR_ARG, "nearest: the handle was bound to another upload (generation " + std::to_string(h->scene.generation) + ", the scene's is " +
                                            std::to_string(s->generation) + "): bind again");
    if (!tree_rule::box_ok(s->root_min, s->root_max)) return fail(GPUART_HIP_ERR_ARG, "nearest: the root box is not finite and ordered");
    return 0;
}

/// What every run checks before its own arrays: the handle, its binding, the query count and the user sphere.
int check_queries(gpuart_nearest *h, const gpuart_hip_scene *s, size_t n, const float us[4]) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (int rc = check_bound(h, s)) return rc;
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "nearest: too many queries: " + std::to_string(n));
    return check_user_sphere(us);
}

/// What the runs that answer with records check: of the k nearest, k and n * k first; of the closest points (k = 0) one record a query.
int check_hits(gpuart_nearest *h, const gpuart_hip_scene *s, const void *points, size_t n, size_t k, bool knn, const float us[4], const void *hits, size_t align) {
    if (int rc = check_queries(h, s, n, us)) return rc;
    if (knn) {
        if (k < 1 || k > GPUART_NEAREST_KNN_MAX) return fail(GPUART_HIP_ERR_ARG, "nearest: k is " + std::to_string(k) + ": not in 1 .. " + std::to_string(GPUART_NEAREST_KNN_MAX));
        if (n * k > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "nearest: too many records: " + std::to_string(n) + " queries of k = " + std::to_string(k));
    }
    if (n && (!points || !hits)) return fail(GPUART_HIP_ERR_ARG, "nearest: points or hits is NULL");
    if (misaligned({points, hits}, align)) return fail(GPUART_HIP_ERR_ARG, "nearest: misaligned pointer (points and hits need " + std::to_string(align) + " bytes)");
    if (n && overlaps(points, n * 16, hits, n * (knn ? k : 1) * 32)) return fail(GPUART_HIP_ERR_ARG, "nearest: hits overlaps points");
    return 0;
}

int check_within(gpuart_nearest *h, const gpuart_hip_scene *s, const void *points, size_t n, const float us[4], const void *offsets, size_t align) {
    if (int rc = check_queries(h, s, n, us)) return rc;
    if (n && (!points || !offsets)) return fail(GPUART_HIP_ERR_ARG, "nearest: points or offsets is NULL");
    if (misaligned({points}, align) || misaligned({offsets}, 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: misaligned pointer (points needs " + std::to_string(align) + " bytes, offsets 4)");
    if (n && overlaps(points, n * 16, offsets, (n + 1) * 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets overlaps points");
    return 0;
}

int check_margin(float margin) {
    return nr::overlap_margin_ok(margin) ? 0 : fail(GPUART_HIP_ERR_ARG, "nearest: the margin is NaN, infinite or negative");
}

/// What the box queries check before a launch: the handle and its binding, n, the user sphere, the margin, the two arrays.
int check_overlap(gpuart_nearest *h, const gpuart_hip_scene *s, const void *boxes, size_t n, float margin, const float us[4], const void *offsets) {
    if (int rc = check_queries(h, s, n, us)) return rc;
    if (int rc = check_margin(margin)) return rc;
    if (n && (!boxes || !offsets)) return fail(GPUART_HIP_ERR_ARG, "nearest: boxes or offsets is NULL");
    if (misaligned({boxes, offsets}, 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: misaligned pointer (boxes and offsets need 4 bytes)");
    if (n && overlaps(boxes, n * 24, offsets, (n + 1) * 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets overlaps boxes");
    return 0;
}

/// What the pairs check: the handle and its binding, the margin, the offsets.
int check_pairs(gpuart_nearest *h, const gpuart_hip_scene *s, float margin, const void *offsets) {
    if (int rc = check_queries(h, s, s ? s->n_prims : 0, nullptr)) return rc;
    if (int rc = check_margin(margin)) return rc;
    if (!offsets) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets is NULL");
    if (misaligned({offsets}, 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: misaligned pointer (offsets needs 4 bytes)");
    return 0;
}

int check_items_aligned(const void *items, size_t align) {
    return misaligned({items}, align) ? fail(GPUART_HIP_ERR_ARG, "nearest: misaligned pointer (items needs " + std::to_string(align) + " bytes)") : 0;
}

int too_many(uint64_t total, uint64_t cap) {
    return fail(GPUART_HIP_ERR_ARG, "nearest: the lists hold " + std::to_string(total) + " items, more than the " + std::to_string(cap) + " a result may hold");
}

/// What every launch over n queries in device memory begins with: the grid — the blocks the spill budget pays for (a column entry is what
/// the kernel's stack holds: the lists' 4 bytes are half of k_nearest's), the blocks the work fills, and the kernel's `slot` under the
/// handle's limit —, the lanes' stack columns, the arguments every kernel has (its queries are the caller's to set), and the cursor at zero.
template <class A>
int prepare(gpuart_nearest *h, const gpuart_hip_scene *s, uint32_t n, const float us[4], uint32_t slot, A &a, uint32_t &grid) {
    const size_t levels = (size_t)s->max_depth + 2, block_bytes = levels * sizeof(*a.spill) * BLOCK;
    const size_t by_budget = std::max<size_t>(1, h->spill_budget / block_bytes);
    const size_t by_work = ((size_t)n + (size_t)CHUNK * WAVES - 1) / ((size_t)CHUNK * WAVES);
    grid = (uint32_t)std::min({by_budget, by_work, (size_t)std::min(h->max_blocks, h->blocks[slot])});
    if (int rc = ensure(h->stream, h->spill, block_bytes * grid)) return rc;
    a.sc = view_of(s);
    a.n = n;
    a.us = us ? make_float4(us[0], us[1], us[2], us[3]) : make_float4(0, 0, 0, 0);
    a.use_us = us ? 1u : 0u;
    a.spill = (decltype(a.spill))h->spill.mem;
    a.cap = (uint32_t)levels;
    a.cursor = h->cursor;
    a.status = h->status;
    HIP_TRY(hipMemsetAsync(h->cursor, 0, sizeof(uint32_t), h->stream));
    return 0;
}

/// One kernel on the handle's stream between the first two marks of `timer`, and the bookkeeping of a launch.
template <class A>
int launch_timed(gpuart_nearest *h, int timer, void (*kernel)(A), const A &a, uint32_t grid) {
    StepTimer &t = h->timers[timer];
    t.start(h->stream);
    HIP_TRY(t.mark());
    kernel<<<grid, BLOCK, 0, h->stream>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(t.mark());
    h->recorded[timer] = true;
    h->last_blocks = grid;
    h->last_launches++;
    return 0;
}

/// What a finished stream may have left in a word of the status: the word is read and, where it is set, cleared and the run fails with `text`.
int read_flag(gpuart_nearest *h, uint32_t *flag, const char *text) {
    uint32_t set = 0;
    HIP_TRY(hipMemcpyAsync(&set, flag, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (set) {
        HIP_TRY(hipMemsetAsync(flag, 0, 4, h->stream));
        return fail(GPUART_HIP_ERR_ARG, text);
    }
    return 0;
}

/// A walk that met a full stack column.
int read_overflow(gpuart_nearest *h) {
    return read_flag(h, &h->status->overflow, "nearest: a walk met a full stack: the tree is deeper than the descriptor's max_depth says; the results are void");
}

/// A fill whose lists were not what its offsets said.
int read_mismatch(gpuart_nearest *h) {
    return read_flag(h, &h->status->mismatch, "nearest: the offsets are not this query set's count: the results are void");
}

/// One launch of k_nearest (k = 0) or of the k_knn whose capacity holds k.
int launch(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, uint32_t n, uint32_t k, const float us[4], gpuart_nearest_hit *hits) {
    auto go = [&](auto a, void (*kernel)(decltype(a)), uint32_t slot, int timer) {
        uint32_t grid;
        if (int rc = prepare(h, s, n, us, slot, a, grid)) return rc;
        a.points = (const float4 *)points;
        a.hits = hits;
        return launch_timed(h, timer, kernel, a, grid);
    };
    if (!k) return go(Launch{}, k_nearest, K_NEAREST, T_WALK);
    KnnLaunch a{};
    a.k = k;
    const uint32_t size = knn_capacity(k);
    return go(a, KNN_KERNELS[size], K_KNN + size, T_KWALK);
}

/// A run of `launch` through host memory, staged in chunks: a chunk's records are no more than host_chunk, so of the k nearest it is
/// host_chunk / k queries, at least one. The staging buffer: a chunk's points, then its records.
int run_staged(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, size_t k, const float us[4], gpuart_nearest_hit *hits) {
    const size_t per = k ? k : 1, chunk = std::min(n, std::max<size_t>(1, h->host_chunk / per));
    h->last_launches = 0;
    if (int rc = ensure(h->stream, h->staging, chunk * (16 + 32 * per))) return rc;
    float *dpoints = (float *)h->staging.mem;
    gpuart_nearest_hit *dhits = (gpuart_nearest_hit *)((char *)h->staging.mem + chunk * 16);
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        HIP_TRY(hipMemcpyAsync(dpoints, points + 4 * at, m * 16, hipMemcpyHostToDevice, h->stream));
        if (int rc = launch(h, s, dpoints, (uint32_t)m, (uint32_t)k, us, dhits)) return rc;
        HIP_TRY(hipMemcpyAsync(hits + at * per, dhits, m * per * 32, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return read_overflow(h);
}

// ---- the lists: what the neighbour lists, the box queries and the pairs share on the host ------------------------------------------------
/// A launch struct with its queries set: the points of the neighbour lists; n boxes at `boxes` (device), or — pairs — the scene's own
/// boxes from the ordinal `first` on.
WLaunch within_launch(const void *points) {
    WLaunch a{};
    a.points = (const float4 *)points;
    return a;
}
OLaunch overlap_launch(const void *boxes, float margin, bool pairs = false, size_t first = 0) {
    OLaunch a{};
    a.boxes = (const float *)boxes;
    a.self0 = (uint32_t)first;
    a.pairs = pairs ? 1u : 0u;
    a.margin = margin;
    return a;
}
OLaunch pairs_launch(const gpuart_hip_scene *s, float margin, size_t first = 0) { return overlap_launch((const float *)s->prim_boxes + 6 * first, margin, true, first); }

/// The count of a's n queries into offsets[0 .. n] (device), scanned in place; the total stays in the status.
template <class A>
int launch_count(gpuart_nearest *h, const gpuart_hip_scene *s, A a, uint32_t n, const float us[4], int kind, uint32_t *offsets) {
    const ListKernels<A> &ks = kernels_of(a);
    uint32_t grid;
    if (int rc = prepare(h, s, n, us, ks.slot, a, grid)) return rc;
    a.offsets = offsets;
    size_t scan_bytes = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, scan_bytes, offsets, offsets, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), h->stream));
    if (int rc = ensure(h->stream, h->scan_temp, scan_bytes + 16)) return rc;
    HIP_TRY(hipMemsetAsync(&h->status->total, 0, sizeof(unsigned long long), h->stream));
    HIP_TRY(hipMemsetAsync(offsets + n, 0, sizeof(uint32_t), h->stream));
    if (int rc = launch_timed(h, ks.timer, ks.count, a, grid)) return rc;
    HIP_TRY(rocprim::exclusive_scan(h->scan_temp.mem, scan_bytes, offsets, offsets, 0u, (size_t)n + 1, rocprim::plus<uint32_t>(), h->stream));
    HIP_TRY(h->timers[ks.timer].mark());
    h->total_read = false;
    h->counted_n = n;
    h->counted_kind = kind;
    return 0;
}

/// A count of no queries launches nothing.
void counted_nothing(gpuart_nearest *h, int kind) {
    h->last_total = 0;
    h->total_read = true;
    h->counted_n = 0;
    h->counted_kind = kind;
}

/// The fill of a's n queries: list i into items from offsets[i] on (device), below `capacity`.
template <class A, class Item>
int launch_fill(gpuart_nearest *h, const gpuart_hip_scene *s, A a, uint32_t n, const float us[4], const uint32_t *offsets, Item *items, uint32_t capacity) {
    const ListKernels<A> &ks = kernels_of(a);
    uint32_t grid;
    if (int rc = prepare(h, s, n, us, ks.slot + 1, a, grid)) return rc;
    a.offsets = const_cast<uint32_t *>(offsets);
    a.items = items;
    a.capacity = capacity;
    if (int rc = launch_timed(h, ks.timer + 1, ks.fill, a, grid)) return rc;
    h->fill_pending = true;
    return 0;
}

/// Waits for the stream and reads the last count's total.
int read_total(gpuart_nearest *h) {
    if (h->total_read) return 0;
    unsigned long long t = 0;
    HIP_TRY(hipMemcpyAsync(&t, &h->status->total, 8, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_total = t;
    h->total_read = true;
    return 0;
}

/// What a device fill of `kind` checks behind its queries: items, the last count — its n, its kind, its total against the caps and the
/// capacity — and what items may not overlap. `items_are`: what an item is called ("records", "ordinals"), `queries_are` likewise.
/// Returns 1 where there is nothing to fill.
int check_fill(gpuart_nearest *h, int kind, size_t n, const void *queries, size_t query_bytes, const char *queries_are, const uint32_t *offsets, const void *items,
               size_t item_bytes, size_t item_align, const char *items_are, size_t &capacity) {
    if (int rc = check_items_aligned(items, item_align)) return rc;
    if (n != h->counted_n) return fail(GPUART_HIP_ERR_ARG, "nearest: the last count was of " + std::to_string(h->counted_n) + " queries, not of " + std::to_string(n));
    // A fill of no neighbour lists succeeds whatever the last count was of; the other two kinds look at whose it was first. The difference
    // is the entry points' as they were written, kept as it is (tests/test_overlap.py holds the table).
    if (!n && kind == COUNT_WITHIN) return 1;
    if (h->counted_kind != kind)
        return fail(GPUART_HIP_ERR_ARG, std::string("nearest: the last count was of ") + COUNT_NAMES[h->counted_kind] + ", this fill is of " + COUNT_NAMES[kind]);
    if (!n) return 1;
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = read_total(h)) return rc;
    if (h->last_total > h->max_items) return too_many(h->last_total, h->max_items);
    if (capacity < h->last_total)
        return fail(GPUART_HIP_ERR_ARG, "nearest: items has room for " + std::to_string(capacity) + " " + items_are + ", the last count's total is " + std::to_string(h->last_total));
    if (capacity && !items) return fail(GPUART_HIP_ERR_ARG, "nearest: items is NULL");
    capacity = std::min<size_t>(capacity, GPUART_NEAREST_WITHIN_MAX_ITEMS);
    if (capacity && ((queries && overlaps(items, capacity * item_bytes, queries, query_bytes)) || overlaps(items, capacity * item_bytes, offsets, (n + 1) * 4)))
        return fail(GPUART_HIP_ERR_ARG, std::string("nearest: items overlaps ") + queries_are + " or offsets");
    h->last_launches = 0;
    return 0;
}

/// What a _fill_host entry checks of the caller's offsets (host) and items behind its queries. Returns 1 where there is nothing to fill.
int check_host_fill(gpuart_nearest *h, size_t n, const uint32_t *offsets, const void *items, const char *items_are, size_t capacity) {
    if (!offsets) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets is NULL");
    if (int rc = check_items_aligned(items, 4)) return rc;
    if (offsets[0] != 0) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets[0] is not 0");
    for (size_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return fail(GPUART_HIP_ERR_ARG, "nearest: the offsets decrease at query " + std::to_string(i));
    const uint64_t total = offsets[n];
    if (total > h->max_items) return too_many(total, h->max_items);
    if (capacity < total)
        return fail(GPUART_HIP_ERR_ARG, "nearest: items has room for " + std::to_string(capacity) + " " + items_are + ", the offsets end at " + std::to_string(total));
    if (total && !items) return fail(GPUART_HIP_ERR_ARG, "nearest: items is NULL");
    h->last_launches = 0;
    if (!n) return 1;
    HIP_TRY(hipSetDevice(h->device));
    return 0;
}

/// What the entries that read something back open with: the handle, where to put it (`name` for the text), the device, a finished stream.
int open_read(gpuart_nearest *h, const void *out, const char *name) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!out) return fail(GPUART_HIP_ERR_ARG, std::string("nearest: ") + name + " is NULL");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

/// gpuart_nearest_*_step_ms: the steps of the timers first .. first + count - 1, read where they have been recorded.
int step_ms(gpuart_nearest *h, int first, int count, double *ms) {
    if (int rc = open_read(h, ms, "ms")) return rc;
    for (int t = first; t < first + count; t++) {
        if (h->recorded[t])  // (bind reads its own: T_CHECK is never marked as recorded)
            if (int rc = h->timers[t].read()) return rc;
        for (int k = 0; k < TIMER_STEPS[t]; k++) *ms++ = h->timers[t].ms[k];
    }
    return 0;
}

/// The two NEAREST_COUNT counters of the status from `first` on, read once the stream has finished, and zeroed.
int read_counts(gpuart_nearest *h, unsigned long long Status::*first, uint64_t out[2]) {
    if (int rc = open_read(h, out, "out")) return rc;
    unsigned long long c[2];
    HIP_TRY(hipMemcpy(c, &(h->status->*first), 16, hipMemcpyDeviceToHost));
    out[0] = c[0]; out[1] = c[1];
    HIP_TRY(hipMemset(&(h->status->*first), 0, 16));
    return 0;
}

/// Both passes of a list run into host memory, staged in chunks of host_chunk queries. The count: a chunk's queries go up (query_bytes each;
/// 0 for the pairs, whose launch takes its first ordinal), its lengths come back and are rebased by the running total. The fill: the
/// offsets, made local to the chunk, go up with the queries and the chunk's items come back to items + offsets[chunk]. fill_only: the
/// offsets (ascending, n + 1) are the caller's. make(at, queries): the launch struct of the chunk that begins at query `at`, its queries
/// in device memory. The staging buffer: a chunk's queries, then its offsets, then — on a 16-byte boundary — its items.
template <class Item, class Make>
int lists_staged(gpuart_nearest *h, const gpuart_hip_scene *s, const void *queries, size_t query_bytes, size_t n, const float us[4], int kind, uint32_t *offsets,
                 Item *items, size_t capacity, uint64_t *total, bool fill_only, Make make) {
    const size_t chunk = std::min(n, h->host_chunk);
    h->host_offsets.resize(chunk + 1);
    uint32_t *local = h->host_offsets.data();
    const size_t head = (chunk * query_bytes + (chunk + 1) * 4 + 15) / 16 * 16;
    auto doffsets = [&] { return (uint32_t *)((char *)h->staging.mem + chunk * query_bytes); };
    auto send_queries = [&](size_t at, size_t m) {
        return query_bytes ? hipMemcpyAsync(h->staging.mem, (const char *)queries + at * query_bytes, m * query_bytes, hipMemcpyHostToDevice, h->stream) : hipSuccess;
    };
    if (!fill_only) {
        if (int rc = ensure(h->stream, h->staging, head)) return rc;
        uint64_t base = 0;
        for (size_t at = 0; at < n; at += chunk) {
            const size_t m = std::min(chunk, n - at);
            HIP_TRY(send_queries(at, m));
            if (int rc = launch_count(h, s, make(at, h->staging.mem), (uint32_t)m, us, kind, doffsets())) return rc;
            HIP_TRY(hipMemcpyAsync(local, doffsets(), m * 4, hipMemcpyDeviceToHost, h->stream));
            if (int rc = read_total(h)) return rc;
            for (size_t k = 0; k < m; k++) offsets[at + k] = (uint32_t)(base + local[k]);  // (rebased: the chunk's lists follow the earlier chunks')
            base += h->last_total;
        }
        offsets[n] = (uint32_t)base;
        *total = base;
        h->last_total = base;
        h->counted_n = n;
        if (int rc = read_overflow(h)) return rc;
        if (base > h->max_items) return too_many(base, h->max_items);
        if (!items || capacity < base) return 0;
    }
    for (size_t at = 0; at < n; at += chunk) {
        const size_t m = std::min(chunk, n - at);
        const size_t room = offsets[at + m] - offsets[at];
        if (int rc = ensure(h->stream, h->staging, head + room * sizeof(Item))) return rc;
        Item *ditems = (Item *)((char *)h->staging.mem + head);
        for (size_t k = 0; k <= m; k++) local[k] = offsets[at + k] - offsets[at];
        HIP_TRY(send_queries(at, m));
        HIP_TRY(hipMemcpyAsync(doffsets(), local, (m + 1) * 4, hipMemcpyHostToDevice, h->stream));
        if (int rc = launch_fill(h, s, make(at, h->staging.mem), (uint32_t)m, us, doffsets(), ditems, (uint32_t)room)) return rc;
        if (room) HIP_TRY(hipMemcpyAsync(items + offsets[at], ditems, room * sizeof(Item), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->fill_pending = false;
    if (int rc = read_overflow(h)) return rc;
    return read_mismatch(h);
}

/// What the three _host entries do behind their checks: an empty result, then the staged run.
template <class Item, class Make>
int lists_host(gpuart_nearest *h, const gpuart_hip_scene *s, const void *queries, size_t query_bytes, size_t n, const float us[4], int kind, uint32_t *offsets,
               Item *items, size_t capacity, uint64_t *total, Make make) {
    if (int rc = check_items_aligned(items, 4)) return rc;
    offsets[0] = 0;
    *total = 0;
    h->last_launches = 0;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(h->device));
    return lists_staged(h, s, queries, query_bytes, n, us, kind, offsets, items, capacity, total, false, make);
}

// ---- the definitions on host arrays -------------------------------------------------------------------------------------------------------
int tree_order(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, size_t n_prims, std::vector<uint32_t> &order);

/// The two passes of a definition: visit(i, emit) calls emit(item) for every item of list i, in the contract's order. Offsets and the total
/// from a first pass, the cap, and — with room for them — the items from a second.
template <class Item, class Visit>
int two_passes(size_t n, Visit visit, uint32_t *offsets, Item *items, size_t capacity, uint64_t *total) {
    uint64_t sum = 0;
    for (size_t i = 0; i < n; i++) {
        offsets[i] = (uint32_t)sum;
        visit(i, [&](const Item &) { sum++; });
    }
    offsets[n] = (uint32_t)sum;
    *total = sum;
    if (sum > GPUART_NEAREST_WITHIN_MAX_ITEMS) return too_many(sum, GPUART_NEAREST_WITHIN_MAX_ITEMS);
    if (!items || capacity < sum) return 0;
    size_t at = 0;
    for (size_t i = 0; i < n; i++) visit(i, [&](const Item &item) { items[at++] = item; });
    return 0;
}

/// The definition on host arrays, for box queries (boxes != NULL) and pairs: every primitive tested in the tree's order.
int overlap_brute(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims, const float *boxes, size_t n,
                  float margin, const float us[4], uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    const bool pairs = !boxes;
    if (int rc = check_margin(margin)) return rc;
    if (int rc = check_user_sphere(us)) return rc;
    std::vector<uint32_t> order;
    if (int rc = tree_order(recs, n_recs, root_ref, prims, n_prims, order)) return rc;
    auto visit = [&](size_t i, auto &&emit) {
        const float *box = pairs ? prim_boxes + 6 * i : boxes + 6 * i;
        float qlo[3], qhi[3];
        if (!nr::overlap_query_ok(box)) return;
        nr::overlap_inflate(box, margin, qlo, qhi);
        if (us) {
            PrimData d;
            user_sphere_prim(us[0], us[1], us[2], us[3], d);
            if (nr::overlap_test(qlo, qhi, d.box, d.box + 3)) emit((int32_t)nr::USER_SPHERE);
        }
        for (const uint32_t k : order) {
            const float *b = prim_boxes + 6 * (size_t)k;
            if (nr::overlap_test(qlo, qhi, b, b + 3) && (!pairs || nr::pairs_keep((uint32_t)i, k))) emit((int32_t)k);
        }
    };
    return two_passes(n, visit, offsets, items, capacity, total);
}

/// The ordinals in the order of the unpruned depth-first walk from root_ref, lower child first; 0, or why the records are refused.
int tree_order(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, size_t n_prims, std::vector<uint32_t> &order) {
    order.clear();
    if (!n_prims) return 0;
    std::vector<uint32_t> stack{root_ref};
    size_t visited = 0;
    while (!stack.empty()) {
        const uint32_t ref = stack.back();
        stack.pop_back();
        if (!(ref & REF_LEAF)) {
            if (ref >= n_recs || ++visited > n_recs) return fail(GPUART_HIP_ERR_ARG, "nearest: a ref is out of range, or the records are no tree");
            uint32_t lo, hi;
            memcpy(&lo, recs + 16 * (size_t)ref + 3, 4);
            memcpy(&hi, recs + 16 * (size_t)ref + 7, 4);
            stack.push_back(hi);
            stack.push_back(lo);
            continue;
        }
        const uint32_t first = ref & REF_INDEX;
        if (first >= n_prims) return fail(GPUART_HIP_ERR_ARG, "nearest: a leaf is out of range");
        uint32_t w;
        memcpy(&w, prims + 12 * (size_t)first + 3, 4);
        const uint32_t count = (ref & (REF_TRIS | REF_SMALL)) ? ((ref & REF_TWO) ? 2u : 1u) : w >> 2;
        if (count > n_prims - first || order.size() + count > n_prims) return fail(GPUART_HIP_ERR_ARG, "nearest: a leaf is out of range, or the records are no tree");
        for (uint32_t k = 0; k < count; k++) order.push_back(first + k);
    }
    if (order.size() != n_prims) return fail(GPUART_HIP_ERR_ARG, "nearest: the records reach " + std::to_string(order.size()) + " of " + std::to_string(n_prims) + " primitives");
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_nearest_last_error(void) { return g_last_error.c_str(); }

int gpuart_nearest_create(int device, gpuart_nearest **out) {
    const int rc = create_tree_handle(LIB, device, out, gpuart_nearest_destroy, [](gpuart_nearest *h) {
        hipError_t e = hipMalloc((void **)&h->status, sizeof(Status));
        if (e == hipSuccess) e = hipMalloc((void **)&h->cursor, sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemset(h->status, 0, sizeof(Status));
        for (int t = 0; t < TIMERS && e == hipSuccess; t++) e = h->timers[t].create(TIMER_STEPS[t]);
        return e;
    });
    if (rc) return rc;
    gpuart_nearest *h = *out;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 1;
    auto held = [&](uint32_t slot, auto kernel) {  // the workgroups of `kernel` the device holds at once
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, BLOCK, 0) != hipSuccess || per_cu < 1) per_cu = 1;
        h->blocks[slot] = (uint32_t)per_cu * (uint32_t)cus;
    };
    held(K_NEAREST, k_nearest);
    held(K_WCOUNT, k_within_count);
    held(K_WFILL, k_within_fill);
    held(K_OCOUNT, k_overlap_count);
    held(K_OFILL, k_overlap_fill);
    for (uint32_t k = 0; k < KNN_SIZES; k++) held(K_KNN + k, KNN_KERNELS[k]);  // (the lists' LDS sets it: 2 KiB per entry of the capacity beside the ring's 16 KiB)
    h->max_blocks = h->blocks[K_NEAREST];
    return 0;
}

int gpuart_nearest_destroy(gpuart_nearest *h) {
    if (!h) return 0;
    destroy_handle(h, {h->status, h->cursor, h->spill.mem, h->staging.mem, h->scan_temp.mem});
    for (StepTimer &t : h->timers) t.destroy();
    delete h;
    return 0;
}

int gpuart_nearest_finish(gpuart_nearest *h) {
    if (int rc = finish_handle(LIB, h)) return rc;
    if (int rc = read_overflow(h)) return rc;
    if (!h->fill_pending) return 0;
    h->fill_pending = false;
    return read_mismatch(h);
}

int gpuart_nearest_bind(gpuart_nearest *h, const gpuart_hip_scene *s) {
    if (int rc = check_handle(LIB, h)) return rc;
    h->bound = false;
    h->counted_n = 0;  // (the status is zeroed below, the last count's total with it: a fill wants a count of this binding)
    h->last_total = 0;
    h->total_read = true;
    h->counted_kind = 0;
    if (!s) return fail(GPUART_HIP_ERR_ARG, "nearest: scene is NULL");
    if (int rc = check_descriptor(s, LIB, "", "queried for closest points", true)) return rc;
    if (misaligned({s->recs, s->prims}, 16) || misaligned({s->prim_boxes}, 4)) return fail(GPUART_HIP_ERR_ARG, "nearest: misaligned arrays");
    if (!tree_rule::box_ok(s->root_min, s->root_max)) return fail(GPUART_HIP_ERR_ARG, "nearest: the root box is not finite and ordered");
    if (s->max_depth > GPUART_NEAREST_MAX_DEPTH)
        return fail(GPUART_HIP_ERR_ARG, "nearest: the descriptor says a tree of " + std::to_string(s->max_depth) + " levels: more than " +
                                            std::to_string(GPUART_NEAREST_MAX_DEPTH) + ", the deepest tree an upload or a rebuild accepts");
    if (!tree_rule::root_ref_ok(s->root_ref, s->n_recs, s->n_prims)) return fail(GPUART_HIP_ERR_ARG, "nearest: the root ref is neither record 0 nor a leaf inside the primitives");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->status, 0, sizeof(Status), h->stream));
    StepTimer &check = h->timers[T_CHECK];
    check.start(h->stream);
    HIP_TRY(check.mark());
    k_nr_nesting<<<blocks(s->n_recs + 1), 256, 0, h->stream>>>(view_of(s), h->status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(check.mark());
    uint32_t refused = 0;
    HIP_TRY(hipMemcpyAsync(&refused, &h->status->refused, 4, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (int rc = check.read()) return rc;
    if (refused) {
        const char *const why[4] = {"", "a box it holds is not finite and ordered", "a ref or a leaf's count it holds is out of range, or an interior child is not behind its parent",
                                    "a child's boxes (or a leaf's primitive boxes) do not lie inside the box it holds for that child"};
        const uint32_t r = refused_index(refused);
        return fail(GPUART_HIP_ERR_ARG, "nearest: " + (r == s->n_recs ? std::string("the root") : "record " + std::to_string(r)) + " refused: " + why[~refused & 3u] +
                                            "; a pruned walk is exact only in a tree of nested boxes");
    }
    h->scene = *s;
    h->bound = true;
    return 0;
}

int gpuart_nearest_run(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], gpuart_nearest_hit *hits) {
    if (int rc = check_hits(h, s, points, n, 0, false, us, hits, 16)) return rc;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(h->device));
    h->last_launches = 0;
    return launch(h, s, points, (uint32_t)n, 0, us, hits);
}

int gpuart_nearest_run_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], gpuart_nearest_hit *hits) {
    if (int rc = check_hits(h, s, points, n, 0, false, us, hits, 4)) return rc;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(h->device));
    return run_staged(h, s, points, n, 0, us, hits);
}

int gpuart_nearest_brute_host(gpuart_nearest *, const float *, size_t, const float *prims, const float *prim_boxes, size_t n_prims, const float *points, size_t n,
                              const float us[4], gpuart_nearest_hit *hits) {
    if ((n_prims && (!prims || !prim_boxes)) || (n && (!points || !hits))) return fail(GPUART_HIP_ERR_ARG, "nearest: prims, prim_boxes, points or hits is NULL");
    if (n_prims > REF_INDEX) return fail(GPUART_HIP_ERR_ARG, "nearest: too many primitives: " + std::to_string(n_prims));
    if (int rc = check_user_sphere(us)) return rc;
    for (size_t i = 0; i < n; i++) {
        const float *p = points + 4 * i, r = p[3], r2 = r * r;
        float best = INFINITY, bq[3] = {0, 0, 0}, q[3];
        uint32_t ord = nr::NO_PRIM, type = 0;
        if (nr::query_ok(p, r)) {
            if (us) {
                PrimData d;
                user_sphere_prim(us[0], us[1], us[2], us[3], d);
                const float d2 = nr::closest_on_prim(nr::SPHERE, d.rec, d.box, p, q);
                if (nr::better(d2, nr::USER_SPHERE, r2, best, ord)) { best = d2; ord = nr::USER_SPHERE; type = nr::SPHERE; memcpy(bq, q, 12); }
            }
            for (size_t k = 0; k < n_prims; k++) {
                const float *rec = prims + 12 * k;
                uint32_t w;
                memcpy(&w, rec + 3, 4);
                const float d2 = nr::closest_on_prim(w & 3u, rec, prim_boxes + 6 * k, p, q);
                if (nr::better(d2, (uint32_t)k, r2, best, ord)) { best = d2; ord = (uint32_t)k; type = w & 3u; memcpy(bq, q, 12); }
            }
        }
        gpuart_nearest_hit &o = hits[i];
        if (ord == nr::NO_PRIM) o = gpuart_nearest_hit{-1.0f, {0, 0, 0}, 0.0f, -1, -1, 0};
        else o = gpuart_nearest_hit{sqrtf(best), {bq[0], bq[1], bq[2]}, best, (int32_t)ord, (int32_t)type, 0};
    }
    return 0;
}

int gpuart_nearest_step_ms(gpuart_nearest *h, double ms[2]) { return step_ms(h, T_CHECK, 2, ms); }

int gpuart_nearest_set_limits(gpuart_nearest *h, uint32_t max_blocks, size_t spill_bytes, size_t host_chunk) {
    if (int rc = check_handle(LIB, h)) return rc;
    h->max_blocks = max_blocks ? std::min(max_blocks, h->blocks[K_NEAREST]) : h->blocks[K_NEAREST];
    h->spill_budget = spill_bytes ? spill_bytes : SPILL_BUDGET;
    h->host_chunk = host_chunk ? std::min(host_chunk, HOST_CHUNK) : HOST_CHUNK;
    return 0;
}

int gpuart_nearest_last_launch(gpuart_nearest *h, uint32_t *blocks, uint32_t *launches) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (blocks) *blocks = h->last_blocks;
    if (launches) *launches = h->last_launches;
    return 0;
}

int gpuart_nearest_counts(gpuart_nearest *h, uint64_t out[2]) { return read_counts(h, &Status::box_steps, out); }

// ---- the neighbour lists --------------------------------------------------------------------------------------------------------------
int gpuart_nearest_within_count(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], uint32_t *offsets) {
    if (int rc = check_within(h, s, points, n, us, offsets, 16)) return rc;
    h->last_launches = 0;
    if (!n) {
        counted_nothing(h, COUNT_WITHIN);
        return 0;
    }
    HIP_TRY(hipSetDevice(h->device));
    return launch_count(h, s, within_launch(points), (uint32_t)n, us, COUNT_WITHIN, offsets);
}

int gpuart_nearest_within_total(gpuart_nearest *h, uint64_t *total) {
    if (int rc = check_handle(LIB, h)) return rc;
    if (!total) return fail(GPUART_HIP_ERR_ARG, "nearest: total is NULL");
    HIP_TRY(hipSetDevice(h->device));
    if (int rc = read_total(h)) return rc;
    *total = h->last_total;
    return h->last_total > h->max_items ? too_many(h->last_total, h->max_items) : 0;
}

int gpuart_nearest_within_fill(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], const uint32_t *offsets,
                               gpuart_nearest_hit *items, size_t capacity) {
    if (int rc = check_within(h, s, points, n, us, offsets, 16)) return rc;
    if (int rc = check_fill(h, COUNT_WITHIN, n, points, n * 16, "points", offsets, items, 32, 16, "records", capacity)) return rc < 0 ? rc : 0;
    return launch_fill(h, s, within_launch(points), (uint32_t)n, us, offsets, items, (uint32_t)capacity);
}

int gpuart_nearest_within_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], uint32_t *offsets,
                               gpuart_nearest_hit *items, size_t capacity, uint64_t *total) {
    if (int rc = check_within(h, s, points, n, us, offsets, 4)) return rc;
    if (!offsets || !total) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets or total is NULL");
    return lists_host(h, s, points, 16, n, us, COUNT_WITHIN, offsets, items, capacity, total, [](size_t, const void *staged) { return within_launch(staged); });
}

int gpuart_nearest_within_fill_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, const float us[4], const uint32_t *offsets,
                                    gpuart_nearest_hit *items, size_t capacity) {
    if (int rc = check_within(h, s, points, n, us, offsets, 4)) return rc;
    if (int rc = check_host_fill(h, n, offsets, items, "records", capacity)) return rc < 0 ? rc : 0;
    return lists_staged(h, s, points, 16, n, us, COUNT_WITHIN, const_cast<uint32_t *>(offsets), items, capacity, nullptr, true,
                        [](size_t, const void *staged) { return within_launch(staged); });
}

int gpuart_nearest_within_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims,
                                     const float *points, size_t n, const float us[4], uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity,
                                     uint64_t *total) {
    if ((n_prims && (!prims || !prim_boxes)) || (n_recs && !recs) || (n && !points) || !offsets || !total)
        return fail(GPUART_HIP_ERR_ARG, "nearest: recs, prims, prim_boxes, points, offsets or total is NULL");
    if (n_prims > REF_INDEX || n_recs > REF_INDEX) return fail(GPUART_HIP_ERR_ARG, "nearest: too many primitives or records: " + std::to_string(n_prims));
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "nearest: too many queries: " + std::to_string(n));
    if (int rc = check_user_sphere(us)) return rc;
    std::vector<uint32_t> order;
    if (int rc = tree_order(recs, n_recs, root_ref, prims, n_prims, order)) return rc;
    // one rule for both passes: visit(i, emit) calls emit(record) for every item of list i, in the contract's order
    auto visit = [&](size_t i, auto &&emit) {
        const float *p = points + 4 * i, r = p[3], r2 = r * r;
        float q[3];
        if (!nr::query_ok(p, r)) return;
        if (us) {
            PrimData d;
            user_sphere_prim(us[0], us[1], us[2], us[3], d);
            const float d2 = nr::closest_on_prim(nr::SPHERE, d.rec, d.box, p, q);
            if (nr::within_accept(d2, r2)) emit(gpuart_nearest_hit{sqrtf(d2), {q[0], q[1], q[2]}, d2, (int32_t)nr::USER_SPHERE, (int32_t)nr::SPHERE, 0});
        }
        for (const uint32_t k : order) {
            const float *rec = prims + 12 * (size_t)k;
            uint32_t w;
            memcpy(&w, rec + 3, 4);
            const float d2 = nr::closest_on_prim(w & 3u, rec, prim_boxes + 6 * (size_t)k, p, q);
            if (nr::within_accept(d2, r2)) emit(gpuart_nearest_hit{sqrtf(d2), {q[0], q[1], q[2]}, d2, (int32_t)k, (int32_t)(w & 3u), 0});
        }
    };
    return two_passes(n, visit, offsets, items, capacity, total);
}

int gpuart_nearest_within_set_max_items(gpuart_nearest *h, uint64_t max_items) {
    if (int rc = check_handle(LIB, h)) return rc;
    h->max_items = max_items ? std::min<uint64_t>(max_items, GPUART_NEAREST_WITHIN_MAX_ITEMS) : GPUART_NEAREST_WITHIN_MAX_ITEMS;
    return 0;
}

int gpuart_nearest_within_step_ms(gpuart_nearest *h, double ms[3]) { return step_ms(h, T_WCOUNT, 2, ms); }

int gpuart_nearest_within_counts(gpuart_nearest *h, uint64_t out[2]) { return read_counts(h, &Status::w_box_steps, out); }

// ---- the k nearest ----------------------------------------------------------------------------------------------------------------------
int gpuart_nearest_knn_run(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, size_t k, const float us[4], gpuart_nearest_hit *hits) {
    if (int rc = check_hits(h, s, points, n, k, true, us, hits, 16)) return rc;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(h->device));
    h->last_launches = 0;
    return launch(h, s, points, (uint32_t)n, (uint32_t)k, us, hits);
}

int gpuart_nearest_knn_run_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *points, size_t n, size_t k, const float us[4], gpuart_nearest_hit *hits) {
    if (int rc = check_hits(h, s, points, n, k, true, us, hits, 4)) return rc;
    if (!n) return 0;
    HIP_TRY(hipSetDevice(h->device));
    return run_staged(h, s, points, n, k, us, hits);
}

int gpuart_nearest_knn_brute_host(gpuart_nearest *, const float *, size_t, const float *prims, const float *prim_boxes, size_t n_prims, const float *points, size_t n,
                                  size_t k, const float us[4], gpuart_nearest_hit *hits) {
    if ((n_prims && (!prims || !prim_boxes)) || (n && (!points || !hits))) return fail(GPUART_HIP_ERR_ARG, "nearest: prims, prim_boxes, points or hits is NULL");
    if (n_prims > REF_INDEX) return fail(GPUART_HIP_ERR_ARG, "nearest: too many primitives: " + std::to_string(n_prims));
    if (k < 1 || k > GPUART_NEAREST_KNN_MAX) return fail(GPUART_HIP_ERR_ARG, "nearest: k is " + std::to_string(k) + ": not in 1 .. " + std::to_string(GPUART_NEAREST_KNN_MAX));
    if (int rc = check_user_sphere(us)) return rc;
    std::vector<gpuart_nearest_hit> accepted;
    for (size_t i = 0; i < n; i++) {
        const float *p = points + 4 * i, r = p[3], r2 = r * r;
        accepted.clear();
        if (nr::query_ok(p, r)) {
            float q[3];
            for (size_t c = 0; c < n_prims + (us ? 1 : 0); c++) {  // every primitive, the user sphere behind them
                PrimData d;
                const bool sphere = c == n_prims;
                if (sphere) {
                    user_sphere_prim(us[0], us[1], us[2], us[3], d);
                } else {
                    memcpy(d.rec, prims + 12 * c, 48);
                    memcpy(d.box, prim_boxes + 6 * c, 24);
                }
                uint32_t w;
                memcpy(&w, d.rec + 3, 4);
                const float d2 = nr::closest_on_prim(w & 3u, d.rec, d.box, p, q);
                if (nr::within_accept(d2, r2))
                    accepted.push_back(gpuart_nearest_hit{sqrtf(d2), {q[0], q[1], q[2]}, d2, (int32_t)(sphere ? nr::USER_SPHERE : (uint32_t)c), (int32_t)(w & 3u), 0});
            }
        }
        const size_t found = std::min(k, accepted.size());
        std::partial_sort(accepted.begin(), accepted.begin() + found, accepted.end(), [](const gpuart_nearest_hit &x, const gpuart_nearest_hit &y) {
            return nr::knn_before(x.d2, (uint32_t)x.prim, y.d2, (uint32_t)y.prim);
        });
        for (size_t j = 0; j < k; j++) hits[i * k + j] = j < found ? accepted[j] : gpuart_nearest_hit{-1.0f, {0, 0, 0}, 0.0f, -1, -1, 0};
    }
    return 0;
}

int gpuart_nearest_knn_step_ms(gpuart_nearest *h, double ms[1]) { return step_ms(h, T_KWALK, 1, ms); }

int gpuart_nearest_knn_counts(gpuart_nearest *h, uint64_t out[2]) { return read_counts(h, &Status::k_box_steps, out); }

// ---- box overlap: box queries ---------------------------------------------------------------------------------------------------------------
int gpuart_nearest_overlap_count(gpuart_nearest *h, const gpuart_hip_scene *s, const float *boxes, size_t n, float margin, const float us[4], uint32_t *offsets) {
    if (int rc = check_overlap(h, s, boxes, n, margin, us, offsets)) return rc;
    h->last_launches = 0;
    if (!n) {
        counted_nothing(h, COUNT_OVERLAP);
        return 0;
    }
    HIP_TRY(hipSetDevice(h->device));
    return launch_count(h, s, overlap_launch(boxes, margin), (uint32_t)n, us, COUNT_OVERLAP, offsets);
}

int gpuart_nearest_overlap_total(gpuart_nearest *h, uint64_t *total) { return gpuart_nearest_within_total(h, total); }

int gpuart_nearest_overlap_fill(gpuart_nearest *h, const gpuart_hip_scene *s, const float *boxes, size_t n, float margin, const float us[4], const uint32_t *offsets,
                                int32_t *items, size_t capacity) {
    if (int rc = check_overlap(h, s, boxes, n, margin, us, offsets)) return rc;
    if (int rc = check_fill(h, COUNT_OVERLAP, n, boxes, n * 24, "boxes", offsets, items, 4, 4, "ordinals", capacity)) return rc < 0 ? rc : 0;
    return launch_fill(h, s, overlap_launch(boxes, margin), (uint32_t)n, us, offsets, items, (uint32_t)capacity);
}

int gpuart_nearest_overlap_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *boxes, size_t n, float margin, const float us[4], uint32_t *offsets,
                                int32_t *items, size_t capacity, uint64_t *total) {
    if (int rc = check_overlap(h, s, boxes, n, margin, us, offsets)) return rc;
    if (!offsets || !total) return fail(GPUART_HIP_ERR_ARG, "nearest: offsets or total is NULL");
    return lists_host(h, s, boxes, 24, n, us, COUNT_OVERLAP, offsets, items, capacity, total, [&](size_t, const void *staged) { return overlap_launch(staged, margin); });
}

int gpuart_nearest_overlap_fill_host(gpuart_nearest *h, const gpuart_hip_scene *s, const float *boxes, size_t n, float margin, const float us[4],
                                     const uint32_t *offsets, int32_t *items, size_t capacity) {
    if (int rc = check_overlap(h, s, boxes, n, margin, us, offsets)) return rc;
    if (int rc = check_host_fill(h, n, offsets, items, "ordinals", capacity)) return rc < 0 ? rc : 0;
    return lists_staged(h, s, boxes, 24, n, us, COUNT_OVERLAP, const_cast<uint32_t *>(offsets), items, capacity, nullptr, true,
                        [&](size_t, const void *staged) { return overlap_launch(staged, margin); });
}

int gpuart_nearest_overlap_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims,
                                      const float *boxes, size_t n, float margin, const float us[4], uint32_t *offsets, int32_t *items, size_t capacity,
                                      uint64_t *total) {
    if ((n_prims && (!prims || !prim_boxes)) || (n_recs && !recs) || (n && !boxes) || !offsets || !total)
        return fail(GPUART_HIP_ERR_ARG, "nearest: recs, prims, prim_boxes, boxes, offsets or total is NULL");
    if (n_prims > REF_INDEX || n_recs > REF_INDEX) return fail(GPUART_HIP_ERR_ARG, "nearest: too many primitives or records: " + std::to_string(n_prims));
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "nearest: too many queries: " + std::to_string(n));
    const float none[6] = {0, 0, 0, 0, 0, 0};
    return overlap_brute(recs, n_recs, root_ref, prims, prim_boxes, n_prims, n ? boxes : none, n, margin, us, offsets, items, capacity, total);
}

int gpuart_nearest_overlap_step_ms(gpuart_nearest *h, double ms[3]) { return step_ms(h, T_OCOUNT, 2, ms); }

int gpuart_nearest_overlap_counts(gpuart_nearest *h, uint64_t out[2]) { return read_counts(h, &Status::o_box_steps, out); }

// ---- box overlap: pairs -----------------------------------------------------------------------------------------------------------------------
int gpuart_nearest_pairs_count(gpuart_nearest *h, const gpuart_hip_scene *s, float margin, uint32_t *offsets) {
    if (int rc = check_pairs(h, s, margin, offsets)) return rc;
    h->last_launches = 0;
    HIP_TRY(hipSetDevice(h->device));
    return launch_count(h, s, pairs_launch(s, margin), (uint32_t)s->n_prims, nullptr, COUNT_PAIRS, offsets);
}

int gpuart_nearest_pairs_fill(gpuart_nearest *h, const gpuart_hip_scene *s, float margin, const uint32_t *offsets, int32_t *items, size_t capacity) {
    if (int rc = check_pairs(h, s, margin, offsets)) return rc;
    if (int rc = check_fill(h, COUNT_PAIRS, s->n_prims, nullptr, 0, "boxes", offsets, items, 4, 4, "ordinals", capacity)) return rc < 0 ? rc : 0;
    return launch_fill(h, s, pairs_launch(s, margin), (uint32_t)s->n_prims, nullptr, offsets, items, (uint32_t)capacity);
}

int gpuart_nearest_pairs_host(gpuart_nearest *h, const gpuart_hip_scene *s, float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    if (int rc = check_pairs(h, s, margin, offsets)) return rc;
    if (!total) return fail(GPUART_HIP_ERR_ARG, "nearest: total is NULL");
    return lists_host(h, s, nullptr, 0, s->n_prims, nullptr, COUNT_PAIRS, offsets, items, capacity, total, [&](size_t first, const void *) { return pairs_launch(s, margin, first); });
}

int gpuart_nearest_pairs_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims, float margin,
                                    uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    if ((n_prims && (!prims || !prim_boxes)) || (n_recs && !recs) || !offsets || !total)
        return fail(GPUART_HIP_ERR_ARG, "nearest: recs, prims, prim_boxes, offsets or total is NULL");
    if (n_prims > REF_INDEX || n_recs > REF_INDEX) return fail(GPUART_HIP_ERR_ARG, "nearest: too many primitives or records: " + std::to_string(n_prims));
    return overlap_brute(recs, n_recs, root_ref, prims, prim_boxes, n_prims, nullptr, n_prims, margin, nullptr, offsets, items, capacity, total);
}

}  // extern "C"
