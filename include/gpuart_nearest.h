/* gpuart_nearest.h — C ABI of libgpuart_nearest.so: closest-point queries over an uploaded scene's tree, on the device (MI355X, gfx950).
 * "Which primitive is nearest to this point, where on it, and how far": the question of contact, proximity, snapping and distance
 * fields, answered from the tree the context already keeps current through refits, rebuilds and edits (include/gpuart_refit.h,
 * gpuart_build.h, gpuart_ploc.h, gpuart_edit.h). The library reads the arrays gpuart_hip_scene_device hands out, writes nothing of them
 * and knows nothing of contexts. DESIGN.md "Closest points".
 *
 * The contract (csrc/hip/nearest_rule.h states it for host and device, tests/nearest_ref.py restates it in NumPy float32; plain fp32, no
 * contraction, IEEE division and square root, denormals kept):
 *   point     closest_on_prim(type, record, box, p): q_raw, the point of the primitive's SURFACE nearest to p — a sphere's surface (a p
 *             inside is at r - |p - c|; a p at the centre goes to +x), a disc's plane projection or its rim, a triangle's seven Voronoi
 *             regions, a cone's lateral surface between t = 0 and t = length (what the intersector hits: no caps; a p on the axis takes
 *             a fixed perpendicular) —, then q = min(max(q_raw, box_lo), box_hi) per component into the primitive's own box
 *             (prim_boxes), d = p - q and d2 = (d.x*d.x + d.y*d.y) + d.z*d.z. A degenerate primitive (zero area, radius or length)
 *             yields a finite point of its box: zero denominators select the start of the edge or axis, a NaN is clamped to box_lo;
 *   answer    of the query (p, r): among the primitives with d2 <= r*r (fp32 product; r = +inf accepts everything) the one of least d2;
 *             equal d2 goes to the lowest device ordinal. With a user sphere (c, R) the sphere takes part with ordinal -2, clamped to
 *             c -+ R, and loses ties to every tree primitive;
 *   miss      r NaN or negative, a word of p that is not finite, or nothing accepted: dist = -1, q = 0, d2 = 0, prim = -1, type = -1.
 *             A hit writes dist = sqrtf(d2), q, d2, the ordinal and the primitive's type (0 sphere, 1 disc, 2 triangle, 3 cone);
 *   walk      a child is skipped if and only if the squared distance of p to its box is > the best d2 so far, strictly, or > r*r. Since
 *             q lies in the primitive's box and the tree's boxes are nested, that distance never exceeds the d2 of anything below the
 *             child, bit for bit (the lemma of nearest_rule.h): the pruned walk returns the record of the brute force over all
 *             primitives, in any child order. The kernel enters the nearer child first.
 *
 * The lemma needs nested boxes. Uploads refuse leaves that do not hold their primitives (exact_boxes), and refits, rebuilds and edits
 * fold boxes exactly; only a hand-compiled tree can hold a child's box that leaves its parent's. gpuart_nearest_bind therefore checks
 * every record in one streaming launch — an interior child's two boxes inside the box its parent's record holds for it, a leaf child's
 * prim_boxes likewise, refs and leaf counts in range, an interior child behind its parent (pre-order) — and refuses the tree otherwise.
 * An in-place refit keeps nesting by construction and the generation: no second bind.
 *
 * Limits: one GPU; scenes the uploader classified irregular or disorderly (exact_boxes) are refused; the answer is the nearest SURFACE
 * point under the clamp — for a cone whose derived constants sit at the edge of the primitive rule's tolerance the clamp may move q by
 * that tolerance.
 *
 * Conventions as gpuart_edit.h: 0 or a negative gpuart_hip_status; the last failure's message (per thread) from
 * gpuart_nearest_last_error(), beginning "nearest:". One handle per device; it owns its HIP stream, its traversal stacks and staging. */
#ifndef GPUART_NEAREST_H
#define GPUART_NEAREST_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_nearest gpuart_nearest;

#define GPUART_NEAREST_CHUNK 64u /* queries a wave of k_nearest takes from the cursor at a time */
#define GPUART_NEAREST_RING 8u   /* stack entries a lane keeps in LDS; a walk that stacks more spills to the lane's global column, which is
                                  * sized from scene->max_depth */

#define GPUART_NEAREST_MAX_DEPTH 1024u /* bind refuses a descriptor whose max_depth is above this: the deepest tree an upload or a rebuild
                                        * accepts, and what bounds the lanes' spill columns */

typedef struct gpuart_nearest_hit {
    float dist, q[3]; /* sqrtf(d2) and the point; a miss: -1, 0 */
    float d2;
    int32_t prim;     /* device ordinal; -1 none, -2 the user sphere */
    int32_t type;     /* 0..3; -1 none */
    uint32_t zero;
} gpuart_nearest_hit; /* 32 bytes */

int gpuart_nearest_create(int device, gpuart_nearest **out);
int gpuart_nearest_destroy(gpuart_nearest *h);

/* Checks the descriptor (layout, exact_boxes, arrays, counts, alignment, a finite ordered root box, the root ref, max_depth <=
 * GPUART_NEAREST_MAX_DEPTH) and the nesting of
 * every record (one launch, one small read-back; synchronous), and remembers scene->generation and the arrays. GPUART_HIP_ERR_ARG with
 * the handle unbound when a check fails; the message names the first offending record. */
int gpuart_nearest_bind(gpuart_nearest *h, const gpuart_hip_scene *scene);

/* points: n x 4 floats {p.xyz, r}; hits: n records — device memory, 16-byte aligned, asynchronous on the handle's stream
 * (gpuart_nearest_finish before the results are used). userSphere: {c.xyz, R} in host memory, NULL = none; finite words and R >= 0.
 * GPUART_HIP_ERR_ARG, with nothing written, for a descriptor that is not the bound one (another generation or other arrays: bind again),
 * an unbound handle, NULL or misaligned pointers, hits overlapping points, such a user sphere and n > GPUART_HIP_MAX_RAYS; n = 0 does
 * nothing. */
int gpuart_nearest_run(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                       gpuart_nearest_hit *hits);
/* The same in host memory (4-byte alignment), synchronous, staged through the handle's memory in chunks of 2^20 queries. */
int gpuart_nearest_run_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                            gpuart_nearest_hit *hits);
/* The definition itself, with no device: recs (n_recs x 16 words; ignored), prims (n_prims x 12 words), prim_boxes (n_prims x 6), points
 * and hits all in host memory; every primitive is tested in ordinal order. h may be NULL. What the CPU tests hold nearest_rule.h to, and
 * what a caller without a GPU can use. GPUART_HIP_ERR_ARG for NULL pointers where the matching count is above zero. */
int gpuart_nearest_brute_host(gpuart_nearest *h, const float *recs, size_t n_recs, const float *prims, const float *prim_boxes, size_t n_prims,
                              const float *points, size_t n, const float userSphere[4], gpuart_nearest_hit *hits);

/* How a run is cut up, for callers with little memory and for the tests, which reach the cursor, a shrunk grid and the staging loop with
 * a few hundred queries: the most workgroups of 256 lanes a launch takes (0: what the device holds at once, the default, which also
 * caps it; a launch never takes more than ceil(n / 256)), the most bytes of the lanes' spill columns (0: 512 MiB; (max_depth + 2) x 2 KiB
 * per workgroup, 1 KiB for the walks of the neighbour lists, whose stack entries are 4 bytes; at least one workgroup runs), and the queries per staged launch of gpuart_nearest_run_host (0: 2^20, which also caps
 * it). The answers do not depend on any of them. */
int gpuart_nearest_set_limits(gpuart_nearest *h, uint32_t max_blocks, size_t spill_bytes, size_t host_chunk);
/* The workgroups of the last launch, and the launches of the last gpuart_nearest_run (1) or gpuart_nearest_run_host; either may be NULL. */
int gpuart_nearest_last_launch(gpuart_nearest *h, uint32_t *blocks, uint32_t *launches);

/* Device time in ms of the steps of the last bind and the last run: the nesting check, the walk. */
int gpuart_nearest_step_ms(gpuart_nearest *h, double ms[2]);
/* Box steps and primitive tests of the runs since the last call, summed over the queries — in a counting build of the library
 * (-DNEAREST_COUNT, tools/nearest_time.py); the shipped kernel does not count and this yields zeros. Synchronous. */
int gpuart_nearest_counts(gpuart_nearest *h, uint64_t out[2]);
/* Waits for the handle's stream; GPUART_HIP_ERR_ARG if a walk since the last call met a full stack (a descriptor whose max_depth is below
 * the tree's depth: the results are void; nothing is written out of bounds). */
int gpuart_nearest_finish(gpuart_nearest *h);
const char *gpuart_nearest_last_error(void);

/* ---- Neighbour lists: every primitive within r of a point (DESIGN.md "Neighbour lists"; tests/within_ref.py restates this) ----------
 *   query     (p, r), exactly as above;
 *   list      one gpuart_nearest_hit per primitive whose d2 = dist2(p, closest_on_prim(..)) satisfies d2 <= r*r (the product in fp32, the
 *             comparison <=; r = +inf lists every primitive). An item is, bit for bit, the record gpuart_nearest_run writes for (p, +inf)
 *             if that primitive were alone in the scene: sqrtf(d2), q, d2, the device ordinal, the type, 0. With a user sphere the sphere
 *             takes part with ordinal -2 under the same acceptance. An invalid query (r NaN or negative, a word of p that is not finite)
 *             has an empty list;
 *   order     inside a list: the user sphere first, if accepted; then the primitives in the order of the UNPRUNED depth-first walk of the
 *             tree, lower child first, a leaf's primitives by ascending ordinal. The order is a function of the tree alone: equal for
 *             equal trees, kept by a refit, changed by a rebuild or an edit. A caller may rely on nothing beyond that — not on distance,
 *             not on ordinal;
 *   walk      a child is skipped if and only if the squared distance of p to its box is > r*r; the root likewise. There is no best so
 *             far. Corollary of the lemma of nearest_rule.h: that distance is <= the d2 of everything below the child, so what is skipped
 *             has d2 > r*r and the pruned walk loses no item;
 *   output    CSR: offsets[n + 1] (uint32; offsets[0] = 0, offsets[i + 1] - offsets[i] the length of list i, offsets[n] the total) and
 *             items[total]. The total is computed exactly in 64 bits. A total above GPUART_NEAREST_WITHIN_MAX_ITEMS, or above the lower
 *             cap gpuart_nearest_within_set_max_items sets, is refused (GPUART_HIP_ERR_ARG) and nothing is written to items.
 * Two passes over the same queries: a count, which walks every query, writes the lengths and scans them in place, and a fill, which walks
 * again and writes the items where the offsets put them. All of these need a bound handle as gpuart_nearest_run does, and make its
 * refusals with nothing written. */
#define GPUART_NEAREST_WITHIN_MAX_ITEMS 0x7fffffffu /* 2^31 - 1: an int32 holds every offset */

/* points: n x 4 floats, offsets: n + 1 words — device memory (16- and 4-byte aligned, not overlapping), asynchronous on the handle's
 * stream. n = 0 does nothing. */
int gpuart_nearest_within_count(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                                uint32_t *offsets);
/* Waits for the stream and yields the exact total of the last count. GPUART_HIP_ERR_ARG, with *total written, if it is above the cap. */
int gpuart_nearest_within_total(gpuart_nearest *h, uint64_t *total);
/* Writes list i at items[offsets[i] ..] in the contract's order: the same points, n and user sphere as the last count, and its offsets.
 * items: `capacity` records in device memory, 16-byte aligned (NULL with capacity 0). Asynchronous. Every store is guarded: an index
 * >= offsets[i + 1] or >= capacity is not written, and a list that is longer or shorter than its offsets say marks the run:
 * gpuart_nearest_finish then returns GPUART_HIP_ERR_ARG, "the offsets are not this query set's count: the results are void". A fill
 * never writes outside items[0 .. capacity), whatever it is handed. Refused before any launch: a capacity below the last count's total
 * (the call waits for the stream to learn it), that total above the cap, another n than the last count's, a last count of another kind
 * (box overlap, below). */
int gpuart_nearest_within_fill(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                               const uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity);
/* Both passes in host memory (4-byte alignment), synchronous, staged in chunks of the host_chunk of gpuart_nearest_set_limits; a chunk's
 * offsets are rebased on the host, so the result is the unstaged one's byte for byte. Always writes offsets[0 .. n] and *total; writes
 * items only when items != NULL and capacity >= total — a short capacity is no error: call again with room for *total. A total above
 * the cap is GPUART_HIP_ERR_ARG. gpuart_nearest_last_launch counts the launches of both passes. */
int gpuart_nearest_within_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                               uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity, uint64_t *total);
/* The fill pass alone in host memory, staged likewise: for the caller who has the offsets of gpuart_nearest_within_host(items = NULL) and
 * now has room for offsets[n] items — the queries are walked twice in all, not three times. offsets must start at 0 and ascend, capacity
 * must hold offsets[n] (GPUART_HIP_ERR_ARG otherwise, nothing written); offsets that are not these queries' count are reported as by
 * gpuart_nearest_finish, and nothing is written outside items[0 .. offsets[n]). */
int gpuart_nearest_within_fill_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, const float userSphere[4],
                                    const uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity);
/* The definition itself, with no device and no pruning: the tree order is derived from recs (n_recs x 16 words) and root_ref by an
 * unpruned walk, and every primitive is tested. Host memory; offsets, items, capacity and total as gpuart_nearest_within_host.
 * GPUART_HIP_ERR_ARG for NULL pointers where the matching count is above zero, and for records that do not reach every primitive once. */
int gpuart_nearest_within_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims,
                                     const float *points, size_t n, const float userSphere[4], uint32_t *offsets, gpuart_nearest_hit *items,
                                     size_t capacity, uint64_t *total);
/* Lowers the cap on a total (0: GPUART_NEAREST_WITHIN_MAX_ITEMS, which also caps it): for callers with little memory, and for the tests. */
int gpuart_nearest_within_set_max_items(gpuart_nearest *h, uint64_t max_items);
/* Device time in ms of the last count, its scan and the last fill. */
int gpuart_nearest_within_step_ms(gpuart_nearest *h, double ms[3]);
/* gpuart_nearest_counts for the walks of the lists, both passes. */
int gpuart_nearest_within_counts(gpuart_nearest *h, uint64_t out[2]);

/* ---- k nearest: the k nearest primitives of a point (DESIGN.md "k nearest"; tests/knn_ref.py restates this) ---------------------------
 *   query       (p, r), exactly as above, and one k per call, 1 <= k <= GPUART_NEAREST_KNN_MAX;
 *   candidates  every primitive whose d2 = dist2(p, closest_on_prim(..)) satisfies d2 <= r*r (fp32 product, <=), and with a user sphere
 *               the sphere, ordinal -2, under the same acceptance. An invalid query (r NaN or negative, a word of p that is not finite)
 *               has no candidates;
 *   order       ascending d2 (fp32 compare); equal d2: tree primitives by ascending device ordinal, and the user sphere — as the uint32
 *               0xfffffffe above every ordinal — behind every tree primitive of equal d2 (nearest_rule.h: knn_before);
 *   answer      hits[i * k + j], j = 0 .. k - 1, is the j-th candidate of query i in that order: bit for bit the record the neighbour
 *               list holds for that primitive — sqrtf(d2), q, d2, the ordinal, the type, 0. Slots past the number of candidates hold the
 *               miss record: dist = -1, q = 0, d2 = 0, prim = -1, type = -1, 0. For k = 1 the output is gpuart_nearest_run's byte for byte;
 *   walk        a child — and the root — is skipped if and only if the squared distance of p to its box is > r*r, or k candidates are kept
 *               and it is > the d2 of the worst kept, strictly (nearest_rule.h: knn_pruned). While fewer than k are kept only the radius
 *               prunes. By the lemma that distance is <= the d2 of everything below the child: what is skipped comes strictly behind every
 *               kept candidate, and the kept only ever improve, so the walk returns the brute force's records in any child order; at
 *               equality a primitive of lower ordinal may lie below, which is why the prune is strict. The kernel enters the nearer child
 *               first.
 * One walk per query and a fixed-size answer: no count, no scan, no second pass. A bound handle as gpuart_nearest_run needs it, the same
 * refusals with nothing written, and gpuart_nearest_set_limits applies (max_blocks, the spill budget, host_chunk). */
#define GPUART_NEAREST_KNN_MAX 32u /* the most k: a lane's kept list lives in LDS, 8 bytes per entry */

/* points: n x 4 floats; hits: n * k records — device memory, 16-byte aligned, asynchronous on the handle's stream; gpuart_nearest_finish
 * reports a full stack as for gpuart_nearest_run. GPUART_HIP_ERR_ARG, with nothing written, for k = 0 or k > GPUART_NEAREST_KNN_MAX,
 * n * k > GPUART_HIP_MAX_RAYS, hits overlapping points and everything gpuart_nearest_run refuses; n = 0 does nothing. */
int gpuart_nearest_knn_run(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, size_t k, const float userSphere[4],
                           gpuart_nearest_hit *hits);
/* The same in host memory (4-byte alignment), synchronous, staged through the handle's memory in chunks of host_chunk / k queries (at
 * least one), so that a chunk's records are no more than a chunk of gpuart_nearest_run_host holds. */
int gpuart_nearest_knn_run_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *points, size_t n, size_t k, const float userSphere[4],
                                gpuart_nearest_hit *hits);
/* The definition itself, with no device: every primitive tested, the accepted sorted; arguments as gpuart_nearest_brute_host (recs is
 * ignored, h may be NULL). GPUART_HIP_ERR_ARG for NULL pointers where the matching count is above zero and for k = 0 or
 * k > GPUART_NEAREST_KNN_MAX. */
int gpuart_nearest_knn_brute_host(gpuart_nearest *h, const float *recs, size_t n_recs, const float *prims, const float *prim_boxes, size_t n_prims,
                                  const float *points, size_t n, size_t k, const float userSphere[4], gpuart_nearest_hit *hits);
/* Device time in ms of the last k-nearest walk. */
int gpuart_nearest_knn_step_ms(gpuart_nearest *h, double ms[1]);
/* gpuart_nearest_counts for the k-nearest walks. */
int gpuart_nearest_knn_counts(gpuart_nearest *h, uint64_t out[2]);

/* ---- Box overlap: every primitive whose box meets a box, and the overlapping pairs of the scene's own primitives (DESIGN.md "Box
 * overlap"; tests/overlap_ref.py restates this). Plain fp32, comparisons only, no tolerance -------------------------------------------------
 *   query     a box {lo.xyz, hi.xyz}, six floats in the layout of prim_boxes, and one margin per call. The inflated box is qlo = lo - margin,
 *             qhi = hi + margin, each component one fp32 operation; an overflow to -+inf is allowed. A query with a word that is not finite
 *             or with lo > hi on some axis has an empty list. A margin that is NaN, infinite or negative is refused before any launch;
 *   item      the device ordinal (int32) of every primitive whose own box prim_boxes[j] = (blo, bhi) satisfies, on all three axes,
 *             qlo <= bhi && blo <= qhi: touching counts. With a user sphere (c, R) the sphere takes part through its box c -+ R, ordinal -2;
 *   order     as the neighbour lists: the user sphere first, then the unpruned depth-first walk, lower child first, a leaf's primitives by
 *             ascending ordinal. A function of the tree alone;
 *   walk      a child, and the root, is skipped if and only if its box fails the same test against (qlo, qhi). If b lies inside B and q
 *             overlaps b then q overlaps B (nearest_rule.h), and gpuart_nearest_bind has checked the nesting; only stored numbers are
 *             compared, so nothing rounds and the pruned walk loses no item;
 *   output    CSR exactly as the neighbour lists: offsets[n + 1] (uint32), items[total] (int32), the exact 64-bit total, the cap of
 *             GPUART_NEAREST_WITHIN_MAX_ITEMS and the lower cap of gpuart_nearest_within_set_max_items, nothing written above it;
 *   pairs     query i is prim_boxes[i] of the bound scene, i = 0 .. n_prims - 1, inflated by the margin and read on the device; list i holds
 *             the ordinals j > i that this box query lists, in the same order; no user sphere. A pair {i, j} appears once, in the lower
 *             ordinal's list, and THE LOWER ORDINAL'S BOX IS THE INFLATED ONE: in fp32 fl(lo_i - m) <= hi_j and lo_i <= fl(hi_j + m) can
 *             disagree (lo_i = 1, hi_j = 1 - 2^-24, m = 2^-25: false, true), so a symmetric-looking implementation lists other pairs.
 *             Adjacent triangles of a mesh share vertices and therefore always overlap: filtering topological neighbours is the caller's.
 * Count and fill as the neighbour lists, with the same refusals, each with nothing written. The handle remembers one "last count" — its n,
 * its total and whose it was —: a fill of one kind (within, overlap, pairs) after a count of another is refused. gpuart_nearest_set_limits
 * applies; the spill columns cost 1 KiB per level and workgroup. */

/* boxes: n x 6 floats, offsets: n + 1 words — device memory, 4-byte aligned, not overlapping; asynchronous. n = 0 does nothing. */
int gpuart_nearest_overlap_count(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *boxes, size_t n, float margin, const float userSphere[4],
                                 uint32_t *offsets);
/* Waits for the stream and yields the exact total of the last count (of any kind). GPUART_HIP_ERR_ARG, with *total written, above the cap. */
int gpuart_nearest_overlap_total(gpuart_nearest *h, uint64_t *total);
/* Writes list i at items[offsets[i] ..]: the boxes, n, margin and user sphere of the last count, and its offsets. items: `capacity` ordinals
 * in device memory, 4-byte aligned (NULL with capacity 0), overlapping neither boxes nor offsets. Asynchronous. Every store is guarded by
 * the list's end and the capacity; a list longer or shorter than its offsets say is reported by gpuart_nearest_finish ("the offsets are not
 * this query set's count"). Refused before any launch: a capacity below the last count's total, that total above the cap, another n than the
 * last count's, a last count of another kind. */
int gpuart_nearest_overlap_fill(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *boxes, size_t n, float margin, const float userSphere[4],
                                const uint32_t *offsets, int32_t *items, size_t capacity);
/* Both passes in host memory, synchronous, staged in chunks of host_chunk queries with offsets rebased on the host: the two-call protocol of
 * gpuart_nearest_within_host (offsets and *total always; items only when items != NULL and capacity >= *total). */
int gpuart_nearest_overlap_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *boxes, size_t n, float margin, const float userSphere[4],
                                uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total);
/* The fill pass alone in host memory, as gpuart_nearest_within_fill_host. */
int gpuart_nearest_overlap_fill_host(gpuart_nearest *h, const gpuart_hip_scene *scene, const float *boxes, size_t n, float margin, const float userSphere[4],
                                     const uint32_t *offsets, int32_t *items, size_t capacity);
/* The definition itself, with no device and no pruning: the tree order derived from recs and root_ref (prims gives an unflagged leaf's
 * count), every primitive's box tested. Host memory; offsets, items, capacity and total as gpuart_nearest_overlap_host. */
int gpuart_nearest_overlap_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims,
                                      const float *boxes, size_t n, float margin, const float userSphere[4], uint32_t *offsets, int32_t *items,
                                      size_t capacity, uint64_t *total);
/* Device time in ms of the last overlap or pairs count, its scan and the last such fill. */
int gpuart_nearest_overlap_step_ms(gpuart_nearest *h, double ms[3]);
/* gpuart_nearest_counts for the overlap walks: box steps and box tests, both passes, box queries and pairs. */
int gpuart_nearest_overlap_counts(gpuart_nearest *h, uint64_t out[2]);

/* The pairs of the bound scene: offsets: n_prims + 1 words, items: `capacity` ordinals — device memory, 4-byte aligned; asynchronous. The
 * total is gpuart_nearest_overlap_total's; the fill takes the margin of the count and its offsets. Nothing is uploaded. */
int gpuart_nearest_pairs_count(gpuart_nearest *h, const gpuart_hip_scene *scene, float margin, uint32_t *offsets);
int gpuart_nearest_pairs_fill(gpuart_nearest *h, const gpuart_hip_scene *scene, float margin, const uint32_t *offsets, int32_t *items, size_t capacity);
/* Both passes with the results in host memory, synchronous, staged over ranges of host_chunk ordinals (a launch takes a first ordinal); the
 * two-call protocol of gpuart_nearest_overlap_host. */
int gpuart_nearest_pairs_host(gpuart_nearest *h, const gpuart_hip_scene *scene, float margin, uint32_t *offsets, int32_t *items, size_t capacity,
                              uint64_t *total);
/* The definition of the pairs with no device: list i = the box query prim_boxes[i] with every j <= i removed. */
int gpuart_nearest_pairs_brute_host(const float *recs, size_t n_recs, uint32_t root_ref, const float *prims, const float *prim_boxes, size_t n_prims,
                                    float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total);

#ifdef __cplusplus
}
#endif
#endif /* GPUART_NEAREST_H */
