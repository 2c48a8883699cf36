/* capi.h — flat C API over the C++ Renderer/Scene library (libgpuart.so), used by the Python
 * plumbing (ctypes) in tests and bench.py. Thin by design: one call per Renderer method. */
#ifndef GPUART_CAPI_H
#define GPUART_CAPI_H

#include <stddef.h>
#include <stdint.h>

#include "gpuart_adaptive.h"
#include "gpuart_antilag.h"
#include "gpuart_converge.h"
#include "gpuart_denoise.h"
#include "gpuart_despeckle.h"
#include "gpuart_display.h"
#include "gpuart_edges.h"
#include "gpuart_hip.h"
#include "gpuart_nearest.h"
#include "gpuart_moments.h"
#include "gpuart_refine.h"
#include "gpuart_temporal.h"
#include "gpuart_upscale.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A primitive description: sphere {c r}, disc {c n r}, triangle {v0 v1 v2}, cone {c1 c2 r1 r2}. */
typedef struct gpuart_prim_desc {
    int32_t type;
    float f[9];
} gpuart_prim_desc;

typedef struct gpuart_renderer gpuart_renderer;

/* ---- pure host functions (no device needed) ---- */
/* BoundingVolumesHierarchy(prims, maxLevels, minPrims).Compile(); free *quads with gpuart_free. */
int gpuart_compile_bvh(const gpuart_prim_desc *prims, int n, unsigned maxLevels, unsigned minPrims, float **quads,
                       size_t *nquads, unsigned *depth);
/* The same for a scene file: kind 0 = ASCII PLY mesh (Utils::LoadMeshFromPLY), 1 = primitive list
 * (Utils::LoadPrimitives); `extra` primitives are appended after the loaded ones. */
int gpuart_compile_bvh_from_file(int kind, const char *path, float magnification, const float translation[3],
                                 const gpuart_prim_desc *extra, int nextra, float **quads, size_t *nquads,
                                 unsigned *depth, size_t *nloaded);
void gpuart_free(void *p);
/* BoundingVolumesHierarchy::Refit without a device: the compiled tree `quads` (nquads quads, what gpuart_compile_bvh returns) with
 * the data quads of the primitives `ordinals` (n, strictly ascending, numbered as the tree's leaves hold them) replaced by `payloads`
 * (n x 16 floats, zero-padded) and every box refitted (include/gpuart_refit.h states the contract), written to `out` (nquads quads).
 * touchedOnly != 0: Refit's form that recomputes only the moved primitives' leaves and their ancestors (Renderer::UpdatePrimitives' form).
 * 0; -1 for a malformed tree or NULL pointers; -2 for a refused update (*firstBad, if given, is its index in the list), `out` untouched. */
int gpuart_refit_tree(const float *quads, size_t nquads, const uint32_t *ordinals, const float *payloads, size_t n, float *out,
                      size_t *firstBad, int touchedOnly);
/* BoundingVolumesHierarchy::RebuildMorton without a device: the tree of the compiled tree `quads` rebuilt in Morton order
 * (include/gpuart_build.h states the contract) and compiled again; *out is malloc'ed (gpuart_free), *nout its quads; newToOld receives
 * the n_prims old ordinals by new ordinal. `order` NULL: the library sorts; else n_prims ordinals that are only checked.
 * 0; -1 for a malformed tree or NULL pointers; -2 for an empty tree or an order that is not the contract's. */
int gpuart_rebuild_tree(const float *quads, size_t nquads, const uint32_t *order, float **out, size_t *nout, uint32_t *newToOld);
/* BoundingVolumesHierarchy::AdoptTopology without a device: the canonical compiled tree `quads` takes over the topology the clustered
 * rebuild made on the device (include/gpuart_ploc.h) and is compiled again; *out is malloc'ed (gpuart_free), *nout its quads. `order`:
 * n_prims old ordinals by new ordinal; `refs`: the two child refs of each of the n_recs records in pre-order (csrc/hip/tree_rule.h).
 * 0; -1 for a malformed tree or NULL pointers; -2 for an order that is no permutation or refs that are not a tree over it in pre-order
 * with leaves of one or two. */
int gpuart_adopt_tree(const float *quads, size_t nquads, const uint32_t *order, const uint32_t *refs, size_t n_recs, float **out, size_t *nout);
/* What the library itself spent in the last gpuart_compile_bvh / _from_file of this process: out[0] = BoundingVolumesHierarchy's
 * constructor (the build), out[1] = its compilation into quads, in ms — without the harness around them (making and deleting one
 * Primitive object per description, copying the result into the caller's language). */
void gpuart_last_build_ms(double out[2]);
/* The permutation the BVH build applies to a node's primitives: perm[i] = position (before sorting) of the element that
 * std::sort leaves at i when sorting by `keys` with operator< — computed by exact_sort.h on up to `threads` threads. */
void gpuart_sort_permutation(const float *keys, size_t n, unsigned threads, uint32_t *perm);
/* out[13] = Pos(3) BottomLeft(3) DeltaHorz(3) DeltaVert(3) PixelSize */
void gpuart_camera_basis(const float pos[3], const float dir[3], const float up[3], float fovY, float screenDist,
                         unsigned width, unsigned height, float out[13]);
void gpuart_sun_direction(float azimuth, float altitude, float out[3]);
/// Every Vec3<float> / Vec3<double> operation of math_types.h once (parity hook: tests/golden/host_math.npz holds what the
/// reference's own src/math_types.h computes): out = {length, sqrlength, a*b} + normalized + a^b + a+b + a-b + a*s + s*a + a/s +
/// vrotx(s) + vroty(s) + vrotz(s) + (-a).
void gpuart_vec3f_ops(const float a[3], const float b[3], float s, float out[36]);
void gpuart_vec3d_ops(const double a[3], const double b[3], double s, double out[36]);

/* ---- gpuart::Renderer ---- */
gpuart_renderer *gpuart_renderer_create(unsigned width, unsigned height, const float pos[3], const float dir[3],
                                        const float up[3], float fovY, float screenDist, int device);
void gpuart_renderer_destroy(gpuart_renderer *r);
int gpuart_renderer_is_ok(gpuart_renderer *r);
void gpuart_renderer_set_primitives(gpuart_renderer *r, const gpuart_prim_desc *prims, int n, int printInfo);
/* Renderer::UpdatePrimitives: primitives `indices` (n distinct indices, in any order) become `descs` (the same types); the tree is
 * refitted on the device, its topology and the histories are kept. After gpuart_renderer_set_primitives the indices number that call's
 * `prims` array AS THE CALLER PASSED IT, as the ordinals of gpuart_renderer_trace_rays do; after an init_* scene they are positions in
 * the renderer's sorted list. 1 on success, 0 — with the scene unchanged — on any refusal. */
int gpuart_renderer_update_primitives(gpuart_renderer *r, const uint32_t *indices, const gpuart_prim_desc *descs, int n);
/* Renderer::RebuildTree. newToOld (n_prims entries, may be NULL) receives, per new device ordinal, the old one. The ordinals of
 * gpuart_renderer_trace_rays and the indices of gpuart_renderer_update_primitives keep numbering the caller's descriptions after
 * gpuart_renderer_set_primitives. 1 on success, 0 — with the scene unchanged — on any refusal. */
int gpuart_renderer_rebuild_tree(gpuart_renderer *r, uint32_t *newToOld);
/* The same with Renderer::RebuildTree's mode: 0 the Morton build (what gpuart_renderer_rebuild_tree does), 1 Renderer::TREE_CLUSTERED,
 * the clustered build of include/gpuart_ploc.h — slower to build, cheaper to walk. */
int gpuart_renderer_rebuild_tree_mode(gpuart_renderer *r, int mode, uint32_t *newToOld);
/* Renderer::EditPrimitives. `remove`: nRemove distinct indices into the caller's descriptions, in any order; `added`: nAdd descriptions of
 * any types. Afterwards the caller's descriptions are the ones that were not removed, in their order, followed by `added`: that list is
 * what the ordinals of gpuart_renderer_trace_rays and the indices of gpuart_renderer_update_primitives number from now on. source (n_new
 * entries, may be NULL) receives, per new device ordinal, the old device ordinal of a survivor or n_old + k for added[k]; *n_new (may be
 * NULL) the new count. mode as gpuart_renderer_rebuild_tree_mode. 1 on success, 0 — with the scene unchanged — on any refusal. */
int gpuart_renderer_edit_primitives(gpuart_renderer *r, const uint32_t *remove, int nRemove, const gpuart_prim_desc *added, int nAdd, int mode,
                                    uint32_t *source, size_t *n_new);
/* BoundingVolumesHierarchy::EditPrimitives without a device: the compiled tree `quads` with the primitives `remove` (nRemove strictly
 * ascending device ordinals) removed and nAdd primitives of `addTypes` / `addPayloads` (16 floats each) appended, then rebuilt — with
 * adopt == 0 in Morton order (`order` as for gpuart_rebuild_tree: NULL, or the permutation to check), else by AdoptTopology of `order`
 * and `refs` (nRecs records) — and compiled; *out is malloc'ed (gpuart_free), *nout its quads. newToOld (may be NULL) receives the
 * rebuild's permutation of the edited list. 0, -1 for a malformed tree or NULL arguments, -2 for a refused edit (*firstBad, may be NULL,
 * the first offender or SIZE_MAX), -3 for a refused order or topology. */
int gpuart_edit_tree(const float *quads, size_t nquads, const uint32_t *remove, size_t nRemove, const uint32_t *addTypes, const float *addPayloads,
                     size_t nAdd, int adopt, const uint32_t *order, const uint32_t *refs, size_t nRecs, float **out, size_t *nout, uint32_t *newToOld,
                     size_t *firstBad);
/* Renderer::TreeCost. 1 on success. */
int gpuart_renderer_tree_cost(gpuart_renderer *r, double *cost);
/* {total, host tree} ms of the last gpuart_renderer_rebuild_tree. */
void gpuart_renderer_last_rebuild_ms(gpuart_renderer *r, double out[2]);
/* GetBVH().Compile(): *quads is malloc'ed (gpuart_free), *nquads its length in quads. 0, or -1. */
int gpuart_renderer_compile_bvh(gpuart_renderer *r, float **quads, size_t *nquads);
void gpuart_renderer_init_box(gpuart_renderer *r);
int gpuart_renderer_init_dragon(gpuart_renderer *r, const char *plyPath);
/* InitCluster / InitTree (reference src/scenes.cpp:69-103) on a primitive-list file; NULL = the reference's own path. */
int gpuart_renderer_init_cluster(gpuart_renderer *r, const char *datPath);
int gpuart_renderer_init_tree(gpuart_renderer *r, const char *datPath);
int gpuart_renderer_set_camera(gpuart_renderer *r, const float pos[3], const float dir[3], const float up[3], float fovY,
                               float screenDist);
int gpuart_renderer_update_viewport(gpuart_renderer *r, unsigned width, unsigned height);
int gpuart_renderer_set_tile(gpuart_renderer *r, unsigned x0, unsigned y0, unsigned w, unsigned h);
int gpuart_renderer_set_interleaved_tile(gpuart_renderer *r, unsigned x0, unsigned y0, unsigned w, unsigned localRows,
                                         unsigned bandRows, unsigned bandStride);
void gpuart_renderer_set_sun(gpuart_renderer *r, float azimuth, float altitude, int directLighting);
void gpuart_renderer_set_user_sphere(gpuart_renderer *r, const float pos[3], float radius, float emittance, int specular,
                                     int fuzzy);
/* Renderer::SetUserSpherePos: the position alone; with the temporal history on it commits the view and keeps the history. */
void gpuart_renderer_set_user_sphere_pos(gpuart_renderer *r, const float pos[3]);
void gpuart_renderer_set_max_path_segments(gpuart_renderer *r, unsigned n);
void gpuart_renderer_set_seed(gpuart_renderer *r, uint32_t seed);
void gpuart_renderer_render_direct(gpuart_renderer *r);
void gpuart_renderer_restart_path_tracing(gpuart_renderer *r, unsigned pathsPerPass, unsigned pathsPerPixel);
unsigned gpuart_renderer_path_tracing_pass(gpuart_renderer *r);
int gpuart_renderer_read_direct(gpuart_renderer *r, float *rgba);
int gpuart_renderer_read_radiance(gpuart_renderer *r, float *rgba, int normalized);
/* Renderer::ReadDenoised: the denoised preview of the normalised accumulator (include/gpuart_denoise.h); p = NULL: the defaults.
 * 1 on success, 0 on error. */
int gpuart_renderer_read_denoised(gpuart_renderer *r, float *rgba, const gpuart_denoise_params *p);
/* Renderer::SetMinWeight / SetNearestFirst (1 on success). */
void gpuart_renderer_set_min_weight(gpuart_renderer *r, float w);
int gpuart_renderer_set_nearest_first(gpuart_renderer *r, uint32_t minPrims);
/* Renderer::SetTemporalHistory: carry path-traced history across camera and user-sphere moves (include/gpuart_temporal.h); off by
 * default. tp = NULL: the library's defaults. 1 on success, 0 for parameters out of range. */
int gpuart_renderer_set_temporal_history(gpuart_renderer *r, int on, const gpuart_temporal_params *tp);
/* Renderer::ReadPreview: the history blended with the accumulator, then denoised; what gpuart_renderer_read_denoised returns while
 * there is no history. dn, tp = NULL: the defaults / what gpuart_renderer_set_temporal_history was given. 1 on success, 0 on error. */
int gpuart_renderer_read_preview(gpuart_renderer *r, float *rgba, const gpuart_denoise_params *dn, const gpuart_temporal_params *tp);
/* Renderer::RenderUntil: render on in batches of at least batchPaths paths until at most maxAboveShare of the tile's pixels have a
 * relative standard error above threshold (include/gpuart_converge.h). 1 converged, 0 the path target was reached first, -1 error;
 * last (may be NULL) is filled whenever a measure ran. */
int gpuart_renderer_render_until(gpuart_renderer *r, float threshold, float maxAboveShare, unsigned batchPaths, float lumFloor,
                                 gpuart_converge_summary *last);
/* Renderer::ReadErrorMap: the error per tile pixel as of the last batch; 1 on success, 0 before the second batch or on error. */
int gpuart_renderer_read_error_map(gpuart_renderer *r, float *e, float lumFloor);
/* Renderer::ReadRefined: the normalised accumulator filtered by the error map of the last batch (include/gpuart_refine.h); p = NULL:
 * the defaults. 1 on success, 0 before the second batch or on error. */
int gpuart_renderer_read_refined(gpuart_renderer *r, float *rgba, float lumFloor, const gpuart_refine_params *p);
/* Renderer::ReadDisplay: the frame `source` names (a gpuart_display_source) as 8-bit RGBA encoded on the device
 * (include/gpuart_display.h), tile-sized, 4 bytes per pixel; dp = NULL: the defaults; lumFloor for the guided preview and the refined
 * frame. 1 on success; 0 wherever the Read* of that source gives 0, for parameters out of range, or on error. */
int gpuart_renderer_read_display(gpuart_renderer *r, uint8_t *rgba8, int source, const gpuart_display_params *dp, float lumFloor);
/* Renderer::ReadUpscaled: the frame `source` names (a gpuart_display_source) upsampled `scale` (2..4) times under the guidance of a
 * G-buffer of the larger frame (include/gpuart_upscale.h): scale*w * scale*h * 4 floats for a tile of w x h, row 0 = bottom row; p = NULL:
 * the defaults. 1 on success; 0 for scale out of range, an interleaved tile, parameters out of range, and wherever the source's read
 * fails. */
int gpuart_renderer_read_upscaled(gpuart_renderer *r, float *rgba, int source, uint32_t scale, float lumFloor, const gpuart_upscale_params *p);
/* Renderer::ReadUpscaledDisplay: the same plane as 8-bit RGBA (include/gpuart_display.h), scale*w * scale*h * 4 bytes. */
int gpuart_renderer_read_upscaled_display(gpuart_renderer *r, uint8_t *rgba8, int source, uint32_t scale, const gpuart_display_params *dp,
                                          float lumFloor, const gpuart_upscale_params *p);
/* Renderer::SetHistoryVariance: carry the luminance's moments through a second history (include/gpuart_moments.h); toggling drops the
 * temporal history. p = NULL: the defaults. 1 on success, 0 for parameters out of range. */
int gpuart_renderer_set_history_variance(gpuart_renderer *r, int on, const gpuart_moments_params *p);
/* Renderer::SetHistoryAntiLag: carry the radiance through a third, short history and let the guided preview follow it where the lighting
 * changed (include/gpuart_antilag.h); toggling drops the temporal history. p = NULL: the defaults. 1 on success, 0 for parameters out
 * of range. */
int gpuart_renderer_set_history_antilag(gpuart_renderer *r, int on, const gpuart_antilag_params *p);
/* Renderer::SetEdgeResolve: the filtered reads (denoised, preview, guided preview, refined, and the display of them) end in mark,
 * sub-pixel rays and resolve (include/gpuart_edges.h). p = NULL: the defaults. 1 on success, 0 for parameters out of range.
 * gpuart_renderer_get_edge_resolve: 1 while on. */
int gpuart_renderer_set_edge_resolve(gpuart_renderer *r, int on, const gpuart_edges_params *p);
int gpuart_renderer_get_edge_resolve(gpuart_renderer *r);
/* Renderer::SetFireflyClamp: the view every filtered read and every temporal commit stages is clamped in place first
 * (include/gpuart_despeckle.h); changing the switch or its parameters drops the temporal history. p = NULL: the defaults. 1 on success,
 * 0 for parameters out of range. gpuart_renderer_get_firefly_clamp: 1 while on. gpuart_renderer_read_firefly_summary: the counts of the
 * last clamp that ran; 0 before the first. */
int gpuart_renderer_set_firefly_clamp(gpuart_renderer *r, int on, const gpuart_despeckle_params *p);
int gpuart_renderer_get_firefly_clamp(gpuart_renderer *r);
int gpuart_renderer_read_firefly_summary(gpuart_renderer *r, gpuart_despeckle_summary *out);
/* Renderer::ReadGuidedPreview: the history blend filtered by gpuart_refine_run with the error map of the history's measured variance.
 * rf, tp = NULL: the defaults / what gpuart_renderer_set_temporal_history was given. 1 on success; 0 while the variance or the
 * history is off, before the view's first path, or on error. */
int gpuart_renderer_read_guided_preview(gpuart_renderer *r, float *rgba, float lumFloor, const gpuart_refine_params *rf,
                                        const gpuart_temporal_params *tp);
/* Renderer::RenderAdaptive: 1 no block is active any more, 0 the cap was reached first, -1 error; last (may be NULL) is filled whenever
 * a select ran. */
int gpuart_renderer_render_adaptive(gpuart_renderer *r, float threshold, unsigned minPaths, unsigned batchPaths, float lumFloor,
                                    gpuart_adaptive_summary *last);
/* Renderer::ReadSampleCounts: paths accumulated into every tile pixel, tile-sized, row 0 = bottom row; 1 on success. */
int gpuart_renderer_read_sample_counts(gpuart_renderer *r, uint32_t *perPixel);
/* Renderer::GatherRadiance: the shares of renderers 0 .. n-1 (Renderer::SetShare k of n) as one full frame in fullFrame on `root`'s
 * host; 1 on success, 0 on error, and while a rank's path counts are not uniform (RenderAdaptive retired blocks). */
int gpuart_renderer_gather_radiance(gpuart_renderer *const *ranks, int n, int root, int normalized, float *fullFrame);
int gpuart_renderer_finish(gpuart_renderer *r);
int gpuart_renderer_save_checkpoint(gpuart_renderer *r, const char *path);
int gpuart_renderer_load_checkpoint(gpuart_renderer *r, const char *path);
/* Renderer::TraceRays / Renderer::Pick (host memory, synchronous; 1 on success, 0 on error): rays n x 8 floats {origin.xyz, tmax}
 * {dir.xyz, unused}, xy[2n] frame pixels. After gpuart_renderer_set_primitives, prims[i] (prims may be NULL) indexes the `prims` array
 * AS THE CALLER PASSED IT (the build's reordering is undone here); after an init_* scene it is the position in the renderer's sorted list.
 * -1: nothing hit, -2: the user sphere. */
int gpuart_renderer_trace_rays(gpuart_renderer *r, const float *rays, size_t n, int occlusion, int withUserSphere, gpuart_ray_hit *hits,
                               int32_t *prims);
int gpuart_renderer_pick(gpuart_renderer *r, const uint32_t *xy, size_t n, int withUserSphere, gpuart_ray_hit *hits, int32_t *prims);
/* Renderer::ClosestPoints (host memory, synchronous; 1 on success, 0 on refusal or error): points n x 4 floats {p.xyz, r}, hits n records
 * of include/gpuart_nearest.h; a hit's prim is the device ordinal, the position in the renderer's sorted list (-2: the user sphere). */
int gpuart_renderer_closest_points(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, gpuart_nearest_hit *hits);
/* Renderer::NearestPrimitives (host memory, synchronous; 1 on success, 0 on refusal or error): points n x 4 floats {p.xyz, r}, hits n * k
 * records, query i's k nearest at hits[i * k ..] in ascending distance, misses behind them; 1 <= k <= GPUART_NEAREST_KNN_MAX. */
int gpuart_renderer_nearest_primitives(gpuart_renderer *r, const float *points, size_t n, size_t k, int withUserSphere, gpuart_nearest_hit *hits);
/* Renderer::PrimitivesWithin (host memory, synchronous; 1 on success, 0 on refusal or error) by the two-call protocol of
 * gpuart_nearest_within_host: offsets[n + 1] and *total are always written; items (capacity records) only when it is not NULL and
 * capacity >= *total — call once with items = NULL to learn the total, then again with room for it. Ordinals as closest_points'. */
int gpuart_renderer_primitives_within(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, uint32_t *offsets,
                                      gpuart_nearest_hit *items, size_t capacity, uint64_t *total);
/* The second call without its count: Renderer::FillPrimitivesWithin fills items (capacity >= offsets[n]) for the offsets the first call
 * wrote, so the queries are walked twice in all and not three times. */
int gpuart_renderer_primitives_within_fill(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, const uint32_t *offsets,
                                           gpuart_nearest_hit *items, size_t capacity);
/* Renderer::PrimitivesOverlapping (host memory, synchronous; 1 on success, 0 on refusal or error) by the two-call protocol of
 * gpuart_nearest_overlap_host: boxes n x 6 floats {lo.xyz, hi.xyz}, one margin; offsets[n + 1] and *total are always written; items
 * (capacity ordinals) only when it is not NULL and capacity >= *total. Ordinals as closest_points'. */
int gpuart_renderer_primitives_overlapping(gpuart_renderer *r, const float *boxes, size_t n, float margin, int withUserSphere, uint32_t *offsets,
                                           int32_t *items, size_t capacity, uint64_t *total);
/* The second call without its count: Renderer::FillPrimitivesOverlapping fills items (capacity >= offsets[n]) for the offsets the first
 * call wrote. */
int gpuart_renderer_primitives_overlapping_fill(gpuart_renderer *r, const float *boxes, size_t n, float margin, int withUserSphere, const uint32_t *offsets,
                                                int32_t *items, size_t capacity);
/* Renderer::OverlappingPairs by the same two-call protocol: offsets has n_prims + 1 words; list i holds the ordinals j > i whose box meets
 * primitive i's box inflated by margin. */
int gpuart_renderer_overlapping_pairs(gpuart_renderer *r, float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total);
gpuart_hip_ctx *gpuart_renderer_backend(gpuart_renderer *r);
void gpuart_renderer_params(gpuart_renderer *r, gpuart_params *out);
/* What the renderer's last SetPrimitives spent inside the library, ms: whole call, BVH build, compilation, re-layout + upload. */
void gpuart_renderer_last_setprims_ms(gpuart_renderer *r, double out[4]);
void gpuart_renderer_scene_info(gpuart_renderer *r, uint64_t *nodes, uint64_t *prims, unsigned *depth);

#ifdef __cplusplus
}
#endif
#endif
