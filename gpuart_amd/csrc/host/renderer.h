// renderer.h — gpuart::Camera and gpuart::Renderer: the reference's public API
// (src/renderer.h:39-49,183-296), re-hosted on the MI355X back end (include/gpuart_hip.h)
// instead of OpenGL. Every reference method keeps its name, arguments and behaviour
// (including: every setter silently restarts the path-tracing accumulation; failures are
// reported through bool returns / GetIsOK() and std::cerr, never exceptions).
//
// Additions (the reference draws into the GL framebuffer, which no longer exists, and has
// MAX_PATH_SEGMENTS / the RNG seed / the viewport fixed at compile time):
//   ReadDirectLighting, ReadRadiance, Finish, SetMaxPathSegments, SetMinWeight, SetSeed,
//   SetTile, GetBackend, ComputeScreenBasis, GetNumPathsRendered, ReadDenoised, SetTemporalHistory, ReadPreview, RenderUntil,
//   ReadErrorMap, ReadRefined, SetHistoryVariance, SetHistoryAntiLag, ReadGuidedPreview, ReadDisplay, SetEdgeResolve,
//   SetFireflyClamp, ReadFireflySummary, UpdatePrimitives, RebuildTree, TreeCost.
#ifndef GPUART_RENDERER_H
#define GPUART_RENDERER_H

#include <chrono>
#include <cstdint>
#include <random>
#include <vector>

#include "bvh.h"
#include "core.h"
#include "gpuart_adaptive.h"
#include "gpuart_antilag.h"
#include "gpuart_build.h"
#include "gpuart_ploc.h"
#include "gpuart_edit.h"
#include "gpuart_nearest.h"
#include "gpuart_converge.h"
#include "gpuart_denoise.h"
#include "gpuart_despeckle.h"
#include "gpuart_display.h"
#include "gpuart_edges.h"
#include "gpuart_hip.h"
#include "gpuart_moments.h"
#include "gpuart_refine.h"
#include "gpuart_refit.h"
#include "gpuart_temporal.h"
#include "gpuart_upscale.h"
#include "math_types.h"

/// The luminance floor of the error estimates where none is given: one step of an 8-bit output (gpuart_cli --until-floor,
/// binding.CONVERGE_DEFAULT_FLOOR).
constexpr float GPUART_CONVERGE_DEFAULT_FLOOR = 1.0f / 256;

namespace gpuart {

class Camera {
public:
    Vec3f Pos;         ///< camera position
    Vec3f Dir;         ///< viewing direction
    Vec3f Up;          ///< "up" direction
    float FovY;        ///< vertical field of view, degrees
    float ScreenDist;  ///< distance from Pos to the virtual screen the rays start on
};

class Renderer {
public:
    /// The four uniforms of the reference's cameraInit program (src/renderer.cpp:135-166).
    struct ScreenBasis {
        Vec3f Pos, BottomLeft, DeltaHorz, DeltaVert;
    };
    static ScreenBasis ComputeScreenBasis(const Camera &cam, unsigned width, unsigned height);
    /// PixelSize uniform (src/renderer.cpp:573-574).
    static float ComputePixelSize(const Camera &cam, unsigned height);
    /// SunDirAlt.xyz (src/renderer.h:175-179).
    static Vec3f ComputeSunDirection(float azimuth, float altitude);

    /// Use GetIsOK() to verify successful initialisation. `device` = HIP device ordinal.
    Renderer(unsigned viewportWidth, unsigned viewportHeight, const Camera &camera, int device = 0);
    ~Renderer();
    Renderer(const Renderer &) = delete;
    Renderer &operator=(const Renderer &) = delete;

    /// May reorder `primitives`; keeps nothing of them afterwards.
    void SetPrimitives(std::vector<Primitive *> &primitives, bool printInfo);
    /// Moves primitives of the scene SetPrimitives built and refits its tree on the device (include/gpuart_refit.h); the topology stays, so
    /// the boxes loosen as primitives drift: a long drift wants a SetPrimitives. `indices`: n strictly ascending indices into the vector
    /// SetPrimitives left behind (the ordinals TraceRays returns), `moved` the primitives they become, of the same types. Like
    /// SetUserSpherePos it first commits the view it is about to leave, so the temporal histories survive: their tap validation by hit
    /// point, normal and class discards what moved, and the lighting elsewhere lags by at most the history window, as for a moved
    /// diffuse user sphere. The accumulation restarts (ResetPathTracing, which also clears a non-uniform adaptive accumulator: no
    /// state of RenderAdaptive refuses an update). False — the scene, the tree and the images as they were; std::cerr says why — for
    /// indices that are not ascending or out of range, a changed type, and a primitive outside csrc/hip/prim_rule.h (a word that is not
    /// finite or beyond 2^20, a negative radius), and for a scene whose tree the uploader classified irregular or disorderly.
    bool UpdatePrimitives(const uint32_t *indices, Primitive *const *moved, size_t n);
    /// Rebuilds the scene's tree on the device in Morton order (include/gpuart_build.h) — what a long drift of UpdatePrimitives wants,
    /// without SetPrimitives' host build, upload and dropped histories. The primitives are renumbered: the primitive with ordinal p
    /// (TraceRays, UpdatePrimitives) is the one that had ordinal (*newToOld)[p] before — reorder a kept vector by it, and ordinal i is
    /// primitives[i] again as after SetPrimitives. The temporal histories are kept as for UpdatePrimitives (the view is committed first);
    /// the accumulation restarts; GetBVH() is the rebuilt tree. False — everything as it was; std::cerr says why — for a scene whose
    /// tree the uploader classified irregular or disorderly and for an empty scene.
    /// `mode`: TREE_MORTON, the build above (0.3-0.6 ms on the device, a tree that walks badly), or TREE_CLUSTERED, the clustered build of
    /// include/gpuart_ploc.h (locally-ordered clustering from the same order; more launches, a tree of lower cost): Morton when the
    /// build time is what matters, clustered when the tree will be walked for more than a few passes. The clustered tree's topology
    /// comes back from the device (two ref words per record) and the host tree adopts it (BoundingVolumesHierarchy::AdoptTopology)
    /// before the device arrays are swapped: every refusal leaves everything as it was.
    enum TreeMode { TREE_MORTON = 0, TREE_CLUSTERED = 1 };
    bool RebuildTree(std::vector<uint32_t> *newToOld = nullptr, int mode = TREE_MORTON);
    /// Removes the primitives with the device ordinals `remove` (strictly ascending) from the scene, appends `added` (any types) and
    /// builds the tree of the result on the device in `mode` (include/gpuart_edit.h): device to device but for the lists, with no host
    /// build and no upload. The host tree gives its verdict first; the device edits into staging arrays and builds into the spare set,
    /// so a refusal up to there leaves both trees as they were; then the host tree follows (BoundingVolumesHierarchy::EditPrimitives,
    /// then the device's order or topology) and the context adopts the result (gpuart_hip_scene_replaced). `*source` receives, per new
    /// device ordinal, the old ordinal of a survivor or nOld + k for added[k]. The temporal histories are kept exactly as for
    /// RebuildTree; UpdatePrimitives, RebuildTree, TreeCost, TraceRays and Pick work on the edited scene. The caller keeps `added`.
    bool EditPrimitives(const uint32_t *remove, size_t nRemove, Primitive *const *added, size_t nAdd, std::vector<uint32_t> *source = nullptr,
                        int mode = TREE_CLUSTERED);
    /// The tree's cost as gpuart_build_cost measures it on the device arrays: the sum over the records of both children's half-areas
    /// over the root's. It grows as refitted boxes loosen; RebuildTree brings it back down.
    bool TreeCost(double *cost);
    /// {total, host tree} ms of the last RebuildTree.
    const double *GetLastRebuildMs() const { return LastRebuildMs; }
    bool UpdateViewportSize(unsigned width, unsigned height);
    bool SetCamera(const Camera &cam);

    void SetSunAzimuth(float azimuth) { Lighting.azimuth = azimuth; DropTemporalHistory(); ResetPathTracing(); }
    float GetSunAzimuth() const { return Lighting.azimuth; }
    void SetSunAltitude(float altitude) { Lighting.altitude = altitude; DropTemporalHistory(); ResetPathTracing(); }
    float GetSunAltitude() const { return Lighting.altitude; }
    void SetSunDirectLighting(bool enabled = true) { Lighting.directLightingEnabled = enabled; DropTemporalHistory(); ResetPathTracing(); }
    bool IsSunDirectLightingEnabled() const { return Lighting.directLightingEnabled; }

    /// Use radius = 0 to effectively disable the user-controlled sphere.
    void SetUserSphere(const Vec3f &pos, float radius, float emittance);
    void SetUserSphereSpecular(bool specular) { SetFlag(SPECULAR, specular); }
    void SetUserSphereFuzzy(bool fuzzy) { SetFlag(FUZZY, fuzzy); }
    void SetUserSphereRadius(float radius) { CommitTemporalView(); UserSphere.radius = radius; ResetPathTracing(); }
    void SetUserSpherePos(const Vec3f &pos) { CommitTemporalView(); UserSphere.pos = pos; ResetPathTracing(); }
    void SetUserSphereEmittance(float em);
    Vec3f GetUserSpherePos() const { return UserSphere.pos; }
    float GetUserSphereRadius() const { return UserSphere.radius; }
    float GetUserSphereEmittance() const { return UserSphere.emittance; }

    void RenderDirectLighting();
    void RestartPathTracing(unsigned pathsPerPass, unsigned pathsPerPixel);
    /// Renders one progressive pass (if paths remain); returns paths per pixel rendered so far.
    unsigned RenderPathTracingPass();
    unsigned GetPathsPerPixel() const { return PathTracing.pathsPerPixel; }
    bool GetIsOK() const { return IsOK; }

    // ---- additions -------------------------------------------------------------------------
    /// RGBA32F, tile-sized, row 0 = bottom row. Synchronises.
    bool ReadDirectLighting(float *rgba);
    /// Accumulated radiance; normalized = divided by the paths rendered (what ptracingNormalize shows).
    bool ReadRadiance(float *rgba, bool normalized);
    /// The denoised preview of the accumulator (include/gpuart_denoise.h): the radiance divided by the paths rendered, filtered with the
    /// G-buffer of the tile (gpuart_hip_gbuffer with the current user sphere, kept until the camera, the scene, the user sphere or the
    /// tile changes). RGBA32F, tile-sized, row 0 = bottom row; p = nullptr: the defaults. The accumulator, the passes that follow and
    /// the counters are not touched. Synchronises.
    bool ReadDenoised(float *rgba, const gpuart_denoise_params *p = nullptr);
    /// Carries path-traced history across camera and user-sphere moves (include/gpuart_temporal.h); off by default. While it is on,
    /// SetCamera, SetUserSpherePos and SetUserSphereRadius first commit the view they are about to leave, if it has at least one path
    /// rendered: its normalised accumulator and G-buffer are blended with the history (parameters `tp`; nullptr: the library's
    /// defaults) and become the history. Every other call that restarts the accumulation drops the history — the scene, the Sun, the
    /// user sphere's emittance and flags (SetUserSphere included: it sets the emittance), the path limits, the seed, the visiting
    /// order, the viewport, the tile or share, a loaded checkpoint — and so does switching it off. RestartPathTracing keeps it.
    /// While it is off no setter does any work for it. False for parameters out of range (nothing changes).
    bool SetTemporalHistory(bool on, const gpuart_temporal_params *tp = nullptr);
    bool GetTemporalHistory() const { return TemporalOn; }
    /// The preview while things move: the history re-sampled into the current view and blended with the current accumulator
    /// (gpuart_temporal_accumulate without commit; tp = nullptr: what SetTemporalHistory was given), then filtered like ReadDenoised
    /// (dn). Exactly ReadDenoised while history is off, before the first commit, and before the view's first path. The history, the
    /// accumulator, the passes that follow and the counters are not touched. Synchronises.
    bool ReadPreview(float *rgba, const gpuart_denoise_params *dn = nullptr, const gpuart_temporal_params *tp = nullptr);
    /// Carries the moments of the luminance through a second history (include/gpuart_moments.h); off by default. While it is on, every
    /// commit of SetTemporalHistory also commits the packed image {L, L*L, 1/s, a} of the same view to a second gpuart_temporal handle,
    /// with the same G-buffer, view and parameters; if either commit fails both histories are dropped. Turning it on or off drops the
    /// temporal history: the two handles must have seen the same commits. p = nullptr: the library's defaults. False for parameters out
    /// of range (nothing changes).
    bool SetHistoryVariance(bool on, const gpuart_moments_params *p = nullptr);
    bool GetHistoryVariance() const { return VarianceOn; }
    /// Carries the radiance through a third, short history as well and lets ReadGuidedPreview follow it where the lighting has changed
    /// (include/gpuart_antilag.h); off by default, and without effect unless SetTemporalHistory and SetHistoryVariance are both on.
    /// While it is on, every commit also commits the same staged view to a third gpuart_temporal handle, with the same G-buffer, view
    /// and parameters but max_history = min(fast_history, the commits' max_history); if any of the three commits fails all three
    /// histories are dropped. ReadGuidedPreview then blends that history too and gpuart_antilag_mix moves the long blend and its len
    /// towards the short one before the error map is made. Turning it on or off drops the temporal history: the three handles must
    /// have seen the same commits. p = nullptr: the library's defaults. False for parameters out of range (nothing changes).
    bool SetHistoryAntiLag(bool on, const gpuart_antilag_params *p = nullptr);
    bool GetHistoryAntiLag() const { return AntiLagOn; }
    /// Resolves geometric edges in the filtered frames from a sub-pixel G-buffer (include/gpuart_edges.h); off by default. While it is
    /// on, ReadDenoised, ReadPreview, ReadGuidedPreview and ReadRefined — and ReadDisplay of them — end in gpuart_edges_mark on the
    /// view's G-buffer, gpuart_hip_trace_subpixel for the listed pixels with the header's offset table, and gpuart_edges_resolve of the
    /// filtered plane into a plane of its own. The list and the sub-pixel records are cached with the G-buffer: they are made again when
    /// it is (a new camera, user sphere, tile or scene), when the user sphere's flags change, and when this call changes anything. The
    /// accumulator, the passes that follow, the counters, the estimates, the temporal commits and the moments never see a resolved
    /// value. p = nullptr: the library's defaults. False for parameters out of range (nothing changes). With the switch off every
    /// read launches what it launched before the switch existed.
    bool SetEdgeResolve(bool on, const gpuart_edges_params *p = nullptr);
    bool GetEdgeResolve() const { return EdgeOn; }
    /// Clamps fireflies ahead of the filters and the temporal history (include/gpuart_despeckle.h); off by default. While it is on, the
    /// view every filtered read and every commit stages — the normalised accumulator with the view's cached G-buffer — is clamped in
    /// place by gpuart_despeckle_run before anything reads it: ReadDenoised, ReadPreview, ReadGuidedPreview, ReadRefined and ReadDisplay
    /// of them filter the clamped frame, and the commits of SetTemporalHistory (so also the moments' and the fast history's input) take
    /// it. ReadRadiance, ReadDirectLighting, ReadDisplay(RADIANCE / DIRECT), the accumulator, the passes that follow, the counters and
    /// timings, the convergence and adaptive estimates (they read the raw accumulator), the cached G-buffer and the edge list never see a
    /// clamped value. The clamp is biased: it removes energy, and with a history that energy does not come back; ReadFireflySummary
    /// says how many pixels it touched. Switching it on or off, or changing its parameters, drops the temporal history: the existing
    /// one has seen other inputs. p = nullptr: the library's defaults. False for parameters out of range (nothing changes). With the
    /// switch off every read launches what it launched before the switch existed.
    bool SetFireflyClamp(bool on, const gpuart_despeckle_params *p = nullptr);
    bool GetFireflyClamp() const { return FireflyOn; }
    /// The counts of the last clamp a read or a commit ran (gpuart_despeckle_read_summary); false before the first.
    bool ReadFireflySummary(gpuart_despeckle_summary *out);
    /// The preview guided by the history's measured variance: the radiance and the packed moments of the current accumulator are blended
    /// with their histories (gpuart_temporal_accumulate without commit; tp = nullptr: what SetTemporalHistory was given),
    /// gpuart_moments_error turns the two blends into an error map for lumFloor, and gpuart_refine_run (rf; nullptr: its defaults)
    /// filters the blended radiance with it. Before the first commit the same sequence runs: every pixel then takes the spatial
    /// estimate. False while SetHistoryVariance or SetTemporalHistory is off and before the view's first path. The histories, the
    /// accumulator, the passes that follow, the counters, RenderUntil's estimate and the cached G-buffer are not touched. Synchronises.
    bool ReadGuidedPreview(float *rgba, float lumFloor, const gpuart_refine_params *rf = nullptr, const gpuart_temporal_params *tp = nullptr);
    /// Render until the noise is below a threshold (include/gpuart_converge.h): continues the current accumulation in batches of at
    /// least batchPaths paths per pixel (whole RenderPathTracingPass calls; the target of RestartPathTracing / ExtendPathTracing is the
    /// cap). After every batch the raw accumulator goes to the estimator, from the second batch on the frame is measured: e = the
    /// standard error of a pixel's mean luminance over max(that luminance, lumFloor). Returns 1 as soon as at most maxAboveShare of the
    /// tile's pixels have !(e <= threshold), 0 when the cap was reached first, -1 on error (arguments out of range included: threshold
    /// finite and >= 0, maxAboveShare >= 0, batchPaths >= 1, lumFloor finite and > 0). `last` is filled whenever a measure ran. The
    /// RandSeed draws, and so the accumulator, are those of the same number of plain RenderPathTracingPass calls; passes rendered by
    /// such calls in between simply join the next batch, and paths the estimate has never seen (a loaded checkpoint, plain passes
    /// after a restart) are its first batch, of their own weight, before anything is rendered. Every call that restarts the accumulation restarts the estimate. A batch
    /// ends in a wait for the device.
    int RenderUntil(float threshold, float maxAboveShare, unsigned batchPaths, float lumFloor, gpuart_converge_summary *last = nullptr);
    /// e per tile pixel (Tile.w*Tile.h floats, row 0 = bottom row) as of RenderUntil's last batch; false before its second batch.
    bool ReadErrorMap(float *e, float lumFloor);
    /// The frame RenderUntil leaves, filtered by its own error estimate (include/gpuart_refine.h): the radiance divided by the paths
    /// rendered and the G-buffer of the tile, as ReadDenoised stages them, and the error map of RenderUntil's last batch for lumFloor
    /// (measured into a device buffer of the Renderer's own). RGBA32F, tile-sized, row 0 = bottom row; p = nullptr: the defaults. False
    /// before RenderUntil's second batch, exactly where ReadErrorMap is. Paths rendered by plain passes after the last batch are in the
    /// filtered image but not in the map: the map is then slightly too large and the filter slightly too strong. The accumulator, the
    /// passes that follow, the counters, the estimate and RenderUntil's later summaries, the temporal history and the cached G-buffer
    /// are not touched. Synchronises.
    bool ReadRefined(float *rgba, float lumFloor, const gpuart_refine_params *p = nullptr);
    /// One of the frames above as 8-bit RGBA, encoded on the device (include/gpuart_display.h): Tile.w*Tile.h*4 bytes, row 0 = bottom row,
    /// alpha 255. It runs exactly the device sequence of the Read* that `source` names — ReadRadiance(normalized), ReadDirectLighting,
    /// ReadDenoised, ReadPreview, ReadGuidedPreview or ReadRefined, the filters with their default parameters, lumFloor for the last
    /// two — then gpuart_display_run on that sequence's plane in device memory (dp = nullptr: the defaults, which are the bytes
    /// gpuart_cli --ppm makes of the float frame), and copies 4 bytes per pixel back instead of 16. False wherever that Read* is false,
    /// and for parameters out of range. The dither pattern's origin is the tile's (x0, y0); on an interleaved share it follows the
    /// share's local rows, not the frame's. With auto_exposure the adapted gain lives in the Renderer's display handle: SetCamera and
    /// the user-sphere moves keep it (adapting across views is what `adapt` is for), everything that drops the temporal history —
    /// see SetTemporalHistory — forgets it. The accumulator, the passes that follow, the counters, the estimates, the temporal
    /// histories and the cached G-buffer are what they are without the call. Synchronises.
    bool ReadDisplay(uint8_t *rgba8, gpuart_display_source source, const gpuart_display_params *dp = nullptr,
                     float lumFloor = GPUART_CONVERGE_DEFAULT_FLOOR);
    /// One of the frames above `scale` (2..4) times larger in each direction, upsampled under the guidance of a G-buffer of the larger
    /// frame (include/gpuart_upscale.h): scale*Tile.w x scale*Tile.h RGBA32F, row 0 = bottom row, the tile (scale*x0, scale*y0) of a
    /// frame of scale times the viewport. It runs the device sequence of the Read* that `source` names (any source of ReadDisplay; the
    /// filters with their default parameters, lumFloor where they take one) with edge resolve skipped for this call even while
    /// SetEdgeResolve is on — the upscaler places every output pixel on its own surface, which is what edge resolve approximates by
    /// averaging; the switch, its cache and every other read are untouched —, ensures the view's G-buffer also for RADIANCE and DIRECT,
    /// takes the larger frame's G-buffer from gpuart_hip_gbuffer_scaled into a buffer of its own (cached like the view's G-buffer: made
    /// again after a new camera, user sphere, tile or scene, and when `scale` changes; 52 bytes per output pixel with the plane) and
    /// runs gpuart_upscale_run (p = nullptr: the defaults). False, with a message and nothing changed, for scale outside 2..4, for an
    /// interleaved tile or a share of several GPUs, for parameters out of range, and wherever the Read* of `source` is false. It never
    /// commits a history; the accumulator, the passes that follow, the counters, the estimates, the histories and the cached G-buffer
    /// are what they are without the call, and while it is unused nothing launches that did not launch before. Synchronises.
    bool ReadUpscaled(float *rgba, gpuart_display_source source, uint32_t scale, float lumFloor = GPUART_CONVERGE_DEFAULT_FLOOR,
                      const gpuart_upscale_params *p = nullptr);
    /// The same plane as 8-bit RGBA through the Renderer's one display handle, at the scaled size and the scaled tile origin:
    /// scale*Tile.w * scale*Tile.h * 4 bytes leave the device. Its exposure state adapts as ReadDisplay's does.
    bool ReadUpscaledDisplay(uint8_t *rgba8, gpuart_display_source source, uint32_t scale, const gpuart_display_params *dp = nullptr,
                             float lumFloor = GPUART_CONVERGE_DEFAULT_FLOOR, const gpuart_upscale_params *p = nullptr);
    /// Adaptive sampling (include/gpuart_adaptive.h, gpuart_hip_set_active_blocks): RenderUntil's loop with the estimate kept per 8x8
    /// block of the tile. It continues the current accumulation in batches of at least batchPaths paths per pixel towards the cap of
    /// RestartPathTracing / ExtendPathTracing; after every batch the raw accumulator and the blocks' path counts go to the estimator,
    /// and from the second batch on every block whose pixels all have e <= threshold, and which holds at least minPaths paths and two
    /// batches, is retired: the passes that follow render the remaining blocks only. Blocks never come back. Returns 1 when no block
    /// is active, 0 at the cap, -1 on error (arguments out of range included: RenderUntil's checks and minPaths >= 1) and while
    /// temporal history is on (the blend takes one path count). `last` is filled whenever a select ran. One RandSeed is drawn per pass
    /// whatever the list is — the draws are those of the same number of plain calls — and a pixel's randomness depends on nothing
    /// else, so a block that ends with n paths is, bit for bit, that block of a plain render stopped at n paths. Paths already in the
    /// accumulator (plain passes, a loaded checkpoint, an earlier RenderUntil) are the first batch, of their own weight.
    /// GetNumPathsRendered keeps counting issued paths: the largest block count. Once a block has been retired the counts are not
    /// uniform any more: ReadRadiance(normalized), ReadDenoised, ReadPreview and ReadRefined then divide every block by its own count,
    /// ReadErrorMap / ReadRefined take this estimate's map while it saw the last batch, and RenderUntil, SaveCheckpoint, GatherRadiance
    /// and SetTemporalHistory(true) are refused until something restarts the accumulation (which also resets this estimate).
    int RenderAdaptive(float threshold, unsigned minPaths, unsigned batchPaths, float lumFloor, gpuart_adaptive_summary *last = nullptr);
    /// Paths accumulated into every tile pixel (Tile.w*Tile.h words, row 0 = bottom row): its block's count.
    bool ReadSampleCounts(uint32_t *perPixel);
    bool Finish();
    void SetMaxPathSegments(unsigned n) { MaxPathSegments = n; DropTemporalHistory(); ResetPathTracing(); }
    void SetMinWeight(float w) { MinWeight = w; DropTemporalHistory(); ResetPathTracing(); }
    void SetSeed(uint32_t seed) { RndGen.seed(seed); DropTemporalHistory(); ResetPathTracing(); }
    /// Opts in to the nearer-child-first BVH walk for trees of at least minPrims primitives (0xffffffff = never, the default): ~10 % faster,
    /// soak-verified but NOT proven to return the reference's winner — the reference's phantom hits of grazing triangles are a property
    /// of its own visiting order (include/gpuart_hip.h gpuart_hip_set_nearest_first). Restarts the accumulation like every setter.
    bool SetNearestFirst(uint32_t minPrims);
    /// Restricts this renderer to a tile of the frame (screen-space sharding across GPUs).
    bool SetTile(unsigned x0, unsigned y0, unsigned w, unsigned h);
    /// Row bands interleaved with other renderers (rank r of N: y0 = bandRows*r, bandStride = bandRows*N).
    bool SetInterleavedTile(unsigned x0, unsigned y0, unsigned w, unsigned localRows, unsigned bandRows, unsigned bandStride);
    /// One frame on several GPUs: this renderer renders share `rank` of `nranks` — 8-row bands of
    /// the frame dealt round-robin (gpuart_hip_share_of_rank). Every rank sets up the same scene, camera, lighting and
    /// seed, so all ranks draw the same RandSeed sequence; nothing is exchanged per pass.
    bool SetShare(int rank, int nranks);
    /// Assembles the shares of `ranks[0..n)` (renderer k = SetShare(k, n), one GPU each, all driven by this thread) into
    /// one frame in host memory: W*H RGBA32F, row 0 = bottom row. The rows travel over RCCL to `root`'s GPU
    /// (gpuart_hip_gather_all), normalized = divided by the paths rendered. Replaces the normalise-to-display step of the
    /// reference (src/renderer.cpp:601-616) for a frame that lives on several GPUs.
    static bool GatherRadiance(Renderer *const *ranks, int n, int root, bool normalized, float *fullFrame);
    /// Gives the communicator GatherRadiance made back (ncclCommDestroy per rank) as a named, watched phase of its own, instead
    /// of leaving it to the renderers' destructors at exit. False if a rank's destroy failed or did not return within its bound
    /// (gpuart_hip_comm_stuck() tells which): the caller should then end the process without unwinding.
    static bool ReleaseCommunicator(Renderer *const *ranks, int n);
    unsigned GetNumPathsRendered() const { return PathTracing.numPathsRendered; }
    /// Progressive-render checkpoint: accumulator + pass counters + RNG state of this tile.
    /// After LoadCheckpoint the following passes are bit-identical to those of the uninterrupted run. The
    /// scene, camera, lighting and viewport/tile must have been set up as they were when saving.
    bool SaveCheckpoint(const char *fileName);
    bool LoadCheckpoint(const char *fileName);
    /// Continues the current accumulation towards a new target without clearing it (RestartPathTracing would): used
    /// after LoadCheckpoint to render on to more paths per pixel than the checkpointed run asked for.
    void ExtendPathTracing(unsigned pathsPerPass, unsigned pathsPerPixel);
    gpuart_hip_ctx *GetBackend() const { return Backend; }
    /// What the last SetPrimitives spent, in ms: the whole call, the BVH build, its compilation, re-layout + upload (for tools/setprims_time.py).
    const double *GetLastSetPrimitivesMs() const { return LastSetPrimitivesMs; }
    /// Batched ray queries (include/gpuart_hip.h gpuart_hip_trace_rays): `rays` = n x 8 floats {origin.xyz, tmax}{dir.xyz, unused} in host
    /// memory; closest hit — or, with `occlusion`, "is 0 < closest-hit pos < tmax?" — as the reference's CheckBVHIntersection answers it,
    /// including the current user sphere when `withUserSphere`. `prims` (may be null): per ray the index of the hit primitive in the
    /// vector SetPrimitives left behind (-1 none, -2 the user sphere). Synchronous; no image changes. False on error (std::cerr says why).
    bool TraceRays(const float *rays, size_t n, bool occlusion, bool withUserSphere, gpuart_ray_hit *hits, int32_t *prims);
    /// Closest hit under frame pixels xy[2n] = (x, y), row 0 = bottom, any pixel of the viewport: the camera ray RenderDirectLighting
    /// traces for that pixel. Otherwise as TraceRays.
    bool Pick(const uint32_t *xy, size_t n, gpuart_ray_hit *hits, int32_t *prims, bool withUserSphere = true);
    /// Closest-point queries (include/gpuart_nearest.h): `points` = n x 4 floats {p.xyz, r} in host memory; per query the nearest surface
    /// point among the scene's primitives within r (and the current user sphere when `withUserSphere`, ordinal -2), its distance and the
    /// primitive's index in the vector SetPrimitives left behind, as that header defines them. Synchronous; no image changes. The handle
    /// is made by the first call and bound again after SetPrimitives, RebuildTree and EditPrimitives (a refit keeps the binding). False
    /// on refusal — an empty scene, a tree with irregular boxes — or error (std::cerr says why).
    bool ClosestPoints(const float *points, size_t n, bool withUserSphere, gpuart_nearest_hit *hits);
    /// The k nearest primitives of each query (include/gpuart_nearest.h, "k nearest"; 1 <= k <= GPUART_NEAREST_KNN_MAX): hits[i * k + j] is the
    /// j-th nearest of query i within its r, in ascending distance (equal distances by ordinal, the user sphere last), as the record a
    /// neighbour list holds for that primitive; the slots behind the last one found are misses. The handle, its binding and the refusals
    /// are ClosestPoints'. Synchronous; no image changes.
    bool NearestPrimitives(const float *points, size_t n, size_t k, bool withUserSphere, gpuart_nearest_hit *hits);
    /// Neighbour lists (include/gpuart_nearest.h, "Neighbour lists"): per query every primitive within r, as CSR — list i is
    /// items[offsets[i] .. offsets[i + 1]), in the tree's order, the user sphere (ordinal -2) first. The ordinals are those ClosestPoints
    /// reports; the handle, its binding and the refusals are ClosestPoints'. Synchronous; no image changes.
    bool PrimitivesWithin(const float *points, size_t n, bool withUserSphere, std::vector<uint32_t> &offsets, std::vector<gpuart_nearest_hit> &items);
    /// The same by the two-call protocol of gpuart_nearest_within_host: offsets[n + 1] and *total are always written, items only when
    /// it is not NULL and `capacity` records hold the total.
    bool PrimitivesWithin(const float *points, size_t n, bool withUserSphere, uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity, uint64_t *total);
    /// The fill alone, for the offsets a call with items = NULL has just written (gpuart_nearest_within_fill_host): the second step of the
    /// vector form above, which so walks the queries twice and not three times.
    bool FillPrimitivesWithin(const float *points, size_t n, bool withUserSphere, const uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity);
    /// Box overlap (include/gpuart_nearest.h, "Box overlap"): `boxes` = n x 6 floats {lo.xyz, hi.xyz} in host memory; per query, inflated by
    /// `margin` on every side, the ordinals of every primitive whose own box meets it, as CSR — list i is items[offsets[i] .. offsets[i + 1]),
    /// in the tree's order, the user sphere (ordinal -2) first. The ordinals are those ClosestPoints reports; the handle, its binding and the
    /// refusals are ClosestPoints'. Synchronous; no image changes.
    bool PrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, std::vector<uint32_t> &offsets, std::vector<int32_t> &items);
    /// The same by the two-call protocol of gpuart_nearest_overlap_host: offsets[n + 1] and *total are always written, items only when it
    /// is not NULL and `capacity` ordinals hold the total.
    bool PrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total);
    /// The fill alone, for the offsets a call with items = NULL has just written (gpuart_nearest_overlap_fill_host).
    bool FillPrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, const uint32_t *offsets, int32_t *items, size_t capacity);
    /// The overlapping pairs of the scene's own primitives at `margin` (gpuart_nearest_pairs_host): list i holds the ordinals j > i whose box
    /// meets primitive i's inflated box; offsets has GetNumPrimitives() + 1 words. Adjacent triangles of a mesh always overlap: filtering
    /// topological neighbours is the caller's. The vector form, and the two-call protocol as above.
    bool OverlappingPairs(float margin, std::vector<uint32_t> &offsets, std::vector<int32_t> &items);
    bool OverlappingPairs(float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total);
    unsigned GetTileWidth() const { return Tile.w; }
    unsigned GetTileHeight() const { return Tile.h; }
    const BoundingVolumesHierarchy &GetBVH() const { return Tree; }
    gpuart_params MakeParams() const;

private:
    enum UserSphereFlags : uint32_t { EM_NONZERO = 1u << 0, SPECULAR = 1u << 1, FUZZY = 1u << 2 };

    bool IsOK = false;
    int Device = 0;
    /// Device memory for the tile's pixels, or for its 8x8 blocks: allocated again, its content lost, whenever their number changes.
    struct PixelBuffer {
        void *mem = nullptr;
        size_t count = 0;
        bool Fit(size_t n, size_t bytesPerElement, const char *what);  ///< false if `what` failed (std::cerr says why)
        void Release();
    };
    gpuart_denoise *Denoiser = nullptr;  ///< made by the first ReadDenoised
    PixelBuffer DenoiseMem;              ///< radiance (16 B), G-buffer record (32), filtered (16), ordinal (4) per tile pixel
    bool GBufferValid = false;           ///< DenoiseMem holds the G-buffer of this camera, scene and tile for GBufferSphere
    float GBufferSphere[4] = {0, 0, 0, 0};
    gpuart_temporal *Temporal = nullptr;  ///< made by the first commit
    bool TemporalOn = false;
    bool HistoryCommitted = false;        ///< Temporal holds a history
    gpuart_temporal_params TemporalParams{};  ///< of the commits (SetTemporalHistory)
    bool VarianceOn = false;                  ///< SetHistoryVariance: the commits also go to TemporalMoments
    gpuart_temporal *TemporalMoments = nullptr;  ///< the second history: the packed moments, committed whenever Temporal is
    gpuart_moments *Moments = nullptr;        ///< made with TemporalMoments
    gpuart_moments_params MomentsParams{};    ///< of ReadGuidedPreview's error map (SetHistoryVariance)
    PixelBuffer MomentsMem;                   ///< the packed moments (16 B), their blend (16), len (4) and e (4) per tile pixel
    bool AntiLagOn = false;                   ///< SetHistoryAntiLag: while VarianceOn too, the commits also go to TemporalFast
    gpuart_temporal *TemporalFast = nullptr;  ///< the third history: the radiance again, over a short window
    gpuart_antilag *AntiLag = nullptr;        ///< made with TemporalFast
    gpuart_antilag_params AntiLagParams{};    ///< of the third history's window and ReadGuidedPreview's mix (SetHistoryAntiLag)
    PixelBuffer AntiLagMem;                   ///< the fast blend (16 B), its len (4) and alpha (4) per tile pixel
    bool EdgeOn = false;                      ///< SetEdgeResolve
    gpuart_edges *Edges = nullptr;            ///< made by the first read while EdgeOn
    gpuart_edges_params EdgeParams{};         ///< of mark, the sub-pixel rays and resolve (SetEdgeResolve)
    PixelBuffer EdgeMem;                      ///< the resolved plane (16 B) and the list (4) per tile pixel, then the count: Fit(n + 1, 20)
    PixelBuffer EdgeSubMem;                   ///< a record (32 B) and an ordinal (4) per listed pixel and sub-sample
    bool EdgeListValid = false;               ///< EdgeMem's list and EdgeSubMem are those of the cached G-buffer for EdgeFlags
    uint32_t EdgeFlags = 0, EdgeCount = 0;
    bool FireflyOn = false;                   ///< SetFireflyClamp: StageView ends in the clamp
    gpuart_despeckle *Despeckle = nullptr;    ///< made by the first StageView while FireflyOn
    gpuart_despeckle_params FireflyParams{};  ///< of the clamp (SetFireflyClamp)
    gpuart_converge *Converge = nullptr;  ///< made by the first RenderUntil
    unsigned ConvergeBatches = 0, ConvergeTotal = 0;  ///< what Converge has seen since its last reset
    gpuart_adaptive *Adaptive = nullptr;  ///< made by the first RenderAdaptive
    /// The raw accumulator of the last batch an estimate was shown, or the frame a non-uniform ReadRadiance normalises: 16 B per tile
    /// pixel. Nothing reads it after the call that filled it has returned, so the two estimates and that read share it.
    PixelBuffer AccumMem;
    PixelBuffer BlockPathsMem;            ///< one word per 8x8 block of the tile, the counts of the last batch or normalisation
    unsigned AdaptiveBatches = 0, AdaptiveTotal = 0;  ///< what Adaptive has seen since its last reset
    unsigned AdaptiveActive = 0;          ///< blocks on the back end's list while NonUniform
    bool NonUniform = false;              ///< a block has been retired: the blocks' path counts differ
    bool AdaptiveIsLast = false;          ///< the last batch any estimate saw was RenderAdaptive's
    unsigned CountBase = 0;               ///< paths per pixel a loaded checkpoint brought: the back end's block counts begin above them
    gpuart_refine *Refine = nullptr;      ///< made by the first ReadRefined
    PixelBuffer ErrorMem;                 ///< the error map of ReadErrorMap and ReadRefined, 4 B per tile pixel
    gpuart_display *Display = nullptr;    ///< made by the first ReadDisplay
    PixelBuffer DisplayMem;               ///< ReadDisplay's: the plane of RADIANCE and DIRECT (16 B) and the 8-bit frame (4 B) per tile pixel
    gpuart_upscale *Upscaler = nullptr;   ///< made by the first ReadUpscaled
    PixelBuffer UpscaleMem;               ///< per output pixel the larger frame's record (32 B), the upsampled plane (16) and the ordinal (4)
    PixelBuffer UpscaleWords;             ///< ReadUpscaledDisplay's 8-bit frame, 4 B per output pixel
    bool UpscaleValid = false;            ///< UpscaleMem holds the larger frame's G-buffer of the cached G-buffer's view for UpscaleScale
    uint32_t UpscaleScale = 0;
    ScreenBasis CurrentBasis;             ///< what SetCamera gave the back end
    double LastSetPrimitivesMs[4] = {0, 0, 0, 0};
    gpuart_hip_ctx *Backend = nullptr;
    gpuart_refit *Refitter = nullptr;     ///< made by the first UpdatePrimitives; bound again after every upload (the scene's generation)
    uint64_t RefitGeneration = 0;         ///< the generation Refitter is bound to (0: none; the first upload's is 1)
    gpuart_build *Builder = nullptr;      ///< made by the first RebuildTree or TreeCost
    gpuart_ploc *Clusterer = nullptr;     ///< made by the first RebuildTree(TREE_CLUSTERED)
    gpuart_edit *Editor = nullptr;        ///< made by the first EditPrimitives
    gpuart_nearest *Nearest = nullptr;    ///< made by the first ClosestPoints or PrimitivesWithin
    uint64_t NearestGeneration = 0;       ///< the generation Nearest is bound to (0: none)
    /// The scene's descriptor with Nearest made and bound to it; false on refusal (`who` names the caller on std::cerr) or error.
    bool BindNearest(const char *who, gpuart_hip_scene &scene);
    /// What BuildIntoSpare hands out beside the spare set's descriptor: new_to_old, the two ref words of each of the nRecs records (the
    /// clustered build's; the Morton order implies its own) and when the device run returned.
    struct BuiltTree {
        std::vector<uint32_t> order, refs;
        uint64_t nRecs = 0;
        std::chrono::high_resolution_clock::time_point ran;
    };
    /// The opening refusal of RebuildTree and EditPrimitives (`fn`): an empty scene, irregular boxes, or a host tree of another count is not `done`.
    bool RefusesTreeChange(const gpuart_hip_scene &scene, const char *fn, const char *done);
    bool EnsureBuilder(bool clustered);
    /// The tree of `src`'s primitives built into the spare set, which is reserved first (`withPrims`: with primitive arrays of its own, for
    /// a list that is not the scene's) and then described by `spare`; `commit`: the view is committed between making the handle and the
    /// run. Failures are reported under `what` (the run) and `fn` (the read-back of the refs) and leave everything as it was.
    bool BuildIntoSpare(const gpuart_hip_scene &src, bool clustered, bool withPrims, bool commit, const char *fn, const char *what, gpuart_hip_scene &spare,
                        BuiltTree &built);
    /// The host tree follows the device's: the Morton order checked and rebuilt, or the clustered topology checked and adopted.
    bool TreeFollows(bool clustered, const BuiltTree &built);
    /// After the device's primitives or tree changed: the G-buffer, the edge list and the accumulator are those of another scene; with
    /// `newArrays` the refit handle is bound to the old ones, and the next UpdatePrimitives binds again.
    void TreeChanged(bool newArrays);
    double LastRebuildMs[2] = {0, 0};
    BoundingVolumesHierarchy Tree;
    struct { unsigned width, height; } Viewport{0, 0};
    struct { unsigned x, y, w, h; } Tile{0, 0, 0, 0};  ///< the part of the frame this renderer owns
    Camera CurrentCamera;
    struct { float azimuth, altitude; bool directLightingEnabled; } Lighting;
    struct { Vec3f pos; float radius, emittance; uint32_t flags; } UserSphere;
    struct { unsigned numPathsRendered, pathsPerPixel, pathsPerPass; } PathTracing;
    unsigned MaxPathSegments = 5;  ///< MAX_PATH_SEGMENTS of the reference shader
    float MinWeight = 0.01f;       ///< MIN_WEIGHT of the reference shader
    std::mt19937 RndGen;           ///< default seed, never re-seeded by the reference

    void SetFlag(uint32_t flag, bool on);
    void ResetPathTracing();
    /// The device buffers of ReadDenoised / ReadPreview / a commit, the G-buffer of the current view (cached) and the normalised accumulator.
    bool StageView();
    /// StageView's first half: DenoiseMem for the tile and in it the G-buffer of the current view and user sphere, made where it is stale.
    bool EnsureGBuffer();
    /// The device half of ReadUpscaled and ReadUpscaledDisplay: the upsampled plane in UpscaleMem, complete, `n` its pixels.
    bool StageUpscaled(gpuart_display_source source, uint32_t scale, float lumFloor, const gpuart_upscale_params *p, const float *&plane, size_t &n);
    bool MakeTemporalView(gpuart_temporal_view &v) const;
    void CommitTemporalView();
    /// Temporal, TemporalMoments, Moments and MomentsMem for the tile, made where missing.
    bool EnsureVarianceHandles();
    /// Makes the handle `h` of the image or tree library `lib` if it is missing.
    template <class H, class L> bool Ensure(H *&h, const L &lib);
    /// Run, then wait for that handle: `status` is what the call just issued on `h` returned; both failures are reported under `what`.
    template <class H, class L> bool Run(int status, H *h, const L &lib, const char *what);
    /// The staged view (StageView) blended with the radiance history into the view's filtered plane, `len` (may be null) the blend's
    /// length per pixel; tp = nullptr: TemporalParams; with `commit` the blend becomes the history. BlendMoments: the same for the
    /// second history, the view's moments packed and blended with theirs in MomentsMem.
    bool BlendHistory(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit, float *len);
    bool BlendMoments(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit);
    /// The third history is kept and mixed in: both switches are on.
    bool AntiLagActive() const { return AntiLagOn && VarianceOn; }
    /// TemporalFast, AntiLag and AntiLagMem for the tile, made where missing.
    bool EnsureAntiLagHandles();
    /// BlendHistory for the third history, into AntiLagMem with its len: tp's (nullptr: TemporalParams') max_history is capped by
    /// fast_history.
    bool BlendFast(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit);
    /// The device halves of the Read* of the same names: each leaves its frame in device memory, complete, and says where.
    bool StageDenoised(const gpuart_denoise_params *p, const float *&plane);
    bool StagePreview(const gpuart_denoise_params *dn, const gpuart_temporal_params *tp, const float *&plane);
    bool StageGuidedPreview(float lumFloor, const gpuart_refine_params *rf, const gpuart_temporal_params *tp, const float *&plane);
    bool StageRefined(float lumFloor, const gpuart_refine_params *p, const float *&plane);
    /// Where EdgeOn, the filtered frame `plane` (of the view StageView staged) resolved into EdgeMem's plane, which `plane` then names.
    bool ResolveEdges(const float *&plane);
    /// The one table of the frames a read can ask for: the Stage* that `source` names with the parameters it takes, or for RADIANCE and
    /// DIRECT the export into `own` (tile-sized device memory; may be null for the others). False for a source that does not exist.
    bool StageSource(gpuart_display_source source, float lumFloor, const gpuart_denoise_params *dn, const gpuart_refine_params *rf,
                     const gpuart_temporal_params *tp, float *own, const float *&plane);
    /// A float Read*: StageSource and ReadPlane, Tile.w*Tile.h elements of device memory into host memory (`what` names a failed copy).
    bool ReadStaged(float *rgba, const char *what, gpuart_display_source source, float lumFloor, const gpuart_denoise_params *dn,
                    const gpuart_refine_params *rf, const gpuart_temporal_params *tp);
    bool ReadPlane(void *host, const void *plane, size_t bytesPerPixel, const char *what);
    /// Which estimate saw the last batch, and so whose error map counts: RenderAdaptive's while it did, else RenderUntil's; NONE before
    /// that one's second batch. StageErrorMap leaves that map for lumFloor in ErrorMem, complete on return (false for NONE).
    enum Estimate { NONE, UNIFORM, ADAPTIVE };
    Estimate LastEstimate() const {
        return Adaptive && AdaptiveIsLast && AdaptiveBatches >= 2 ? ADAPTIVE : Converge && ConvergeBatches >= 2 ? UNIFORM : NONE;
    }
    bool StageErrorMap(float lumFloor, const float *&map);
    /// The loop of RenderUntil and RenderAdaptive on an estimate that has seen `batches` batches and `total` paths (both read again after
    /// every show): show() gives it the accumulator as one more batch, judge() is asked from the second batch on and ends the loop
    /// with anything but 0. 0 at the cap, -1 where a pass or show failed.
    template <class Show, class Judge> int RenderBatches(unsigned batchPaths, const unsigned &batches, const unsigned &total, Show show, Judge judge);
    /// Every call that drops the history also forgets the display stage's adapted exposure.
    void DropTemporalHistory() { if (Display) gpuart_display_reset(Display); if (HistoryCommitted) DropTemporalHistoryNow(); }
    void DropTemporalHistoryNow();
    void ResetConvergeNow();
    void ResetAdaptiveNow();
    size_t TileBlocks() const { return (size_t)((Tile.w + 7) / 8) * ((Tile.h + 7) / 8); }
    /// The blocks' path counts (the checkpoint's included) into BlockPathsMem; complete after the next gpuart_hip_finish.
    bool StageBlockPaths();
    /// What a normalised read divides by: the paths rendered, which is the reference's ptracingNormalize program
    /// (shaders/pt_normalize.glsl:44-47); 1 for a raw read and before the first path.
    float Divisor(bool normalized) const { return normalized && PathTracing.numPathsRendered ? (float)PathTracing.numPathsRendered : 1.0f; }
    /// Image `which` of the back end (0 direct lighting, 1 the accumulator) divided by `div` into tile-sized device memory, with the
    /// blocks' counts in BlockPathsMem where asked; complete on return.
    bool Export(int which, float *device, float div, bool withBlockPaths = false);
    /// The one normalisation: the accumulator divided by the paths rendered into tile-sized device memory, complete on return. While the
    /// counts are uniform gpuart_hip_export's scalar division, as ever; otherwise the raw export and gpuart_adaptive_normalize.
    bool ExportNormalized(float *device);
    /// A status of the back end or, with their gpuart_*_last_error, of one of the image libraries: false (std::cerr says why) unless 0.
    bool Check(int status, const char *what, const char *(*lastError)(void) = gpuart_hip_last_error);
};

}  // namespace gpuart
#endif
