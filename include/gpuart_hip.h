/* gpuart_hip.h — C ABI of libgpuart_hip.so, the MI355X (gfx950) device back end of gpuart.
 *
 * Drop-in boundary: this library replaces the reference's OpenGL wrapper layer
 * (reference src/gl_utils.h:108-379 — GL::Buffer/Texture/Shader/Program/Framebuffer and
 * GL::Utils::DrawFullscreenQuad) together with the GLSL programs the reference's Renderer
 * launches through it (reference src/renderer.cpp:259-359). The C++ `gpuart::Renderer`
 * (gpuart_amd/csrc/host/renderer.{h,cpp}) keeps the reference's public API and calls only the
 * functions below; INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes, no C++ types, no exceptions across the boundary.
 * Every function returns 0 on success or a negative gpuart_hip_status; the message of the last
 * failure (per thread) is available from gpuart_hip_last_error(). One context per device;
 * contexts are independent. Host buffers are caller-owned. Work is asynchronous on the
 * context's own HIP stream until gpuart_hip_finish() / a read-back.
 *
 * Image convention (as the reference's full-screen quad): row 0 is the BOTTOM row; pixels are
 * RGBA32F; a context renders only its tile [x0,x0+tw) x [y0,y0+th) of the W x H frame and its
 * buffers are tile-sized.
 */
#ifndef GPUART_HIP_H
#define GPUART_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gpuart_hip_ctx gpuart_hip_ctx;

typedef enum gpuart_hip_status {
    GPUART_HIP_OK = 0,
    GPUART_HIP_ERR_ARG = -1,      /* bad argument / call order (e.g. render before upload) */
    GPUART_HIP_ERR_DEVICE = -2,   /* a HIP runtime call failed */
    GPUART_HIP_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
    GPUART_HIP_ERR_TIMEOUT = -4,  /* a bounded wait ran out (gpuart_hip_wait, the waits of the gather, an RCCL call that did not return): a peer is missing */
    GPUART_HIP_ERR_NO_COMM = -5   /* the contexts are not (or no longer) the ranks of one communicator: make one and call again */
} gpuart_hip_status;

/* The uniforms of the reference's directLighting / pathTracing programs
 * (reference src/renderer.cpp:51-79,383-398,567-589; shaders/path_tracing.glsl:82-108). */
typedef struct gpuart_params {
    float sunDirAlt[4];       /* SunDirAlt: unit direction towards the Sun, altitude (rad) */
    int32_t sunEnabled;       /* SunDirectLightingEnabled */
    float userSphere[4];      /* UserSphere: centre, radius (radius 0 = disabled) */
    float userSphereEm[3];    /* UserSphereEm */
    uint32_t userSphereFlags; /* UserSphereFlags: 1 = EM_NONZERO, 2 = SPECULAR, 4 = FUZZY */
    float pixelSize;          /* PixelSize */
    float cameraPos[3];       /* CameraPos */
    int32_t maxSegments;      /* MAX_PATH_SEGMENTS, a shader const (5) in the reference; at most GPUART_HIP_MAX_SEGMENTS */
    float minWeight;          /* MIN_WEIGHT, a shader const (0.01) in the reference */
} gpuart_params;

#define GPUART_HIP_MAX_SEGMENTS 1024 /* gpuart_hip_pt_pass rejects larger maxSegments (one launch + counters per segment) */

/* Exact work counters (closest-hit queries as the reference performs them). */
typedef struct gpuart_counters {
    uint64_t rays;          /* closest-hit BVH queries: camera, bounce and shadow rays */
    uint64_t nodes;         /* distinct BVH nodes whose box was tested, summed over rays */
    uint64_t prim_tests[4]; /* tested primitives by type: sphere, disc, triangle, cone */
    uint64_t segments;      /* path segments traced */
    uint64_t box_steps;     /* interior-node visits (one 64-byte record fetch each) */
    uint64_t box_steps_top; /* ... of nodes above level GPUART_HIP_TOP_DEPTH (environment, read at upload; diagnostic) */
    uint64_t rewalks;       /* mode 4: closest-hit queries whose nearest-child-first walk could not certify its answer and that
                             * were walked again in the reference's order (their second walk's nodes / primitives are counted) */
} gpuart_counters;

const char *gpuart_hip_last_error(void);

/* Replaces GL::Init + the Renderer constructor's shader/program creation
 * (reference src/gl_utils.cpp:133-155, src/renderer.cpp:217-359). */
int gpuart_hip_create(int device, gpuart_hip_ctx **out);
int gpuart_hip_destroy(gpuart_hip_ctx *ctx);

/* Replaces Renderer::InitPerPixelTextures (reference src/renderer.cpp:169-194): frame size and
 * the tile this context owns (default: the whole frame). Clears the accumulator. */
int gpuart_hip_resize(gpuart_hip_ctx *ctx, uint32_t width, uint32_t height);
int gpuart_hip_set_tile(gpuart_hip_ctx *ctx, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th);
/* Row-interleaved tile for load-balanced multi-GPU sharding: the context owns th_local rows, local row ly being
 * frame row y0 + (ly / band_rows) * band_stride + ly % band_rows (e.g. rank r of N: y0 = 8r, band_rows = 8,
 * band_stride = 8N). Buffers and read-backs are tw x th_local, local row order. */
int gpuart_hip_set_tile_interleaved(gpuart_hip_ctx *ctx, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th_local,
                                    uint32_t band_rows, uint32_t band_stride);

/* Replaces the GL_TEXTURE_BUFFER upload of Renderer::SetPrimitives (reference
 * src/renderer.cpp:472-475). `quads` is the reference's canonical compiled tree
 * (BoundingVolumesHierarchy::Compile, reference src/bvh.cpp:161-222), nquads RGBA32F quads;
 * it is re-laid out on upload into the flat SoA device arrays described in DESIGN.md. */
int gpuart_hip_upload_bvh(gpuart_hip_ctx *ctx, const float *quads, size_t nquads);

/* Replaces the cameraInit program (reference shaders/cam_init.glsl:45-50, launched from
 * Renderer::SetCamera, src/renderer.cpp:151-161): stores Pos/BottomLeft/DeltaHorz/DeltaVert;
 * primary rays are regenerated in-kernel instead of being written to two ray textures. */
int gpuart_hip_set_camera(gpuart_hip_ctx *ctx, const float pos[3], const float bottomLeft[3],
                          const float deltaHorz[3], const float deltaVert[3]);

/* Replaces the directLighting draw (reference src/renderer.cpp:372-404,
 * shaders/direct_lighting.glsl:134-207). Result in the context's frame buffer. */
int gpuart_hip_render_direct(gpuart_hip_ctx *ctx, const gpuart_params *p);

/* Replaces the accumulator clear of Renderer::ResetPathTracing (reference src/renderer.cpp:490-500). */
int gpuart_hip_pt_reset(gpuart_hip_ctx *ctx);

/* Scheduling hint, no reference counterpart: how many gpuart_hip_pt_pass calls the caller expects to make before it
 * observes the result (Renderer::RestartPathTracing knows it: pathsPerPixel / pathsPerPass, reference
 * src/renderer.cpp:502-508). Sizes the pipeline runs the passes are grouped into; 0 = unknown. Never changes results. */
int gpuart_hip_pt_plan(gpuart_hip_ctx *ctx, uint32_t passes);

/* Replaces one pathTracing draw (reference src/renderer.cpp:534-599,
 * shaders/path_tracing.glsl:133-256): accum += radiance of `npaths` paths per pixel. */
int gpuart_hip_pt_pass(gpuart_hip_ctx *ctx, const gpuart_params *p, const float randSeed[4], int npaths);

/* Read-back (the reference draws to the GL framebuffer instead; ptracingNormalize,
 * reference shaders/pt_normalize.glsl:44-47, is the `divide_by` of the accumulator).
 * which: 0 = direct-lighting frame, 1 = path-tracing accumulator. divide_by <= 0 means 1.
 * rgba_host receives tw*th*4 floats. Synchronises the stream. */
int gpuart_hip_read(gpuart_hip_ctx *ctx, int which, float *rgba_host, float divide_by);

/* The inverse of gpuart_hip_read for which = 1: replaces the path-tracing accumulator of the tile with tw*th*4 floats
 * from the host (resuming a checkpointed progressive render; the reference has no equivalent). */
int gpuart_hip_write(gpuart_hip_ctx *ctx, int which, const float *rgba_host);

/* Same, device to device, into caller-owned device memory (for the multi-GPU gather: the caller
 * hands it to RCCL). Asynchronous on the context's stream; call gpuart_hip_finish before use. */
int gpuart_hip_export(gpuart_hip_ctx *ctx, int which, void *rgba_device, float divide_by);

/* ---- adaptive sampling: passes over some of the tile's 8x8 blocks (no reference counterpart) ----------------------------
 * The tile's pixels form ceil(tw/8) x ceil(th/8) blocks of 8x8 (ragged at the right and top edges), numbered row-major in the
 * tile's local order. With an active list set, gpuart_hip_pt_pass does for every pixel of a listed block, and for no other pixel,
 * what it does without one: a pixel's randomness depends on the pass's RandSeed and the path's own hit points only. So after any
 * sequence of passes and list changes accum[p] is the fp32 sum, in pass order, of the pass colours of exactly those passes whose
 * list held p's block.
 *
 * blocks: host memory, n indices, strictly ascending, each below the number of blocks; anything else is GPUART_HIP_ERR_ARG and
 * nothing changes. blocks == NULL: all blocks again (and the library's own birth order). n == 0 with a pointer: the empty list —
 * passes succeed, launch nothing and count nothing. Collected passes are flushed first. gpuart_hip_pt_reset clears the list and the
 * counts; gpuart_hip_resize, _set_tile, _set_tile_interleaved and _set_share drop both. A list is honoured in modes 0, 3 and 5;
 * gpuart_hip_pt_pass in modes 1, 2 and 4 with a list set is GPUART_HIP_ERR_ARG. */
int gpuart_hip_set_active_blocks(gpuart_hip_ctx *ctx, const uint32_t *blocks, size_t n);
/* Paths per pixel accumulated into each block since the last gpuart_hip_pt_reset, one word per block, with or without a list ever
 * set (gpuart_hip_write does not count). _read: to host memory, synchronises the stream. _export: to caller-owned device memory,
 * asynchronous on the context's stream like gpuart_hip_export. Both flush collected passes first. */
int gpuart_hip_read_block_paths(gpuart_hip_ctx *ctx, uint32_t *host);
int gpuart_hip_export_block_paths(gpuart_hip_ctx *ctx, void *device);

/* ---- one frame on several GPUs ---------------------------------------------------------------
 * The frame is sharded by rows: bands of `band_rows` rows dealt round-robin to the ranks; ranks exchange nothing per pass;
 * when the passes are done every rank sends its rows to one root over RCCL (point-to-point over xGMI) and the root scatters
 * them into the full frame on its device. Replaces the reference's normalise-to-display step for a frame that lives on
 * several GPUs (reference src/renderer.cpp:601-616, shaders/pt_normalize.glsl:44-47: `divide_by`). */
typedef struct gpuart_tile_geom {
    uint32_t W, H;                    /* the frame */
    uint32_t x0, y0, tw, th;          /* the share: tw x th local pixels; th may be 0 (more ranks than bands) */
    uint32_t band_rows, band_stride;  /* local row ly = frame row y0 + (ly / band_rows) * band_stride + ly % band_rows */
} gpuart_tile_geom;

/* Pure host helpers (no device needed): rank's share of a W x H frame split over nranks in bands of band_rows rows (8 keeps
 * the 8x8 pixel tiles of the path state intact); frame row of a local row; host version of the root's scatter. */
int gpuart_hip_share_of_rank(uint32_t W, uint32_t H, int rank, int nranks, uint32_t band_rows, gpuart_tile_geom *out);
uint32_t gpuart_hip_frame_row(const gpuart_tile_geom *g, uint32_t local_row);
int gpuart_hip_scatter_rows_host(const gpuart_tile_geom *g, const float *tile_rgba, float *full_rgba);

/* The context renders share `g` of its frame (= gpuart_hip_set_tile_interleaved); the share it currently renders. */
int gpuart_hip_set_share(gpuart_hip_ctx *ctx, const gpuart_tile_geom *g);
int gpuart_hip_get_share(gpuart_hip_ctx *ctx, gpuart_tile_geom *g);

/* Communicator. One process per GPU: rank 0 obtains an id (gpuart_hip_comm_unique_id = ncclGetUniqueId), hands its
 * GPUART_HIP_UNIQUE_ID_BYTES bytes to the other ranks by any means (bench.py: torch.distributed broadcast), every rank calls
 * gpuart_hip_comm_init (= ncclCommInitRank on the context's device). One process driving several GPUs (gpuart_cli --gpus N):
 * gpuart_hip_comm_init_all over its contexts (= ncclCommInitAll; context k becomes rank k). A caller that already owns an
 * ncclComm_t attaches it instead (not destroyed with the context). RCCL is loaded on first use. */
#define GPUART_HIP_UNIQUE_ID_BYTES 128
int gpuart_hip_comm_unique_id(void *id128);
int gpuart_hip_comm_init(gpuart_hip_ctx *ctx, int nranks, int rank, const void *id128);
int gpuart_hip_comm_attach(gpuart_hip_ctx *ctx, void *nccl_comm, int nranks, int rank);
int gpuart_hip_comm_init_all(gpuart_hip_ctx *const *ctxs, int n);
int gpuart_hip_comm_destroy(gpuart_hip_ctx *ctx);
/* Which RCCL the library resolved its entry points from (dladdr of ncclCommInitRank): a process that also holds another
 * framework's RCCL — torch.distributed's, say — can record that both are the same file. Loads RCCL if nothing has yet. */
int gpuart_hip_comm_library(char *path, size_t size);
/* What the communicator itself says (ncclCommCount, ncclCommUserRank); GPUART_HIP_ERR_ARG without one. */
int gpuart_hip_comm_info(gpuart_hip_ctx *ctx, int *nranks, int *rank);

/* Collective over the communicator: every rank contributes buffer `which` (0 direct lighting, 1 accumulator) of its share,
 * divided by `divide_by`; on `root`, full_frame_device (W*H*4 floats in the root's device memory, frame row order) receives
 * the assembled frame (other ranks pass NULL). Shares are exchanged through the communicator itself. Asynchronous on the
 * contexts' streams after a short host synchronisation: call gpuart_hip_finish on the root before using the frame.
 * gpuart_hip_gather_all is the same for the ranks 0..n-1 of a gpuart_hip_comm_init_all communicator, from one thread. */
/* Failure behaviour: everything that can fail on one rank alone (pending passes, buffers, arguments) happens BEFORE the
 * ranks commit to a transfer, and its verdict travels with the share, so a rank that cannot take part makes every rank
 * return an error rather than leaving its peers blocked in a receive. The shares must be full-width rows covering every frame
 * row exactly once (gpuart_hip_share_of_rank; a rank beyond the number of bands holds an empty share and sends nothing). The
 * host-side wait for the share exchange is bounded (GPUART_HIP_GATHER_TIMEOUT_MS, default 60 000, 0 = unbounded):
 * GPUART_HIP_ERR_TIMEOUT means a peer never entered the collective.
 * EVERY host-side wait of this section is bounded (round 5; until then only the share exchange of gpuart_hip_gather was):
 *   - waits on the context's stream — the share exchange, the read-back of gpuart_hip_gather_all_read, gpuart_hip_comm_destroy
 *     and gpuart_hip_destroy of a context whose gather gave up — by GPUART_HIP_GATHER_TIMEOUT_MS;
 *   - RCCL calls that return only when peers or RCCL's bootstrap play along — ncclCommInitRank / ncclCommInitAll, the
 *     ncclAllGather enqueue, ncclGroupStart..ncclGroupEnd of the transfers, ncclCommDestroy — by GPUART_HIP_COMM_TIMEOUT_MS
 *     (default 120 000, 0 = unbounded): they run on a helper thread; when the bound runs out the call returns
 *     GPUART_HIP_ERR_TIMEOUT naming the RCCL call, the helper stays parked in it, and from then on every entry point of this
 *     section fails at once with GPUART_HIP_ERR_TIMEOUT (gpuart_hip_comm_stuck() == 1): end the process with _exit.
 * GPUART_HIP_RCCL_LIBRARY names the RCCL to load instead of the system's librccl.so.1. */
int gpuart_hip_gather(gpuart_hip_ctx *ctx, int which, float divide_by, int root, void *full_frame_device);
int gpuart_hip_gather_all(gpuart_hip_ctx *const *ctxs, int n, int which, float divide_by, int root, void *full_frame_device);
/* gpuart_hip_gather_all into host memory (W*H*4 floats): the frame is assembled on the root's device, then read back. */
int gpuart_hip_gather_all_read(gpuart_hip_ctx *const *ctxs, int n, int which, float divide_by, int root, float *full_frame_host);

/* 1 once an RCCL call of this process has outlived GPUART_HIP_COMM_TIMEOUT_MS (see above), else 0. */
int gpuart_hip_comm_stuck(void);

/* Phase watchdog (pure host code; no reference counterpart — the reference's render loop, src/main.cpp:549-599, has nothing
 * that waits for another process). The caller names what it is about to do and how long that may take; gpuart_hip_phase_end
 * disarms. A watcher thread that sees the phase outlive its bound writes the phase, how long it has run and the most recent
 * error messages of libgpuart_hip.so of ALL threads to stderr and ends the process with _exit(86) — no unwinding, nothing is
 * re-executed. One phase at a time (a second begin replaces the first). timeout_ms 0: only the phase lines. Every begin / end
 * writes one line to stderr unless GPUART_HIP_PHASE_LOG=0. gpuart_cli --gpus N and the ranks of bench.py bracket communicator
 * creation, the gather and communicator destruction with it. */
int gpuart_hip_phase_begin(const char *name, uint32_t timeout_ms);
int gpuart_hip_phase_end(void);
/* Phase lines on (1) / off (0) from now on, overriding GPUART_HIP_PHASE_LOG; returns the previous setting. The watchdog is not
 * affected: a caller that brackets something inside a timed region (bench.py's gathers) keeps the bound and drops the two lines. */
int gpuart_hip_phase_log(int on);
/* glFlush() equivalent. gpuart_hip_pt_pass may only *collect* a pass: passes with identical parameters are launched
 * together as one run of the pipeline (path slot = pixel x passes of the run + pass, up to 16M paths, so that the persistent
 * BVH-query waves take many rays per lane and same-pixel rays of different passes share a wavefront), and up to 8 runs are in flight at once on separate HIP streams (fewer when their path state would
 * exceed 16 GB); results are accumulated strictly in pass order. Everything
 * that observes or changes state (read, export, finish, reset, set_camera, ...) flushes by itself. */
int gpuart_hip_flush(gpuart_hip_ctx *ctx);

/* glFinish() equivalent (reference src/main.cpp:564,584). */
int gpuart_hip_finish(gpuart_hip_ctx *ctx);
/* gpuart_hip_finish with a bound: GPUART_HIP_ERR_TIMEOUT if the context's work (e.g. the transfers of a gather whose peer
 * died) is not complete after timeout_ms milliseconds (0: no bound). Nothing is cancelled: the caller decides (bench.py exits). */
int gpuart_hip_wait(gpuart_hip_ctx *ctx, uint32_t timeout_ms);

/* Execution mode of gpuart_hip_pt_pass / gpuart_hip_render_direct (images are identical, bit for bit, in all modes):
 *   0 (default) fast: the launch-per-stage wavefront pipeline (per segment a persistent BVH-query launch that also carries
 *               the previous segment's Sun-shadow queries, and a shading launch; Sun-shadow queries stop at the first accepted
 *               hit and are skipped for surfaces facing away from the Sun), or — when the whole planned pass sequence is
 *               small (an interactive frame) — one persistent kernel per run (k_run) without the chain of dependent launches;
 *   1 "reference work": every query the reference performs is performed as a full closest-hit query, and exact counters
 *               are kept (gpuart_hip_counters); runs through k_run;
 *   2 megakernel: one thread runs a whole path (the first correct version; kept for A/B and cross-checks);
 *   3 the launch pipeline always;   5 k_run always;
 *   4 as 0, with counters of the work the fast mode really executes (rays, nodes, primitives); runs through k_run.
 * Direct lighting: 1 one thread per pixel with counters, 2 one thread per pixel, otherwise persistent lanes. */
int gpuart_hip_set_mode(gpuart_hip_ctx *ctx, int mode);
int gpuart_hip_counters(gpuart_hip_ctx *ctx, gpuart_counters *out, int reset);

/* HIP-event timing on the context's stream. Level 0: none; 1 (default): one event pair around every
 * render call (class 0); 2: additionally one pair around every BVH-query kernel (class 1).
 * gpuart_hip_kernel_time returns the sum and the count of class `cls` since its last reset. */
int gpuart_hip_set_timing(gpuart_hip_ctx *ctx, int level);
int gpuart_hip_kernel_time(gpuart_hip_ctx *ctx, int cls, double *total_ms, uint64_t *launches, int reset);

/* Scene statistics after upload: node count, primitive count, tree depth, device bytes. */
int gpuart_hip_scene_info(gpuart_hip_ctx *ctx, uint64_t *nodes, uint64_t *prims, uint32_t *max_depth,
                          uint64_t *device_bytes);

/* ---- the uploaded scene's device arrays, for a refit in place (include/gpuart_refit.h; DESIGN.md "Refit") ----------------------
 * The arrays stay the context's: they are valid until the next gpuart_hip_upload_bvh or gpuart_hip_destroy, and `generation`, which
 * every upload increments, tells a holder of this struct that it is stale. */
typedef struct gpuart_hip_scene {
    uint32_t layout;      /* 1: the records of DESIGN.md section 3 (64-byte two-children records, 48-byte primitive records) */
    uint32_t exact_boxes; /* the uploader classified the tree irregular or disorderly (gpuart_hip_tree_order: 2) */
    void *recs;           /* device: n_recs records of four float4, pre-order */
    uint64_t n_recs;      /* 0: the root is a leaf */
    void *prims;          /* device: n_prims records of three float4, in the order the leaves are met */
    uint64_t n_prims;
    void *prim_boxes;     /* device: n_prims x 6 floats, the box each primitive's constructor gives it (min xyz, max xyz) — which the
                           * records no longer say: a triangle keeps its edges, a cone one centre. Made on the first call after an upload. */
    float root_min[3], root_max[3];
    uint32_t root_ref;
    float box_slack;
    uint32_t max_depth;
    uint64_t generation;
} gpuart_hip_scene;
/* Flushes the collected passes and waits for every pass lane and the primary stream — passes requested before the call render the
 * scene as it is now — and fills *out. GPUART_HIP_ERR_ARG without a scene or with out == NULL. */
int gpuart_hip_scene_device(gpuart_hip_ctx *ctx, gpuart_hip_scene *out);
/* Adopts a refit of the arrays in place (the caller has waited for it): the new root box; box_slack by the uploader's own rule, +inf
 * when `subnormal` (some box plane is within 2^-60 of zero without being zero) or quick boxes are off, else the slack of the root's
 * largest plane; and the pass kernels' block order is counted again by the next run. The primitive count, the type mask, the tree
 * order, max_depth and the root ref do not change. GPUART_HIP_ERR_ARG, with nothing changed, without a scene, on a tree the uploader
 * classified irregular or disorderly, and for a root box that is not finite and ordered. */
int gpuart_hip_scene_refitted(gpuart_hip_ctx *ctx, const float root_min[3], const float root_max[3], int subnormal);
/* ---- a rebuild on the device (include/gpuart_build.h; DESIGN.md "Rebuild") ---------------------------------------------------------
 * Hands out a spare set of arrays the context owns — room for n_recs records and for the scene's n_prims primitives and boxes —,
 * allocated on the first call and reused while it is large enough (the records beyond n_recs are zeroed again, as behind an upload's);
 * the next upload frees it. *out: layout 1, the three arrays, n_recs
 * and n_prims = the room, generation = the scene's; everything else zero. Rendering is unaffected: nothing reads the spare set.
 * GPUART_HIP_ERR_ARG without a scene. */
int gpuart_hip_scene_reserve(gpuart_hip_ctx *ctx, uint64_t n_recs, gpuart_hip_scene *out);
/* Adopts a tree built into the spare set (the caller has waited for the build): flushes the collected passes and waits for them — they
 * render the old tree —, then the spare set becomes the scene and the old arrays the spare set. Root box, root_ref, n_recs and max_depth
 * are taken from *built; box_slack by the uploader's rule for that root box, +inf when built->box_slack is +inf (the builder met a
 * subnormal plane) or quick boxes are off; the traversal stacks are sized for the new depth; `generation` grows, so a refit handle
 * bound to the old arrays is stale and says so; the block order is counted again by the next run. The primitive count, the type mask
 * and the tree order stay: primitives keep their types, and their device ordinals are now the built order's.
 * GPUART_HIP_ERR_ARG, with nothing changed, for arrays that are not the reserved ones or were reserved before another upload or
 * rebuild, a changed n_prims, n_recs beyond the room, max_depth > 1024, a root box that is not finite and ordered, a root_ref that is
 * neither 0 with records nor a leaf ref inside n_prims without, a failure to size the traversal stacks, and on a tree
 * the uploader classified irregular or disorderly. */
int gpuart_hip_scene_rebuilt(gpuart_hip_ctx *ctx, const gpuart_hip_scene *built);
/* ---- an edit on the device (include/gpuart_edit.h; DESIGN.md "Edit") ----------------------------------------------------------------
 * gpuart_hip_scene_reserve with room for n_prims >= 1 primitives and boxes instead of the scene's own count: a spare set that is
 * large enough in both counts is reused (*out says its room, which may be more than was asked for), else it is made anew. Beyond the
 * n_recs records and behind the n_prims primitives and boxes the set is zeroed, so what a builder writes there ends as an upload's
 * arrays do. The context remembers the room of the spare set and of the scene's own arrays apart from the counts: after an adoption
 * the former scene arrays are the spare set with their own room, and a later gpuart_hip_scene_reserve, which wants a set of exactly the
 * scene's count, makes a new one where the room differs. GPUART_HIP_ERR_ARG without a scene, for n_prims = 0 or beyond the uploader's
 * bound (0x05555540). */
int gpuart_hip_scene_reserve_prims(gpuart_hip_ctx *ctx, uint64_t n_recs, uint64_t n_prims, gpuart_hip_scene *out);
/* gpuart_hip_scene_rebuilt for a tree of another primitive list: n_prims becomes built->n_prims (1 <= n_prims <= the reserved room) and
 * the type mask, which selects the kernel specialisation, becomes type_mask (bit t: primitives of type t are present; non-zero, at most
 * 15) — the caller vouches for it as for the root box. What follows from the two is computed as an upload computes it: the tree order
 * against the nearest-first threshold, the scene's bytes and node count, the traversal stacks, box_slack; `generation` grows.
 * GPUART_HIP_ERR_ARG, with nothing changed, for everything gpuart_hip_scene_rebuilt refuses but a changed count, for such a type mask
 * and for a count of 0 or beyond the room. */
int gpuart_hip_scene_replaced(gpuart_hip_ctx *ctx, const gpuart_hip_scene *built, uint32_t type_mask);

/* How the fast kernels walk the uploaded tree: 1 (the default for every tree of regular boxes since round 5) in the reference's order —
 * lower child first, shaders/bvh_intersection.glsl:432-441 — which is the only order PROVEN to return the reference's winner; 2 in the
 * reference's order with comparison-form box tests, because a box is irregular or does not bound its contents
 * (gpuart_hip_test_tree_class); 0 nearer child first with a certificate and a second walk where the certificate fails — ~10 % fewer node
 * visits, OPT-IN: gpuart_hip_set_nearest_first(ctx, min_prims) or GPUART_HIP_NEAREST_MIN_PRIMS=min_prims in the environment at
 * gpuart_hip_create (trees of at least min_prims primitives; 0xffffffff: never). Why opt-in: the reference accepts whatever parameter
 * its intersectors compute, and at grazing angles below ~1e-5 rad triangle.glsl:50-76 computes phantom hits far in front of the
 * triangle's own box; a walk that prunes that box after seeing a surface in between never tests the triangle and returns another winner
 * than the reference (tests/golden/order_adversary.npz: 16 constructed scenes, expected values from the reference's GLSL). No image of
 * a 3.7e11-ray soak of the benchmark scenes ever differed — the walk is soak-verified, not proven. */
int gpuart_hip_set_nearest_first(gpuart_hip_ctx *ctx, uint32_t min_prims);
int gpuart_hip_scene_order(gpuart_hip_ctx *ctx, int *order);

/* ---- batched ray queries (no reference counterpart: the reference's CheckBVHIntersection, shaders/bvh_intersection.glsl:405-441, and
 * CheckIntersectionInclUserSphere, shaders/intersection.glsl:71-111, for rays the caller chooses) --------------------------------------
 * Every query walks the uploaded tree in the reference's order — whatever gpuart_hip_set_nearest_first says — and returns the reference's
 * answer bit for bit.
 *   closest hit: pos, point p, normal n and primitive type (0 sphere, 1 disc, 2 triangle, 3 cone) of the reference's closest hit; with a
 *                user sphere (`userSphere` = centre, radius; NULL = none) the user sphere takes part as in the reference. A miss writes
 *                pos = -1, p = n = 0, type = -1.
 *   occlusion (GPUART_HIP_RAYS_OCCLUSION): is 0 < the reference's closest-hit pos < tmax? The walk stops at the first accepted hit below
 *                tmax (exact: DESIGN.md "Batched ray queries"). Occluded: pos and primitive of the hit that ended the walk, p = n = 0, its
 *                type; not occluded: pos = -1, type = -1. tmax = +inf: any hit; tmax <= 0 or NaN: never occluded.
 * `prims` (may be NULL) receives per query the primitive's ordinal — its index among the device primitives, which follow the leaves of
 * the compiled tree in order —, -1 for none, -2 for the user sphere.
 * Queries run on the context's primary stream; collected passes are not flushed (no image depends on a query, no query on a pass);
 * queries change neither gpuart_hip_counters nor gpuart_hip_kernel_time. GPUART_HIP_ERR_ARG without a scene (pick: without a frame size
 * or camera), for NULL or misaligned pointers, a pixel outside the W x H frame or n > GPUART_HIP_MAX_RAYS; n = 0 does nothing. */
typedef struct gpuart_ray_hit {
    float pos, p[3];
    float n[3];
    int32_t type;
} gpuart_ray_hit; /* 32 bytes */
#define GPUART_HIP_RAYS_OCCLUSION 1u
#define GPUART_HIP_MAX_RAYS 0x7fffffffu /* queries per call */
/* Device memory, asynchronous on the context's stream (gpuart_hip_finish before the results are used). rays: n x 8 floats,
 * {origin.xyz, tmax}{dir.xyz, unused} (tmax is read in occlusion mode only); rays and hits 16-byte aligned, prims 4-byte aligned. */
int gpuart_hip_trace_rays(gpuart_hip_ctx *ctx, const float *rays, size_t n, uint32_t flags, const float userSphere[4],
                          gpuart_ray_hit *hits, int32_t *prims);
/* The same in host memory, synchronous (staged through the context's scratch, in chunks of 2^21 queries). */
int gpuart_hip_trace_rays_host(gpuart_hip_ctx *ctx, const float *rays, size_t n, uint32_t flags, const float userSphere[4],
                               gpuart_ray_hit *hits, int32_t *prims);
/* Closest hit of the camera rays of frame pixels xy[2n] = (x, y), row 0 = bottom, any pixel of the W x H frame (not only the
 * context's tile): the ray gpuart_hip_render_direct traces for that pixel. Host memory, synchronous. */
int gpuart_hip_pick(gpuart_hip_ctx *ctx, const uint32_t *xy, size_t n, const float userSphere[4], gpuart_ray_hit *hits,
                    int32_t *prims);
/* The G-buffer of the context's tile: for every tile pixel the record and ordinal that picking that frame pixel returns (the same camera
 * ray, the same user sphere semantics), in the tile's local order as gpuart_hip_read lays it out: record ly * tw + lx is local pixel
 * (lx, ly), row 0 at the bottom, and local row ly is frame row y0 + (ly / band_rows) * band_stride + ly % band_rows (rectangular tiles
 * and interleaved shares alike). Device memory, asynchronous on the context's stream as gpuart_hip_trace_rays: hits (tw*th records)
 * 16-byte aligned, prims (tw*th ordinals, may be NULL) 4-byte aligned. Collected passes are not flushed; counters and timings do not
 * change. An empty share writes nothing. GPUART_HIP_ERR_ARG without a scene, a frame size or a camera, and for a NULL or misaligned
 * pointer. include/gpuart_denoise.h filters a frame with it. */
int gpuart_hip_gbuffer(gpuart_hip_ctx *ctx, const float userSphere[4], gpuart_ray_hit *hits, int32_t *prims);
/* A G-buffer above the pixel grid (include/gpuart_upscale.h upsamples a filtered frame with it): the G-buffer the context would give at
 * the same camera and user sphere if its frame were scale*W x scale*H and its tile (scale*x0, scale*y0, scale*tw, scale*th), bit for bit
 * what gpuart_hip_gbuffer returns on a context resized and tiled that way. Record ly * (scale*tw) + lx is pixel (lx, ly) of the scaled
 * tile, row 0 at the bottom. The camera rays are those of the scaled frame (its own UV plane equations, computed where a resize
 * computes them), walked by the query kernel gpuart_hip_gbuffer launches. Device memory, asynchronous on the context's stream: hits
 * (scale^2 * tw*th records) 16-byte aligned, prims (as many ordinals) 4-byte aligned. The context's frame, tile, accumulators, collected
 * passes, counters and timings do not change; the context keeps the table of the scaled tile's pixels (8 bytes per scaled pixel) until
 * the tile or the scale changes. An empty share writes nothing. GPUART_HIP_ERR_ARG, with nothing written, for scale outside 2..4, without
 * a scene, a frame size or a camera, for a NULL or misaligned pointer, for an interleaved share (more than one band and band_stride !=
 * band_rows: its scaled tile would be no rectangle), for a scaled tile above GPUART_HIP_MAX_RAYS pixels or a scaled frame side above
 * 65536. */
int gpuart_hip_gbuffer_scaled(gpuart_hip_ctx *ctx, uint32_t scale, const float userSphere[4], gpuart_ray_hit *hits, int32_t *prims);
/* Sub-pixel camera rays of listed tile pixels: a G-buffer below the pixel grid (include/gpuart_edges.h resolves geometric edges with
 * it). pixels: device memory, n local pixel indices ly * tw + lx in the order of gpuart_hip_gbuffer, in any order, repeats allowed. uv:
 * host memory, 2 * n_sub values in [0, 1). Ray (i, k) is the first segment gpuart_hip_pt_pass traces for pixel pixels[i] when its two
 * jitter draws are rand1 = uv[2k] and rand2 = uv[2k + 1] (reference shaders/path_tracing.glsl:144-170: rdirOrtho1/2, PixelSize,
 * rdir = rstart - CameraPos), with PixelSize = pixelSize (gpuart_params.pixelSize: the context keeps none between passes) and CameraPos =
 * the pos of gpuart_hip_set_camera. It is answered as gpuart_hip_trace_rays answers a closest-hit query — the reference's order, the
 * user sphere taking part, ordinals -1 / -2 — into hits[k * n + i] and prims[k * n + i] (prims may be NULL): n * n_sub records, device
 * memory, hits 16-byte aligned, pixels and prims 4-byte aligned. A generation pass writes the rays into the context's scratch
 * (32 bytes per ray) and the persistent query kernel walks them (two launches of that kernel), on the context's stream; collected passes are not flushed, counters
 * and timings do not change. The list is range-checked on the device, so the call waits for the generation pass — not for the walk:
 * gpuart_hip_finish before the results are used. GPUART_HIP_ERR_ARG, with nothing written, without a scene, a frame size or a camera,
 * for n_sub outside 1..GPUART_HIP_MAX_SUBPIXEL, a uv outside [0, 1), a pixelSize that is negative or not finite, n * n_sub >
 * GPUART_HIP_MAX_RAYS, NULL or misaligned pointers, or an index >= tw * th; n = 0 does nothing. */
#define GPUART_HIP_MAX_SUBPIXEL 16u
int gpuart_hip_trace_subpixel(gpuart_hip_ctx *ctx, const uint32_t *pixels, size_t n, const float *uv, uint32_t n_sub, float pixelSize,
                              const float userSphere[4], gpuart_ray_hit *hits, int32_t *prims);

/* The test hooks (gpuart_hip_test_*: the run planner, the uploader's verdicts, the share-table check, birth orders, a stream stall, the
 * device functions one by one) are NOT part of this interface: include/gpuart_hip_test.h declares them, and only a library built with
 * -DGPUART_HIP_TEST_HOOKS (gpuart_amd/lib_test/, what the test suite loads) defines them. */

#ifdef __cplusplus
}
#endif
#endif /* GPUART_HIP_H */
