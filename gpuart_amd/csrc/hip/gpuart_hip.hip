// gpuart_hip.hip — context, scheduling and the C-ABI launcher of libgpuart_hip.so (gfx950 only); the kernels live in
// kernels_pipeline.h / kernels_test.h, the tree re-layout in converter.h.
// See include/gpuart_hip.h for the boundary and DESIGN.md for layout / kernel notes.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>
#include <utility>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "device_shade.h"
#include "gpuart_hip.h"
#include "gpuart_hip_test.h"

#include "kernels_pipeline.h"
#include "kernel_run.h"
#include "kernels_query.h"
#ifdef GPUART_HIP_TEST_HOOKS
#include "kernels_test.h"  // kernels of the device-function hooks (include/gpuart_hip_test.h)
#endif
#include "converter.h"
#include "gather.h"
#include "run_planner.h"
#include "bounded.h"

// =================================================================================================
// Host side: context, upload, launches
// =================================================================================================
namespace {

thread_local std::string g_last_error;

// Every pipeline run in flight has its own stream (+ the primary stream). ROCm maps HIP streams onto GPU_MAX_HW_QUEUES
// hardware queues (default 4) and kernels of streams that share a queue serialise, which would undo the overlap
// the pass lanes exist for; ask for more queues unless the user has chosen a value. Must happen before the HIP
// runtime initialises, hence a load-time constructor (bench.py also sets it before importing torch).
// Measured in round 5 (rocprofv3 kernel traces, profiles/r05/planner_even_runs.txt): whatever the value, the streams of a process share
// EIGHT hardware queues on this platform — the primary stream's and seven more, so the eighth pass lane shares one (a stream created
// with a priority gets a queue of its own: tried for the primary stream, nine queues, same times). Sharing by itself costs nothing
// measurable; sequences of seven runs that rotated over eight lanes were 1-3 % slower than on seven, so drain() restarts the rotation.
__attribute__((constructor)) void request_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "32", 0); }

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    bounded_ns::log_error(code, msg);  // (all threads' recent errors: what the phase watchdog prints, bounded.h)
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(GPUART_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// llvmpipe's plane equation of one interpolated attribute over one triangle (DESIGN.md "UV").
void plane_coef(float x0, float y0, float x1, float y1, float x2, float y2, float a0, float a1, float a2, float c[3]) {
    float x0c = x0 - 0.5f, y0c = y0 - 0.5f;
    float dx01 = x0 - x1, dy01 = y0 - y1, dx20 = x2 - x0, dy20 = y2 - y0;
    float e = dx01 * dy20, f = dy01 * dx20;
    float ooa = 1.0f / (e - f);
    float dy20o = dy20 * ooa, dy01o = dy01 * ooa, dx20o = dx20 * ooa, dx01o = dx01 * ooa;
    float da01 = a0 - a1, da20 = a2 - a0;
    float dadx = da01 * dy20o - da20 * dy01o;
    float dady = da20 * dx01o - da01 * dx20o;
    c[0] = a0 - (dadx * x0c + dady * y0c);
    c[1] = dadx;
    c[2] = dady;
}

struct TimedLaunch {
    hipEvent_t start, stop;
    int cls;  ///< 0: a whole render call (direct frame / path-tracing pass), 1: one BVH-query kernel
};

}  // namespace

/// Everything one run of the pipeline (a group of path-tracing passes) needs while it is in flight. Several runs are in
/// flight at once, each on its own stream; their kernels fill each other's tails.
struct PassLane {
    hipStream_t main = nullptr;    ///< every kernel of the run, in order
    PathBuffers pb{};              ///< wavefront path state (passes of the run x tile slots)
    void *pathmem = nullptr;
    float4 *passcolor = nullptr;   ///< colour per pass and pixel, added to the accumulator by k_accumulate
    uint4 *spill_main = nullptr;   ///< traversal-stack overflow of the lane's BVH-query launches
    uint32_t counter_segments = 0; ///< pb.counters holds 4*(counter_segments+1) words
    uint32_t *run_cursor = nullptr;  ///< chunk cursor of the lane's k_run launch
    hipEvent_t ev_done = nullptr;  ///< the run has finished (main stream)
    hipEvent_t ev_free = nullptr;  ///< its colour has been accumulated (primary stream): the lane may be reused
    bool used = false;
};

struct gpuart_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  ///< primary stream: accumulation (in pass order), direct lighting, copies, test hooks
    Frame frame{};
    bool have_camera = false, have_scene = false;
    bool empty_share = false;      ///< gpuart_hip_set_share with th == 0: nothing to render, still a member of the gather
    float4 *d_recs = nullptr, *d_prims = nullptr;
    uint32_t *d_cursor = nullptr;  ///< pixel cursor of k_direct_persistent
    uint32_t *d_query_cursor = nullptr;  ///< chunk cursor of k_ray_query (primary stream, like d_spill)
    uint2 *d_tile_xy = nullptr;    ///< gpuart_hip_gbuffer: the frame pixel of every tile pixel, in local order (freed by realloc_tile, built on use)
    uint2 *d_scaled_xy = nullptr;  ///< gpuart_hip_gbuffer_scaled: the same table of the tile scaled by scaled_xy_scale (freed by realloc_tile, built on use)
    uint32_t scaled_xy_scale = 0;
    uint4 *d_spill = nullptr;      ///< [spill_levels][grid_lanes] traversal-stack overflow for kernels on the primary stream
    // Birth order of the paths of a run (Frame::tile_order, k_tile_order): the tile's 8x8 blocks, most expensive first. The first run
    // after the tile was (re)allocated — and the first after every change of camera or scene — counts the shaded segments per block
    // (`gathers`), a sort behind it writes the buffer that is not in use, and the runs launched once that has finished use it.
    uint32_t *d_tile_order[2] = {nullptr, nullptr};
    uint32_t *d_tile_cost = nullptr;
    hipEvent_t ev_order = nullptr;     ///< the sort into d_tile_order[order_next] has finished
    int order_cur = -1, order_next = 0; ///< buffer in use (-1: none yet, row-major), buffer being written
    bool order_sorting = false;        ///< a gathering run + sort is under way
    bool order_stale = true;           ///< the order in use (or none) was not counted with this camera / scene
    bool order_auto = true;            ///< GPUART_HIP_TILE_ORDER (default 1)
    bool order_from_hook = false;      ///< gpuart_hip_test_tile_order set Frame::tile_order: it stays until the hook clears it
    // Adaptive sampling (gpuart_hip_set_active_blocks): the blocks the passes to come render — Frame::tile_order of every run, which
    // then has 64 x active_n path slots — and the paths accumulated per block. While every pass since the last reset covered every block
    // the host's own count serves (uniform_paths) and the plain k_accumulate runs; the first list makes the device array.
    uint32_t *d_active = nullptr;      ///< the list (room for every block of the tile)
    uint32_t active_n = 0;
    bool have_list = false;
    uint32_t *d_block_paths = nullptr; ///< one word per block (valid while have_counts)
    bool have_counts = false;
    uint32_t uniform_paths = 0;        ///< paths per pixel since the last reset while !have_counts
    std::vector<PassLane> lanes;
    uint32_t next_lane = 0;
    uint32_t spill_levels = 0;
    uint32_t num_cus = 256;
    uint32_t grid_waves = 4096;    ///< persistent grid: one wave per block
    uint32_t direct_waves = 4096;  ///< grid of k_direct_persistent (runs alone: needs the whole occupancy itself)
    uint32_t shade_waves = 4096;   ///< grid of the streaming kernels (k_gen, k_shade): latency-bound, so more waves than k_trace
    uint32_t run_waves = 5120;     ///< grid of k_run: fills every SIMD by itself (5 waves per SIMD)
    TraceTuning tune{128, 16, 16, 3};
    bool lean_kernels = true;      ///< use the BVH-query kernels specialised for the primitive types present
    // passes requested through gpuart_hip_pt_pass but not launched yet (same params, one seed each)
    std::vector<float4> pend_seeds;
    gpuart_params pend_params{};
    int pend_npaths = 0;
    uint64_t n_nodes = 0, n_prims = 0, scene_bytes = 0;
    uint32_t ref_order = 0;       ///< a small tree of regular boxes: the fast kernels keep the reference's order (GD_REF_ORDER variants)
    uint32_t nearest_min_prims = 0xffffffffu;  ///< GPUART_HIP_NEAREST_MIN_PRIMS / gpuart_hip_set_nearest_first: trees with at least this many primitives are
                                                ///< walked nearer child first (OPT-IN since round 5: that walk is not the reference's on phantom hits,
                                                ///< device_scene.h); default: never — every walk keeps the reference's order
    uint32_t type_mask = 0;  ///< bit t set: the scene holds primitives of type t
    float root_min[3] = {0, 0, 0}, root_max[3] = {0, 0, 0};
    uint32_t root_ref = 0;
    bool chunk_from_env = false;  ///< GPUART_HIP_CHUNK was given: no per-launch choice of the chunk size
    float box_slack = __builtin_inff();  ///< box_quick.h's slack constant of the uploaded tree (+inf — also before any upload —: quick box answers are never taken)
    uint32_t quick_boxes = 1;     ///< GPUART_HIP_QUICK_BOXES (0: box_slack stays +inf — every box test runs its six face tests)
    uint32_t packet = 2;          ///< GPUART_HIP_PACKET (default 2): packet walks in k_trace (trav_packet) for 1 — the camera rays, 2 — also the Sun-shadow
                                  ///< rays of segment 0; 0 — none. Trees walked in the reference's order with fast-form boxes only
    uint32_t packet_max_prims = 1u << 19;  ///< GPUART_HIP_PACKET_MAX_PRIMS: ... and with at most this many primitives. The lanes of a packet follow
                                           ///< each other while a pixel block sees few primitives: the 871 200-triangle mesh at 1080p ran 2 % SLOWER
                                           ///< with packets, the 100 352-triangle one 7 % faster (profiles/r07/ab_runs.txt; sizes between: not measured)
    uint32_t gen_walk = 1;        ///< GPUART_HIP_GEN_WALK (default 1): where the camera rays' launch would walk packets and a later k_trace launch follows,
                                  ///< k_gen walks the camera rays it generates and that launch is not made (launch_run); 0 — always the separate launch
    uint32_t gen_shade = 2;       ///< GPUART_HIP_GEN_SHADE (default 2): where k_gen walks and the run has a segment 1, 1 — k_gen also shades segment 0 of the paths it
                                  ///< walked and k_shade(0) is not launched; 2 — and walks their Sun-shadow queries as packets of its own; 0 — the separate launches
    uint32_t shadow_pool = 1;     ///< GPUART_HIP_SHADOW_POOL (default 1): at GPUART_HIP_GEN_SHADE = 2, k_gen pools the Sun-shadow queries of its packets per wave and walks
                                  ///< them 64 at a time (k_gen's `shade` = 3); 0 — each packet walks the shadow lanes of its own 64 slots
    uint32_t pool_chunk = 256;    ///< GPUART_HIP_POOL_CHUNK (default 256): the slots k_gen takes from its cursor at a time where it pools; the pool is emptied at a chunk's end
    uint32_t pool_min_passes = 8; ///< GPUART_HIP_POOL_MIN_PASSES (default 8): ... and it pools only in runs of at least this many passes
    uint32_t block_order = 2;     ///< GPUART_HIP_BLOCK_ORDER (default 2): the order of the 64 path slots of an 8x8 block (Frame::block_order): 0 — row-major, 1 — Z-order,
                                  ///< 2 — Z-order in the runs of the launch pipeline of at least 4 passes (a packet is at most 16 pixels, 4x2 at 8 passes), else row-major
    uint32_t exact_boxes = 0;     ///< the uploaded tree holds an irregular box, or a box that does not bound what it holds (converter.h):
                                  ///< box tests take the comparison form and every walk keeps the reference's order
    uint32_t max_depth = 0;
    // For a refit in place (gpuart_hip_scene_device): the record count, the uploads so far, and every primitive's own box — kept on the
    // host by the upload, moved to the device by the first gpuart_hip_scene_device after it (a context that is never refitted pays no device memory).
    uint64_t n_recs = 0, generation = 0;
    std::vector<float, UninitAlloc<float>> h_prim_boxes;
    float *d_prim_boxes = nullptr;
    // For a rebuild (gpuart_hip_scene_reserve): a spare set of the three arrays, which a rebuild fills and gpuart_hip_scene_rebuilt swaps
    // with the scene's. Freed by the next upload.
    float4 *d_spare_recs = nullptr, *d_spare_prims = nullptr;
    float *d_spare_boxes = nullptr;
    uint64_t spare_recs = 0, spare_prims = 0;  ///< what the spare set holds room for
    uint64_t prims_room = 0;  ///< primitives and boxes the scene's own arrays hold room for: n_prims after an upload, more after an edit that shrank the scene
    float4 *d_direct = nullptr, *d_accum = nullptr;
    unsigned long long *d_counters = nullptr;
    /// Tile size, run lengths, lanes in use, execution mode (gpuart_hip_set_mode: 0 fast — launch pipeline, or k_run for a small
    /// sequence —, 1 reference work + counters (k_run), 2 megakernel, 3 launch pipeline always, 4 fast with counters of the
    /// executed work (k_run), 5 k_run always) and the passes collected but not launched: run_planner.h
    RunPlanner plan;
    std::vector<TimedLaunch> pending, free_events;
    double timed_ms[2] = {0, 0};
    uint64_t timed_launches[2] = {0, 0};
    int timing_level = 1;  ///< 0 none, 1 per render call, 2 also per BVH-query kernel
    float *d_scratch = nullptr;  // test hooks
    size_t scratch_bytes = 0;
    // multi-GPU gather (gather.h)
    ncclComm_t comm = nullptr;
    int comm_rank = 0, comm_nranks = 0;
    bool comm_owned = false;          ///< made by gpuart_hip_comm_init / _init_all (destroyed with the context)
    float4 *d_send = nullptr, *d_stage = nullptr;
    size_t send_pixels = 0, stage_pixels = 0;
    void *d_hello = nullptr;          ///< [1 + nranks] GatherHello: own share + status, then everybody's (ncclAllGather)
    void *h_frame = nullptr;          ///< pinned landing area of gpuart_hip_gather_all_read's read-back (the bounded wait comes after the copy is queued)
    size_t h_frame_bytes = 0;
    void *h_hello = nullptr;          ///< pinned host copy of that table: the exchange's device-to-host copy must be truly asynchronous
                                      ///< (the bounded wait comes AFTER it is queued) and its target must outlive a timed-out call
    uint64_t comm_group = 0;          ///< which communicator this context is a rank of: contexts joined by one _comm_init_all (or one
                                      ///< unique id) share it; gpuart_hip_gather_all refuses ranks of different communicators
    uint32_t gather_timeout_ms = 60000;  ///< GPUART_HIP_GATHER_TIMEOUT_MS: bound on the host-side wait for the peers (0: none)
    bool abandoned = false;           ///< a bounded wait on the primary stream ran out: what is queued there may never complete, so
                                      ///< every later wait of this context (comm_destroy, destroy) is bounded too
#ifdef GPUART_HIP_TEST_HOOKS
    std::vector<const void *> launched;  ///< launch ledger (gpuart_hip_test_launches): host handles of the kernels launched, each once
#endif
};

namespace {

// The launch ledger of the test build: every launch site of a product kernel notes the kernel's host handle on its context
// (gpuart_hip_test_launches names them); in the product build GD_LEDGER is nothing at all.
#ifdef GPUART_HIP_TEST_HOOKS
void ledger_note(gpuart_hip_ctx *c, const void *kernel) {
    if (std::find(c->launched.begin(), c->launched.end(), kernel) == c->launched.end()) c->launched.push_back(kernel);
}
#define GD_LEDGER(c, ...) ledger_note((c), reinterpret_cast<const void *>(&__VA_ARGS__))
#else
#define GD_LEDGER(c, ...) ((void)0)
#endif

// ---- the kernel choice ----------------------------------------------------------------------------------------------------------
// k_direct_persistent, k_run, k_trace and k_ray_query are compiled once per tree class. `kernel_choice` is the one statement of which
// instantiation a launch runs (pure host code: gpuart_hip_test_kernel_choice), `with_types` the one place that makes it a template argument.
enum { KC_DIRECT = 0, KC_RUN = 1, KC_TRACE = 2, KC_QUERY = 3 };  ///< the launch sites that choose
enum { KC_COUNT = 0x100, KC_REFWORK = 0x200 };                  ///< beside k_run's TYPES: its COUNT and REFWORK

/// The rule. A tree with exact boxes takes the comparison-form kernel with every type. Otherwise the lean kernels (GPUART_HIP_LEAN_KERNELS)
/// serve trees of flat (discs, triangles) or round (spheres, discs) primitives only, and the path tracer's kernels carry GD_REF_ORDER while
/// the tree is walked in the reference's order; k_direct_persistent and k_ray_query have no such variant. k_run in mode 1 does the
/// reference's work with its counters: every type, never the order bit. In mode 4 it counts the executed work: a flat but no round variant.
int kernel_choice(uint32_t type_mask, bool exact_boxes, bool ref_order, bool lean_kernels, int mode, int entry) {
    const int run = entry != KC_RUN ? 0 : mode == 1 ? KC_COUNT | KC_REFWORK : mode == 4 ? KC_COUNT : 0;
    if (exact_boxes) return run | GD_ALL_TYPES | GD_EXACT_BOXES;
    if (run & KC_REFWORK) return run | GD_ALL_TYPES;
    const bool flat = lean_kernels && (type_mask & ~(uint32_t)GD_FLAT_TYPES) == 0;            // triangle meshes + discs
    const bool round = lean_kernels && (type_mask & ~(uint32_t)GD_ROUND_TYPES) == 0 && !run;  // spheres + discs
    const int types = flat ? GD_FLAT_TYPES : round ? GD_ROUND_TYPES : GD_ALL_TYPES;
    return run | types | (ref_order && (entry == KC_RUN || entry == KC_TRACE) ? GD_REF_ORDER : 0);
}
int kernel_choice(const gpuart_hip_ctx *c, int entry) {
    return kernel_choice(c->type_mask, c->exact_boxes != 0, c->ref_order != 0, c->lean_kernels, c->plan.mode, entry);
}

/// The instantiations that exist, per kernel: the dispatcher makes no other (tests/test_kernel_variants.py holds the code object to them).
template <int... T> using TypeList = std::integer_sequence<int, T...>;
using LeafTypes = TypeList<GD_FLAT_TYPES, GD_ROUND_TYPES, GD_ALL_TYPES, GD_ALL_TYPES | GD_EXACT_BOXES>;  // k_direct_persistent, k_ray_query x 2 sources
using TraceTypes = TypeList<GD_FLAT_TYPES, GD_ROUND_TYPES, GD_ALL_TYPES, GD_ALL_TYPES | GD_EXACT_BOXES, GD_FLAT_TYPES | GD_REF_ORDER,
                            GD_ROUND_TYPES | GD_REF_ORDER, GD_ALL_TYPES | GD_REF_ORDER>;                  // k_trace<false, .>
using RunTypes = TypeList<GD_FLAT_TYPES, GD_ROUND_TYPES, GD_ALL_TYPES, GD_ALL_TYPES | GD_EXACT_BOXES, GD_FLAT_TYPES | GD_REF_ORDER,
                          GD_ROUND_TYPES | GD_REF_ORDER, GD_ALL_TYPES | GD_REF_ORDER, KC_COUNT | GD_FLAT_TYPES, KC_COUNT | GD_ALL_TYPES,
                          KC_COUNT | GD_ALL_TYPES | GD_EXACT_BOXES, KC_COUNT | GD_FLAT_TYPES | GD_REF_ORDER, KC_COUNT | GD_ALL_TYPES | GD_REF_ORDER,
                          KC_COUNT | KC_REFWORK | GD_ALL_TYPES, KC_COUNT | KC_REFWORK | GD_ALL_TYPES | GD_EXACT_BOXES>;  // k_run

/// The dispatcher: `launch(std::integral_constant<int, T>)` for the T of the kernel's list that equals `choice`; an error for any other.
template <int... T, class Launch>
int with_types(int choice, TypeList<T...>, const char *kernel, Launch launch) {
    if (((choice == T && (launch(std::integral_constant<int, T>()), true)) || ...)) return 0;
    return fail(GPUART_HIP_ERR_DEVICE, std::string("internal: no ") + kernel + " for choice " + std::to_string(choice));
}

/// Waits for everything this context has enqueued, on all of its streams.
int drain(gpuart_hip_ctx *c) {
    for (auto &l : c->lanes) {
        if (l.main) HIP_TRY(hipStreamSynchronize(l.main));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->next_lane = 0;  // every lane is idle: the next sequence starts on the first one again (a plan of seven runs stays off the eighth lane, see above)
    return 0;
}


/// Waits for the context's primary stream, but not for ever: a peer that never arrives must not hang this process.
int wait_stream(gpuart_hip_ctx *c, uint32_t timeout_ms, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(c->stream);
        if (e == hipSuccess) { c->abandoned = false; return 0; }
        if (e != hipErrorNotReady) return fail(GPUART_HIP_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
        if (timeout_ms && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms)) {
            c->abandoned = true;  // what is queued on the stream may never complete: later waits of this context stay bounded (destroy included)
            return fail(GPUART_HIP_ERR_TIMEOUT, std::string(what) + ": not complete after " + std::to_string(timeout_ms) +
                        " ms (rank " + std::to_string(c->comm_rank) + " of " + std::to_string(c->comm_nranks) + "; a peer has not joined the collective)");
        }
        // (a gather's waits sit inside bench.py's timed region, where a rank's whole job is ~3 ms at N = 8: the first few milliseconds are
        //  polled without sleeping — a sleep of 50 us returns after 100-150 —, a wait that lasts longer is not in a hurry)
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(5)) std::this_thread::sleep_for(std::chrono::microseconds(50));
        else std::this_thread::yield();
    }
}
}  // namespace
extern "C" int gpuart_hip_flush(gpuart_hip_ctx *c);
namespace {

int realloc_tile(gpuart_hip_ctx *c) {
    int r = gpuart_hip_flush(c);
    if (r) return r;
    if ((r = drain(c))) return r;
    c->empty_share = false;
    for (auto &o : c->d_tile_order) if (o) { (void)hipFree(o); o = nullptr; }
    if (c->d_tile_cost) { (void)hipFree(c->d_tile_cost); c->d_tile_cost = nullptr; }
    c->frame.tile_order = nullptr; c->frame.tile_cost = nullptr;
    c->order_cur = -1; c->order_sorting = false; c->order_stale = true; c->order_from_hook = false;
    if (c->d_active) { (void)hipFree(c->d_active); c->d_active = nullptr; }
    if (c->d_block_paths) { (void)hipFree(c->d_block_paths); c->d_block_paths = nullptr; }
    c->have_list = false; c->active_n = 0; c->have_counts = false; c->uniform_paths = 0;
    if (c->d_tile_xy) { (void)hipFree(c->d_tile_xy); c->d_tile_xy = nullptr; }
    if (c->d_scaled_xy) { (void)hipFree(c->d_scaled_xy); c->d_scaled_xy = nullptr; c->scaled_xy_scale = 0; }
    if (c->d_direct) { (void)hipFree(c->d_direct); c->d_direct = nullptr; }
    if (c->d_accum) { (void)hipFree(c->d_accum); c->d_accum = nullptr; }
    c->plan.tile_pixels = (size_t)c->frame.tw * c->frame.th;
    if (!c->plan.tile_pixels) { c->plan.set_tile(0, 0); return 0; }
    HIP_TRY(hipMalloc(&c->d_direct, c->plan.tile_pixels * sizeof(float4)));
    HIP_TRY(hipMalloc(&c->d_accum, c->plan.tile_pixels * sizeof(float4)));
    HIP_TRY(hipMemsetAsync(c->d_direct, 0, c->plan.tile_pixels * sizeof(float4), c->stream));
    HIP_TRY(hipMemsetAsync(c->d_accum, 0, c->plan.tile_pixels * sizeof(float4), c->stream));
    // wavefront path state: one slot per pixel of the 8x8-tile-padded tile, per pass in flight
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    const size_t n = tiles * 64;
    if (n > 0xfffffff0ull) return fail(GPUART_HIP_ERR_ARG, "tile too large");
    // Several passes run through the pipeline together (slot = pass x pixel) while that stays within `batch_paths`
    // paths: a persistent k_trace wave then takes many rays per lane, and the drain at the end of every launch — waves
    // finishing their last, long rays with few lanes busy — shrinks relative to the useful work (SQ_INSTS_VALU per
    // ray falls by a quarter from 2M to 16M paths per launch at 1080p). run_planner.h decides how many.
    if (n * std::max<size_t>(1, std::min<size_t>(c->plan.batch_limit, c->plan.batch_paths / n)) > 0x7fffffc0ull)
        return fail(GPUART_HIP_ERR_ARG, "tile too large");  // two queues share one 32-bit index space in k_trace (the second from a multiple of 64 on)
    for (auto &l : c->lanes) {
        if (l.pathmem) { (void)hipFree(l.pathmem); l.pathmem = nullptr; }
        l.used = false;
    }
    c->next_lane = 0;
    c->pend_seeds.clear();
    c->plan.set_tile((uint32_t)n, c->plan.tile_pixels);
    // Lanes within the memory budget; when the device cannot give that much (other tenants), fewer lanes and then
    // smaller runs are tried before giving up — results do not depend on either.
    for (;;) {
        const size_t bytes = c->plan.lane_bytes(c->plan.max_batch);
        size_t got = 0;
        while (got < c->plan.lanes_in_use && hipMalloc(&c->lanes[got].pathmem, bytes) == hipSuccess) got++;
        if (got == c->plan.lanes_in_use) break;
        (void)hipGetLastError();  // clear the out-of-memory error
        for (size_t li = 0; li < got; li++) { (void)hipFree(c->lanes[li].pathmem); c->lanes[li].pathmem = nullptr; }
        if (!c->plan.shrink()) return fail(GPUART_HIP_ERR_DEVICE, "out of device memory for the path state of one pass");
    }
    const size_t B = c->plan.max_batch, lanes = c->plan.lanes_in_use;
    for (size_t li = 0; li < lanes; li++) {
        PassLane &l = c->lanes[li];
        char *m = (char *)l.pathmem;
        PathBuffers &b = l.pb;
        const size_t nb = n * B;
        b.ray_o = (float4 *)m; m += nb * sizeof(float4);
        b.ray_d = (float4 *)m; m += nb * sizeof(float4);
        b.cw = (float4 *)m; m += nb * sizeof(float4);
        b.pc = (float4 *)m; m += nb * sizeof(float4);
        b.sun = (float4 *)m; m += nb * sizeof(float4);
        b.color = (float4 *)m; m += nb * sizeof(float4);
        l.passcolor = (float4 *)m; m += B * c->plan.tile_pixels * sizeof(float4);
        b.hit = (uint2 *)m; m += nb * sizeof(uint2);
        b.queue[0] = (uint32_t *)m; m += nb * sizeof(uint32_t);
        b.queue[1] = (uint32_t *)m; m += nb * sizeof(uint32_t);
        b.shadow_queue = (uint32_t *)m;
        b.n_slots = (uint32_t)n;
        b.batch = 1;
        b.tile_pixels = (uint32_t)c->plan.tile_pixels;
    }
    return 0;
}

int ensure_segment_counters(gpuart_hip_ctx *c, PassLane &l, uint32_t nseg) {
    if (l.pb.counters && l.counter_segments >= nseg) return 0;
    if (l.pb.counters) { int r = drain(c); if (r) return r; (void)hipFree(l.pb.counters); l.pb.counters = nullptr; }
    HIP_TRY(hipMalloc(&l.pb.counters, 20 * ((size_t)nseg + 1) * sizeof(uint32_t)));  // 4 words per segment + 16 per-XCD cursors (experiment)
    l.pb.xcd_cursors = l.pb.counters + 4 * ((size_t)nseg + 1);
    l.counter_segments = nseg;
    return 0;
}

int ensure_spill(gpuart_hip_ctx *c) {
    const uint32_t levels = c->max_depth > GD_RING ? c->max_depth - GD_RING : 0;
    if (c->d_spill && c->spill_levels >= levels) return 0;
    int r = drain(c);
    if (r) return r;
    const size_t bytes = ((size_t)levels + 1) * std::max({c->grid_waves, c->direct_waves, c->run_waves}) * BLOCK * sizeof(uint4);
    if (c->d_spill) { (void)hipFree(c->d_spill); c->d_spill = nullptr; }
    HIP_TRY(hipMalloc(&c->d_spill, bytes));
    for (auto &l : c->lanes) {
        if (l.spill_main) { (void)hipFree(l.spill_main); l.spill_main = nullptr; }
        HIP_TRY(hipMalloc(&l.spill_main, bytes));
    }
    c->spill_levels = levels;
    return 0;
}

/// The UV plane equations of a frame of f.W x f.H pixels: the one statement of them, for the context's frame at a resize and for the
/// scaled frame of gpuart_hip_gbuffer_scaled.
void update_uv(Frame &f) {
    float w = (float)f.W, h = (float)f.H;
    float *k = f.uv_coef;
    plane_coef(w, 0, 0, 0, w, h, 1, 0, 1, k + 0);  // A.u (V1,V0,V2)
    plane_coef(w, 0, 0, 0, w, h, 0, 0, 1, k + 3);  // A.v
    plane_coef(w, h, 0, 0, 0, h, 1, 0, 0, k + 6);  // B.u (V2,V0,V3)
    plane_coef(w, h, 0, 0, 0, h, 1, 0, 1, k + 9);  // B.v
}

/// box_quick.h's slack constant for a converted tree: its margins are sized by the largest plane coordinate of the tree — the root's,
/// since every box was checked to lie inside its parent's — and its lemmas want planes that are normal numbers or zero. +inf (no quick
/// box answers) for a tree with irregular or non-bounding boxes or a subnormal plane.
float slack_of_root(bool unfit, const float bmin[3], const float bmax[3]) {
    if (unfit) return __builtin_inff();
    float pmax = 0;
    for (int k = 0; k < 3; k++) pmax = std::max(pmax, std::max(std::fabs(bmin[k]), std::fabs(bmax[k])));
    return gq_slack_of_tree(pmax);
}
float tree_slack(const Converter &cv, const Converter::Child &root) {
    return slack_of_root(cv.irregular || cv.disorderly || cv.subnormal, root.bmin, root.bmax);
}

void drop_spare(gpuart_hip_ctx *c) {
    void *ptrs[] = {c->d_spare_recs, c->d_spare_prims, c->d_spare_boxes};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    c->d_spare_recs = c->d_spare_prims = nullptr;
    c->d_spare_boxes = nullptr;
    c->spare_recs = c->spare_prims = 0;
}

Scene scene_of(const gpuart_hip_ctx *c) {
    Scene s;
    s.recs = c->d_recs;
    memcpy(s.root_min, c->root_min, 12); memcpy(s.root_max, c->root_max, 12);
    s.root_ref = c->root_ref;
    s.exact_boxes = c->exact_boxes;
    s.box_slack = c->box_slack;
    s.prims = c->d_prims;
    return s;
}


int fold_timings(gpuart_hip_ctx *c) {
    for (auto &t : c->pending) {
        HIP_TRY(hipEventSynchronize(t.stop));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, t.start, t.stop));
        c->timed_ms[t.cls] += ms;
        c->timed_launches[t.cls]++;
        c->free_events.push_back(t);
    }
    c->pending.clear();
    return 0;
}

int begin_timed(gpuart_hip_ctx *c, TimedLaunch &t, int cls, hipStream_t stream = nullptr) {
    if (!stream) stream = c->stream;
    t.cls = cls;
    t.start = t.stop = nullptr;
    if (c->timing_level < 1) return 0;
    if (c->pending.size() >= 4096) { int r = fold_timings(c); if (r) return r; }
    if (!c->free_events.empty()) { t = c->free_events.back(); c->free_events.pop_back(); t.cls = cls; }
    else { HIP_TRY(hipEventCreate(&t.start)); HIP_TRY(hipEventCreate(&t.stop)); }
    HIP_TRY(hipEventRecord(t.start, stream));
    return 0;
}
int end_timed(gpuart_hip_ctx *c, TimedLaunch &t, hipStream_t stream = nullptr) {
    if (!t.start) return 0;
    if (!stream) stream = c->stream;
    HIP_TRY(hipEventRecord(t.stop, stream));
    c->pending.push_back(t);
    return 0;
}

template <class T, class A>
int upload_vec(gpuart_hip_ctx *c, T *&dst, const std::vector<T, A> &v) {
    if (dst) { (void)hipFree(dst); dst = nullptr; }
    size_t bytes = (v.size() + 4) * sizeof(T);  // a little slack past the end
    HIP_TRY(hipMalloc(&dst, bytes));
    HIP_TRY(hipMemsetAsync(dst, 0, bytes, c->stream));
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int ensure_scratch(gpuart_hip_ctx *c, size_t bytes) {
    if (c->scratch_bytes >= bytes) return 0;
    if (c->d_scratch) (void)hipFree(c->d_scratch);
    c->d_scratch = nullptr;
    c->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&c->d_scratch, bytes));
    c->scratch_bytes = bytes;
    return 0;
}

/// Runs a test kernel: copies `nin` (n x 4 float) inputs up, launches, copies `nout` outputs back.
template <class Launch>
int run_hook(gpuart_hip_ctx *c, int n, const float *const *ins, int nin, float *const *outs, int nout, Launch launch) {
    if (!c || n < 0) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    size_t one = (size_t)n * 16;
    int r = ensure_scratch(c, one * (nin + nout));
    if (r) return r;
    float4 *base = (float4 *)c->d_scratch;
    std::vector<float4 *> di, dout;
    for (int k = 0; k < nin; k++) {
        di.push_back(base + (size_t)k * n);
        HIP_TRY(hipMemcpyAsync(di[k], ins[k], one, hipMemcpyHostToDevice, c->stream));
    }
    for (int k = 0; k < nout; k++) dout.push_back(base + (size_t)(nin + k) * n);
    launch(di, dout);
    HIP_TRY(hipGetLastError());
    for (int k = 0; k < nout; k++) HIP_TRY(hipMemcpyAsync(outs[k], dout[k], one, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_hip_last_error(void) { return g_last_error.c_str(); }

int gpuart_hip_destroy(gpuart_hip_ctx *c);
static int comm_drop(gpuart_hip_ctx *c);

int gpuart_hip_create(int device, gpuart_hip_ctx **out) {
    if (!out) return fail(GPUART_HIP_ERR_ARG, "out == NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(GPUART_HIP_ERR_NO_DEVICE, "no HIP device");
    if (device < 0 || device >= count) return fail(GPUART_HIP_ERR_ARG, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GPUART_HIP_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    gpuart_hip_ctx *c = new (std::nothrow) gpuart_hip_ctx();
    if (!c) return fail(GPUART_HIP_ERR_DEVICE, "out of host memory");
    c->device = device;
    auto env_u32 = [](const char *name, uint32_t dflt, uint32_t lo, uint32_t hi) {
        const char *v = getenv(name);
        if (!v) return dflt;
        long x = strtol(v, nullptr, 10);
        return (uint32_t)std::min<long>(hi, std::max<long>(lo, x));
    };
    c->num_cus = prop.multiProcessorCount > 0 ? (uint32_t)prop.multiProcessorCount : 256u;
    c->grid_waves = c->num_cus * env_u32("GPUART_HIP_WAVES_PER_CU", 8, 1, 32);  // persistent grids of one-wave workgroups
    c->direct_waves = c->num_cus * env_u32("GPUART_HIP_DIRECT_WAVES_PER_CU", 16, 1, 32);
    c->shade_waves = c->num_cus * env_u32("GPUART_HIP_SHADE_WAVES_PER_CU", 24, 1, 64);
    c->run_waves = c->num_cus * env_u32("GPUART_HIP_RUN_WAVES_PER_CU", 4 * GD_RUN_WAVES, 1, 32);
    c->tune.chunk = env_u32("GPUART_HIP_CHUNK", 128, 16, 4096);
    c->chunk_from_env = getenv("GPUART_HIP_CHUNK") != nullptr;
    c->tune.refill_lanes = env_u32("GPUART_HIP_REFILL_LANES", 16, 1, 64);
    c->tune.leaf_lanes = env_u32("GPUART_HIP_LEAF_LANES", 16, 1, 64);
    c->tune.leaf_share = env_u32("GPUART_HIP_LEAF_SHARE", 3, 1, 64);
    c->tune.xcd_queues = env_u32("GPUART_HIP_XCD_QUEUES", 0, 0, 1);
    c->order_auto = env_u32("GPUART_HIP_TILE_ORDER", 1, 0, 1) != 0;
    c->nearest_min_prims = getenv("GPUART_HIP_NEAREST_MIN_PRIMS") ? env_u32("GPUART_HIP_NEAREST_MIN_PRIMS", 1024, 0, 0x7fffffff) : 0xffffffffu;
    c->quick_boxes = env_u32("GPUART_HIP_QUICK_BOXES", 1, 0, 1);
    c->packet = env_u32("GPUART_HIP_PACKET", 2, 0, 2);
    c->packet_max_prims = env_u32("GPUART_HIP_PACKET_MAX_PRIMS", 1u << 19, 0, 0xffffffffu);
    c->gen_walk = env_u32("GPUART_HIP_GEN_WALK", 1, 0, 1);
    c->gen_shade = env_u32("GPUART_HIP_GEN_SHADE", 2, 0, 2);
    c->shadow_pool = env_u32("GPUART_HIP_SHADOW_POOL", 1, 0, 1);
    c->pool_chunk = env_u32("GPUART_HIP_POOL_CHUNK", 256, 16, 4096);
    c->pool_min_passes = env_u32("GPUART_HIP_POOL_MIN_PASSES", 8, 1, MAX_BATCH);
    c->block_order = env_u32("GPUART_HIP_BLOCK_ORDER", 2, 0, 2);
    c->frame.block_order = c->block_order == 1 ? 1u : 0u;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return fail(GPUART_HIP_ERR_DEVICE, "hipStreamCreate failed"); }
    c->lanes.resize(env_u32("GPUART_HIP_PASSES_IN_FLIGHT", 8, 1, 32));
    c->plan.lanes_total = (uint32_t)c->lanes.size();
    c->plan.batch_limit = env_u32("GPUART_HIP_MAX_BATCH", MAX_BATCH, 1, MAX_BATCH);
    c->plan.batch_paths = (size_t)env_u32("GPUART_HIP_BATCH_MPATHS", 16, 1, 256) << 20;
    c->plan.plan_run_factor = env_u32("GPUART_HIP_PLAN_RUN_PERCENT", 0, 0, 1000) / 100.0;  // 0: as many equal runs as lanes (run_planner.h)
    c->lean_kernels = env_u32("GPUART_HIP_LEAN_KERNELS", 1, 0, 1) != 0;
    c->plan.min_run_paths = (size_t)env_u32("GPUART_HIP_MIN_RUN_KPATHS", 2048, 64, 65536) << 10;
    c->plan.lane_budget = (size_t)env_u32("GPUART_HIP_LANE_BUDGET_MB", 32768, 64, 262144) << 20;
    c->plan.small_paths = (size_t)env_u32("GPUART_HIP_SMALL_KPATHS", 8500, 0, 1 << 20) << 10;
    c->gather_timeout_ms = env_u32("GPUART_HIP_GATHER_TIMEOUT_MS", 60000, 0, 3600000);
    for (auto &l : c->lanes) {
        if (hipStreamCreateWithFlags(&l.main, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&l.ev_done, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&l.ev_free, hipEventDisableTiming) != hipSuccess) {
            gpuart_hip_destroy(c);
            return fail(GPUART_HIP_ERR_DEVICE, "stream / event creation failed");
        }
    }
    if (hipMalloc(&c->d_counters, 16 * sizeof(unsigned long long)) != hipSuccess ||
        hipMemsetAsync(c->d_counters, 0, 16 * sizeof(unsigned long long), c->stream) != hipSuccess) {
        (void)hipStreamDestroy(c->stream); delete c; return fail(GPUART_HIP_ERR_DEVICE, "counter allocation failed");
    }
    *out = c;
    return 0;
}

int gpuart_hip_destroy(gpuart_hip_ctx *c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    c->pend_seeds.clear();
    if (c->abandoned || bounded_ns::stuck().load()) {
        // the primary stream may hold transfers whose peer never came: one more bounded look, then the context is LEAKED rather
        // than waited for (its memory goes with the process)
        if (wait_stream(c, std::min<uint32_t>(c->gather_timeout_ms ? c->gather_timeout_ms : 2000u, 2000u), "gpuart_hip_destroy"))
            return fail(GPUART_HIP_ERR_TIMEOUT, "gpuart_hip_destroy: the context's stream never drained (a gather was abandoned); the context is leaked, not freed");
        c->abandoned = false;
    }
    (void)drain(c);
    for (auto &t : c->pending) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (auto &t : c->free_events) { (void)hipEventDestroy(t.start); (void)hipEventDestroy(t.stop); }
    for (auto &l : c->lanes) {
        if (l.ev_done) (void)hipEventDestroy(l.ev_done);
        if (l.ev_free) (void)hipEventDestroy(l.ev_free);
        void *lp[] = {l.pathmem, l.spill_main, l.pb.counters, l.run_cursor};
        for (void *p : lp) if (p) (void)hipFree(p);
        if (l.main) (void)hipStreamDestroy(l.main);
    }
    // A communicator call that never returned (bounded.h) may still be using the communicator and the buffers it was given:
    // they are left alone, and so is the communicator (the process is about to end; nothing is waited for a second time).
    const bool comm_stuck = bounded_ns::stuck().load();
    if (c->comm && !comm_stuck) (void)comm_drop(c);
    void *ptrs[] = {c->d_recs, c->d_prims, c->d_spill, c->d_direct, c->d_accum, c->d_counters, c->d_scratch, c->d_cursor,
                    c->d_query_cursor, c->d_tile_order[0], c->d_tile_order[1], c->d_tile_cost, c->d_tile_xy, c->d_scaled_xy, c->d_active, c->d_block_paths,
                    c->d_prim_boxes, c->d_spare_recs, c->d_spare_prims, c->d_spare_boxes};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    void *comm_ptrs[] = {c->d_send, c->d_stage, c->d_hello};
    for (void *p : comm_ptrs) if (p && !comm_stuck) (void)hipFree(p);
    if (c->ev_order) (void)hipEventDestroy(c->ev_order);
    if (c->h_hello && !comm_stuck) (void)hipHostFree(c->h_hello);  // (after drain: no copy into it is queued any more)
    if (c->h_frame && !comm_stuck) (void)hipHostFree(c->h_frame);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int gpuart_hip_resize(gpuart_hip_ctx *c, uint32_t width, uint32_t height) {
    if (!c || width == 0 || height == 0 || width > 65536 || height > 65536) return fail(GPUART_HIP_ERR_ARG, "bad frame size");
    HIP_TRY(hipSetDevice(c->device));
    c->frame.W = width; c->frame.H = height;
    c->frame.x0 = 0; c->frame.y0 = 0; c->frame.tw = width; c->frame.th = height;
    c->frame.band_rows = height; c->frame.band_stride = height;
    update_uv(c->frame);
    return realloc_tile(c);
}

int gpuart_hip_set_tile(gpuart_hip_ctx *c, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th) {
    if (!c || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "set_tile before resize");
    if (tw == 0 || th == 0 || (uint64_t)x0 + tw > c->frame.W || (uint64_t)y0 + th > c->frame.H)
        return fail(GPUART_HIP_ERR_ARG, "tile outside the frame");
    HIP_TRY(hipSetDevice(c->device));
    c->frame.x0 = x0; c->frame.y0 = y0; c->frame.tw = tw; c->frame.th = th;
    c->frame.band_rows = th; c->frame.band_stride = th;
    return realloc_tile(c);
}

int gpuart_hip_set_tile_interleaved(gpuart_hip_ctx *c, uint32_t x0, uint32_t y0, uint32_t tw, uint32_t th_local,
                                    uint32_t band_rows, uint32_t band_stride) {
    if (!c || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "set_tile before resize");
    if (tw == 0 || th_local == 0 || band_rows == 0 || band_stride < band_rows || (uint64_t)x0 + tw > c->frame.W)
        return fail(GPUART_HIP_ERR_ARG, "bad interleaved tile");
    // the last local row must still lie inside the frame
    const uint64_t last = (uint64_t)y0 + (uint64_t)((th_local - 1) / band_rows) * band_stride + (th_local - 1) % band_rows;
    if (last >= c->frame.H) return fail(GPUART_HIP_ERR_ARG, "interleaved tile outside the frame");
    HIP_TRY(hipSetDevice(c->device));
    c->frame.x0 = x0; c->frame.y0 = y0; c->frame.tw = tw; c->frame.th = th_local;
    c->frame.band_rows = band_rows; c->frame.band_stride = band_stride;
    return realloc_tile(c);
}

int gpuart_hip_upload_bvh(gpuart_hip_ctx *c, const float *quads, size_t nquads) {
    if (!c || !quads || nquads < 3 || nquads > (1ull << 29)) return fail(GPUART_HIP_ERR_ARG, "bad tree");
    HIP_TRY(hipSetDevice(c->device));
    Converter cv;
    cv.q = quads; cv.nq = nquads;
    if (const char *e = getenv("GPUART_HIP_TOP_DEPTH")) cv.top_depth = (uint32_t)atoi(e);
    Converter::Child root;
    unsigned upload_threads = nquads >= (1u << 20) ? 8u : 1u;  // the fill pass of a big tree on several threads (disjoint writes)
    if (const char *e = getenv("GPUART_HIP_UPLOAD_THREADS")) upload_threads = (unsigned)std::min(64, std::max(1, atoi(e)));
    if (!cv.convert(root, upload_threads))
        return fail(GPUART_HIP_ERR_ARG, "malformed compiled BVH: " + cv.err);
    int r;
    if ((r = gpuart_hip_flush(c))) return r;
    if ((r = drain(c))) return r;
    if ((r = upload_vec(c, c->d_recs, cv.recs))) return r;
    if ((r = upload_vec(c, c->d_prims, cv.prims))) return r;
    memcpy(c->root_min, root.bmin, 12); memcpy(c->root_max, root.bmax, 12);
    c->root_ref = root.ref;
    c->exact_boxes = (cv.irregular || cv.disorderly) ? 1u : 0u;
    c->box_slack = c->quick_boxes ? tree_slack(cv, root) : __builtin_inff();
    c->type_mask = cv.type_mask;
    c->n_nodes = cv.num_nodes;
    c->n_prims = cv.prims.size() / 3;
    c->prims_room = c->n_prims;
    c->ref_order = (!c->exact_boxes && c->n_prims < c->nearest_min_prims) ? 1u : 0u;
    c->max_depth = cv.max_depth;
    c->scene_bytes = cv.recs.size() * 16 + cv.prims.size() * 16;
    c->n_recs = cv.recs.size() / 4;
    c->generation++;
    if (c->d_prim_boxes) { (void)hipFree(c->d_prim_boxes); c->d_prim_boxes = nullptr; }
    c->h_prim_boxes.swap(cv.pbox);
    drop_spare(c);
    if ((r = ensure_spill(c))) return r;
    c->have_scene = true;
    c->order_stale = true;
    return 0;
}

int gpuart_hip_set_camera(gpuart_hip_ctx *c, const float pos[3], const float bl[3], const float dh[3], const float dv[3]) {
    if (!c || !pos || !bl || !dh || !dv) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }  // batched passes were requested with the old camera
    c->order_stale = true;  // the blocks' cost is counted again by the next run (run_frame)
    memcpy(c->frame.cam_pos, pos, 12); memcpy(c->frame.bottom_left, bl, 12);
    memcpy(c->frame.delta_horz, dh, 12); memcpy(c->frame.delta_vert, dv, 12);
    c->have_camera = true;
    return 0;
}

static int check_ready(gpuart_hip_ctx *c, const gpuart_params *p) {
    if (!c || !p) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    if (c->empty_share) return 1;  // nothing to render (the callers return success)
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (!c->have_camera) return fail(GPUART_HIP_ERR_ARG, "no camera set");
    if (!c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
    return 0;
}

/// The chunks of a launch of `n` entries through the persistent-lane loop (k_direct_persistent, k_ray_query): its tail is the last chunk a
/// wave takes from the cursor (128 pixels are two rounds of two dependent queries). Small launches take 64-entry chunks — a 1080p frame
/// 0.92 -> 0.75 ms; 4K stays at 128 (1.74 against 1.85): fewer cursor atomics, longer coherent runs (32 and 16 are far worse: 1.0 / 1.7 ms).
static TraceTuning direct_tuning(const gpuart_hip_ctx *c, size_t n) {
    TraceTuning tune = c->tune;
    if (!c->chunk_from_env && n / ((size_t)c->direct_waves * 8) < 128) tune.chunk = 64;
    return tune;
}

int gpuart_hip_render_direct(gpuart_hip_ctx *c, const gpuart_params *p) {
    int r = check_ready(c, p);
    if (r) return r > 0 ? 0 : r;
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    HIP_TRY(hipSetDevice(c->device));
    dim3 grid(std::min<uint32_t>(c->grid_waves, c->plan.n_slots / BLOCK));
    Scene sc = scene_of(c);
    TimedLaunch t;
    if ((r = begin_timed(c, t, 0))) return r;
    if (c->plan.mode == 1) {
        GD_LEDGER(c, k_direct<true>);
        k_direct<true><<<grid, BLOCK, 0, c->stream>>>(sc, c->frame, *p, c->plan.n_slots, c->d_direct, c->d_spill, c->d_counters);
    } else if (c->plan.mode == 2) {
        GD_LEDGER(c, k_direct<false>);
        k_direct<false><<<grid, BLOCK, 0, c->stream>>>(sc, c->frame, *p, c->plan.n_slots, c->d_direct, c->d_spill, c->d_counters);
    } else {
        // fast mode: persistent lanes, one pixel at a time per lane (kernels_pipeline.h)
        if (!c->d_cursor) HIP_TRY(hipMalloc(&c->d_cursor, 64));
        HIP_TRY(hipMemsetAsync(c->d_cursor, 0, sizeof(uint32_t), c->stream));
        const dim3 pgrid(c->direct_waves);  // alone on the GPU: 16 waves per CU measured best
        const TraceTuning dtune = direct_tuning(c, c->plan.n_slots);
        if ((r = with_types(kernel_choice(c, KC_DIRECT), LeafTypes(), "k_direct_persistent", [&](auto T) {
                GD_LEDGER(c, k_direct_persistent<T()>);
                k_direct_persistent<T()><<<pgrid, BLOCK, 0, c->stream>>>(sc, c->frame, *p, c->plan.n_slots, c->d_direct, c->d_spill, c->d_cursor, dtune);
            })))
            return r;
    }
    HIP_TRY(hipGetLastError());
    return end_timed(c, t);
}

int gpuart_hip_pt_plan(gpuart_hip_ctx *c, uint32_t passes) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    c->plan.set_plan(passes);
    return 0;
}

int gpuart_hip_pt_reset(gpuart_hip_ctx *c) {
    if (c && c->empty_share) return 0;
    if (!c || !c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    // passes still in flight belong to the accumulation that is being discarded: let them finish first
    int r = drain(c);
    if (r) return r;
    c->plan.plan_done = 0;  // a new accumulation: the planned sequence, if any, begins again
    c->have_list = false; c->active_n = 0; c->have_counts = false; c->uniform_paths = 0;  // every block again, nothing counted
    if (c->plan.active_slots) c->plan.set_active(0);
    HIP_TRY(hipMemsetAsync(c->d_accum, 0, c->plan.tile_pixels * sizeof(float4), c->stream));
    return 0;
}

/// Upper bound on the number of segments any path can have. colorWeight is multiplied per segment by the albedo
/// of the primitive type that was hit (path_tracing.glsl:123-126,204) and the loop stops as soon as ANY channel
/// is <= minWeight, so channel c survives at most as long as (largest albedo.c among the primitive types present
/// in the scene)^n > minWeight; the bound is the smallest such n over the channels. The bound may only ever be too
/// LARGE (a launch that finds an empty queue costs microseconds; a missing one would leave paths uncommitted), so the
/// comparison is relaxed by 1e-4: fp32 products of mixed albedos can round differently from the powers taken here.
/// k_shade additionally commits a path whose next segment would lie beyond the launched ones (belt and braces).
static uint32_t segment_bound(const gpuart_hip_ctx *c, const gpuart_params *p) {
    if (p->maxSegments <= 0 || !(1.0f > p->minWeight)) return 0;
    uint32_t n = (uint32_t)p->maxSegments;
    if (!(p->minWeight > 0)) return n;
    static const float ALBEDO[4][3] = {{0.65f, 0.4f, 0.35f}, {0.1f, 0.2f, 0.1f}, {0.3f, 0.3f, 0.3f}, {0.3f, 0.3f, 0.3f}};
    // The user sphere shades as a sphere, and even with radius 0 (= "disabled") its quadratic can report a hit through
    // rounding (sphere.glsl:47-52), so the sphere albedo always takes part in the bound.
    const uint32_t types = c->type_mask | 1u;
    uint32_t bound = n;
    for (int ch = 0; ch < 3; ch++) {
        float a = 0;
        for (int t = 0; t < 4; t++) if (types & (1u << t)) a = std::max(a, ALBEDO[t][ch]);
        float w = 1.0f;
        uint32_t k = 0;
        while (k < n && w > p->minWeight * 0.9999f) { w *= a; k++; }
        bound = std::min(bound, k);
    }
    return std::max<uint32_t>(bound, 1);
}

extern "C++" {
namespace {
/// The frame as the kernels of ONE run see it: with the birth order of its paths (one order for all launches of the run: path
/// slots keep their pixels from launch to launch) and, if this run is to count the cost of the tile's blocks, the counters.
/// The library orders by itself only where that was measured to pay (profiles/r04/birth_order.txt): runs of ONE pass through k_run
/// — the frame-by-frame use, where the run's tail is a third of its time. Longer runs keep the row-major order: most expensive
/// first shortens their (relatively smaller) tail too but puts all heavy blocks in flight at once, which costs the main phase more.
int run_frame(gpuart_hip_ctx *c, Frame &f, bool &gathers, bool single_pass_run) {
    f = c->frame;
    gathers = false;
    if (c->have_list) { f.tile_order = c->d_active; return 0; }  // an active block list is the run's order: nothing gathered, nothing sorted
    if (c->order_from_hook || !c->order_auto || !single_pass_run || (c->plan.mode != 0 && c->plan.mode != 5)) return 0;
    if (c->order_sorting && hipEventQuery(c->ev_order) == hipSuccess) {  // (hipErrorNotReady: keep the order in use a little longer)
        c->order_cur = c->order_next;
        c->order_sorting = false;
    }
    (void)hipGetLastError();
    f.tile_order = c->order_cur >= 0 ? c->d_tile_order[c->order_cur] : nullptr;
    if (!c->order_sorting && c->order_stale) {
        const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
        if (!c->d_tile_cost) {
            HIP_TRY(hipMalloc(&c->d_tile_cost, tiles * sizeof(uint32_t)));
            HIP_TRY(hipMemset(c->d_tile_cost, 0, tiles * sizeof(uint32_t)));  // (k_tile_order zeroes what it has read)
            for (auto &o : c->d_tile_order) if (!o) HIP_TRY(hipMalloc(&o, tiles * sizeof(uint32_t)));
            if (!c->ev_order) HIP_TRY(hipEventCreateWithFlags(&c->ev_order, hipEventDisableTiming));
        }
        f.tile_cost = c->d_tile_cost;
        gathers = true;
    }
    return 0;
}

/// Behind a gathering run on its lane's stream: the sort into the order buffer that no run uses — none launched so far may still
/// read it (the lanes' ev_done), and the runs to come take it only once ev_order has been seen complete (run_frame).
int sort_tile_order(gpuart_hip_ctx *c, PassLane &l) {
    for (auto &o : c->lanes) if (&o != &l && o.used) HIP_TRY(hipStreamWaitEvent(l.main, o.ev_done, 0));
    c->order_next = c->order_cur == 0 ? 1 : 0;
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    GD_LEDGER(c, k_tile_order);
    k_tile_order<<<1, TO_THREADS, 0, l.main>>>(c->d_tile_cost, c->d_tile_order[c->order_next], (uint32_t)tiles);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev_order, l.main));
    c->order_sorting = true;
    c->order_stale = false;
    return 0;
}

/// The end of every run: its colour is accumulated in pass order on the primary stream, which releases the lane; a gathering run is sorted.
int finish_run(gpuart_hip_ctx *c, PassLane &l, bool gathers) {
    int r;
    HIP_TRY(hipEventRecord(l.ev_done, l.main));
    HIP_TRY(hipStreamWaitEvent(c->stream, l.ev_done, 0));
    GD_LEDGER(c, k_accumulate);
    if (c->have_counts) {  // the run's blocks only (all of them without a list), and their path counts
        const uint32_t entries = l.pb.n_slots;
        k_accumulate<<<dim3((entries + 255) / 256), 256, 0, c->stream>>>(c->d_accum, l.passcolor, c->plan.tile_pixels, l.pb.batch,
                                                                          c->have_list ? c->d_active : nullptr, c->d_block_paths, entries,
                                                                          c->frame.tw, c->frame.th, l.pb.batch * (uint32_t)c->pend_npaths);
    } else {
        k_accumulate<<<dim3((unsigned)((c->plan.tile_pixels + 255) / 256)), 256, 0, c->stream>>>(c->d_accum, l.passcolor, c->plan.tile_pixels, l.pb.batch,
                                                                                                 nullptr, nullptr, 0, 0, 0, 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(l.ev_free, c->stream));
    if (gathers && (r = sort_tile_order(c, l))) return r;
    l.used = true;
    return 0;
}

/// The collected passes [first, first + count) as ONE persistent kernel per path of the pass (k_run, kernel_run.h) on
/// pass lane `l`; then their colour planes are added to the accumulator in pass order on the primary stream.
int launch_run_persistent(gpuart_hip_ctx *c, PassLane &l, size_t first, size_t count) {
    int r;
    const gpuart_params *p = &c->pend_params;
    const int npaths = c->pend_npaths;
    Scene sc = scene_of(c);
    SeedBatch seeds{};
    for (size_t k = 0; k < count; k++) seeds.seed[k] = c->pend_seeds[first + k];
    if (!l.run_cursor) HIP_TRY(hipMalloc(&l.run_cursor, 64));
    const PathBuffers &b = l.pb;
    // k_run's list entries carry the path slot in RUN_SLOT's bits beside their flags
    // (the LARGEST slot index, n_slots x batch - 1, must fit: a run of exactly 2^28 slots does; the planner never plans a longer one
    //  for mode 0 — run_planner.h RUN_KERNEL_SLOTS — so only modes 1 / 4 / 5 on a tile beyond 2^28 pixels can get here)
    if ((uint64_t)b.n_slots * b.batch > (uint64_t)RUN_SLOT + 1)
        return fail(GPUART_HIP_ERR_ARG, "modes 1, 4 and 5 run through k_run, whose list entries address 2^28 path slots per run; this tile has " +
                    std::to_string((uint64_t)b.n_slots * b.batch) + " (use mode 0 or 3, or a smaller tile)");
    const uint32_t chunks = b.n_slots * b.batch / BLOCK;
    const dim3 grid(std::min<uint32_t>(c->run_waves, std::max<uint32_t>(1, chunks)));
    TimedLaunch t;
    Frame fr;
    bool gathers;
    if ((r = run_frame(c, fr, gathers, count == 1))) return r;
    if (l.used) HIP_TRY(hipStreamWaitEvent(l.main, l.ev_free, 0));  // the lane's previous run has been accumulated
    if ((r = begin_timed(c, t, 0, l.main))) return r;
    for (int j = 0; j < npaths; j++) {
        TimedLaunch tt;
        HIP_TRY(hipMemsetAsync(l.run_cursor, 0, sizeof(uint32_t), l.main));
        if (c->timing_level >= 2 && (r = begin_timed(c, tt, 1, l.main))) return r;
        if ((r = with_types(kernel_choice(c, KC_RUN), RunTypes(), "k_run", [&](auto K) {
                constexpr bool C = (K() & KC_COUNT) != 0, R = (K() & KC_REFWORK) != 0;
                constexpr int T = K() & (KC_COUNT - 1);
                GD_LEDGER(c, k_run<C, R, T>);
                k_run<C, R, T><<<grid, BLOCK, 0, l.main>>>(sc, fr, *p, seeds, b, j, npaths, l.passcolor, l.spill_main, c->d_counters, c->tune, l.run_cursor);
            })))
            return r;
        if (c->timing_level >= 2 && (r = end_timed(c, tt, l.main))) return r;
    }
    if ((r = end_timed(c, t, l.main))) return r;
    return finish_run(c, l, gathers);
}

/// One run of the wavefront pipeline for the pending passes [first, first + count) on the next pass lane.
int launch_run(gpuart_hip_ctx *c, size_t first, size_t count) {
    int r;
    const gpuart_params *p = &c->pend_params;
    const int npaths = c->pend_npaths;
    Scene sc = scene_of(c);
    TimedLaunch t;
    // a lane's path buffers hold max_batch passes (realloc_tile): a longer run would write past them (run_planner.h)
    if (const char *bad = c->plan.check(count)) return fail(GPUART_HIP_ERR_DEVICE, std::string("internal: ") + bad);
    PassLane &l = c->lanes[c->next_lane];
    c->next_lane = (c->next_lane + 1) % c->plan.lanes_in_use;
    l.pb.batch = (uint32_t)count;
    l.pb.n_slots = (uint32_t)c->plan.slots();  // (every grid, chunk count and counter below comes from the run's slots)
    if (c->plan.uses_run_kernel(count)) return launch_run_persistent(c, l, first, count);
    const uint32_t nseg = segment_bound(c, p);
    SeedBatch seeds{};
    for (size_t k = 0; k < count; k++) seeds.seed[k] = c->pend_seeds[first + k];
    if ((r = ensure_segment_counters(c, l, nseg))) return r;
    const PathBuffers &b = l.pb;
    const bool detail = c->timing_level >= 2;
    const dim3 pgrid(c->grid_waves);
    const dim3 sgrid(std::min<uint32_t>(c->shade_waves, b.n_slots * b.batch / BLOCK));  // k_gen / k_shade: grid-stride loops
    int j_cur = 0;
    Frame fr;
    bool gathers;
    if ((r = run_frame(c, fr, gathers, false))) return r;  // (an order set through gpuart_hip_test_tile_order applies here too)
    // by the run: from 4 passes on a packet holds at most 16 pixels, a strip of one or two rows in row-major order; the 21 1/3 pixels of 3 passes
    // are 8 x 3 there, and cut a Z-curve badly (1 and 2 passes: the whole or half block in either order)
    if (c->block_order == 2) fr.block_order = count >= 4 ? 1u : 0u;
    if (l.used) HIP_TRY(hipStreamWaitEvent(l.main, l.ev_free, 0));  // the lane's previous pass has been accumulated
    if ((r = begin_timed(c, t, 0, l.main))) return r;
    // packet walks (GPUART_HIP_PACKET; the GD_REF_ORDER kernels only): the camera rays' launch, the Sun-shadow queries of segment 0
    const int trace_choice = kernel_choice(c, KC_TRACE);
    const uint32_t packet = c->n_prims <= c->packet_max_prims ? c->packet : 0u;
    // k_gen walks the camera rays itself (GPUART_HIP_GEN_WALK) exactly where their launch would walk them as packets — the knob, the tree's
    // size, a fast-box kernel in the reference's order — and a later k_trace launch follows in the run; then trace(0, -1) is not launched
    const bool gen_walk = c->gen_walk && packet >= 1 && (trace_choice & GD_REF_ORDER) && !(trace_choice & GD_EXACT_BOXES) && nseg > 0 &&
                          (nseg >= 2 || p->sunEnabled == 1);
    // ... and shades segment 0 of what it walked (GPUART_HIP_GEN_SHADE) where k_shade(1) follows; at level 2 it walks segment 0's Sun-shadow queries too
    const int gen_shade = gen_walk && nseg >= 2 ? (int)c->gen_shade : 0;
    // ... pooled per wave into full packets (GPUART_HIP_SHADOW_POOL): k_gen's level 3, which takes longer chunks (a chunk's end empties the pool).
    // By the run: at 3 passes per run the pool saves few packet steps and parking the queries costs more.
    const int gen_level = gen_shade == 2 && c->shadow_pool && count >= c->pool_min_passes ? 3 : gen_shade;
    const uint32_t gen_chunk = gen_level == 3 ? c->pool_chunk : c->tune.chunk;
    const dim3 wgrid(std::max<uint32_t>(1u, std::min<uint32_t>(c->grid_waves, (b.n_slots * b.batch + gen_chunk - 1) / gen_chunk)));  // (l.spill_main holds grid_waves columns at least)
    // one BVH-query launch: closest-hit queries of segment seg_c and / or Sun-shadow queries of segment seg_s
    auto trace = [&](int seg_c, int seg_s) -> int {
        TimedLaunch tt;
        int rr;
        if (detail && (rr = begin_timed(c, tt, 1, l.main))) return rr;
        TraceTuning tune = c->tune;
        tune.packet = (packet >= 1 && seg_c == 0) ? 1u : (packet >= 2 && seg_s == 0) ? 2u : 0u;
        if ((rr = with_types(trace_choice, TraceTypes(), "k_trace", [&](auto T) {
                GD_LEDGER(c, k_trace<false, T()>);
                k_trace<false, T()><<<pgrid, BLOCK, 0, l.main>>>(sc, fr, *p, b, seg_c, seg_s, 1, j_cur, npaths, l.passcolor, l.spill_main, c->d_counters, tune);
            })))
            return rr;
        if (detail && (rr = end_timed(c, tt, l.main))) return rr;
        return 0;
    };
    for (int j = 0; j < npaths; j++) {
        j_cur = j;
        HIP_TRY(hipMemsetAsync(b.counters, 0, 4 * ((size_t)nseg + 1) * sizeof(uint32_t), l.main));
        if (c->tune.xcd_queues) HIP_TRY(hipMemsetAsync(b.xcd_cursors, 0, 16 * ((size_t)nseg + 1) * sizeof(uint32_t), l.main));
        GD_LEDGER(c, k_gen);
        if (gen_walk) {  // in the per-launch bracket the camera rays' launch had
            TimedLaunch tt;
            if (detail && (r = begin_timed(c, tt, 1, l.main))) return r;
            k_gen<<<wgrid, BLOCK, 0, l.main>>>(sc, fr, *p, seeds, j, npaths, b, l.passcolor, l.spill_main, gen_chunk, trace_choice, gen_level);
            if (detail && (r = end_timed(c, tt, l.main))) return r;
            if (gen_shade && (r = trace(1, gen_shade < 2 && p->sunEnabled == 1 ? 0 : -1))) return r;
        } else {
            k_gen<<<sgrid, BLOCK, 0, l.main>>>(sc, fr, *p, seeds, j, npaths, b, l.passcolor, l.spill_main, c->tune.chunk, 0, 0);
            if (nseg && (r = trace(0, -1))) return r;
        }
        for (uint32_t seg = gen_shade ? 1 : 0; seg < nseg; seg++) {
            GD_LEDGER(c, k_shade<false>);
            k_shade<false><<<sgrid, BLOCK, 0, l.main>>>(sc, fr, *p, seeds, b, (int)seg, (int)nseg, j, npaths, l.passcolor, c->d_counters);
            // the Sun-shadow queries of this segment travel with the closest-hit queries of the next one
            const int next_c = seg + 1 < nseg ? (int)seg + 1 : -1, sh = p->sunEnabled == 1 ? (int)seg : -1;
            if ((next_c >= 0 || sh >= 0) && (r = trace(next_c, sh))) return r;
        }
        HIP_TRY(hipGetLastError());
    }
    if ((r = end_timed(c, t, l.main))) return r;
    return finish_run(c, l, gathers);
}
}  // namespace
}  // extern "C++"

/// `npaths` more paths in every pixel that no k_accumulate launch counts: the host's count while all passes covered all blocks; with
/// counts on the device (mode 2 after a list was dropped) they go there and back.
static int count_whole_pass(gpuart_hip_ctx *c, uint32_t npaths) {
    if (!npaths) return 0;
    if (!c->have_counts) { c->uniform_paths += npaths; return 0; }
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    std::vector<uint32_t> h(tiles);
    HIP_TRY(hipMemcpyAsync(h.data(), c->d_block_paths, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (auto &v : h) v += npaths;
    HIP_TRY(hipMemcpyAsync(c->d_block_paths, h.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int gpuart_hip_set_active_blocks(gpuart_hip_ctx *c, const uint32_t *blocks, size_t n) {
    if (!c || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "active blocks: no frame size set");
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    if (blocks) {  // validated here, on the host: the kernels index pixels and counts with these words
        if (c->empty_share || !tiles) return fail(GPUART_HIP_ERR_ARG, "active blocks: an empty share has no blocks");
        if (n > tiles) return fail(GPUART_HIP_ERR_ARG, "active blocks: " + std::to_string(n) + " entries for a tile of " + std::to_string(tiles) + " blocks");
        for (size_t k = 0; k < n; k++) {
            if (blocks[k] >= tiles)
                return fail(GPUART_HIP_ERR_ARG, "active blocks: entry " + std::to_string(k) + " is " + std::to_string(blocks[k]) + ", the tile has " + std::to_string(tiles) + " blocks");
            if (k && blocks[k] <= blocks[k - 1]) return fail(GPUART_HIP_ERR_ARG, "active blocks: entry " + std::to_string(k) + " is not above its predecessor (strictly ascending, please)");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    int r = gpuart_hip_flush(c);  // what was collected belongs to the old list
    if (r || (r = drain(c))) return r;  // (and no run in flight reads the list while it is replaced)
    if (!blocks) {
        c->have_list = false; c->active_n = 0;
        c->plan.set_active(0);
        return 0;
    }
    if (!c->d_active) HIP_TRY(hipMalloc(&c->d_active, tiles * sizeof(uint32_t)));
    if (!c->have_counts) {  // from here on the blocks' counts differ: the device array, every block at the host's count
        if (!c->d_block_paths) HIP_TRY(hipMalloc(&c->d_block_paths, tiles * sizeof(uint32_t)));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->d_block_paths, (int)c->uniform_paths, tiles, c->stream));
        c->have_counts = true;
    }
    if (n) HIP_TRY(hipMemcpyAsync(c->d_active, blocks, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (the lanes' streams read the list; `blocks` is the caller's)
    c->have_list = true; c->active_n = (uint32_t)n;
    c->plan.set_active((uint32_t)n * 64);
    return 0;
}

static int block_paths_to(gpuart_hip_ctx *c, void *dst, bool host) {
    if (!c || !dst || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "block paths: bad argument");
    if ((uintptr_t)dst % 4) return fail(GPUART_HIP_ERR_ARG, "block paths: misaligned pointer");
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    if (c->empty_share || !tiles) return 0;
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    if (c->have_counts) HIP_TRY(hipMemcpyAsync(dst, c->d_block_paths, tiles * sizeof(uint32_t), host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    else if (host) std::fill((uint32_t *)dst, (uint32_t *)dst + tiles, c->uniform_paths);
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dst, (int)c->uniform_paths, tiles, c->stream));
    if (host) HIP_TRY(hipStreamSynchronize(c->stream));  // (like gpuart_hip_read, also where the host's count served)
    return 0;
}
int gpuart_hip_read_block_paths(gpuart_hip_ctx *c, uint32_t *host) { return block_paths_to(c, host, true); }
int gpuart_hip_export_block_paths(gpuart_hip_ctx *c, void *device) { return block_paths_to(c, device, false); }

int gpuart_hip_flush(gpuart_hip_ctx *c) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    const size_t pending = c->pend_seeds.size();
    if (!pending) return 0;
    HIP_TRY(hipSetDevice(c->device));
    // What is still pending when something observes or changes state (read-back, finish, ...) is split into runs
    // (RunPlanner::on_flush)
    c->plan.pending = pending;
    int r = 0;
    size_t first = 0;
    for (size_t count : c->plan.on_flush()) {
        if ((r = launch_run(c, first, count))) break;
        first += count;
    }
    c->pend_seeds.clear();
    return r;
}


int gpuart_hip_pt_pass(gpuart_hip_ctx *c, const gpuart_params *p, const float randSeed[4], int npaths) {
    int r = check_ready(c, p);
    if (r) return r > 0 ? 0 : r;
    if (!randSeed || npaths < 0) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    if (p->maxSegments > GPUART_HIP_MAX_SEGMENTS) return fail(GPUART_HIP_ERR_ARG, "maxSegments exceeds GPUART_HIP_MAX_SEGMENTS");
    if (c->have_list && (c->plan.mode == 1 || c->plan.mode == 2 || c->plan.mode == 4))
        return fail(GPUART_HIP_ERR_ARG, "an active block list is set: mode " + std::to_string(c->plan.mode) + " renders whole tiles only (modes 0, 3 and 5 honour a list)");
    if (npaths == 0 || (c->have_list && c->active_n == 0)) return 0;
    HIP_TRY(hipSetDevice(c->device));
    const float4 seed = make_float4(randSeed[0], randSeed[1], randSeed[2], randSeed[3]);
    if (c->plan.mode == 2) {  // megakernel: the whole path in one thread, on the primary stream (ablation / cross-check)
        if ((r = gpuart_hip_flush(c))) return r;
        Scene sc = scene_of(c);
        TimedLaunch t;
        if ((r = begin_timed(c, t, 0))) return r;
        dim3 grid(std::min<uint32_t>(c->grid_waves, c->plan.n_slots / BLOCK));
        GD_LEDGER(c, k_pt_mega<false>);
        k_pt_mega<false><<<grid, BLOCK, 0, c->stream>>>(sc, c->frame, *p, seed, npaths, c->plan.n_slots, c->d_accum, c->d_spill, c->d_counters);
        HIP_TRY(hipGetLastError());
        if ((r = end_timed(c, t))) return r;
        return count_whole_pass(c, (uint32_t)npaths);
    }
    if ((r = count_whole_pass(c, c->have_counts ? 0u : (uint32_t)npaths))) return r;  // (with counts on the device k_accumulate counts the run)
    // Passes are collected and launched run_passes at a time (plan_runs). A pass with different parameters
    // starts a new batch; anything that observes or changes state flushes first.
    if (!c->pend_seeds.empty() && (memcmp(&c->pend_params, p, sizeof *p) != 0 || c->pend_npaths != npaths))
        if ((r = gpuart_hip_flush(c))) return r;
    c->pend_params = *p;
    c->pend_npaths = npaths;
    c->pend_seeds.push_back(seed);
    c->plan.pending = c->pend_seeds.size() - 1;
    if (const size_t count = c->plan.on_pass()) {
        r = launch_run(c, 0, count);
        c->pend_seeds.clear();
        return r;
    }
    return 0;
}

int gpuart_hip_export(gpuart_hip_ctx *c, int which, void *rgba_device, float divide_by) {
    if (!c || !rgba_device || (which != 0 && which != 1) || !c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    const float4 *src = which == 0 ? c->d_direct : c->d_accum;
    if (!(divide_by > 0)) divide_by = 1.0f;
    size_t n = c->plan.tile_pixels;
    GD_LEDGER(c, k_scale_copy);
    k_scale_copy<<<dim3((unsigned)((n + 255) / 256)), 256, 0, c->stream>>>(src, (float4 *)rgba_device, n, divide_by);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gpuart_hip_read(gpuart_hip_ctx *c, int which, float *rgba_host, float divide_by) {
    if (!c || !rgba_host || (which != 0 && which != 1) || !c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    size_t bytes = c->plan.tile_pixels * sizeof(float4);
    const float4 *src = which == 0 ? c->d_direct : c->d_accum;
    if (divide_by > 0 && divide_by != 1.0f) {
        int r = ensure_scratch(c, bytes);
        if (r) return r;
        r = gpuart_hip_export(c, which, c->d_scratch, divide_by);
        if (r) return r;
        src = (const float4 *)c->d_scratch;
    }
    HIP_TRY(hipMemcpyAsync(rgba_host, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int gpuart_hip_write(gpuart_hip_ctx *c, int which, const float *rgba_host) {
    if (!c || !rgba_host || which != 1 || !c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    HIP_TRY(hipMemcpyAsync(c->d_accum, rgba_host, c->plan.tile_pixels * sizeof(float4), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
}

int gpuart_hip_finish(gpuart_hip_ctx *c) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    return drain(c);
}

int gpuart_hip_set_mode(gpuart_hip_ctx *c, int mode) {
    if (!c || mode < 0 || mode > 5) return fail(GPUART_HIP_ERR_ARG, "bad mode");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    int r = drain(c);  // modes use different streams; keep their passes ordered
    if (r) return r;
    c->plan.mode = mode;
    c->plan.plan();
    return 0;
}

int gpuart_hip_set_timing(gpuart_hip_ctx *c, int level) {
    if (!c || level < 0 || level > 2) return fail(GPUART_HIP_ERR_ARG, "bad timing level");
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    c->timing_level = level;
    return 0;
}

int gpuart_hip_counters(gpuart_hip_ctx *c, gpuart_counters *out, int reset) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    unsigned long long h[16];
    int rr = drain(c);
    if (rr) return rr;
    HIP_TRY(hipMemcpyAsync(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (out) {
        out->rays = h[0]; out->nodes = h[1];
        for (int k = 0; k < 4; k++) out->prim_tests[k] = h[2 + k];
        out->segments = h[6];
        out->box_steps = h[7];
        out->box_steps_top = h[8];
        out->rewalks = h[9];
    }
    if (reset) HIP_TRY(hipMemsetAsync(c->d_counters, 0, sizeof h, c->stream));
    return 0;
}

int gpuart_hip_set_nearest_first(gpuart_hip_ctx *c, uint32_t min_prims) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }  // (passes collected so far were requested under the old choice; both give... the reference's image or, opted in, the walk's)
    c->nearest_min_prims = min_prims;
    if (c->have_scene) c->ref_order = (!c->exact_boxes && c->n_prims < c->nearest_min_prims) ? 1u : 0u;
    return 0;
}

int gpuart_hip_scene_order(gpuart_hip_ctx *c, int *order) {
    if (!c || !order || !c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    *order = c->exact_boxes ? 2 : c->ref_order ? 1 : 0;
    return 0;
}

int gpuart_hip_kernel_time(gpuart_hip_ctx *c, int cls, double *total_ms, uint64_t *launches, int reset) {
    if (!c || cls < 0 || cls > 1) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    int r = fold_timings(c);
    if (r) return r;
    if (total_ms) *total_ms = c->timed_ms[cls];
    if (launches) *launches = c->timed_launches[cls];
    if (reset) { c->timed_ms[cls] = 0; c->timed_launches[cls] = 0; }
    return 0;
}

int gpuart_hip_scene_info(gpuart_hip_ctx *c, uint64_t *nodes, uint64_t *prims, uint32_t *max_depth, uint64_t *device_bytes) {
    if (!c || !c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (nodes) *nodes = c->n_nodes;
    if (prims) *prims = c->n_prims;
    if (max_depth) *max_depth = c->max_depth;
    if (device_bytes) *device_bytes = c->scene_bytes;
    return 0;
}

// ---- a refit in place (include/gpuart_refit.h): host code only ------------------------------------------------------------------
int gpuart_hip_scene_device(gpuart_hip_ctx *c, gpuart_hip_scene *out) {
    if (!c || !out) return fail(GPUART_HIP_ERR_ARG, "gpuart_hip_scene_device: bad argument");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    HIP_TRY(hipSetDevice(c->device));
    int r;
    if ((r = gpuart_hip_flush(c))) return r;
    if ((r = drain(c))) return r;
    if (!c->d_prim_boxes) {
        HIP_TRY(hipMalloc(&c->d_prim_boxes, c->h_prim_boxes.size() * sizeof(float) + 16));
        HIP_TRY(hipMemcpy(c->d_prim_boxes, c->h_prim_boxes.data(), c->h_prim_boxes.size() * sizeof(float), hipMemcpyHostToDevice));
        std::vector<float, UninitAlloc<float>>().swap(c->h_prim_boxes);
    }
    out->layout = 1;
    out->exact_boxes = c->exact_boxes;
    out->recs = c->d_recs; out->n_recs = c->n_recs;
    out->prims = c->d_prims; out->n_prims = c->n_prims;
    out->prim_boxes = c->d_prim_boxes;
    memcpy(out->root_min, c->root_min, 12); memcpy(out->root_max, c->root_max, 12);
    out->root_ref = c->root_ref;
    out->box_slack = c->box_slack;
    out->max_depth = c->max_depth;
    out->generation = c->generation;
    return 0;
}

int gpuart_hip_scene_refitted(gpuart_hip_ctx *c, const float root_min[3], const float root_max[3], int subnormal) {
    if (!c || !root_min || !root_max) return fail(GPUART_HIP_ERR_ARG, "gpuart_hip_scene_refitted: bad argument");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (c->exact_boxes) return fail(GPUART_HIP_ERR_ARG, "gpuart_hip_scene_refitted: a tree with irregular boxes (or boxes that do not bound their contents) is not refitted");
    if (!tree_rule::box_ok(root_min, root_max)) return fail(GPUART_HIP_ERR_ARG, "gpuart_hip_scene_refitted: the root box is not finite and ordered");
    int r;
    if ((r = gpuart_hip_flush(c))) return r;
    if ((r = drain(c))) return r;
    memcpy(c->root_min, root_min, 12); memcpy(c->root_max, root_max, 12);
    c->box_slack = c->quick_boxes ? slack_of_root(subnormal != 0, c->root_min, c->root_max) : __builtin_inff();
    c->order_stale = true;
    return 0;
}

// ---- a rebuild on the device (include/gpuart_build.h) and an edit (include/gpuart_edit.h): host code only ----------------------------
/// The spare set with room for n_recs records and n_prims primitives and boxes. `exact`: a set whose primitive room is not n_prims is
/// made anew (gpuart_hip_scene_reserve: the builders are told the room as the count to expect); else one that is large enough is reused.
static int reserve_spare(gpuart_hip_ctx *c, uint64_t n_recs, uint64_t n_prims, bool exact, gpuart_hip_scene *out, const char *name) {
    if (!c || !out) return fail(GPUART_HIP_ERR_ARG, std::string(name) + ": bad argument");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (n_recs > 0x03fffff0u) return fail(GPUART_HIP_ERR_ARG, std::string(name) + ": too many records");
    if (!exact && (n_prims < 1 || n_prims >= 0x05555540u)) return fail(GPUART_HIP_ERR_ARG, std::string(name) + ": the primitive count is 0 or beyond the uploader's bound");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_spare_prims || c->spare_recs < n_recs || (exact ? c->spare_prims != n_prims : c->spare_prims < n_prims)) {
        drop_spare(c);
        // (the same slack past the end as an upload's arrays, and like theirs zeroed)
        const size_t rb = ((size_t)n_recs * 4 + 4) * sizeof(float4), pb = ((size_t)n_prims * 3 + 4) * sizeof(float4), bb = (size_t)n_prims * 24 + 16;
        HIP_TRY(hipMalloc(&c->d_spare_recs, rb));
        HIP_TRY(hipMalloc(&c->d_spare_prims, pb));
        HIP_TRY(hipMalloc(&c->d_spare_boxes, bb));
        HIP_TRY(hipMemset(c->d_spare_recs, 0, rb));
        HIP_TRY(hipMemset(c->d_spare_prims, 0, pb));
        HIP_TRY(hipMemset(c->d_spare_boxes, 0, bb));
        c->spare_recs = n_recs;
        c->spare_prims = n_prims;
    } else {
        // a reused set (after a rebuild: the scene's former arrays) still holds the records of the tree it was; beyond the n_recs
        // about to be written it is zeroed again, so the arrays of a rebuilt scene end as an upload's do — and so is what lies behind
        // the n_prims primitives and boxes about to be written, where the set has room for more
        HIP_TRY(hipMemset((char *)c->d_spare_recs + (size_t)n_recs * 64, 0, (size_t)(c->spare_recs - n_recs) * 64 + 4 * sizeof(float4)));
        if (c->spare_prims > n_prims) {
            HIP_TRY(hipMemset((char *)c->d_spare_prims + (size_t)n_prims * 48, 0, (size_t)(c->spare_prims - n_prims) * 48 + 4 * sizeof(float4)));
            HIP_TRY(hipMemset((char *)c->d_spare_boxes + (size_t)n_prims * 24, 0, (size_t)(c->spare_prims - n_prims) * 24 + 16));
        }
    }
    memset(out, 0, sizeof *out);
    out->layout = 1;
    out->recs = c->d_spare_recs; out->n_recs = c->spare_recs;
    out->prims = c->d_spare_prims; out->n_prims = c->spare_prims;
    out->prim_boxes = c->d_spare_boxes;
    out->generation = c->generation;
    return 0;
}

int gpuart_hip_scene_reserve(gpuart_hip_ctx *c, uint64_t n_recs, gpuart_hip_scene *out) {
    return reserve_spare(c, n_recs, c ? c->n_prims : 0, true, out, "gpuart_hip_scene_reserve");
}

int gpuart_hip_scene_reserve_prims(gpuart_hip_ctx *c, uint64_t n_recs, uint64_t n_prims, gpuart_hip_scene *out) {
    return reserve_spare(c, n_recs, n_prims, false, out, "gpuart_hip_scene_reserve_prims");
}

/// Adopts the tree built into the spare set. `replace`: the primitive count and the type mask change too (gpuart_hip_scene_replaced).
static int adopt_built(gpuart_hip_ctx *c, const gpuart_hip_scene *b, bool replace, uint32_t type_mask, const std::string &name) {
    if (!c || !b) return fail(GPUART_HIP_ERR_ARG, name + ": bad argument");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (c->exact_boxes) return fail(GPUART_HIP_ERR_ARG, name + ": a tree with irregular boxes (or boxes that do not bound their contents) is not rebuilt");
    if (!c->d_spare_prims || b->recs != (void *)c->d_spare_recs || b->prims != (void *)c->d_spare_prims || b->prim_boxes != (void *)c->d_spare_boxes ||
        b->generation != c->generation || b->layout != 1)
        return fail(GPUART_HIP_ERR_ARG, name + ": the arrays are not the ones gpuart_hip_scene_reserve handed out for this scene");
    if (!replace && b->n_prims != c->n_prims) return fail(GPUART_HIP_ERR_ARG, name + ": the primitive count changed");
    if (replace && (b->n_prims < 1 || b->n_prims > c->spare_prims))
        return fail(GPUART_HIP_ERR_ARG, name + ": the primitive count " + std::to_string(b->n_prims) + " is 0 or beyond the reserved room of " + std::to_string(c->spare_prims));
    if (replace && (type_mask == 0 || type_mask > 15u)) return fail(GPUART_HIP_ERR_ARG, name + ": the type mask is 0 or beyond 15");
    if (b->n_recs > c->spare_recs) return fail(GPUART_HIP_ERR_ARG, name + ": more records than were reserved");
    if (b->max_depth > 1024) return fail(GPUART_HIP_ERR_ARG, name + ": tree deeper than 1024 levels");
    if (!tree_rule::box_ok(b->root_min, b->root_max)) return fail(GPUART_HIP_ERR_ARG, name + ": the root box is not finite and ordered");
    if (!c->d_prim_boxes) return fail(GPUART_HIP_ERR_ARG, name + ": gpuart_hip_scene_device was not called for this scene");
    if (!tree_rule::root_ref_ok(b->root_ref, b->n_recs, b->n_prims))
        return fail(GPUART_HIP_ERR_ARG, name + ": the root ref is neither record 0 of a tree with records nor a leaf inside the primitives");
    HIP_TRY(hipSetDevice(c->device));
    int r;
    if ((r = gpuart_hip_flush(c))) return r;
    if ((r = drain(c))) return r;
    // the traversal stacks for the new depth first: a failure here must leave the scene as it was
    const uint32_t old_depth = c->max_depth;
    c->max_depth = b->max_depth;
    if ((r = ensure_spill(c))) { c->max_depth = old_depth; return r; }
    std::swap(c->d_recs, c->d_spare_recs);
    std::swap(c->d_prims, c->d_spare_prims);
    std::swap(c->d_prim_boxes, c->d_spare_boxes);
    // the former scene arrays are the spare set now, with their own room
    const uint64_t old_recs = c->n_recs;
    c->n_recs = b->n_recs;
    c->spare_recs = old_recs;
    std::swap(c->prims_room, c->spare_prims);
    if (replace) {
        c->n_prims = b->n_prims;
        c->type_mask = type_mask;
        c->ref_order = (!c->exact_boxes && c->n_prims < c->nearest_min_prims) ? 1u : 0u;
    }
    memcpy(c->root_min, b->root_min, 12); memcpy(c->root_max, b->root_max, 12);
    c->root_ref = b->root_ref;
    c->max_depth = b->max_depth;
    c->n_nodes = 2 * c->n_recs + 1;
    c->scene_bytes = (size_t)c->n_recs * 64 + (size_t)c->n_prims * 48;
    // `box_slack` of the built scene says +inf when the builder met a subnormal plane (gpuart_build_result.subnormal)
    c->box_slack = c->quick_boxes ? slack_of_root(std::isinf(b->box_slack), c->root_min, c->root_max) : __builtin_inff();
    c->generation++;
    c->order_stale = true;
    return 0;
}

int gpuart_hip_scene_rebuilt(gpuart_hip_ctx *c, const gpuart_hip_scene *b) { return adopt_built(c, b, false, 0, "gpuart_hip_scene_rebuilt"); }

int gpuart_hip_scene_replaced(gpuart_hip_ctx *c, const gpuart_hip_scene *b, uint32_t type_mask) {
    return adopt_built(c, b, true, type_mask, "gpuart_hip_scene_replaced");
}

// ---- batched ray queries (kernels_query.h) ----------------------------------------------------------------------------
static_assert(sizeof(gpuart_ray_hit) == 32 && offsetof(gpuart_ray_hit, n) == 16 && offsetof(gpuart_ray_hit, type) == 28,
              "a record is the two float4 k_ray_query stores");

/// The checks every query entry point makes before it touches anything: 1 for n == 0 (nothing to do), 0 to go ahead, or the error.
/// `align`: what the pointers must be aligned to (16 for device memory: the kernel loads and stores float4).
static int query_check(gpuart_hip_ctx *c, size_t n, const void *src, const gpuart_ray_hit *hits, const int32_t *prims, size_t align,
                       bool pixels) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "ray query: no scene uploaded");
    if (pixels && !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "pick: no frame size set");
    if (pixels && !c->have_camera) return fail(GPUART_HIP_ERR_ARG, "pick: no camera set");
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "ray query: n = " + std::to_string(n) + " exceeds GPUART_HIP_MAX_RAYS");
    if (n == 0) return 1;
    if (!src || !hits) return fail(GPUART_HIP_ERR_ARG, pixels ? "pick: xy or hits is NULL" : "ray query: rays or hits is NULL");
    if ((uintptr_t)src % align || (uintptr_t)hits % align || (uintptr_t)prims % 4)
        return fail(GPUART_HIP_ERR_ARG, "ray query: misaligned pointer (rays and hits need " + std::to_string(align) + " bytes, prims 4)");
    return 0;
}

/// d_query_cursor's words: k_ray_query's chunk cursor, then gpuart_hip_trace_subpixel's verdict on its list (word 1) and its draws (from word 16)
#define GD_QUERY_WORDS (16 + 2 * GPUART_HIP_MAX_SUBPIXEL)

static RayQuery make_query(size_t n, uint32_t flags, const float us[4]) {
    RayQuery q{};
    q.n = (uint32_t)n;
    q.occlusion = (flags & GPUART_HIP_RAYS_OCCLUSION) ? 1u : 0u;
    q.use_us = us ? 1u : 0u;
    if (us) memcpy(q.us, us, sizeof q.us);
    return q;
}

/// One k_ray_query launch on the primary stream. Its scratch — the chunk cursor and the traversal-stack spill d_spill — belongs to the
/// primary stream, which nothing on the pass lanes' streams uses: a query may run beside pipeline runs in flight. Collected passes are
/// not flushed (a query neither observes nor changes what they render), and neither the work counters nor the render timings see it.
/// `frame`: the frame an RQ_PIXELS query's pixels belong to (gpuart_hip_gbuffer_scaled's); NULL: the context's.
static int launch_ray_query(gpuart_hip_ctx *c, const RayQuery &q, int source, const Frame *frame = nullptr) {
    if (!c->d_query_cursor) HIP_TRY(hipMalloc(&c->d_query_cursor, GD_QUERY_WORDS * sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(c->d_query_cursor, 0, sizeof(uint32_t), c->stream));
    // chunks as the direct-lighting frame takes them; a small batch gets the waves it can fill
    const TraceTuning tune = direct_tuning(c, q.n);
    const dim3 grid(std::max<uint32_t>(1u, std::min<uint32_t>(c->direct_waves, (q.n + tune.chunk - 1) / tune.chunk)));
    const Scene sc = scene_of(c);
    auto query = [&](auto T, auto S) {
        GD_LEDGER(c, k_ray_query<T(), S()>);
        k_ray_query<T(), S()><<<grid, BLOCK, 0, c->stream>>>(sc, frame ? *frame : c->frame, q, c->d_spill, c->d_query_cursor, tune);
    };
    if (int r = with_types(kernel_choice(c, KC_QUERY), LeafTypes(), "k_ray_query", [&](auto T) {
            if (source == RQ_PIXELS) query(T, std::integral_constant<int, RQ_PIXELS>());
            else query(T, std::integral_constant<int, RQ_RAYS>());
        }))
        return r;
    HIP_TRY(hipGetLastError());
    return 0;
}

#define GD_QUERY_STAGE ((size_t)1 << 21)  // queries per staged chunk of the host-memory entry points (136 MB of scratch at most)

int gpuart_hip_trace_rays(gpuart_hip_ctx *c, const float *rays, size_t n, uint32_t flags, const float us[4], gpuart_ray_hit *hits,
                          int32_t *prims) {
    int r = query_check(c, n, rays, hits, prims, 16, false);
    if (r) return r > 0 ? 0 : r;
    if (flags & ~GPUART_HIP_RAYS_OCCLUSION) return fail(GPUART_HIP_ERR_ARG, "ray query: unknown flags");
    HIP_TRY(hipSetDevice(c->device));
    RayQuery q = make_query(n, flags, us);
    q.rays = (const float4 *)rays;
    q.hits = (float4 *)hits;
    q.prims = prims;
    return launch_ray_query(c, q, RQ_RAYS);
}

/// The host-memory entry points: chunks of GD_QUERY_STAGE queries through the context's scratch, `src_bytes` of source per query.
static int staged_query(gpuart_hip_ctx *c, const void *src, size_t src_bytes, size_t n, uint32_t flags, const float us[4], int source,
                        gpuart_ray_hit *hits, int32_t *prims) {
    HIP_TRY(hipSetDevice(c->device));
    const size_t chunk = std::min(n, GD_QUERY_STAGE);
    int r = ensure_scratch(c, chunk * (32 + 32 + 4));
    if (r) return r;
    char *base = (char *)c->d_scratch;
    float4 *d_hits = (float4 *)(base + chunk * 32);  // (the source area is 32 bytes per query for either source)
    int32_t *d_prims = (int32_t *)(base + chunk * 64);
    for (size_t k = 0; k < n; k += chunk) {
        const size_t m = std::min(chunk, n - k);
        HIP_TRY(hipMemcpyAsync(base, (const char *)src + k * src_bytes, m * src_bytes, hipMemcpyHostToDevice, c->stream));
        RayQuery q = make_query(m, flags, us);
        q.rays = (const float4 *)base;
        q.xy = (const uint2 *)base;
        q.hits = d_hits;
        q.prims = prims ? d_prims : nullptr;
        if ((r = launch_ray_query(c, q, source))) return r;
        HIP_TRY(hipMemcpyAsync(hits + k, d_hits, m * 32, hipMemcpyDeviceToHost, c->stream));
        if (prims) HIP_TRY(hipMemcpyAsync(prims + k, d_prims, m * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int gpuart_hip_trace_rays_host(gpuart_hip_ctx *c, const float *rays, size_t n, uint32_t flags, const float us[4], gpuart_ray_hit *hits,
                               int32_t *prims) {
    int r = query_check(c, n, rays, hits, prims, 4, false);
    if (r) return r > 0 ? 0 : r;
    if (flags & ~GPUART_HIP_RAYS_OCCLUSION) return fail(GPUART_HIP_ERR_ARG, "ray query: unknown flags");
    return staged_query(c, rays, 32, n, flags, us, RQ_RAYS, hits, prims);
}

int gpuart_hip_pick(gpuart_hip_ctx *c, const uint32_t *xy, size_t n, const float us[4], gpuart_ray_hit *hits, int32_t *prims) {
    int r = query_check(c, n, xy, hits, prims, 4, true);
    if (r) return r > 0 ? 0 : r;
    for (size_t i = 0; i < n; i++)
        if (xy[2 * i] >= c->frame.W || xy[2 * i + 1] >= c->frame.H)
            return fail(GPUART_HIP_ERR_ARG, "pick: pixel " + std::to_string(i) + " (" + std::to_string(xy[2 * i]) + ", " +
                        std::to_string(xy[2 * i + 1]) + ") lies outside the " + std::to_string(c->frame.W) + " x " +
                        std::to_string(c->frame.H) + " frame");
    return staged_query(c, xy, 8, n, 0, us, RQ_PIXELS, hits, prims);
}

int gpuart_hip_gbuffer(gpuart_hip_ctx *c, const float us[4], gpuart_ray_hit *hits, int32_t *prims) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "gbuffer: no scene uploaded");
    if (!c->frame.W) return fail(GPUART_HIP_ERR_ARG, "gbuffer: no frame size set");
    if (!c->have_camera) return fail(GPUART_HIP_ERR_ARG, "gbuffer: no camera set");
    if (!hits) return fail(GPUART_HIP_ERR_ARG, "gbuffer: hits is NULL");
    if ((uintptr_t)hits % 16 || (uintptr_t)prims % 4) return fail(GPUART_HIP_ERR_ARG, "gbuffer: misaligned pointer (hits needs 16 bytes, prims 4)");
    const size_t n = c->plan.tile_pixels;
    if (n == 0) return 0;  // an empty share
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "gbuffer: the tile exceeds GPUART_HIP_MAX_RAYS pixels");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->d_tile_xy) {  // the table of the tile's frame pixels, once per tile (realloc_tile drops it)
        const Frame &f = c->frame;
        std::vector<uint2> xy(n);
        for (uint32_t ly = 0; ly < f.th; ly++) {
            const uint32_t fy = f.y0 + (ly / f.band_rows) * f.band_stride + ly % f.band_rows;
            for (uint32_t lx = 0; lx < f.tw; lx++) xy[(size_t)ly * f.tw + lx] = make_uint2(f.x0 + lx, fy);
        }
        HIP_TRY(hipMalloc(&c->d_tile_xy, n * sizeof(uint2)));
        HIP_TRY(hipMemcpyAsync(c->d_tile_xy, xy.data(), n * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (xy is freed on return)
    }
    RayQuery q = make_query(n, 0, us);
    q.xy = c->d_tile_xy;
    q.hits = (float4 *)hits;
    q.prims = prims;
    return launch_ray_query(c, q, RQ_PIXELS);
}

int gpuart_hip_gbuffer_scaled(gpuart_hip_ctx *c, uint32_t scale, const float us[4], gpuart_ray_hit *hits, int32_t *prims) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    if (scale < 2 || scale > 4) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: scale = " + std::to_string(scale) + " is not in 2..4");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: no scene uploaded");
    if (!c->frame.W) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: no frame size set");
    if (!c->have_camera) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: no camera set");
    if (!hits || !prims) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: hits or prims is NULL");
    if ((uintptr_t)hits % 16 || (uintptr_t)prims % 4)
        return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: misaligned pointer (hits needs 16 bytes, prims 4)");
    const Frame &lo = c->frame;
    if (lo.th > lo.band_rows && lo.band_stride != lo.band_rows)
        return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: the share is interleaved (its scaled tile would be no rectangle)");
    if ((uint64_t)lo.W * scale > 65536 || (uint64_t)lo.H * scale > 65536)
        return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: a side of the scaled frame exceeds 65536");
    const uint64_t n = (uint64_t)c->plan.tile_pixels * scale * scale;
    if (n > GPUART_HIP_MAX_RAYS) return fail(GPUART_HIP_ERR_ARG, "gbuffer_scaled: the scaled tile exceeds GPUART_HIP_MAX_RAYS pixels");
    if (n == 0) return 0;  // an empty share
    HIP_TRY(hipSetDevice(c->device));
    // the frame the context would have after a resize to scale*W x scale*H and a tile of (scale*x0, scale*y0, scale*tw, scale*th): a copy,
    // the context's own stays as it is
    Frame f = lo;
    f.W = lo.W * scale; f.H = lo.H * scale;
    f.x0 = lo.x0 * scale; f.y0 = lo.y0 * scale; f.tw = lo.tw * scale; f.th = lo.th * scale;
    f.band_rows = f.band_stride = f.th;
    f.tile_order = nullptr; f.tile_cost = nullptr;
    update_uv(f);
    if (!c->d_scaled_xy || c->scaled_xy_scale != scale) {  // the table of the scaled tile's frame pixels, once per tile and scale
        if (c->d_scaled_xy) {
            HIP_TRY(hipStreamSynchronize(c->stream));  // (an earlier query may still read it)
            (void)hipFree(c->d_scaled_xy);
            c->d_scaled_xy = nullptr; c->scaled_xy_scale = 0;
        }
        std::vector<uint2> xy((size_t)n);
        for (uint32_t ly = 0; ly < f.th; ly++)
            for (uint32_t lx = 0; lx < f.tw; lx++) xy[(size_t)ly * f.tw + lx] = make_uint2(f.x0 + lx, f.y0 + ly);
        HIP_TRY(hipMalloc(&c->d_scaled_xy, (size_t)n * sizeof(uint2)));
        HIP_TRY(hipMemcpyAsync(c->d_scaled_xy, xy.data(), (size_t)n * sizeof(uint2), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));  // (xy is freed on return)
        c->scaled_xy_scale = scale;
    }
    RayQuery q = make_query((size_t)n, 0, us);
    q.xy = c->d_scaled_xy;
    q.hits = (float4 *)hits;
    q.prims = prims;
    return launch_ray_query(c, q, RQ_PIXELS, &f);
}

int gpuart_hip_trace_subpixel(gpuart_hip_ctx *c, const uint32_t *pixels, size_t n, const float *uv, uint32_t n_sub, float pixelSize,
                              const float us[4], gpuart_ray_hit *hits, int32_t *prims) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    if (!c->have_scene) return fail(GPUART_HIP_ERR_ARG, "subpixel: no scene uploaded");
    if (!c->frame.W) return fail(GPUART_HIP_ERR_ARG, "subpixel: no frame size set");
    if (!c->have_camera) return fail(GPUART_HIP_ERR_ARG, "subpixel: no camera set");
    if (n_sub < 1 || n_sub > GPUART_HIP_MAX_SUBPIXEL)
        return fail(GPUART_HIP_ERR_ARG, "subpixel: n_sub = " + std::to_string(n_sub) + " is not in 1.." + std::to_string(GPUART_HIP_MAX_SUBPIXEL));
    if (!uv) return fail(GPUART_HIP_ERR_ARG, "subpixel: uv is NULL");
    for (uint32_t k = 0; k < 2 * n_sub; k++)
        if (!(uv[k] >= 0.0f && uv[k] < 1.0f)) return fail(GPUART_HIP_ERR_ARG, "subpixel: uv[" + std::to_string(k) + "] is not in [0, 1)");
    if (!(pixelSize >= 0.0f) || pixelSize - pixelSize != 0.0f) return fail(GPUART_HIP_ERR_ARG, "subpixel: pixelSize must be finite and >= 0");
    if (n > GPUART_HIP_MAX_RAYS / n_sub)
        return fail(GPUART_HIP_ERR_ARG, "subpixel: n * n_sub = " + std::to_string(n) + " * " + std::to_string(n_sub) + " exceeds GPUART_HIP_MAX_RAYS");
    if (n == 0) return 0;
    if (!pixels || !hits) return fail(GPUART_HIP_ERR_ARG, "subpixel: pixels or hits is NULL");
    if ((uintptr_t)pixels % 4 || (uintptr_t)hits % 16 || (uintptr_t)prims % 4)
        return fail(GPUART_HIP_ERR_ARG, "subpixel: misaligned pointer (hits needs 16 bytes, pixels and prims 4)");
    if (c->plan.tile_pixels == 0) return fail(GPUART_HIP_ERR_ARG, "subpixel: pixel index outside the tile (an empty share has no pixel)");
    HIP_TRY(hipSetDevice(c->device));
    const size_t total = n * n_sub;
    if (int r = ensure_scratch(c, total * 32)) return r;
    if (!c->d_query_cursor) HIP_TRY(hipMalloc(&c->d_query_cursor, GD_QUERY_WORDS * sizeof(uint32_t)));
    uint32_t *d_bad = c->d_query_cursor + 1;         // (word 0 is k_ray_query's cursor)
    float *d_uv = (float *)(c->d_query_cursor + 16);
    HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), c->stream));
    HIP_TRY(hipMemcpyAsync(d_uv, uv, 2 * n_sub * sizeof(float), hipMemcpyHostToDevice, c->stream));
    // two launches of the query kernel: the first makes the rays (kernels_query.h: sub_n != 0), the second walks them
    RayQuery g = make_query(total, 0, nullptr);
    g.sub_pixels = pixels;
    g.sub_uv = d_uv;
    g.sub_rays = (float4 *)c->d_scratch;
    g.sub_bad = d_bad;
    g.sub_n = (uint32_t)n;
    g.sub_pixel_size = pixelSize;
    if (int r = launch_ray_query(c, g, RQ_RAYS)) return r;
    // the list lives in device memory: the generation range-checks it, and the call waits for that verdict (not for the walk) so that a
    // bad index is an argument error with nothing written, like everywhere else
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (bad) return fail(GPUART_HIP_ERR_ARG, "subpixel: a pixel index lies outside the " + std::to_string(c->frame.tw) + " x " +
                                                 std::to_string(c->frame.th) + " tile");
    RayQuery q = make_query(total, 0, us);
    q.rays = (const float4 *)c->d_scratch;
    q.hits = (float4 *)hits;
    q.prims = prims;
    return launch_ray_query(c, q, RQ_RAYS);
}

// ---- shares and the multi-GPU gather (gather.h) ---------------------------------------------------------------------
int gpuart_hip_set_share(gpuart_hip_ctx *c, const gpuart_tile_geom *g) {
    if (!c || !g || !geom_ok(*g)) return fail(GPUART_HIP_ERR_ARG, "bad share");
    if (g->W != c->frame.W || g->H != c->frame.H) return fail(GPUART_HIP_ERR_ARG, "share of another frame size (call gpuart_hip_resize first)");
    if (g->th) return gpuart_hip_set_tile_interleaved(c, g->x0, g->y0, g->tw, g->th, g->band_rows, g->band_stride);
    // An empty share (more ranks than bands): the context renders nothing — render calls succeed and do nothing — and still
    // takes part in gpuart_hip_gather, where it sends nothing.
    HIP_TRY(hipSetDevice(c->device));
    c->frame.x0 = g->x0; c->frame.y0 = g->y0; c->frame.tw = g->tw; c->frame.th = 0;
    c->frame.band_rows = g->band_rows; c->frame.band_stride = g->band_stride;
    int r = realloc_tile(c);
    c->empty_share = r == 0;
    return r;
}

int gpuart_hip_get_share(gpuart_hip_ctx *c, gpuart_tile_geom *g) {
    if (!c || !g || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
    g->W = c->frame.W; g->H = c->frame.H; g->x0 = c->frame.x0; g->y0 = c->frame.y0; g->tw = c->frame.tw; g->th = c->frame.th;
    g->band_rows = c->frame.band_rows; g->band_stride = c->frame.band_stride;
    return 0;
}

#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t e_ = (expr);                                                                       \
        if (e_ != ncclSuccess)                                                                          \
            return fail(GPUART_HIP_ERR_DEVICE, std::string(#expr) + ": " + rccl()->GetErrorString(e_)); \
    } while (0)

static int need_rccl() {
    Rccl *r = rccl();
    if (!r->err.empty()) return fail(GPUART_HIP_ERR_DEVICE, r->err);
    return 0;
}

int gpuart_hip_comm_unique_id(void *id128) {
    if (!id128) return fail(GPUART_HIP_ERR_ARG, "id == NULL");
    int r = need_rccl();
    if (r) return r;
    static_assert(sizeof(ncclUniqueId) == GPUART_HIP_UNIQUE_ID_BYTES, "unique id size");
    NCCL_TRY(rccl()->GetUniqueId((ncclUniqueId *)id128));
    return 0;
}

/// An RCCL-facing entry point in a process where an earlier RCCL call never returned (bounded.h): refused at once.
static int comm_layer_ok() {
    if (bounded_ns::stuck().load())
        return fail(GPUART_HIP_ERR_TIMEOUT, "the communicator layer of this process is out of service: " + bounded_ns::stuck_in() + " never returned");
    return 0;
}

/// A bounded RCCL call's outcome as this library's status (the message is set on the CALLING thread).
static int comm_outcome(const bounded_ns::Outcome &o, const char *what) {
    if (o.timed_out) return fail(GPUART_HIP_ERR_TIMEOUT, o.detail);
    if (o.rc != 0) return fail(GPUART_HIP_ERR_DEVICE, std::string(what) + ": " + (o.detail.empty() ? std::string("failed") : o.detail));
    return 0;
}

/// Leaves the context's communicator. ncclCommDestroy waits for the communicator's outstanding work and, for a communicator of
/// several ranks, for its proxy threads — it is one of the calls that had no bound: it runs under bounded() now.
/// A destroy that does not return leaves the handle alone (the context forgets it) and marks the layer stuck.
static int comm_drop(gpuart_hip_ctx *c) {
    int r = 0;
    if (c->comm && c->comm_owned && !bounded_ns::stuck().load()) {
        const ncclComm_t comm = c->comm;
        const int device = c->device;
        const bounded_ns::Outcome o = bounded_ns::bounded("ncclCommDestroy", bounded_ns::comm_timeout_ms(), [comm, device](std::string &d) {
            (void)hipSetDevice(device);
            const ncclResult_t e = rccl()->CommDestroy(comm);
            if (e != ncclSuccess) d = rccl()->GetErrorString(e);
            return (int)e;
        });
        r = comm_outcome(o, "ncclCommDestroy");
    }
    c->comm = nullptr; c->comm_owned = false; c->comm_nranks = 0; c->comm_rank = 0; c->comm_group = 0;
    return r;
}

/// Identity of a communicator for gpuart_hip_gather_all: process-unique serials for _comm_init_all / _comm_attach, a hash of the
/// unique id for _comm_init (the same on every rank that was given that id).
static uint64_t next_comm_group() {
    static std::atomic<uint64_t> serial{1};
    return serial.fetch_add(1);
}

int gpuart_hip_comm_init(gpuart_hip_ctx *c, int nranks, int rank, const void *id128) {
    if (!c || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    int r = comm_layer_ok();
    if (r || (r = need_rccl())) return r;
    HIP_TRY(hipSetDevice(c->device));
    if ((r = comm_drop(c))) return r;
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    // ncclCommInitRank returns when ALL nranks ranks have called it with this id: a rank that never starts leaves the others here
    auto made = std::make_shared<ncclComm_t>(nullptr);
    const int device = c->device;
    const bounded_ns::Outcome o = bounded_ns::bounded("ncclCommInitRank", bounded_ns::comm_timeout_ms(), [made, nranks, id, rank, device](std::string &d) {
        (void)hipSetDevice(device);
        const ncclResult_t e = rccl()->CommInitRank(made.get(), nranks, id, rank);
        if (e != ncclSuccess) d = rccl()->GetErrorString(e);
        return (int)e;
    });
    if ((r = comm_outcome(o, "ncclCommInitRank"))) return r;
    c->comm = *made;
    c->comm_owned = true; c->comm_nranks = nranks; c->comm_rank = rank;
    uint64_t h = 1469598103934665603ull;  // FNV-1a of the 128-byte id; bit 63 set: never a serial
    for (size_t k = 0; k < sizeof id; k++) h = (h ^ ((const unsigned char *)&id)[k]) * 1099511628211ull;
    c->comm_group = h | (1ull << 63);
    return 0;
}

int gpuart_hip_comm_attach(gpuart_hip_ctx *c, void *nccl_comm, int nranks, int rank) {
    if (!c || !nccl_comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    int r = comm_layer_ok();
    if (r || (r = need_rccl())) return r;
    if ((r = comm_drop(c))) return r;
    c->comm = (ncclComm_t)nccl_comm; c->comm_owned = false; c->comm_nranks = nranks; c->comm_rank = rank;
    c->comm_group = 0;  // the caller's communicator: which handles belong together is the caller's to know
    return 0;
}

int gpuart_hip_comm_init_all(gpuart_hip_ctx *const *ctxs, int n) {
    if (!ctxs || n < 1) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    int r = comm_layer_ok();
    if (r || (r = need_rccl())) return r;
    // RCCL refuses two ranks of a communicator on one device. An in-process stand-in (GPUART_HIP_RCCL_LIBRARY, tests/stubs/rccl_stub.cpp)
    // does not: with GPUART_HIP_TEST_SHARED_DEVICE=1 beside it the N > 1 gather runs on a box with one GPU. Test-only, both variables.
    const char *shared = getenv("GPUART_HIP_TEST_SHARED_DEVICE");
    const bool one_device_ok = getenv("GPUART_HIP_RCCL_LIBRARY") && shared && shared[0] == '1';
    std::vector<int> devs(n);
    for (int k = 0; k < n; k++) {
        if (!ctxs[k]) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
        devs[k] = ctxs[k]->device;
        for (int m = 0; m < k; m++) {
            if (ctxs[m] == ctxs[k]) return fail(GPUART_HIP_ERR_ARG, "one context given twice");
            if (devs[m] == devs[k] && !one_device_ok) return fail(GPUART_HIP_ERR_ARG, "two contexts of one communicator on the same device");
        }
    }
    // a context leaves its previous communicator first (with its work drained: nothing of that communicator is in flight)
    for (int k = 0; k < n; k++) {
        if (!ctxs[k]->comm) continue;
        HIP_TRY(hipSetDevice(ctxs[k]->device));
        if ((r = drain(ctxs[k]))) return r;
        if ((r = comm_drop(ctxs[k]))) return r;
    }
    // ncclCommInitAll bootstraps n ranks inside this process (one thread per rank inside RCCL, topology discovery, ring set-up):
    // it has no timeout of its own. Under bounded(): the handles live in a block the parked thread shares.
    auto made = std::make_shared<std::vector<ncclComm_t>>((size_t)n, nullptr);
    const bounded_ns::Outcome o = bounded_ns::bounded("ncclCommInitAll", bounded_ns::comm_timeout_ms(), [made, devs, n](std::string &d) {
        const ncclResult_t e = rccl()->CommInitAll(made->data(), n, devs.data());
        if (e != ncclSuccess) d = rccl()->GetErrorString(e);
        return (int)e;
    });
    if ((r = comm_outcome(o, "ncclCommInitAll"))) return r;
    const uint64_t group = next_comm_group();
    for (int k = 0; k < n; k++) {
        ctxs[k]->comm = (*made)[(size_t)k]; ctxs[k]->comm_owned = true; ctxs[k]->comm_nranks = n; ctxs[k]->comm_rank = k;
        ctxs[k]->comm_group = group;
    }
    return 0;
}

int gpuart_hip_comm_destroy(gpuart_hip_ctx *c) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    if (c->comm) {
        HIP_TRY(hipSetDevice(c->device));
        // (a context whose gather gave up may still have that gather's transfers queued: the wait for them is bounded too)
        int r = c->abandoned ? wait_stream(c, c->gather_timeout_ms, "gpuart_hip_comm_destroy: work queued before the communicator can go") : 0;
        if (!r) r = drain(c);
        if (r) return r;
        return comm_drop(c);
    }
    return 0;
}

extern "C++" {
namespace {
int ensure_pixels(float4 *&buf, size_t &have, size_t want) {
    if (have >= want && buf) return 0;
    if (buf) { (void)hipFree(buf); buf = nullptr; have = 0; }
    HIP_TRY(hipMalloc(&buf, std::max<size_t>(1, want) * sizeof(float4)));
    have = want;
    return 0;
}

/// What every rank tells the others before anything is sent: its share and whether it is able to take part.
struct GatherHello {
    gpuart_tile_geom g;
    uint32_t status;  ///< 0: ready; else the rank could not prepare (out of memory, bad arguments): nobody posts a transfer
    uint32_t which, root, pad;
};
static_assert(sizeof(GatherHello) == 48, "all-gathered as 12 words per rank");

/// Everything of a gather that can fail on THIS rank alone, done before the ranks commit to a transfer: pending passes are
/// launched, the (divided) tile is exported into the rank's send buffer, and the root's staging area — one frame, whatever the
/// shares turn out to be — exists. The verdict travels with the share (GatherHello::status), so that a rank that cannot go on
/// makes every rank return an error instead of leaving its peers blocked in a receive.
int gather_prepare(gpuart_hip_ctx *c, int which, float divide_by, int root, GatherHello &h) {
    int r;
    memset(&h, 0, sizeof h);
    h.which = (uint32_t)which; h.root = (uint32_t)root;
    if ((r = gpuart_hip_get_share(c, &h.g))) return r;
    if ((r = gpuart_hip_flush(c))) return r;
    if (c->plan.tile_pixels) {
        if ((r = ensure_pixels(c->d_send, c->send_pixels, c->plan.tile_pixels))) return r;
        if ((r = gpuart_hip_export(c, which, c->d_send, divide_by))) return r;
    }
    if (c->comm_rank == root && (r = ensure_pixels(c->d_stage, c->stage_pixels, (size_t)c->frame.W * c->frame.H))) return r;
    return 0;
}

/// The shares of all ranks must be full-width rows of one frame that cover every row exactly once: rows nobody renders would
/// stay uninitialised in the root's frame, rows rendered twice would depend on the order of the transfers.
int check_shares(const std::vector<GatherHello> &all, int which, int root) {
    const gpuart_tile_geom &g0 = all[0].g;
    // a rank that could not prepare says so before its (zeroed) share is looked at: rank 0's would otherwise read as a bad frame
    for (size_t k = 0; k < all.size(); k++)
        if (all[k].status) return fail(GPUART_HIP_ERR_DEVICE, "gather: rank " + std::to_string(k) + " could not prepare its share (its own call reports why)");
    // (before anything is sized by it: a share table is other ranks' — or a caller's — data)
    if (!geom_ok(g0) || g0.H > 65536 || g0.W > 65536) return fail(GPUART_HIP_ERR_ARG, "gather: inconsistent shares (frame of rank 0)");
    std::vector<uint8_t> cover(g0.H, 0);
    for (size_t k = 0; k < all.size(); k++) {
        const gpuart_tile_geom &g = all[k].g;
        if ((int)all[k].which != which || (int)all[k].root != root) return fail(GPUART_HIP_ERR_ARG, "gather: the ranks disagree about buffer or root");
        if (!geom_ok(g) || g.W != g0.W || g.H != g0.H) return fail(GPUART_HIP_ERR_ARG, "gather: inconsistent shares");
        if (g.th && (g.x0 != 0 || g.tw != g.W)) return fail(GPUART_HIP_ERR_ARG, "gather: shares must be full-width rows");
        for (uint32_t ly = 0; ly < g.th; ly++) {
            uint8_t &n = cover[gpuart_hip_frame_row(&g, ly)];
            if (n) return fail(GPUART_HIP_ERR_ARG, "gather: shares overlap (a frame row belongs to two ranks)");
            n = 1;
        }
    }
    for (uint32_t y = 0; y < g0.H; y++)
        if (!cover[y]) return fail(GPUART_HIP_ERR_ARG, "gather: frame row " + std::to_string(y) + " belongs to no rank");
    return 0;
}

/// What one rank's transfers need, by value: the closure that posts them may outlive the caller's frame (bounded.h).
struct GatherRank {
    int device, rank;
    ncclComm_t comm;
    hipStream_t stream;
    float4 *send, *stage;
    size_t tile_pixels;
};
GatherRank gather_rank(const gpuart_hip_ctx *c) { return GatherRank{c->device, c->comm_rank, c->comm, c->stream, c->d_send, c->d_stage, c->plan.tile_pixels}; }

/// One rank's transfers, between ncclGroupStart and ncclGroupEnd; nothing in here can fail for a reason of this rank alone
/// (buffers exist, shares are validated): a peer posts its send, the root its receives into the staging area.
ncclResult_t gather_post(const GatherRank &g, int root, const std::vector<GatherHello> &all) {
    const int n = (int)all.size(), me = g.rank;
    if (me != root) {
        if (!g.tile_pixels) return ncclSuccess;  // an empty share (more ranks than bands)
        return rccl()->Send(g.send, g.tile_pixels * 4, ncclFloat, root, g.comm, g.stream);
    }
    size_t off = 0;
    for (int k = 0; k < n; k++) {
        const size_t cnt = (size_t)all[k].g.tw * all[k].g.th;
        if (k != me && cnt) {
            const ncclResult_t e = rccl()->Recv(g.stage + off, cnt * 4, ncclFloat, k, g.comm, g.stream);
            if (e != ncclSuccess) return e;
        }
        off += cnt;
    }
    return ncclSuccess;
}

/// The group of transfers of the given ranks of this process (one for gpuart_hip_gather, all of them for _gather_all), posted
/// from ONE thread — RCCL's group state is per thread — under bounded(): ncclGroupEnd connects peers that have not talked before
/// and returns when that is done, i.e. when every peer has reached its own group; it has no timeout of its own.
int gather_transfers(const std::vector<GatherRank> &ranks, int root, const std::vector<GatherHello> &all) {
    const bounded_ns::Outcome o = bounded_ns::bounded("ncclGroupStart .. ncclGroupEnd (the gather's send / recv group)", bounded_ns::comm_timeout_ms(),
                                                      [ranks, root, all](std::string &d) {
        ncclResult_t e = rccl()->GroupStart();
        if (e != ncclSuccess) { d = std::string("ncclGroupStart: ") + rccl()->GetErrorString(e); return (int)e; }
        ncclResult_t pe = ncclSuccess;
        for (size_t k = 0; k < ranks.size() && pe == ncclSuccess; k++) {
            if (hipSetDevice(ranks[k].device) != hipSuccess) { pe = ncclUnhandledCudaError; break; }
            pe = gather_post(ranks[k], root, all);
        }
        const ncclResult_t ge = rccl()->GroupEnd();
        if (pe != ncclSuccess) { d = std::string("posting the transfers: ") + rccl()->GetErrorString(pe); return (int)pe; }
        if (ge != ncclSuccess) { d = std::string("ncclGroupEnd: ") + rccl()->GetErrorString(ge); return (int)ge; }
        return 0;
    });
    return comm_outcome(o, "gather");
}

/// After the group: the root scatters every share's rows into the full frame (its own straight from its send buffer).
int gather_place(gpuart_hip_ctx *c, const std::vector<GatherHello> &all, float4 *full) {
    size_t off = 0;
    for (size_t k = 0; k < all.size(); k++) {
        const gpuart_tile_geom &g = all[k].g;
        const size_t cnt = (size_t)g.tw * g.th;
        const float4 *src = (int)k == c->comm_rank ? c->d_send : c->d_stage + off;
        if (cnt) GD_LEDGER(c, k_scatter_rows);
        if (cnt) k_scatter_rows<<<dim3((unsigned)((cnt + 255) / 256)), 256, 0, c->stream>>>(g, src, full);
        off += cnt;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace
}  // extern "C++"

#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_share_table(const gpuart_tile_geom *shares, const uint32_t *status, int n, int which, int root) {
    if (!shares || n < 1 || n > 1024) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    try {
        std::vector<GatherHello> all((size_t)n);
        for (int k = 0; k < n; k++) {
            memset(&all[(size_t)k], 0, sizeof(GatherHello));
            all[(size_t)k].g = shares[k];
            all[(size_t)k].status = status ? status[k] : 0u;
            all[(size_t)k].which = (uint32_t)which; all[(size_t)k].root = (uint32_t)root;
        }
        return check_shares(all, which, root);
    } catch (const std::exception &e) {  // no exception crosses the C ABI
        return fail(GPUART_HIP_ERR_ARG, std::string("share table: ") + e.what());
    }
}
#endif

int gpuart_hip_comm_library(char *path, size_t size) {
    if (!path || size < 2) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    int r = need_rccl();
    if (r) return r;
    Dl_info di;
    memset(&di, 0, sizeof di);
    if (!dladdr((void *)rccl()->CommInitRank, &di) || !di.dli_fname) return fail(GPUART_HIP_ERR_DEVICE, "dladdr(ncclCommInitRank) failed");
    snprintf(path, size, "%s", di.dli_fname);
    return 0;
}

int gpuart_hip_comm_info(gpuart_hip_ctx *c, int *nranks, int *rank) {
    if (!c || !c->comm) return fail(GPUART_HIP_ERR_ARG, "no communicator (gpuart_hip_comm_init)");
    int r = need_rccl();
    if (r) return r;
    int n = 0, me = 0;
    NCCL_TRY(rccl()->CommCount(c->comm, &n));
    NCCL_TRY(rccl()->CommUserRank(c->comm, &me));
    if (nranks) *nranks = n;
    if (rank) *rank = me;
    return 0;
}

int gpuart_hip_wait(gpuart_hip_ctx *c, uint32_t timeout_ms) {
    if (!c) return fail(GPUART_HIP_ERR_ARG, "ctx == NULL");
    HIP_TRY(hipSetDevice(c->device));
    { int fr = gpuart_hip_flush(c); if (fr) return fr; }
    // the pass lanes' work reaches the primary stream through their events (accumulation in pass order), so the primary stream
    // is the last to finish
    int r = wait_stream(c, timeout_ms, "gpuart_hip_wait");
    return r ? r : drain(c);
}

int gpuart_hip_gather(gpuart_hip_ctx *c, int which, float divide_by, int root, void *full_frame_device) {
    if (!c || !c->comm) return fail(GPUART_HIP_ERR_ARG, "no communicator (gpuart_hip_comm_init)");
    if (c->comm_nranks > 1024) return fail(GPUART_HIP_ERR_ARG, "more than 1024 ranks");
    HIP_TRY(hipSetDevice(c->device));
    const int n = c->comm_nranks;
    // 1. everything that can fail here alone; the verdict is part of what the ranks exchange
    GatherHello own;
    int mine = 0;
    if (root < 0 || root >= n || (which != 0 && which != 1)) mine = fail(GPUART_HIP_ERR_ARG, "bad argument");
    else if (c->comm_rank == root && !full_frame_device) mine = fail(GPUART_HIP_ERR_ARG, "the root needs a frame buffer");
    else mine = gather_prepare(c, which, divide_by, root, own);
    const std::string my_error = mine ? g_last_error : std::string();
    if (mine) { memset(&own, 0, sizeof own); own.which = (uint32_t)which; own.root = (uint32_t)root; }
    own.status = mine ? 1u : 0u;
    if (!c->d_hello && hipMalloc(&c->d_hello, (size_t)(1 + 1024) * sizeof(GatherHello)) != hipSuccess)
        return fail(GPUART_HIP_ERR_DEVICE, "gather: no device memory for the share table (the other ranks are left waiting: nothing can be told to them)");
    if (!c->h_hello && hipHostMalloc(&c->h_hello, (size_t)(1 + 1024) * sizeof(GatherHello), hipHostMallocDefault) != hipSuccess)
        return fail(GPUART_HIP_ERR_DEVICE, "gather: no pinned host memory for the share table (the other ranks are left waiting: nothing can be told to them)");
    // 2. everybody's share and status, through the communicator itself (12 words per rank). Both host ends of the two copies are
    //    the context's pinned table: the copies are queued, not performed, by these calls — the wait below is the only place this
    //    rank can block, and it is bounded —, and a call that gives up leaves no queued copy pointing at its own stack or heap.
    GatherHello *d = (GatherHello *)c->d_hello, *hh = (GatherHello *)c->h_hello;
    hh[0] = own;
    int r;
    if ((r = comm_layer_ok())) return r;
    HIP_TRY(hipMemcpyAsync(d, hh, sizeof own, hipMemcpyHostToDevice, c->stream));
    {   // (enqueueing a collective may itself wait — the first use of a channel —: under bounded(), bounded.h)
        const GatherRank me = gather_rank(c);
        const bounded_ns::Outcome o = bounded_ns::bounded("ncclAllGather (share exchange)", bounded_ns::comm_timeout_ms(), [me, d](std::string &dt) {
            (void)hipSetDevice(me.device);
            const ncclResult_t e = rccl()->AllGather(d, d + 1, sizeof(GatherHello) / 4, ncclUint32, me.comm, me.stream);
            if (e != ncclSuccess) dt = rccl()->GetErrorString(e);
            return (int)e;
        });
        if ((r = comm_outcome(o, "ncclAllGather"))) return r;
    }
    HIP_TRY(hipMemcpyAsync(hh + 1, d + 1, (size_t)n * sizeof own, hipMemcpyDeviceToHost, c->stream));
    if ((r = wait_stream(c, c->gather_timeout_ms, "gather: exchange of the shares"))) return r;
    if (mine) return fail(mine, my_error);
    std::vector<GatherHello> all(hh + 1, hh + 1 + n);
    // 3. the same table on every rank: the same verdict on every rank
    if ((r = check_shares(all, which, root))) return r;
    // 4. the transfers
    if ((r = gather_transfers({gather_rank(c)}, root, all))) return r;
    if (c->comm_rank == root) return gather_place(c, all, (float4 *)full_frame_device);
    return 0;
}

int gpuart_hip_gather_all(gpuart_hip_ctx *const *ctxs, int n, int which, float divide_by, int root, void *full_frame_device) {
    if (!ctxs || n < 1 || root < 0 || root >= n || !full_frame_device || (which != 0 && which != 1)) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    int r;
    std::vector<GatherHello> all((size_t)n);
    // one thread drives every rank: all local preparation first, transfers only when every rank is ready
    for (int k = 0; k < n; k++) {
        if (!ctxs[k] || !ctxs[k]->comm || ctxs[k]->comm_nranks != n || ctxs[k]->comm_rank != k || ctxs[k]->comm_group != ctxs[0]->comm_group)
            return fail(GPUART_HIP_ERR_NO_COMM, "contexts are not the ranks 0..n-1 of one communicator (gpuart_hip_comm_init_all)");
    }
    for (int k = 0; k < n; k++) {
        HIP_TRY(hipSetDevice(ctxs[k]->device));
        if ((r = gather_prepare(ctxs[k], which, divide_by, root, all[(size_t)k]))) return r;
    }
    if ((r = check_shares(all, which, root))) return r;
    if ((r = comm_layer_ok())) return r;
    std::vector<GatherRank> ranks;
    for (int k = 0; k < n; k++) ranks.push_back(gather_rank(ctxs[k]));
    if ((r = gather_transfers(ranks, root, all))) return r;
    HIP_TRY(hipSetDevice(ctxs[root]->device));
    return gather_place(ctxs[root], all, (float4 *)full_frame_device);
}

int gpuart_hip_gather_all_read(gpuart_hip_ctx *const *ctxs, int n, int which, float divide_by, int root, float *full_frame_host) {
    if (!ctxs || n < 1 || root < 0 || root >= n || !ctxs[root] || !full_frame_host) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    gpuart_hip_ctx *c = ctxs[root];
    const size_t bytes = (size_t)c->frame.W * c->frame.H * sizeof(float4);
    HIP_TRY(hipSetDevice(c->device));
    int r = ensure_scratch(c, bytes);
    if (r) return r;
    if ((r = gpuart_hip_gather_all(ctxs, n, which, divide_by, root, c->d_scratch))) return r;
    HIP_TRY(hipSetDevice(c->device));
    // The copy is queued behind the root's receives: waiting for it is waiting for every peer's rows. Bounded like the exchange of
    // gpuart_hip_gather (this wait was a plain hipStreamSynchronize until round 5 — one of the three unbounded waits on the path
    // of the gpuart_cli child that once did not end, profiles/r05/stall_path.txt). The device-to-host copy goes into PINNED memory
    // owned by the context: into the caller's pageable buffer hipMemcpyAsync is not asynchronous — the call itself would wait for
    // the stream, ahead of the bounded wait (the first version of this fix did exactly that; the test that holds the stream caught
    // it) — and a call that gives up leaves no queued copy pointing at memory the caller may free.
    if (c->h_frame_bytes < bytes) {
        // (hipHostFree waits for the device: if an earlier read-out of this context gave up, its copy into h_frame may still be queued
        // behind the stream that held it — that wait gets its bound first, and the buffer stays if the stream is still held)
        if (c->h_frame && c->abandoned && (r = wait_stream(c, c->gather_timeout_ms, "gather: an abandoned read-back still owns the pinned frame buffer"))) return r;
        if (c->h_frame) { (void)hipHostFree(c->h_frame); c->h_frame = nullptr; c->h_frame_bytes = 0; }
        if (hipHostMalloc(&c->h_frame, bytes, hipHostMallocDefault) != hipSuccess) { c->h_frame = nullptr; return fail(GPUART_HIP_ERR_DEVICE, "gather: no pinned host memory for the frame"); }
        c->h_frame_bytes = bytes;
    }
    HIP_TRY(hipMemcpyAsync(c->h_frame, c->d_scratch, bytes, hipMemcpyDeviceToHost, c->stream));
    if ((r = wait_stream(c, c->gather_timeout_ms, "gather: the peers' rows and the read-back of the frame"))) return r;
    memcpy(full_frame_host, c->h_frame, bytes);
    return 0;
}

// ---- the hooks that need no device (include/gpuart_hip_test.h): what gpuart_hip_upload_bvh decides about a tree -------------------
#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_tree_class(const float *quads, size_t nquads, uint32_t *flags) {
    if (!quads || !nquads || !flags) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    try {
        Converter cv;
        cv.q = quads; cv.nq = nquads;
        Converter::Child root;
        if (!cv.convert(root, 1)) return fail(GPUART_HIP_ERR_ARG, "malformed compiled BVH: " + cv.err);
        *flags = (cv.irregular ? 1u : 0u) | (cv.disorderly ? 2u : 0u) | (cv.subnormal ? 4u : 0u) | (cv.type_mask << 8);
        return 0;
    } catch (const std::exception &e) {
        return fail(GPUART_HIP_ERR_ARG, std::string("tree: ") + e.what());
    }
}

int gpuart_hip_test_tree_slack(const float *quads, size_t nquads, float *slack) {
    if (!quads || !nquads || !slack) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    try {
        Converter cv;
        cv.q = quads; cv.nq = nquads;
        Converter::Child root;
        if (!cv.convert(root, 1)) return fail(GPUART_HIP_ERR_ARG, "malformed compiled BVH: " + cv.err);
        *slack = tree_slack(cv, root);
        return 0;
    } catch (const std::exception &e) {
        return fail(GPUART_HIP_ERR_ARG, std::string("tree: ") + e.what());
    }
}

int gpuart_hip_test_convert(const float *quads, size_t nquads, uint32_t threads, uint32_t top_depth, float *recs, size_t recs_cap,
                            float *prims, size_t prims_cap, uint32_t info[8], float root_box[6]) {
    if (!quads || !nquads || !info || !root_box || (!recs && recs_cap) || (!prims && prims_cap)) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    try {
        Converter cv;
        cv.q = quads; cv.nq = nquads;
        cv.top_depth = top_depth;
        Converter::Child root;
        if (!cv.convert(root, std::min(64u, std::max(1u, threads)))) return fail(GPUART_HIP_ERR_ARG, "malformed compiled BVH: " + cv.err);
        const size_t n_recs = cv.recs.size() / 4, n_prims = cv.prims.size() / 3;
        if ((recs || prims) && (recs_cap < n_recs || prims_cap < n_prims)) return fail(GPUART_HIP_ERR_ARG, "convert: the arrays do not fit");
        if (recs && n_recs) memcpy(recs, cv.recs.data(), n_recs * 64);
        if (prims && n_prims) memcpy(prims, cv.prims.data(), n_prims * 48);
        info[0] = (uint32_t)n_recs; info[1] = (uint32_t)n_prims; info[2] = root.ref; info[3] = (uint32_t)cv.num_nodes;
        info[4] = cv.max_depth; info[5] = cv.type_mask;
        info[6] = (cv.irregular ? 1u : 0u) | (cv.disorderly ? 2u : 0u) | (cv.subnormal ? 4u : 0u); info[7] = 0;
        memcpy(root_box, root.bmin, 12); memcpy(root_box + 3, root.bmax, 12);
        return 0;
    } catch (const std::exception &e) {
        return fail(GPUART_HIP_ERR_ARG, std::string("tree: ") + e.what());
    }
}

// ---- kernel choice hook: the rule the launch sites take their instantiation from, asked without a device
int gpuart_hip_test_kernel_choice(uint32_t type_mask, uint32_t exact_boxes, uint32_t ref_order, uint32_t lean_kernels, int mode, int entry,
                                  uint32_t choice[3]) {
    if (!choice || type_mask > 15 || mode < 0 || mode > 5 || entry < KC_DIRECT || entry > KC_QUERY) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    const int k = kernel_choice(type_mask, exact_boxes != 0, ref_order != 0, lean_kernels != 0, mode, entry);
    choice[0] = (uint32_t)(k & (KC_COUNT - 1)); choice[1] = (k & KC_COUNT) ? 1u : 0u; choice[2] = (k & KC_REFWORK) ? 1u : 0u;
    return 0;
}

// ---- run planner hook: the planner of the context, driven without a device (include/gpuart_hip.h) ---------------------
/// Both planner hooks; `active_ops`: op 7 exists and a record's second word is the run's slots, not the tile's.
static int planner_hook(const uint32_t cfg[8], const uint32_t *ops, int n_ops, uint32_t *runs, int max_runs, bool active_ops) {
    if (!cfg || (!ops && n_ops) || n_ops < 0 || (!runs && max_runs) || max_runs < 0) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    RunPlanner p;
    p.batch_limit = MAX_BATCH;
    if (cfg[0]) p.batch_limit = std::min<uint32_t>(cfg[0], MAX_BATCH);
    if (cfg[1]) p.lanes_total = std::min<uint32_t>(cfg[1], 32);
    if (cfg[2]) p.batch_paths = (size_t)cfg[2] << 20;
    if (cfg[3]) p.min_run_paths = (size_t)cfg[3] << 10;
    if (cfg[4]) p.small_paths = cfg[4] == 0xffffffffu ? 0 : (size_t)cfg[4] << 10;
    if (cfg[5]) p.lane_budget = (size_t)cfg[5] << 20;
    if (cfg[6]) p.plan_run_factor = cfg[6] / 100.0;
    uint32_t W = 0, H = 0, alloc_fails = 0;
    int n_runs = 0;
    auto record = [&](int op, size_t count) {
        if (n_runs < max_runs) {
            uint32_t *o = runs + 6 * (size_t)n_runs;
            o[0] = (uint32_t)op; o[1] = active_ops ? (uint32_t)p.slots() : p.n_slots; o[2] = p.max_batch; o[3] = (uint32_t)count;
            o[4] = p.uses_run_kernel(count) ? 1u : 0u; o[5] = (uint32_t)p.pending;
        }
        n_runs++;
    };
    auto flush = [&](int op) { for (size_t count : p.on_flush()) record(op, count); };
    auto tile = [&](int op, uint32_t tw, uint32_t th) -> int {
        flush(op);  // realloc_tile: what is pending belongs to the old tile
        const size_t n = (size_t)((tw + 7) / 8) * ((th + 7) / 8) * 64;
        if (n > 0xfffffff0ull) return GPUART_HIP_ERR_ARG;
        p.set_tile((uint32_t)n, (size_t)tw * th);
        for (; alloc_fails; alloc_fails--)
            if (!p.shrink()) return GPUART_HIP_ERR_DEVICE;
        return 0;
    };
    for (int k = 0; k < n_ops; k++) {
        const uint32_t op = ops[3 * k], a = ops[3 * k + 1], b = ops[3 * k + 2];
        int r = 0;
        switch (op) {
        case 0:
            if (!a || !b || a > 65536 || b > 65536) return fail(GPUART_HIP_ERR_ARG, "bad frame size");
            W = a; H = b;
            r = tile(k, W, H);
            break;
        case 1: {
            gpuart_tile_geom g;
            if (!W || gpuart_hip_share_of_rank(W, H, (int)a, (int)b, 8, &g) || !g.th) return fail(GPUART_HIP_ERR_ARG, "bad share");
            r = tile(k, g.tw, g.th);
            break;
        }
        case 2: p.set_plan(a); break;
        case 3:
            if (a > 5) return fail(GPUART_HIP_ERR_ARG, "bad mode");
            flush(k); p.mode = (int)a; p.plan();
            break;
        case 4:
            if (!p.n_slots) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
            for (uint32_t i = 0; i < a; i++) {
                if (p.mode == 2) continue;  // the megakernel renders a pass at once: nothing is collected
                if (const size_t count = p.on_pass()) record(k, count);
            }
            break;
        case 5: flush(k); break;
        case 6: alloc_fails = a; break;
        case 7:  // gpuart_hip_set_active_blocks with a list of `a` blocks (0: dropped; the empty list never reaches the planner)
            if (!active_ops) return fail(GPUART_HIP_ERR_ARG, "unknown planner op");
            if (!p.n_slots || a > p.n_slots / 64) return fail(GPUART_HIP_ERR_ARG, "bad active list");
            flush(k); p.set_active(a * 64);
            break;
        default: return fail(GPUART_HIP_ERR_ARG, "unknown planner op");
        }
        if (r) return fail(r, "planner: tile refused");
    }
    return n_runs;
}
int gpuart_hip_test_planner(const uint32_t cfg[8], const uint32_t *ops, int n_ops, uint32_t *runs, int max_runs) {
    return planner_hook(cfg, ops, n_ops, runs, max_runs, false);
}
int gpuart_hip_test_planner_active(const uint32_t cfg[8], const uint32_t *ops, int n_ops, uint32_t *runs, int max_runs) {
    return planner_hook(cfg, ops, n_ops, runs, max_runs, true);
}
#endif

// ---- test hooks ------------------------------------------------------------------------------------
#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), 256, 0, c->stream

#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_random(gpuart_hip_ctx *c, const float *in, int n, float *out) {
    const float *ins[] = {in}; float *outs[] = {out};
    return run_hook(c, n, ins, 1, outs, 1, [&](auto &i, auto &o) { k_test_random<<<GRID1(n)>>>(i[0], n, o[0]); });
}
int gpuart_hip_test_math(gpuart_hip_ctx *c, const float *in, int n, float *out) {
    const float *ins[] = {in}; float *outs[] = {out};
    return run_hook(c, n, ins, 1, outs, 1, [&](auto &i, auto &o) { k_test_math<<<GRID1(n)>>>(i[0], n, o[0]); });
}
int gpuart_hip_test_hemisphere(gpuart_hip_ctx *c, const float *v, const float *ri, int n, float *out) {
    const float *ins[] = {v, ri}; float *outs[] = {out};
    return run_hook(c, n, ins, 2, outs, 1, [&](auto &i, auto &o) { k_test_hemisphere<<<GRID1(n)>>>(i[0], i[1], n, o[0]); });
}
int gpuart_hip_test_inside_cone(gpuart_hip_ctx *c, const float *v, const float *nrm, const float *ri, float ha, int n, float *out) {
    const float *ins[] = {v, nrm, ri}; float *outs[] = {out};
    return run_hook(c, n, ins, 3, outs, 1, [&](auto &i, auto &o) { k_test_inside_cone<<<GRID1(n)>>>(i[0], i[1], i[2], ha, n, o[0]); });
}
int gpuart_hip_test_sky(gpuart_hip_ctx *c, const float *dir, const float sda[4], int n, float *out) {
    if (!sda) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    Float4Arg a; memcpy(a.v, sda, 16);
    const float *ins[] = {dir}; float *outs[] = {out};
    return run_hook(c, n, ins, 1, outs, 1, [&](auto &i, auto &o) { k_test_sky<<<GRID1(n)>>>(i[0], a, n, o[0]); });
}
int gpuart_hip_test_intersect(gpuart_hip_ctx *c, int ptype, const float *rs, const float *rd, const float *quads, int n,
                              float *out0, float *out1) {
    if (ptype < 0 || ptype > 3 || !quads || n < 0) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    // canonical payload (4 quads per sample) -> device records, through the uploader's packer
    std::vector<float4> recs((size_t)n * 3);
    for (int i = 0; i < n; i++) Converter::pack_prim((uint32_t)ptype, quads + 16 * (size_t)i, &recs[3 * (size_t)i]);
    // three record quads are passed as three n x 4 input arrays (de-interleaved), then re-read as records
    std::vector<float> packed((size_t)n * 12);
    memcpy(packed.data(), recs.data(), packed.size() * 4);
    const float *ins[] = {rs, rd, packed.data(), packed.data() + (size_t)n * 4, packed.data() + (size_t)n * 8};
    float *outs[] = {out0, out1};
    // inputs 2,3,4 are contiguous in device scratch, so i[2] addresses all 3n quads
    return run_hook(c, n, ins, 5, outs, 2, [&](auto &i, auto &o) { k_test_intersect<<<GRID1(n)>>>(i[0], i[1], i[2], n, o[0], o[1]); });
}
int gpuart_hip_test_aabb(gpuart_hip_ctx *c, const float *rs, const float *rd, const float *bmin, const float *bmax, int n, float *out) {
    const float *ins[] = {rs, rd, bmin, bmax}; float *outs[] = {out};
    return run_hook(c, n, ins, 4, outs, 1, [&](auto &i, auto &o) { k_test_aabb<<<GRID1(n)>>>(i[0], i[1], i[2], i[3], n, o[0], (int)c->quick_boxes); });
}
int gpuart_hip_test_traverse(gpuart_hip_ctx *c, const float *rs, const float *rd, const float us[4], int n, int any_hit,
                             float *out0, float *out1) {
    if (!c || !c->have_scene || !us) return fail(GPUART_HIP_ERR_ARG, "no scene uploaded");
    if (any_hit == 2 && c->exact_boxes) return fail(GPUART_HIP_ERR_ARG, "a tree with irregular boxes (or boxes that do not bound their contents) is only walked in the reference's order");
    Float4Arg a; memcpy(a.v, us, 16);
    Scene sc = scene_of(c);
    const float *ins[] = {rs, rd}; float *outs[] = {out0, out1};
    return run_hook(c, n, ins, 2, outs, 2, [&](auto &i, auto &o) {
        dim3 grid(std::min<uint32_t>(c->grid_waves, (uint32_t)((n + BLOCK - 1) / BLOCK)));
        if (any_hit == 2) k_test_traverse<false, true><<<grid, BLOCK, 0, c->stream>>>(sc, i[0], i[1], a, n, o[0], o[1], c->d_spill);
        else if (any_hit) k_test_traverse<true><<<grid, BLOCK, 0, c->stream>>>(sc, i[0], i[1], a, n, o[0], o[1], c->d_spill);
        else k_test_traverse<false><<<grid, BLOCK, 0, c->stream>>>(sc, i[0], i[1], a, n, o[0], o[1], c->d_spill);
    });
}
int gpuart_hip_test_cam_rays(gpuart_hip_ctx *c, float *rstart, float *rdir) {
    if (!c || !c->have_camera || !c->plan.tile_pixels) return fail(GPUART_HIP_ERR_ARG, "camera / frame not set");
    int n = (int)c->plan.tile_pixels;
    float *outs[] = {rstart, rdir};
    Frame f = c->frame;
    return run_hook(c, n, nullptr, 0, outs, 2, [&](auto &, auto &o) { k_test_cam_rays<<<GRID1(n)>>>(f, o[0], o[1]); });
}
#endif

#ifdef GPUART_HIP_TEST_HOOKS
namespace {
/// One wave that keeps the stream busy for `ticks` of the 100 MHz wall clock (gpuart_hip_test_stall): it ends by itself.
/// Test builds only, like its launcher: the product code object carries no k_test_* kernel (tests/test_product_library.py).
__global__ void k_test_stall(unsigned long long ticks, unsigned long long *sink) {
    const unsigned long long t0 = wall_clock64();
    unsigned long long n = 0;
    while (wall_clock64() - t0 < ticks) n++;
    if (sink && threadIdx.x == 0) *sink = n;
}
}  // namespace
int gpuart_hip_test_tile_order(gpuart_hip_ctx *c, const uint32_t *order, size_t n) {
    if (!c || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
    HIP_TRY(hipSetDevice(c->device));
    int r = gpuart_hip_flush(c);
    if (r || (r = drain(c))) return r;
    if (!order) { c->frame.tile_order = nullptr; c->order_from_hook = false; c->order_cur = -1; c->order_sorting = false; c->order_stale = true; return 0; }
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    if (n != tiles) return fail(GPUART_HIP_ERR_ARG, "the order must name every 8x8 block of the tile once");
    std::vector<bool> seen(tiles, false);
    for (size_t k = 0; k < n; k++) {
        if (order[k] >= tiles || seen[order[k]]) return fail(GPUART_HIP_ERR_ARG, "the order must name every 8x8 block of the tile once");
        seen[order[k]] = true;
    }
    if (!c->d_tile_order[0]) HIP_TRY(hipMalloc(&c->d_tile_order[0], tiles * sizeof(uint32_t)));
    HIP_TRY(hipMemcpy(c->d_tile_order[0], order, tiles * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->frame.tile_order = c->d_tile_order[0];
    c->order_from_hook = true; c->order_sorting = false;
    return 0;
}
int gpuart_hip_test_current_tile_order(gpuart_hip_ctx *c, uint32_t *order, size_t n) {
    if (!c || !c->frame.W) return fail(GPUART_HIP_ERR_ARG, "no frame size set");
    HIP_TRY(hipSetDevice(c->device));
    int r = gpuart_hip_flush(c);
    if (r || (r = drain(c))) return r;
    if (c->order_sorting) {  // drained: the sort has finished
        c->order_cur = c->order_next;
        c->order_sorting = false;
    }
    const uint32_t *cur = c->order_from_hook ? c->frame.tile_order : c->order_cur >= 0 ? c->d_tile_order[c->order_cur] : nullptr;
    if (!cur) return 0;
    const size_t tiles = (size_t)((c->frame.tw + 7) / 8) * ((c->frame.th + 7) / 8);
    if (!order || n != tiles) return fail(GPUART_HIP_ERR_ARG, "room for one entry per 8x8 block of the tile, please");
    HIP_TRY(hipMemcpy(order, cur, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 1;
}
int gpuart_hip_test_sort_tiles(gpuart_hip_ctx *c, const uint32_t *cost, size_t n, uint32_t *order) {
    if (!c || !cost || !order || n == 0 || n > 0x04000000u) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    uint32_t *d = nullptr;
    HIP_TRY(hipMalloc(&d, 2 * n * sizeof(uint32_t)));
    hipError_t e = hipMemcpyAsync(d, cost, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        k_tile_order<<<1, TO_THREADS, 0, c->stream>>>(d, d + n, (uint32_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(order, d + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    HIP_TRY(e);
    return 0;
}
#endif
// ---- phase watchdog and the bounded-call mechanism (bounded.h; pure host code) ----------------------------------------------
int gpuart_hip_phase_begin(const char *name, uint32_t timeout_ms) { return bounded_ns::phase_begin(name, timeout_ms); }
int gpuart_hip_phase_end(void) { return bounded_ns::phase_end(); }
int gpuart_hip_phase_log(int on) { return bounded_ns::phase_log(on); }
int gpuart_hip_comm_stuck(void) { return bounded_ns::stuck().load() ? 1 : 0; }
#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_bounded_call(uint32_t hold_ms, uint32_t timeout_ms, int mark_stuck) {
    // (the helper's own `stuck` mark is global: the hook restores it unless the test wants to see the layer refuse its entry points)
    const bool was = bounded_ns::stuck().load();
    const bounded_ns::Outcome o = bounded_ns::bounded("gpuart_hip_test_bounded_call", timeout_ms, [hold_ms](std::string &d) {
        std::this_thread::sleep_for(std::chrono::milliseconds(hold_ms));
        d = "held for " + std::to_string(hold_ms) + " ms";
        return 0;
    });
    if (!mark_stuck && !was) bounded_ns::stuck().store(false);
    if (o.timed_out) return fail(GPUART_HIP_ERR_TIMEOUT, o.detail);
    return o.rc;
}
#endif

#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_stall(gpuart_hip_ctx *c, uint32_t ms) {
    if (!c || ms > 5000) return fail(GPUART_HIP_ERR_ARG, "bad argument (at most 5000 ms)");
    HIP_TRY(hipSetDevice(c->device));
    k_test_stall<<<1, 64, 0, c->stream>>>((unsigned long long)ms * 100000ull, nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}
#endif

#ifdef GPUART_HIP_TEST_HOOKS
int gpuart_hip_test_launches(gpuart_hip_ctx *c, char *buf, size_t cap, size_t *len, int reset) {
    if (!c || !len || (cap && !buf)) return fail(GPUART_HIP_ERR_ARG, "bad argument");
    std::string s;
    for (const void *k : c->launched) {
        const char *name = hipKernelNameRefByPtr(k, c->stream);
        if (name && name[0]) {
            s += name;
        } else {  // the runtime cannot name it: where its handle lies in this library (the binding looks the offset up in the symbol table)
            Dl_info di{};
            char off[32];
            snprintf(off, sizeof off, "@%zx", dladdr(k, &di) ? (size_t)((const char *)k - (const char *)di.dli_fbase) : (size_t)0);
            s += off;
        }
        s += '\n';
    }
    (void)hipGetLastError();  // a failed lookup must not surface as the error of a later launch
    *len = s.size();
    if (!buf) return 0;
    if (cap < s.size() + 1) return fail(GPUART_HIP_ERR_ARG, "launch ledger: the buffer holds " + std::to_string(cap) + " bytes, " +
                                        std::to_string(s.size() + 1) + " needed");
    memcpy(buf, s.c_str(), s.size() + 1);
    if (reset) c->launched.clear();
    return 0;
}
#endif

#include "diag_host.h"  // the gpuart_hip_debug_* entry points of the three diagnostic builds
}  // extern "C"
