// renderer.cpp — host control of the hot path over the C-ABI device back end.
#include "renderer.h"

#include <algorithm>
#include <chrono>
#include <iomanip>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>

#include "utils.h"

#include <hip/hip_runtime_api.h>

#define GPUART_PI 3.1415926f  // the reference's PI (src/renderer.cpp:48); feeds tan() of the field of view

namespace gpuart {

// ---- pure host arithmetic (bit-compatible with the reference) -----------------------------------
// reference src/renderer.cpp:135-150
Renderer::ScreenBasis Renderer::ComputeScreenBasis(const Camera &cam, unsigned width, unsigned height) {
    const float aspect = (float)width / height;
    // cam.Up projected onto the plane orthogonal to cam.Dir
    const Vec3f up = ((cam.Dir ^ cam.Up) ^ cam.Dir).normalized();
    const Vec3f target = cam.Pos + cam.Dir.normalized() * cam.ScreenDist;
    // screen centre -> right edge, then centre -> top edge
    const Vec3f a = (cam.Dir.normalized() ^ up) * cam.ScreenDist * aspect * std::tan(cam.FovY / 2 * GPUART_PI / 180);
    const Vec3f b = up * a.length() / aspect;
    ScreenBasis s;
    s.Pos = cam.Pos;
    s.BottomLeft = target - a - b;
    s.DeltaHorz = 2 * a;
    s.DeltaVert = 2 * b;
    return s;
}

// reference src/renderer.cpp:573-574
float Renderer::ComputePixelSize(const Camera &cam, unsigned height) {
    return 2 * cam.ScreenDist * std::tan(cam.FovY / 2 * GPUART_PI / 180) / height;
}

// reference src/renderer.h:175-179
Vec3f Renderer::ComputeSunDirection(float azimuth, float altitude) {
    return Vec3f(1, 0, 0).vroty(-altitude).vrotz(azimuth);
}

// ---- lifecycle ----------------------------------------------------------------------------------
Renderer::Renderer(unsigned viewportWidth, unsigned viewportHeight, const Camera &camera, int device) {
    // defaults of the reference constructor (src/renderer.cpp:202-214)
    Lighting.azimuth = GPUART_PI;
    Lighting.altitude = GPUART_PI / 4;
    Lighting.directLightingEnabled = true;
    UserSphere.pos = Vec3f(0, 0, 0);
    UserSphere.emittance = 0;
    UserSphere.radius = 0;
    UserSphere.flags = 0;
    PathTracing.pathsPerPixel = 5;
    PathTracing.pathsPerPass = PathTracing.pathsPerPixel;
    PathTracing.numPathsRendered = 0;
    CurrentCamera = camera;
    Device = device;
    gpuart_temporal_defaults(&TemporalParams);
    gpuart_moments_defaults(&MomentsParams);
    gpuart_antilag_defaults(&AntiLagParams);
    gpuart_edges_defaults(&EdgeParams);
    gpuart_despeckle_defaults(&FireflyParams);

    if (!Check(gpuart_hip_create(device, &Backend), "creating the device back end")) return;
    if (viewportWidth == 0 || viewportHeight == 0) {
        std::cerr << "Renderer: viewport must not be empty." << std::endl;
        return;
    }
    IsOK = true;  // UpdateViewportSize reports through IsOK
    UpdateViewportSize(viewportWidth, viewportHeight);
}

Renderer::~Renderer() {
    if (Upscaler) gpuart_upscale_destroy(Upscaler);
    UpscaleWords.Release();
    UpscaleMem.Release();
    if (Display) gpuart_display_destroy(Display);
    DisplayMem.Release();
    if (Refine) gpuart_refine_destroy(Refine);
    ErrorMem.Release();
    if (Despeckle) gpuart_despeckle_destroy(Despeckle);
    if (Edges) gpuart_edges_destroy(Edges);
    EdgeSubMem.Release();
    EdgeMem.Release();
    if (Adaptive) gpuart_adaptive_destroy(Adaptive);
    BlockPathsMem.Release();
    if (Converge) gpuart_converge_destroy(Converge);
    AccumMem.Release();
    if (AntiLag) gpuart_antilag_destroy(AntiLag);
    if (TemporalFast) gpuart_temporal_destroy(TemporalFast);
    AntiLagMem.Release();
    if (Moments) gpuart_moments_destroy(Moments);
    if (TemporalMoments) gpuart_temporal_destroy(TemporalMoments);
    MomentsMem.Release();
    if (Temporal) gpuart_temporal_destroy(Temporal);
    if (Denoiser) gpuart_denoise_destroy(Denoiser);
    DenoiseMem.Release();
    if (Refitter) gpuart_refit_destroy(Refitter);
    if (Builder) gpuart_build_destroy(Builder);
    if (Clusterer) gpuart_ploc_destroy(Clusterer);
    if (Editor) gpuart_edit_destroy(Editor);
    if (Nearest) gpuart_nearest_destroy(Nearest);
    if (Backend) gpuart_hip_destroy(Backend);
}

bool Renderer::Check(int status, const char *what, const char *(*lastError)(void)) {
    if (status == 0) return true;
    std::cerr << "Renderer: error " << status << " while " << what << ": " << lastError() << std::endl;
    return false;
}

bool Renderer::UpdateViewportSize(unsigned width, unsigned height) {
    if (!Backend || width == 0 || height == 0) return IsOK = false;
    Viewport.width = width;
    Viewport.height = height;
    DropTemporalHistory();
    PathTracing.numPathsRendered = 0;  // (the resize clears the accumulator: the SetCamera below has no view to commit)
    if (!Check(gpuart_hip_resize(Backend, width, height), "allocating per-pixel buffers")) return IsOK = false;
    Tile.x = Tile.y = 0; Tile.w = width; Tile.h = height;
    GBufferValid = false;
    if (!SetCamera(CurrentCamera)) IsOK = false;
    return IsOK;
}

bool Renderer::SetTile(unsigned x0, unsigned y0, unsigned w, unsigned h) {
    if (!Backend) return false;
    if (!Check(gpuart_hip_set_tile(Backend, x0, y0, w, h), "setting the tile")) return false;
    Tile.x = x0; Tile.y = y0; Tile.w = w; Tile.h = h;
    GBufferValid = false;
    DropTemporalHistory();
    ResetPathTracing();
    return true;
}

bool Renderer::SetInterleavedTile(unsigned x0, unsigned y0, unsigned w, unsigned localRows, unsigned bandRows,
                                  unsigned bandStride) {
    if (!Backend) return false;
    if (!Check(gpuart_hip_set_tile_interleaved(Backend, x0, y0, w, localRows, bandRows, bandStride), "setting the tile"))
        return false;
    Tile.x = x0; Tile.y = y0; Tile.w = w; Tile.h = localRows;
    GBufferValid = false;
    DropTemporalHistory();
    ResetPathTracing();
    return true;
}

bool Renderer::SetNearestFirst(uint32_t minPrims) {
    if (!Backend) return false;
    if (!Check(gpuart_hip_set_nearest_first(Backend, minPrims), "choosing the visiting order")) return false;
    DropTemporalHistory();
    ResetPathTracing();
    return true;
}

bool Renderer::SetShare(int rank, int nranks) {
    if (!Backend) return false;
    gpuart_tile_geom g;
    if (gpuart_hip_share_of_rank(Viewport.width, Viewport.height, rank, nranks, 8, &g) != 0 || g.th == 0) {
        std::cerr << "Renderer: no share " << rank << " of " << nranks << " in a frame of " << Viewport.height << " rows." << std::endl;
        return false;
    }
    return SetInterleavedTile(g.x0, g.y0, g.tw, g.th, g.band_rows, g.band_stride);
}

/// Bound of one phase of the multi-GPU read-out for the library's watchdog (gpuart_hip_phase_begin): GPUART_PHASE_TIMEOUT_MS,
/// default 300 s — above the library's own bounds (GPUART_HIP_COMM_TIMEOUT_MS 120 s, GPUART_HIP_GATHER_TIMEOUT_MS 60 s), which
/// come back with an error first; the watchdog is for whatever those do not wrap.
static uint32_t PhaseTimeoutMs() {
    const char *v = getenv("GPUART_PHASE_TIMEOUT_MS");
    if (!v) return 300000u;
    const long x = strtol(v, nullptr, 10);
    return x <= 0 ? 0u : (uint32_t)x;
}

bool Renderer::GatherRadiance(Renderer *const *ranks, int n, int root, bool normalized, float *fullFrame) {
    if (!ranks || n < 1 || root < 0 || root >= n || !fullFrame) return false;
    std::vector<gpuart_hip_ctx *> ctxs((size_t)n);
    for (int k = 0; k < n; k++) {
        if (!ranks[k] || !ranks[k]->IsOK) return false;
        ctxs[(size_t)k] = ranks[k]->Backend;
    }
    for (int k = 0; k < n; k++)
        if (ranks[k]->NonUniform) {
            std::cerr << "Renderer: GatherRadiance after adaptive sampling retired blocks: the shares' path counts are not uniform." << std::endl;
            return false;
        }
    Renderer &r0 = *ranks[root];
    const float div = r0.Divisor(normalized);
    // One communicator per set of renderers, kept by the contexts themselves. Whether these contexts are (still) the ranks
    // 0..n-1 of one is the library's to say: it answers GPUART_HIP_ERR_NO_COMM before anything is transferred, then one is made.
    // Every step that waits for RCCL or for the other GPUs is a named phase (a line on stderr before and after, and the
    // library's watchdog behind it): a read-out that stalls says where.
    const uint32_t bound = PhaseTimeoutMs();
    gpuart_hip_phase_begin("frame gather (gpuart_hip_gather_all_read)", bound);
    int rc = gpuart_hip_gather_all_read(ctxs.data(), n, 1, div, root, fullFrame);
    gpuart_hip_phase_end();
    if (rc == GPUART_HIP_ERR_NO_COMM) {
        gpuart_hip_phase_begin("communicator init (gpuart_hip_comm_init_all = ncclCommInitAll)", bound);
        const bool made = r0.Check(gpuart_hip_comm_init_all(ctxs.data(), n), "creating the RCCL communicator");
        gpuart_hip_phase_end();
        if (!made) return false;
        gpuart_hip_phase_begin("frame gather (gpuart_hip_gather_all_read)", bound);
        rc = gpuart_hip_gather_all_read(ctxs.data(), n, 1, div, root, fullFrame);
        gpuart_hip_phase_end();
    }
    return r0.Check(rc, "gathering the frame");
}

bool Renderer::ReleaseCommunicator(Renderer *const *ranks, int n) {
    if (!ranks || n < 1) return false;
    bool ok = true;
    gpuart_hip_phase_begin("communicator destroy (gpuart_hip_comm_destroy = ncclCommDestroy)", PhaseTimeoutMs());
    for (int k = 0; k < n; k++)
        if (ranks[k] && ranks[k]->Backend) ok = ranks[k]->Check(gpuart_hip_comm_destroy(ranks[k]->Backend), "destroying the RCCL communicator") && ok;
    gpuart_hip_phase_end();
    return ok;
}

bool Renderer::SetCamera(const Camera &cam) {
    CommitTemporalView();
    CurrentCamera = cam;
    GBufferValid = false;
    if (!Backend) return false;
    const ScreenBasis s = ComputeScreenBasis(cam, Viewport.width, Viewport.height);
    CurrentBasis = s;
    float pos[3], bl[3], dh[3], dv[3];
    s.Pos.storeIn(pos); s.BottomLeft.storeIn(bl); s.DeltaHorz.storeIn(dh); s.DeltaVert.storeIn(dv);
    if (!Check(gpuart_hip_set_camera(Backend, pos, bl, dh, dv), "setting the camera")) return false;
    ResetPathTracing();
    return true;
}

// ---- scene --------------------------------------------------------------------------------------
namespace {
struct ByteCount {
    size_t count;
};
std::ostream &operator<<(std::ostream &os, const ByteCount &bc) {
    static const char *unit[] = {" B", " KiB", " MiB", " GiB"};
    double v = (double)bc.count;
    int u = 0;
    while (v >= 1024 && u < 3) { v /= 1024; u++; }
    return os << std::fixed << std::setprecision(u ? 1 : 0) << v << unit[u];
}
}  // namespace

void Renderer::SetPrimitives(std::vector<Primitive *> &primitives, bool printInfo) {
    auto t0 = std::chrono::high_resolution_clock::now();
    const auto tAll = t0;
    if (printInfo) std::cout << "Constructing BVH tree of " << primitives.size() << " primitives... " << std::flush;
    Tree = BoundingVolumesHierarchy(primitives, 1024, 2);  // reference src/renderer.cpp:454
    const auto tBuilt = std::chrono::high_resolution_clock::now();
    if (printInfo) {
        std::cout << "done (" << Utils::TimeElapsed(t0) << ")." << std::endl;
        std::cout << "Compiling BVH tree... " << std::flush;
        t0 = std::chrono::high_resolution_clock::now();
    }
    // (the reference compiles into a Primitive::Data — src/renderer.cpp:460-466 —; the same quads go into a buffer that is not zeroed
    // first: for an 871 200-triangle mesh that is 105 MB one thread would touch before the threads that fill it)
    const size_t compiledFloats = Tree.CompiledFloats();
    std::unique_ptr<float[]> compiled(new float[compiledFloats]);
    Tree.CompileTo(compiled.get());
    const auto tCompiled = std::chrono::high_resolution_clock::now();
    GBufferValid = false;
    DropTemporalHistory();
    if (printInfo) std::cout << "done (" << Utils::TimeElapsed(t0) << ").\n";
    if (!Backend || !Check(gpuart_hip_upload_bvh(Backend, compiled.get(), compiledFloats / RGBA_ELEMS), "uploading the BVH"))
        IsOK = false;
    if (printInfo) std::cout << "Compiled tree occupies " << ByteCount{compiledFloats * sizeof(float)} << "." << std::endl;
    const auto tEnd = std::chrono::high_resolution_clock::now();
    auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    LastSetPrimitivesMs[0] = ms(tAll, tEnd); LastSetPrimitivesMs[1] = ms(tAll, tBuilt); LastSetPrimitivesMs[2] = ms(tBuilt, tCompiled);
    LastSetPrimitivesMs[3] = ms(tCompiled, tEnd);
    if (std::getenv("GPUART_HOST_TIMING")) {
        fprintf(stderr, "[gpuart] Renderer::SetPrimitives(%zu primitives): %.1f ms (build %.1f + compile %.1f + re-layout and upload %.1f)\n",
                primitives.size(), ms(tAll, tEnd), ms(tAll, tBuilt), ms(tBuilt, tCompiled), ms(tCompiled, tEnd));
    }
    ResetPathTracing();
}

namespace {
/// What the Renderer needs of an image or tree library to make a handle, wait for it and report its failures.
template <class H>
struct Lib {
    int (*create)(int, H **);
    int (*finish)(H *);
    const char *(*lastError)(void);
    const char *creating;
};
const Lib<gpuart_denoise> DN{gpuart_denoise_create, gpuart_denoise_finish, gpuart_denoise_last_error, "creating the denoiser"};
const Lib<gpuart_temporal> TP{gpuart_temporal_create, gpuart_temporal_finish, gpuart_temporal_last_error, "creating the temporal accumulator"};
const Lib<gpuart_temporal> TPM{gpuart_temporal_create, gpuart_temporal_finish, gpuart_temporal_last_error, "creating the moments' temporal accumulator"};
const Lib<gpuart_moments> MO{gpuart_moments_create, gpuart_moments_finish, gpuart_moments_last_error, "creating the moments library's handle"};
const Lib<gpuart_temporal> TPF{gpuart_temporal_create, gpuart_temporal_finish, gpuart_temporal_last_error, "creating the fast history's temporal accumulator"};
const Lib<gpuart_antilag> AL{gpuart_antilag_create, gpuart_antilag_finish, gpuart_antilag_last_error, "creating the anti-lag library's handle"};
const Lib<gpuart_converge> CV{gpuart_converge_create, gpuart_converge_finish, gpuart_converge_last_error, "creating the convergence estimator"};
const Lib<gpuart_adaptive> AD{gpuart_adaptive_create, gpuart_adaptive_finish, gpuart_adaptive_last_error, "creating the adaptive estimator"};
const Lib<gpuart_refine> RF{gpuart_refine_create, gpuart_refine_finish, gpuart_refine_last_error, "creating the variance-guided filter"};
const Lib<gpuart_edges> ED{gpuart_edges_create, gpuart_edges_finish, gpuart_edges_last_error, "creating the edge resolve's handle"};
const Lib<gpuart_despeckle> DS{gpuart_despeckle_create, gpuart_despeckle_finish, gpuart_despeckle_last_error, "creating the firefly clamp's handle"};
const Lib<gpuart_upscale> UP{gpuart_upscale_create, gpuart_upscale_finish, gpuart_upscale_last_error, "creating the upscaler"};
const Lib<gpuart_display> DP{gpuart_display_create, gpuart_display_finish, gpuart_display_last_error, "creating the display stage"};
const Lib<gpuart_refit> RT{gpuart_refit_create, gpuart_refit_finish, gpuart_refit_last_error, "creating the refit handle"};
const Lib<gpuart_build> BD{gpuart_build_create, gpuart_build_finish, gpuart_build_last_error, "creating the build handle"};
const Lib<gpuart_ploc> PL{gpuart_ploc_create, gpuart_ploc_finish, gpuart_ploc_last_error, "creating the clustered build's handle"};
const Lib<gpuart_edit> ET{gpuart_edit_create, gpuart_edit_finish, gpuart_edit_last_error, "creating the edit handle"};
const Lib<gpuart_nearest> NE{gpuart_nearest_create, gpuart_nearest_finish, gpuart_nearest_last_error, "creating the closest-point handle"};

std::chrono::high_resolution_clock::time_point Now() { return std::chrono::high_resolution_clock::now(); }
template <class T> double Ms(T from, T to) { return std::chrono::duration<double, std::milli>(to - from).count(); }

/// One build into `spare`, which then says what was built: the two builds' result records differ in the name of their fifth word only.
template <class H, class R>
int RunBuild(H *h, int (*runHost)(H *, const gpuart_hip_scene *, const gpuart_hip_scene *, uint32_t *, R *), const gpuart_hip_scene &src, gpuart_hip_scene &spare,
             uint32_t *order) {
    R res;
    const int rc = runHost(h, &src, &spare, order, &res);
    if (rc != 0) return rc;
    spare.n_recs = res.n_recs;
    spare.root_ref = res.root_ref;
    spare.max_depth = res.max_depth;
    memcpy(spare.root_min, res.root_min, 12); memcpy(spare.root_max, res.root_max, 12);
    spare.box_slack = res.subnormal ? __builtin_inff() : 0.0f;
    return 0;
}
}  // namespace

template <class H, class L>
bool Renderer::Ensure(H *&h, const L &lib) {
    return h || Check(lib.create(Device, &h), lib.creating, lib.lastError);
}

// ---- moved primitives: a refit in place (include/gpuart_refit.h) ------------------------------------
// The host tree gives its verdict first and changes last: a refusal, on the host or on the device (they state one rule,
// csrc/hip/prim_rule.h), leaves both trees as they were. The view is committed after the verdict and before the device arrays change,
// while the accumulator and the G-buffer are still those of the scene the paths saw.
bool Renderer::UpdatePrimitives(const uint32_t *indices, Primitive *const *moved, size_t n) {
    if (!IsOK || (n && (!indices || !moved))) return false;
    std::vector<float> payloads(GPUART_REFIT_PAYLOAD * n);
    std::vector<uint32_t> types(n);
    size_t bad = 0;
    for (size_t i = 0; i < n; i++) {
        if (!moved[i]) return false;
        types[i] = BoundingVolumesHierarchy::Payload(*moved[i], payloads.data() + GPUART_REFIT_PAYLOAD * i);
    }
    if (!Tree.CheckRefit(indices, payloads.data(), n, &bad, types.data())) {
        std::cerr << "Renderer: UpdatePrimitives: update " << bad << " refused (indices ascending and in range, the same type, a primitive inside the rule)." << std::endl;
        return false;
    }
    gpuart_hip_scene scene;
    if (!Check(gpuart_hip_scene_device(Backend, &scene), "looking up the scene's device arrays")) return false;
    if (scene.exact_boxes) {
        std::cerr << "Renderer: UpdatePrimitives: a tree with irregular boxes (or boxes that do not bound their contents) is not refitted." << std::endl;
        return false;
    }
    if (!Ensure(Refitter, RT)) return false;
    if (RefitGeneration != scene.generation) {  // (a bind reads every record back: once per upload)
        if (!Check(gpuart_refit_bind(Refitter, &scene), "binding the refit handle", gpuart_refit_last_error)) return false;
        RefitGeneration = scene.generation;
    }
    CommitTemporalView();
    gpuart_refit_result res;
    if (!Check(gpuart_refit_run_host(Refitter, &scene, indices, payloads.data(), n, &res), "refitting the tree", gpuart_refit_last_error)) return false;
    if (!Check(gpuart_hip_scene_refitted(Backend, res.root_min, res.root_max, (int)res.subnormal), "adopting the refitted tree")) return IsOK = false;
    Tree.Refit(indices, payloads.data(), n, nullptr, true);
    TreeChanged(false);
    return true;
}

// ---- a drifted scene: the tree rebuilt on the device (include/gpuart_build.h, include/gpuart_ploc.h) ----
// The device builds into the spare arrays, so every refusal up to the swap leaves the scene as it was. The temporal histories are kept as
// for a refit: their tap validation compares hit point, normal and class, and of the ordinal only "is the user sphere" (-2), which a new
// numbering does not touch. RebuildTree, EditPrimitives and TreeCost state their shared steps once, here.
bool Renderer::RefusesTreeChange(const gpuart_hip_scene &scene, const char *fn, const char *done) {
    if (!scene.exact_boxes && scene.n_prims && Tree.GetNumPrimitives() == scene.n_prims) return false;
    std::cerr << "Renderer: " << fn << ": an empty scene or a tree with irregular boxes (or boxes that do not bound their contents) is not " << done << "." << std::endl;
    return true;
}

bool Renderer::EnsureBuilder(bool clustered) { return clustered ? Ensure(Clusterer, PL) : Ensure(Builder, BD); }

bool Renderer::BuildIntoSpare(const gpuart_hip_scene &src, bool clustered, bool withPrims, bool commit, const char *fn, const char *what, gpuart_hip_scene &spare,
                              BuiltTree &built) {
    const uint64_t n = src.n_prims, room = clustered ? n - 1 : (n + 1) / 2 - 1;
    if (!Check(withPrims ? gpuart_hip_scene_reserve_prims(Backend, room, n, &spare) : gpuart_hip_scene_reserve(Backend, room, &spare), "reserving the spare arrays"))
        return false;
    if (!EnsureBuilder(clustered)) return false;
    if (commit) CommitTemporalView();
    built.order.resize(n);
    const int rc = clustered ? RunBuild(Clusterer, gpuart_ploc_run_host, src, spare, built.order.data())
                             : RunBuild(Builder, gpuart_build_run_host, src, spare, built.order.data());
    if (!Check(rc, what, clustered ? PL.lastError : BD.lastError)) return false;
    built.ran = Now();
    built.nRecs = spare.n_recs;
    built.refs.resize(clustered ? 2 * built.nRecs : 0);
    if (clustered && built.nRecs) {  // the topology is the device's: the two ref words of every record, word 3 of its first two quads
        std::unique_ptr<uint32_t[]> recs(new uint32_t[16 * built.nRecs]);
        if (hipMemcpy(recs.get(), spare.recs, 64 * built.nRecs, hipMemcpyDeviceToHost) != hipSuccess) {
            std::cerr << "Renderer: " << fn << ": reading the built records back failed." << std::endl;
            return false;
        }
        for (uint64_t r = 0; r < built.nRecs; r++) { built.refs[2 * r] = recs[16 * r + 3]; built.refs[2 * r + 1] = recs[16 * r + 7]; }
    }
    return true;
}

bool Renderer::TreeFollows(bool clustered, const BuiltTree &built) {
    return clustered ? Tree.AdoptTopology(built.order.data(), built.refs.data(), built.nRecs) : Tree.RebuildMorton(nullptr, built.order.data());
}

void Renderer::TreeChanged(bool newArrays) {
    if (newArrays) RefitGeneration = 0;
    GBufferValid = false;
    EdgeListValid = false;
    ResetPathTracing();
}

// The two modes commit in different orders (DESIGN.md "The tree libraries' scaffold"). Morton: the context adopts the spare set, then the
// host tree follows from the device's permutation (RebuildMorton checks the order instead of sorting) — a host tree that cannot is an
// inconsistency. Clustered: the host tree checks and adopts the device's topology first — a refusal still leaves both trees as they were
// — and only then are the device arrays swapped; there a device that cannot follow is the inconsistency.
bool Renderer::RebuildTree(std::vector<uint32_t> *newToOld, int mode) {
    if (!IsOK) return false;
    if (mode != TREE_MORTON && mode != TREE_CLUSTERED) {
        std::cerr << "Renderer: RebuildTree: unknown mode " << mode << "." << std::endl;
        return false;
    }
    const bool clustered = mode == TREE_CLUSTERED;
    const auto t0 = Now();
    gpuart_hip_scene scene, spare;
    if (!Check(gpuart_hip_scene_device(Backend, &scene), "looking up the scene's device arrays")) return false;
    if (RefusesTreeChange(scene, "RebuildTree", "rebuilt")) return false;
    BuiltTree built;
    if (!BuildIntoSpare(scene, clustered, false, true, "RebuildTree", "rebuilding the tree", spare, built)) return false;
    if (!clustered && !Check(gpuart_hip_scene_rebuilt(Backend, &spare), "adopting the rebuilt tree")) return false;
    const auto t1 = clustered ? built.ran : Now();
    if (!TreeFollows(clustered, built)) {
        std::cerr << "Renderer: RebuildTree: the device's " << (clustered ? "topology is not a tree over the scene's primitives." : "order is not the contract's.") << std::endl;
        if (!clustered) IsOK = false;
        return false;
    }
    const auto t2 = Now();
    if (clustered && !Check(gpuart_hip_scene_rebuilt(Backend, &spare), "adopting the rebuilt tree")) return IsOK = false;
    LastRebuildMs[0] = Ms(t0, Now());
    LastRebuildMs[1] = Ms(t1, t2);
    if (newToOld) newToOld->swap(built.order);
    TreeChanged(true);
    return true;
}

// ---- a scene that gains or loses primitives: the list edited and its tree built on the device (include/gpuart_edit.h) ----
// The order of the clustered RebuildTree: the host's verdict, the view committed, the device edit into the library's staging
// arrays and the build from them into the spare set — every refusal up to here leaves both trees as they were —, then the host tree
// follows and the context adopts the result.
bool Renderer::EditPrimitives(const uint32_t *remove, size_t nRemove, Primitive *const *added, size_t nAdd, std::vector<uint32_t> *source, int mode) {
    if (!IsOK || (nRemove && !remove) || (nAdd && !added)) return false;
    if (mode != TREE_MORTON && mode != TREE_CLUSTERED) {
        std::cerr << "Renderer: EditPrimitives: unknown mode " << mode << "." << std::endl;
        return false;
    }
    const auto t0 = Now();
    std::vector<float> payloads(GPUART_REFIT_PAYLOAD * nAdd);
    std::vector<uint32_t> types(nAdd);
    for (size_t k = 0; k < nAdd; k++) {
        if (!added[k]) return false;
        types[k] = BoundingVolumesHierarchy::Payload(*added[k], payloads.data() + GPUART_REFIT_PAYLOAD * k);
    }
    size_t bad = 0;
    if (!Tree.CheckEdit(remove, nRemove, types.data(), payloads.data(), nAdd, &bad)) {
        std::cerr << "Renderer: EditPrimitives: refused (removals ascending and in range, added primitives inside the rule, a primitive left); first offender "
                  << (bad == SIZE_MAX ? std::string("none") : std::to_string(bad)) << "." << std::endl;
        return false;
    }
    gpuart_hip_scene scene, edited, spare;
    if (!Check(gpuart_hip_scene_device(Backend, &scene), "looking up the scene's device arrays")) return false;
    if (RefusesTreeChange(scene, "EditPrimitives", "edited")) return false;
    const bool clustered = mode == TREE_CLUSTERED;
    if (!Ensure(Editor, ET) || !EnsureBuilder(clustered)) return false;
    CommitTemporalView();
    const uint64_t n = scene.n_prims - nRemove + nAdd;
    std::vector<int32_t> from(n);
    gpuart_edit_result er;
    if (!Check(gpuart_edit_run_host(Editor, &scene, remove, nRemove, types.data(), payloads.data(), nAdd, from.data(), &edited, &er), "editing the primitive list",
               gpuart_edit_last_error))
        return false;
    BuiltTree built;
    if (!BuildIntoSpare(edited, clustered, true, false, "EditPrimitives", "building the edited tree", spare, built)) return false;
    spare.n_prims = n;
    const auto t1 = Now();
    // (from here the host tree changes: a tree or a device that cannot follow is an inconsistency, not a refusal)
    if (!Tree.EditPrimitives(remove, nRemove, types.data(), payloads.data(), nAdd) || !TreeFollows(clustered, built)) {
        std::cerr << "Renderer: EditPrimitives: the device's tree is not the contract's over the edited primitives." << std::endl;
        return IsOK = false;
    }
    const auto t2 = Now();
    if (!Check(gpuart_hip_scene_replaced(Backend, &spare, er.type_mask), "adopting the edited tree")) return IsOK = false;
    LastRebuildMs[0] = Ms(t0, Now());
    LastRebuildMs[1] = Ms(t1, t2);
    if (source) {
        source->resize(n);
        for (uint64_t p = 0; p < n; p++) (*source)[p] = (uint32_t)from[built.order[p]];
    }
    TreeChanged(true);
    return true;
}

bool Renderer::TreeCost(double *cost) {
    if (!IsOK || !cost) return false;
    gpuart_hip_scene scene;
    if (!Check(gpuart_hip_scene_device(Backend, &scene), "looking up the scene's device arrays")) return false;
    if (!Ensure(Builder, BD)) return false;
    return Check(gpuart_build_cost(Builder, &scene, cost), "measuring the tree's cost", gpuart_build_last_error);
}

// ---- batched ray queries ------------------------------------------------------------------------
// `prims` is the device primitive ordinal, which numbers the primitives in the order of the compiled tree's leaves (the uploader appends
// each leaf's primitives as it meets the leaves in pre-order, lower child first: converter.h `scan`). That is the order of the vector
// SetPrimitives leaves behind: the build writes its sorted items back into it (bvh.cpp:81, `primitives[i] = items[i].p`), every node
// splits its item range [from, to) into a lower child [from, split) and an upper child [split, to) (bvh.cpp Subdivide), a leaf holds
// items [primFirst, primFirst + count) (bvh.cpp:166-167), the compiled tree lays the nodes out in pre-order with the lower child first
// (bvh.cpp CompileTo), and no leaf of a non-empty scene is empty (a range of more than minPrims = 2 items is split strictly inside,
// bvh.cpp:218-221) — so leaf k in pre-order holds the items that follow those of leaves 0 .. k-1, and ordinal i is primitives[i].
bool Renderer::TraceRays(const float *rays, size_t n, bool occlusion, bool withUserSphere, gpuart_ray_hit *hits, int32_t *prims) {
    if (!IsOK) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_hip_trace_rays_host(Backend, rays, n, occlusion ? GPUART_HIP_RAYS_OCCLUSION : 0u, withUserSphere ? us : nullptr,
                                            hits, prims), "tracing rays");
}

bool Renderer::Pick(const uint32_t *xy, size_t n, gpuart_ray_hit *hits, int32_t *prims, bool withUserSphere) {
    if (!IsOK) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_hip_pick(Backend, xy, n, withUserSphere ? us : nullptr, hits, prims), "picking");
}

// ---- closest-point queries (include/gpuart_nearest.h) ---------------------------------------------
// The descriptor is looked up at every call: its generation says whether the handle's binding (the nesting check of every record) still
// holds — an upload, a rebuild and an edit raise it, a refit in place does not.
bool Renderer::BindNearest(const char *who, gpuart_hip_scene &scene) {
    if (!Check(gpuart_hip_scene_device(Backend, &scene), "looking up the scene's device arrays")) return false;
    if (scene.exact_boxes || !Tree.GetNumPrimitives()) {
        std::cerr << "Renderer: " << who << ": an empty scene or a tree with irregular boxes (or boxes that do not bound their contents) is not queried." << std::endl;
        return false;
    }
    if (!Ensure(Nearest, NE)) return false;
    if (NearestGeneration != scene.generation) {
        NearestGeneration = 0;
        if (!Check(gpuart_nearest_bind(Nearest, &scene), "binding the closest-point handle", gpuart_nearest_last_error)) return false;
        NearestGeneration = scene.generation;
    }
    return true;
}

bool Renderer::ClosestPoints(const float *points, size_t n, bool withUserSphere, gpuart_nearest_hit *hits) {
    if (!IsOK || (n && (!points || !hits))) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("ClosestPoints", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_run_host(Nearest, &scene, points, n, withUserSphere ? us : nullptr, hits), "querying closest points", gpuart_nearest_last_error);
}

bool Renderer::NearestPrimitives(const float *points, size_t n, size_t k, bool withUserSphere, gpuart_nearest_hit *hits) {
    if (!IsOK || (n && (!points || !hits))) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("NearestPrimitives", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_knn_run_host(Nearest, &scene, points, n, k, withUserSphere ? us : nullptr, hits), "querying the k nearest primitives",
                 gpuart_nearest_last_error);
}

// ---- neighbour lists (include/gpuart_nearest.h, "Neighbour lists") ----------------------------------
bool Renderer::PrimitivesWithin(const float *points, size_t n, bool withUserSphere, uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity, uint64_t *total) {
    if (!IsOK || (n && !points) || !offsets || !total) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("PrimitivesWithin", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_within_host(Nearest, &scene, points, n, withUserSphere ? us : nullptr, offsets, items, capacity, total),
                 "listing the primitives within a radius", gpuart_nearest_last_error);
}

bool Renderer::PrimitivesWithin(const float *points, size_t n, bool withUserSphere, std::vector<uint32_t> &offsets, std::vector<gpuart_nearest_hit> &items) {
    offsets.assign(n + 1, 0u);
    items.clear();
    uint64_t total = 0;
    if (!PrimitivesWithin(points, n, withUserSphere, offsets.data(), nullptr, 0, &total)) return false;
    if (!total) return true;
    items.resize(total);
    return FillPrimitivesWithin(points, n, withUserSphere, offsets.data(), items.data(), items.size());
}

bool Renderer::FillPrimitivesWithin(const float *points, size_t n, bool withUserSphere, const uint32_t *offsets, gpuart_nearest_hit *items, size_t capacity) {
    if (!IsOK || (n && !points) || !offsets) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("PrimitivesWithin", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_within_fill_host(Nearest, &scene, points, n, withUserSphere ? us : nullptr, offsets, items, capacity),
                 "filling the lists of the primitives within a radius", gpuart_nearest_last_error);
}

// ---- box overlap (include/gpuart_nearest.h, "Box overlap") --------------------------------------------
bool Renderer::PrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    if (!IsOK || (n && !boxes) || !offsets || !total) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("PrimitivesOverlapping", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_overlap_host(Nearest, &scene, boxes, n, margin, withUserSphere ? us : nullptr, offsets, items, capacity, total),
                 "listing the primitives that overlap a box", gpuart_nearest_last_error);
}

bool Renderer::PrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, std::vector<uint32_t> &offsets, std::vector<int32_t> &items) {
    offsets.assign(n + 1, 0u);
    items.clear();
    uint64_t total = 0;
    if (!PrimitivesOverlapping(boxes, n, margin, withUserSphere, offsets.data(), nullptr, 0, &total)) return false;
    if (!total) return true;
    items.resize(total);
    return FillPrimitivesOverlapping(boxes, n, margin, withUserSphere, offsets.data(), items.data(), items.size());
}

bool Renderer::FillPrimitivesOverlapping(const float *boxes, size_t n, float margin, bool withUserSphere, const uint32_t *offsets, int32_t *items, size_t capacity) {
    if (!IsOK || (n && !boxes) || !offsets) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("PrimitivesOverlapping", scene)) return false;
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    return Check(gpuart_nearest_overlap_fill_host(Nearest, &scene, boxes, n, margin, withUserSphere ? us : nullptr, offsets, items, capacity),
                 "filling the lists of the primitives that overlap a box", gpuart_nearest_last_error);
}

bool Renderer::OverlappingPairs(float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    if (!IsOK || !offsets || !total) return false;
    gpuart_hip_scene scene;
    if (!BindNearest("OverlappingPairs", scene)) return false;
    return Check(gpuart_nearest_pairs_host(Nearest, &scene, margin, offsets, items, capacity, total), "listing the overlapping pairs", gpuart_nearest_last_error);
}

bool Renderer::OverlappingPairs(float margin, std::vector<uint32_t> &offsets, std::vector<int32_t> &items) {
    offsets.assign((size_t)Tree.GetNumPrimitives() + 1, 0u);
    items.clear();
    uint64_t total = 0;
    if (!OverlappingPairs(margin, offsets.data(), nullptr, 0, &total)) return false;
    if (!total) return true;
    items.resize(total);
    return OverlappingPairs(margin, offsets.data(), items.data(), items.size(), &total);
}

// ---- lighting / user sphere ---------------------------------------------------------------------
void Renderer::SetUserSphere(const Vec3f &pos, float radius, float emittance) {
    UserSphere.pos = pos;
    UserSphere.radius = radius;
    SetUserSphereEmittance(emittance);
}

void Renderer::SetUserSphereEmittance(float em) {
    UserSphere.emittance = em;
    DropTemporalHistory();
    SetFlag(EM_NONZERO, em > 0);
}

void Renderer::SetFlag(uint32_t flag, bool on) {
    if (on) UserSphere.flags |= flag;
    else UserSphere.flags &= ~flag;
    DropTemporalHistory();
    ResetPathTracing();
}

gpuart_params Renderer::MakeParams() const {
    gpuart_params p{};
    const Vec3f sun = ComputeSunDirection(Lighting.azimuth, Lighting.altitude);
    p.sunDirAlt[0] = sun.x; p.sunDirAlt[1] = sun.y; p.sunDirAlt[2] = sun.z; p.sunDirAlt[3] = Lighting.altitude;
    p.sunEnabled = Lighting.directLightingEnabled ? 1 : 0;
    p.userSphere[0] = UserSphere.pos.x; p.userSphere[1] = UserSphere.pos.y; p.userSphere[2] = UserSphere.pos.z;
    p.userSphere[3] = UserSphere.radius;
    const Vec3f em = Vec3f(1, 1, 1) * UserSphere.emittance;
    p.userSphereEm[0] = em.x; p.userSphereEm[1] = em.y; p.userSphereEm[2] = em.z;
    p.userSphereFlags = UserSphere.flags;
    p.pixelSize = ComputePixelSize(CurrentCamera, Viewport.height);
    p.cameraPos[0] = CurrentCamera.Pos.x; p.cameraPos[1] = CurrentCamera.Pos.y; p.cameraPos[2] = CurrentCamera.Pos.z;
    p.maxSegments = (int32_t)MaxPathSegments;
    p.minWeight = MinWeight;
    return p;
}

// ---- rendering ----------------------------------------------------------------------------------
void Renderer::RenderDirectLighting() {
    if (!IsOK) return;
    const gpuart_params p = MakeParams();
    Check(gpuart_hip_render_direct(Backend, &p), "rendering direct lighting");
}

void Renderer::ResetPathTracing() {
    PathTracing.numPathsRendered = 0;
    CountBase = 0;
    if (Converge) ResetConvergeNow();
    if (Adaptive) ResetAdaptiveNow();
    if (Backend && Viewport.width) {
        gpuart_hip_pt_reset(Backend);
        // the passes RenderPathTracingPass() will submit until pathsPerPixel is reached (a scheduling hint)
        const unsigned per = PathTracing.pathsPerPass ? PathTracing.pathsPerPass : 1;
        gpuart_hip_pt_plan(Backend, (PathTracing.pathsPerPixel + per - 1) / per);
    }
}

void Renderer::RestartPathTracing(unsigned pathsPerPass, unsigned pathsPerPixel) {
    PathTracing.pathsPerPixel = pathsPerPixel;
    PathTracing.pathsPerPass = std::min(pathsPerPass, pathsPerPixel);
    ResetPathTracing();
}

void Renderer::ExtendPathTracing(unsigned pathsPerPass, unsigned pathsPerPixel) {
    PathTracing.pathsPerPixel = std::max(pathsPerPixel, PathTracing.numPathsRendered);
    PathTracing.pathsPerPass = std::max(1u, std::min(pathsPerPass, PathTracing.pathsPerPixel));
    if (Backend && Viewport.width) {
        const unsigned left = PathTracing.pathsPerPixel - PathTracing.numPathsRendered;
        gpuart_hip_pt_plan(Backend, (left + PathTracing.pathsPerPass - 1) / PathTracing.pathsPerPass);
    }
}

unsigned Renderer::RenderPathTracingPass() {
    if (!IsOK) return PathTracing.numPathsRendered;
    if (PathTracing.numPathsRendered < PathTracing.pathsPerPixel) {
        const unsigned pathsToRender =
            std::min(PathTracing.pathsPerPass, PathTracing.pathsPerPixel - PathTracing.numPathsRendered);
        const gpuart_params p = MakeParams();
        // RandSeed: four draws per pass from the never re-seeded generator (reference src/renderer.cpp:585-589)
        std::uniform_real_distribution<float> distr(0, 1);
        float seed[4];
        for (float &s : seed) s = distr(RndGen);
        if (Check(gpuart_hip_pt_pass(Backend, &p, seed, (int)pathsToRender), "rendering a path-tracing pass"))
            PathTracing.numPathsRendered += pathsToRender;
    }
    return PathTracing.numPathsRendered;
}

bool Renderer::ReadDirectLighting(float *rgba) {
    return IsOK && Check(gpuart_hip_read(Backend, 0, rgba, 1.0f), "reading the frame");
}

bool Renderer::ReadRadiance(float *rgba, bool normalized) {
    if (IsOK && normalized && NonUniform)  // every block by its own count, through a device buffer
        return rgba && AccumMem.Fit((size_t)Tile.w * Tile.h, 16, "allocating the normalised frame") && ExportNormalized((float *)AccumMem.mem) &&
               ReadPlane(rgba, AccumMem.mem, 16, "reading the normalised frame");
    return IsOK && Check(gpuart_hip_read(Backend, 1, rgba, Divisor(normalized)), "reading the radiance accumulator");
}

namespace {
bool finite(float x) { return x - x == 0.0f; }
bool checkHip(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    std::cerr << "Renderer: " << what << ": " << hipGetErrorString(e) << std::endl;
    return false;
}
/// The parts of DenoiseMem for a tile of n pixels.
struct ViewBuffers {
    float *radiance;
    gpuart_ray_hit *hits;
    float *filtered;
    int32_t *prims;
    ViewBuffers(void *mem, size_t n)
        : radiance((float *)mem), hits((gpuart_ray_hit *)((char *)mem + n * 16)), filtered((float *)((char *)mem + n * 48)),
          prims((int32_t *)((char *)mem + n * 64)) {}
};
/// MomentsMem's planes: the packed moments, their blend, the radiance blend's len and the error map.
struct MomentBuffers {
    float *packed, *blend, *len, *e;
    MomentBuffers(void *mem, size_t n)
        : packed((float *)mem), blend((float *)((char *)mem + n * 16)), len((float *)((char *)mem + n * 32)), e((float *)((char *)mem + n * 36)) {}
};
/// AntiLagMem's planes: the fast blend, its len and the mix's alpha.
struct AntiLagBuffers {
    float *fast, *len, *alpha;
    AntiLagBuffers(void *mem, size_t n) : fast((float *)mem), len((float *)((char *)mem + n * 16)), alpha((float *)((char *)mem + n * 20)) {}
};
}  // namespace

template <class H, class L>
bool Renderer::Run(int status, H *h, const L &lib, const char *what) {
    return Check(status, what, lib.lastError) && Check(lib.finish(h), what, lib.lastError);
}

void Renderer::PixelBuffer::Release() {
    if (mem) (void)hipFree(mem);
    mem = nullptr;
    count = 0;
}

bool Renderer::PixelBuffer::Fit(size_t n, size_t bytesPerElement, const char *what) {
    if (n == count) return true;
    Release();
    if (!checkHip(hipMalloc(&mem, n * bytesPerElement), what)) return false;
    count = n;
    return true;
}

bool Renderer::ReadPlane(void *host, const void *plane, size_t bytesPerPixel, const char *what) {
    return checkHip(hipMemcpy(host, plane, (size_t)Tile.w * Tile.h * bytesPerPixel, hipMemcpyDeviceToHost), what);
}

bool Renderer::EnsureGBuffer() {
    if (!checkHip(hipSetDevice(Device), "hipSetDevice")) return false;
    const size_t n = (size_t)Tile.w * Tile.h;
    if (n != DenoiseMem.count) GBufferValid = false;
    if (!DenoiseMem.Fit(n, 16 + 32 + 16 + 4, "allocating the denoiser's buffers")) return false;
    const ViewBuffers b(DenoiseMem.mem, n);
    const float us[4] = {UserSphere.pos.x, UserSphere.pos.y, UserSphere.pos.z, UserSphere.radius};
    if (!GBufferValid || memcmp(us, GBufferSphere, sizeof us) != 0) {
        GBufferValid = false;
        EdgeListValid = false;  // (the edge list and the sub-pixel records are this G-buffer's,
        UpscaleValid = false;   //  and so is the larger frame's G-buffer)
        if (!Check(gpuart_hip_gbuffer(Backend, us, b.hits, b.prims), "building the G-buffer")) return false;
        memcpy(GBufferSphere, us, sizeof us);
        GBufferValid = true;
    }
    return true;
}

bool Renderer::StageView() {
    if (!EnsureGBuffer()) return false;
    const ViewBuffers b(DenoiseMem.mem, (size_t)Tile.w * Tile.h);
    if (!ExportNormalized(b.radiance)) return false;
    if (!FireflyOn) return true;
    // in place: every filtered read and every commit takes the clamped frame; the accumulator stays what it is
    return Ensure(Despeckle, DS) &&
           Run(gpuart_despeckle_run(Despeckle, b.radiance, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h, &FireflyParams, b.radiance, nullptr),
               Despeckle, DS, "clamping the fireflies");
}

// ---- the firefly clamp (include/gpuart_despeckle.h) -----------------------------------------------------------------------
bool Renderer::SetFireflyClamp(bool on, const gpuart_despeckle_params *p) {
    gpuart_despeckle_params v;
    if (p) {
        // the ranges gpuart_despeckle_run accepts: a commit inside a setter has nobody to report them to
        if (p->radius < 1 || p->radius > 2 || p->rank < 1 || p->rank > 4 || !finite(p->k) || !(p->k >= 1) || !finite(p->floor) ||
            !(p->floor >= 0) || p->min_count < 1 || p->min_count > 24) {
            std::cerr << "Renderer: firefly-clamp parameters out of range." << std::endl;
            return false;
        }
        v = *p;
    } else {
        gpuart_despeckle_defaults(&v);
    }
    // a history that has seen other inputs
    if (on != FireflyOn || memcmp(&v, &FireflyParams, sizeof v) != 0) DropTemporalHistory();
    FireflyParams = v;
    FireflyOn = on;
    return true;
}

bool Renderer::ReadFireflySummary(gpuart_despeckle_summary *out) {
    return out && Despeckle && checkHip(hipSetDevice(Device), "hipSetDevice") &&
           Check(gpuart_despeckle_read_summary(Despeckle, out), "reading the firefly clamp's summary", gpuart_despeckle_last_error);
}

bool Renderer::StageBlockPaths() {
    const size_t nb = TileBlocks();
    if (!BlockPathsMem.Fit(nb, sizeof(uint32_t), "allocating the block counts")) return false;
    if (!CountBase) return Check(gpuart_hip_export_block_paths(Backend, (uint32_t *)BlockPathsMem.mem), "exporting the block counts");
    // a loaded checkpoint's paths are in the accumulator but not in the back end's counts: added on the way
    std::vector<uint32_t> counts(nb);
    if (!Check(gpuart_hip_read_block_paths(Backend, counts.data()), "reading the block counts")) return false;
    for (uint32_t &c : counts) c += CountBase;
    return checkHip(hipMemcpy(BlockPathsMem.mem, counts.data(), nb * sizeof(uint32_t), hipMemcpyHostToDevice), "staging the block counts");
}

bool Renderer::Export(int which, float *device, float div, bool withBlockPaths) {
    if (!Check(gpuart_hip_export(Backend, which, device, div), "exporting the frame") || (withBlockPaths && !StageBlockPaths())) return false;
    return Check(gpuart_hip_finish(Backend), "waiting for the device");
}

bool Renderer::ExportNormalized(float *device) {
    if (!NonUniform) return Export(1, device, Divisor(true));
    return Export(1, device, 1.0f, true) &&
           Run(gpuart_adaptive_normalize(Adaptive, device, (const uint32_t *)BlockPathsMem.mem, device, Tile.w, Tile.h), Adaptive, AD, "normalising by the blocks' counts");
}

// ---- the frames a read can ask for ------------------------------------------------------------------------------------
bool Renderer::StageSource(gpuart_display_source source, float lumFloor, const gpuart_denoise_params *dn, const gpuart_refine_params *rf,
                           const gpuart_temporal_params *tp, float *own, const float *&plane) {
    switch (source) {
    case GPUART_DISPLAY_RADIANCE: plane = own; return own && ExportNormalized(own);
    case GPUART_DISPLAY_DIRECT: plane = own; return own && Export(0, own, 1.0f);
    case GPUART_DISPLAY_DENOISED: return StageDenoised(dn, plane);
    case GPUART_DISPLAY_PREVIEW: return StagePreview(dn, tp, plane);
    case GPUART_DISPLAY_GUIDED_PREVIEW: return StageGuidedPreview(lumFloor, rf, tp, plane);
    case GPUART_DISPLAY_REFINED: return StageRefined(lumFloor, rf, plane);
    default:
        std::cerr << "Renderer: ReadDisplay: no such source " << (int)source << std::endl;
        return false;
    }
}

bool Renderer::ReadStaged(float *rgba, const char *what, gpuart_display_source source, float lumFloor, const gpuart_denoise_params *dn,
                          const gpuart_refine_params *rf, const gpuart_temporal_params *tp) {
    const float *plane;
    return rgba && StageSource(source, lumFloor, dn, rf, tp, nullptr, plane) && ReadPlane(rgba, plane, 16, what);
}

bool Renderer::ReadDenoised(float *rgba, const gpuart_denoise_params *p) {
    return ReadStaged(rgba, "reading the denoised frame", GPUART_DISPLAY_DENOISED, 0, p, nullptr, nullptr);
}

bool Renderer::ReadPreview(float *rgba, const gpuart_denoise_params *dn, const gpuart_temporal_params *tp) {
    return ReadStaged(rgba, "reading the preview", GPUART_DISPLAY_PREVIEW, 0, dn, nullptr, tp);
}

bool Renderer::ReadGuidedPreview(float *rgba, float lumFloor, const gpuart_refine_params *rf, const gpuart_temporal_params *tp) {
    return ReadStaged(rgba, "reading the guided preview", GPUART_DISPLAY_GUIDED_PREVIEW, lumFloor, nullptr, rf, tp);
}

bool Renderer::ReadRefined(float *rgba, float lumFloor, const gpuart_refine_params *p) {
    return ReadStaged(rgba, "reading the refined frame", GPUART_DISPLAY_REFINED, lumFloor, nullptr, p, nullptr);
}

bool Renderer::StageDenoised(const gpuart_denoise_params *p, const float *&plane) {
    if (!IsOK || !Ensure(Denoiser, DN) || !StageView()) return false;
    const ViewBuffers b(DenoiseMem.mem, (size_t)Tile.w * Tile.h);
    plane = b.filtered;
    return Run(gpuart_denoise_run(Denoiser, b.radiance, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h, p, b.filtered), Denoiser, DN, "denoising") &&
           ResolveEdges(plane);
}

// ---- geometric edges from a sub-pixel G-buffer (include/gpuart_edges.h) ---------------------------------------------------
bool Renderer::SetEdgeResolve(bool on, const gpuart_edges_params *p) {
    gpuart_edges_params v;
    if (p) {
        // the ranges gpuart_edges_mark and gpuart_hip_trace_subpixel accept
        if (p->n_sub < 1 || p->n_sub > GPUART_EDGES_MAX_SUB || !(p->normal_min >= -1) || !(p->normal_min <= 1) || !finite(p->plane_tol) ||
            !(p->plane_tol >= 0)) {
            std::cerr << "Renderer: edge-resolve parameters out of range." << std::endl;
            return false;
        }
        v = *p;
    } else {
        gpuart_edges_defaults(&v);
    }
    if (memcmp(&v, &EdgeParams, sizeof v) != 0) EdgeListValid = false;
    EdgeParams = v;
    EdgeOn = on;
    return true;
}

bool Renderer::ResolveEdges(const float *&plane) {
    if (!EdgeOn) return true;
    if (!checkHip(hipSetDevice(Device), "hipSetDevice") || !Ensure(Edges, ED)) return false;
    const size_t n = (size_t)Tile.w * Tile.h;
    if (n + 1 != EdgeMem.count) EdgeListValid = false;
    if (!EdgeMem.Fit(n + 1, 16 + 4, "allocating the edge resolve's buffers")) return false;
    const ViewBuffers b(DenoiseMem.mem, n);
    float *out = (float *)EdgeMem.mem;
    uint32_t *list = (uint32_t *)((char *)EdgeMem.mem + n * 16), *count = list + n;
    const size_t subs = (size_t)EdgeCount * EdgeParams.n_sub;
    if (!EdgeListValid || EdgeFlags != UserSphere.flags) {
        EdgeListValid = false;
        if (!Run(gpuart_edges_mark(Edges, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h, &EdgeParams, list, count), Edges, ED, "marking the edge pixels") ||
            !checkHip(hipMemcpy(&EdgeCount, count, sizeof EdgeCount, hipMemcpyDeviceToHost), "reading the number of edge pixels"))
            return false;
        const size_t m = (size_t)EdgeCount * EdgeParams.n_sub;
        if (!EdgeSubMem.Fit(m ? m : 1, 32 + 4, "allocating the sub-pixel records")) return false;
        const float pixelSize = ComputePixelSize(CurrentCamera, Viewport.height);
        float uv[2 * GPUART_EDGES_MAX_SUB];
        if (!Check(gpuart_edges_offsets(EdgeParams.n_sub, uv), "making the sub-pixel offsets", gpuart_edges_last_error)) return false;
        if (!Check(gpuart_hip_trace_subpixel(Backend, list, EdgeCount, uv, EdgeParams.n_sub, pixelSize, GBufferSphere,
                                             (gpuart_ray_hit *)EdgeSubMem.mem, (int32_t *)((char *)EdgeSubMem.mem + m * 32)),
                   "tracing the sub-pixel rays") ||
            !Check(gpuart_hip_finish(Backend), "waiting for the device"))
            return false;
        EdgeFlags = UserSphere.flags;
        EdgeListValid = true;
        return ResolveEdges(plane);  // (with the cache valid: once)
    }
    if (!Run(gpuart_edges_resolve(Edges, plane, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h, list, EdgeCount,
                                  (const gpuart_ray_hit *)EdgeSubMem.mem, (const int32_t *)((char *)EdgeSubMem.mem + subs * 32), &EdgeParams, out),
             Edges, ED, "resolving the edges"))
        return false;
    plane = out;
    return true;
}

// ---- temporal history (include/gpuart_temporal.h) ---------------------------------------------------------------------
bool Renderer::SetTemporalHistory(bool on, const gpuart_temporal_params *tp) {
    if (on && NonUniform) {  // (before the parameters are taken: a refusal changes nothing)
        std::cerr << "Renderer: temporal history after adaptive sampling retired blocks: the blend takes one path count." << std::endl;
        return false;
    }
    if (tp) {
        // the ranges gpuart_temporal_accumulate accepts: a commit inside a setter has nobody to report them to
        if (!finite(tp->max_history) || !(tp->max_history >= 0) || !finite(tp->plane_tol) || !(tp->plane_tol >= 0) ||
            !(tp->normal_min >= -1) || !(tp->normal_min <= 1)) {
            std::cerr << "Renderer: temporal parameters out of range." << std::endl;
            return false;
        }
        TemporalParams = *tp;
    } else {
        gpuart_temporal_defaults(&TemporalParams);
    }
    if (!on) DropTemporalHistory();
    TemporalOn = on;
    return true;
}

void Renderer::DropTemporalHistoryNow() {
    if (Temporal) gpuart_temporal_reset(Temporal);
    if (TemporalMoments) gpuart_temporal_reset(TemporalMoments);
    if (TemporalFast) gpuart_temporal_reset(TemporalFast);
    HistoryCommitted = false;
}

bool Renderer::MakeTemporalView(gpuart_temporal_view &v) const {
    CurrentBasis.Pos.storeIn(v.pos); CurrentBasis.BottomLeft.storeIn(v.bottomLeft);
    CurrentBasis.DeltaHorz.storeIn(v.deltaHorz); CurrentBasis.DeltaVert.storeIn(v.deltaVert);
    if (gpuart_hip_get_share(Backend, &v.geom) != 0) return false;
    v.userSphere[0] = UserSphere.pos.x; v.userSphere[1] = UserSphere.pos.y; v.userSphere[2] = UserSphere.pos.z;
    v.userSphere[3] = UserSphere.radius;
    v.userSphereFlags = UserSphere.flags;
    return true;
}

bool Renderer::BlendHistory(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit, float *len) {
    const ViewBuffers b(DenoiseMem.mem, (size_t)Tile.w * Tile.h);
    return Run(gpuart_temporal_accumulate(Temporal, b.radiance, PathTracing.numPathsRendered, b.hits, b.prims, Tile.w, Tile.h, &v,
                                          tp ? tp : &TemporalParams, commit, b.filtered, len),
               Temporal, TP, commit ? "committing the view to the history" : "blending the history");
}

bool Renderer::BlendMoments(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit) {
    const size_t n = (size_t)Tile.w * Tile.h;
    const ViewBuffers b(DenoiseMem.mem, n);
    const MomentBuffers mb(MomentsMem.mem, n);
    return Run(gpuart_moments_pack(Moments, b.radiance, PathTracing.numPathsRendered, Tile.w, Tile.h, mb.packed), Moments, MO, "packing the moments") &&
           Run(gpuart_temporal_accumulate(TemporalMoments, mb.packed, PathTracing.numPathsRendered, b.hits, b.prims, Tile.w, Tile.h, &v,
                                          tp ? tp : &TemporalParams, commit, mb.blend, nullptr),
               TemporalMoments, TPM, commit ? "committing the moments to their history" : "blending the moments' history");
}

void Renderer::CommitTemporalView() {
    if (!TemporalOn || !IsOK || PathTracing.numPathsRendered == 0) return;
    gpuart_temporal_view v;
    // the same commit for the moments and the fast history: the histories have seen the same views or none
    HistoryCommitted = Ensure(Temporal, TP) && StageView() && MakeTemporalView(v) && BlendHistory(v, nullptr, true, nullptr) &&
                       (!VarianceOn || (EnsureVarianceHandles() && BlendMoments(v, nullptr, true))) &&
                       (!AntiLagActive() || (EnsureAntiLagHandles() && BlendFast(v, nullptr, true)));
    if (!HistoryCommitted) DropTemporalHistoryNow();  // A commit that fails leaves no history rather than a stale one.
}

// ---- the history's measured variance (include/gpuart_moments.h) -----------------------------------------------------------
bool Renderer::SetHistoryVariance(bool on, const gpuart_moments_params *p) {
    if (p) {
        // the ranges gpuart_moments_error accepts
        if (!finite(p->min_batches) || !(p->min_batches > 1) || !finite(p->spatial_k) || !(p->spatial_k >= 0)) {
            std::cerr << "Renderer: moments parameters out of range." << std::endl;
            return false;
        }
        MomentsParams = *p;
    } else {
        gpuart_moments_defaults(&MomentsParams);
    }
    if (on != VarianceOn) DropTemporalHistory();  // a history the other handle has not seen
    VarianceOn = on;
    return true;
}

bool Renderer::EnsureVarianceHandles() {
    if (!checkHip(hipSetDevice(Device), "hipSetDevice")) return false;
    if (!Ensure(Temporal, TP) || !Ensure(TemporalMoments, TPM) || !Ensure(Moments, MO)) return false;
    return MomentsMem.Fit((size_t)Tile.w * Tile.h, 16 + 16 + 4 + 4, "allocating the moments' buffers");
}

// ---- a fast history where the lighting changed (include/gpuart_antilag.h) -------------------------------------------------
bool Renderer::SetHistoryAntiLag(bool on, const gpuart_antilag_params *p) {
    if (p) {
        // the ranges gpuart_antilag_mix accepts; fast_history becomes a max_history
        if (!finite(p->fast_history) || !(p->fast_history >= 0) || !finite(p->min_batches) || !(p->min_batches > 1) || !finite(p->min_votes) ||
            !(p->min_votes >= 1) || !finite(p->clip) || !(p->clip > 0) || !finite(p->z_lo) || !(p->z_lo >= 0) || !finite(p->z_hi) ||
            !(p->z_hi > p->z_lo)) {
            std::cerr << "Renderer: anti-lag parameters out of range." << std::endl;
            return false;
        }
        AntiLagParams = *p;
    } else {
        gpuart_antilag_defaults(&AntiLagParams);
    }
    if (on != AntiLagOn) DropTemporalHistory();  // a history the third handle has not seen
    AntiLagOn = on;
    return true;
}

bool Renderer::EnsureAntiLagHandles() {
    if (!checkHip(hipSetDevice(Device), "hipSetDevice")) return false;
    if (!Ensure(TemporalFast, TPF) || !Ensure(AntiLag, AL)) return false;
    return AntiLagMem.Fit((size_t)Tile.w * Tile.h, 16 + 4 + 4, "allocating the anti-lag buffers");
}

bool Renderer::BlendFast(const gpuart_temporal_view &v, const gpuart_temporal_params *tp, bool commit) {
    const size_t n = (size_t)Tile.w * Tile.h;
    const ViewBuffers b(DenoiseMem.mem, n);
    const AntiLagBuffers ab(AntiLagMem.mem, n);
    gpuart_temporal_params fp = tp ? *tp : TemporalParams;
    if (AntiLagParams.fast_history < fp.max_history) fp.max_history = AntiLagParams.fast_history;
    return Run(gpuart_temporal_accumulate(TemporalFast, b.radiance, PathTracing.numPathsRendered, b.hits, b.prims, Tile.w, Tile.h, &v, &fp, commit,
                                          ab.fast, ab.len),
               TemporalFast, TPF, commit ? "committing the view to the fast history" : "blending the fast history");
}

bool Renderer::StageGuidedPreview(float lumFloor, const gpuart_refine_params *rf, const gpuart_temporal_params *tp, const float *&plane) {
    if (!IsOK || !VarianceOn || !TemporalOn || PathTracing.numPathsRendered == 0) return false;
    gpuart_temporal_view v;
    if (!Ensure(Refine, RF) || !EnsureVarianceHandles() || !StageView() || !MakeTemporalView(v)) return false;
    const size_t n = (size_t)Tile.w * Tile.h;
    const ViewBuffers b(DenoiseMem.mem, n);
    const MomentBuffers mb(MomentsMem.mem, n);
    // (without a commit both handles have no history: every blend is its input and len = s)
    if (!BlendHistory(v, tp, false, mb.len) || !BlendMoments(v, tp, false)) return false;
    if (AntiLagActive()) {
        // the long blend and its len move towards the short one where the lighting changed; the error map below sees the mixed len
        if (!EnsureAntiLagHandles() || !BlendFast(v, tp, false)) return false;
        const AntiLagBuffers ab(AntiLagMem.mem, n);
        if (!Run(gpuart_antilag_mix(AntiLag, b.filtered, mb.len, ab.fast, ab.len, mb.blend, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h,
                                    &AntiLagParams, b.filtered, mb.len, ab.alpha),
                 AntiLag, AL, "mixing the fast history in")) return false;
    }
    if (!Run(gpuart_moments_error(Moments, b.filtered, mb.len, mb.blend, b.hits, b.prims, UserSphere.flags, lumFloor, Tile.w, Tile.h, &MomentsParams, mb.e),
             Moments, MO, "measuring the history's variance")) return false;
    plane = b.filtered;  // (the filter may run in place: include/gpuart_refine.h)
    return Run(gpuart_refine_run(Refine, b.filtered, b.hits, b.prims, UserSphere.flags, mb.e, lumFloor, Tile.w, Tile.h, rf, b.filtered), Refine, RF, "filtering") &&
           ResolveEdges(plane);
}

bool Renderer::StagePreview(const gpuart_denoise_params *dn, const gpuart_temporal_params *tp, const float *&plane) {
    if (!TemporalOn || !HistoryCommitted || PathTracing.numPathsRendered == 0) return StageDenoised(dn, plane);
    gpuart_temporal_view v;
    if (!IsOK || !Ensure(Denoiser, DN) || !StageView() || !MakeTemporalView(v) || !BlendHistory(v, tp, false, nullptr)) return false;
    const ViewBuffers b(DenoiseMem.mem, (size_t)Tile.w * Tile.h);
    plane = b.filtered;  // (the filter may run in place: include/gpuart_denoise.h)
    return Run(gpuart_denoise_run(Denoiser, b.filtered, b.hits, b.prims, UserSphere.flags, Tile.w, Tile.h, dn, b.filtered), Denoiser, DN, "denoising") &&
           ResolveEdges(plane);
}

// ---- the batch loop of RenderUntil and RenderAdaptive ---------------------------------------------------------------------------
template <class Show, class Judge>
int Renderer::RenderBatches(unsigned batchPaths, const unsigned &batches, const unsigned &total, Show show, Judge judge) {
    const unsigned &rendered = PathTracing.numPathsRendered;
    // paths the estimate has never seen — a loaded checkpoint, plain passes after a restart, the other estimate's batches — are its
    // first batch, of their own weight
    if (batches == 0 && rendered > 0 && !show()) return -1;
    for (;;) {
        if (rendered < PathTracing.pathsPerPixel) {
            const unsigned target = rendered + std::min(batchPaths, PathTracing.pathsPerPixel - rendered);
            const unsigned per = std::max(1u, PathTracing.pathsPerPass);
            // the passes of this batch are all the back end will see before the export observes them (a scheduling hint)
            gpuart_hip_pt_plan(Backend, (target - rendered + per - 1) / per);
            while (rendered < target) {
                const unsigned before = rendered;
                if (RenderPathTracingPass() == before) return -1;  // (the pass failed: Check has said why)
            }
        }
        if (rendered > total && !show()) return -1;
        if (batches >= 2)
            if (const int rc = judge()) return rc;
        if (rendered >= PathTracing.pathsPerPixel) return 0;
    }
}

// ---- render until converged (include/gpuart_converge.h) -----------------------------------------------------------------
void Renderer::ResetConvergeNow() {
    gpuart_converge_reset(Converge);
    ConvergeBatches = ConvergeTotal = 0;
}

int Renderer::RenderUntil(float threshold, float maxAboveShare, unsigned batchPaths, float lumFloor, gpuart_converge_summary *last) {
    if (!IsOK) return -1;
    if (!finite(threshold) || !(threshold >= 0) || !(maxAboveShare >= 0) || batchPaths == 0 || !finite(lumFloor) || !(lumFloor > 0)) {
        std::cerr << "Renderer: RenderUntil arguments out of range." << std::endl;
        return -1;
    }
    if (NonUniform) {
        std::cerr << "Renderer: RenderUntil after adaptive sampling retired blocks: its estimate keeps one path count for the frame (RenderAdaptive continues)." << std::endl;
        return -1;
    }
    if (!Ensure(Converge, CV) || !checkHip(hipSetDevice(Device), "hipSetDevice")) return -1;
    if (!AccumMem.Fit((size_t)Tile.w * Tile.h, 16, "allocating the estimator's copy of the accumulator")) return -1;
    float *accum = (float *)AccumMem.mem;
    // the raw accumulator as one more batch: divide_by 1 copies the sums exactly; a buffer of its own: the denoiser's cached view
    // (StageView) stays as it is. The wait lets the next export reuse the buffer.
    auto show = [&]() {
        if (!Export(1, accum, 1.0f)) return false;
        if (!Check(gpuart_converge_update(Converge, accum, PathTracing.numPathsRendered, Tile.w, Tile.h), "updating the convergence estimate", CV.lastError))
            return false;
        ConvergeTotal = PathTracing.numPathsRendered;
        ConvergeBatches++;
        AdaptiveIsLast = false;
        return Check(gpuart_converge_finish(Converge), "updating the convergence estimate", CV.lastError);
    };
    auto judge = [&]() {
        gpuart_converge_summary s;
        if (!Check(gpuart_converge_measure(Converge, threshold, lumFloor, nullptr, &s), "measuring the convergence", CV.lastError)) return -1;
        if (last) *last = s;
        return (double)s.above <= (double)maxAboveShare * (double)s.pixels ? 1 : 0;
    };
    return RenderBatches(batchPaths, ConvergeBatches, ConvergeTotal, show, judge);
}

// ---- adaptive sampling (include/gpuart_adaptive.h) ------------------------------------------------------------------------------
void Renderer::ResetAdaptiveNow() {
    gpuart_adaptive_reset(Adaptive);
    AdaptiveBatches = AdaptiveTotal = AdaptiveActive = 0;
    NonUniform = AdaptiveIsLast = false;
}

int Renderer::RenderAdaptive(float threshold, unsigned minPaths, unsigned batchPaths, float lumFloor, gpuart_adaptive_summary *last) {
    if (!IsOK) return -1;
    if (!finite(threshold) || !(threshold >= 0) || minPaths == 0 || batchPaths == 0 || !finite(lumFloor) || !(lumFloor > 0)) {
        std::cerr << "Renderer: RenderAdaptive arguments out of range." << std::endl;
        return -1;
    }
    if (TemporalOn) {
        std::cerr << "Renderer: RenderAdaptive while temporal history is on: the blend takes one path count." << std::endl;
        return -1;
    }
    if (!Ensure(Adaptive, AD) || !checkHip(hipSetDevice(Device), "hipSetDevice")) return -1;
    if (!AccumMem.Fit((size_t)Tile.w * Tile.h, 16, "allocating the estimator's copy of the accumulator")) return -1;
    float *accum = (float *)AccumMem.mem;
    std::vector<uint32_t> list(TileBlocks());
    // the raw accumulator and the blocks' counts as one more batch, outside the denoiser's cached view (RenderUntil's show)
    auto show = [&]() {
        if (!Export(1, accum, 1.0f, true)) return false;
        if (!Check(gpuart_adaptive_update(Adaptive, accum, (const uint32_t *)BlockPathsMem.mem, Tile.w, Tile.h), "updating the adaptive estimate", AD.lastError))
            return false;
        AdaptiveTotal = PathTracing.numPathsRendered;
        AdaptiveBatches++;
        AdaptiveIsLast = true;
        return Check(gpuart_adaptive_finish(Adaptive), "updating the adaptive estimate", AD.lastError);
    };
    auto judge = [&]() {
        gpuart_adaptive_summary s;
        if (!Check(gpuart_adaptive_select(Adaptive, threshold, lumFloor, minPaths, nullptr, list.data(), &s), "selecting the active blocks", AD.lastError)) return -1;
        if (last) *last = s;
        // the list only ever shrinks: the same length is the same list
        if (s.active_blocks < s.blocks && (!NonUniform || s.active_blocks != AdaptiveActive)) {
            if (!Check(gpuart_hip_set_active_blocks(Backend, list.data(), s.active_blocks), "setting the active blocks")) return -1;
            NonUniform = true;
            AdaptiveActive = s.active_blocks;
        }
        return s.active_blocks == 0 ? 1 : 0;
    };
    return RenderBatches(batchPaths, AdaptiveBatches, AdaptiveTotal, show, judge);
}

bool Renderer::ReadSampleCounts(uint32_t *perPixel) {
    if (!IsOK || !perPixel) return false;
    std::vector<uint32_t> counts(TileBlocks());
    if (!Check(gpuart_hip_read_block_paths(Backend, counts.data()), "reading the block counts")) return false;
    const unsigned bw = (Tile.w + 7) / 8;
    for (unsigned y = 0; y < Tile.h; y++)
        for (unsigned x = 0; x < Tile.w; x++) perPixel[(size_t)y * Tile.w + x] = counts[(size_t)(y / 8) * bw + x / 8] + CountBase;
    return true;
}

// ---- the error map of the estimate that saw the last batch ------------------------------------------------------------------
bool Renderer::StageErrorMap(float lumFloor, const float *&map) {
    const Estimate which = LastEstimate();
    if (!IsOK || which == NONE || !checkHip(hipSetDevice(Device), "hipSetDevice")) return false;
    if (!ErrorMem.Fit((size_t)Tile.w * Tile.h, 4, "allocating the error map")) return false;
    float *e = (float *)ErrorMem.mem;
    map = e;
    if (which == ADAPTIVE) return Run(gpuart_adaptive_error_map(Adaptive, lumFloor, e, Tile.w, Tile.h), Adaptive, AD, "measuring the error map");
    // a measure changes nothing of the estimate; it waits for the map itself
    gpuart_converge_summary s;
    return Check(gpuart_converge_measure(Converge, 0.0f, lumFloor, e, &s), "measuring the error map", CV.lastError);
}

bool Renderer::ReadErrorMap(float *e, float lumFloor) {
    const float *map;
    return e && StageErrorMap(lumFloor, map) && ReadPlane(e, map, 4, "reading the error map");
}

bool Renderer::StageRefined(float lumFloor, const gpuart_refine_params *p, const float *&plane) {
    const float *map;
    if (!IsOK || LastEstimate() == NONE || !Ensure(Refine, RF) || !StageView() || !StageErrorMap(lumFloor, map)) return false;
    const ViewBuffers b(DenoiseMem.mem, (size_t)Tile.w * Tile.h);
    plane = b.filtered;
    return Run(gpuart_refine_run(Refine, b.radiance, b.hits, b.prims, UserSphere.flags, map, lumFloor, Tile.w, Tile.h, p, b.filtered), Refine, RF, "filtering") &&
           ResolveEdges(plane);
}

// ---- the display stage (include/gpuart_display.h) ---------------------------------------------------------------------------
bool Renderer::ReadDisplay(uint8_t *rgba8, gpuart_display_source source, const gpuart_display_params *dp, float lumFloor) {
    if (!IsOK || !rgba8) return false;
    if (!checkHip(hipSetDevice(Device), "hipSetDevice") || !Ensure(Display, DP)) return false;
    const size_t n = (size_t)Tile.w * Tile.h;
    if (!DisplayMem.Fit(n, 16 + 4, "allocating the display stage's buffers")) return false;
    uint8_t *words = (uint8_t *)DisplayMem.mem + n * 16;
    const float *plane;
    if (!StageSource(source, lumFloor, nullptr, nullptr, nullptr, (float *)DisplayMem.mem, plane)) return false;
    return Run(gpuart_display_run(Display, plane, words, Tile.w, Tile.h, Tile.x, Tile.y, dp), Display, DP, "encoding the frame") &&
           ReadPlane(rgba8, words, 4, "reading the 8-bit frame");
}

// ---- the upscaler (include/gpuart_upscale.h) --------------------------------------------------------------------------------
bool Renderer::StageUpscaled(gpuart_display_source source, uint32_t scale, float lumFloor, const gpuart_upscale_params *p, const float *&plane,
                             size_t &n) {
    if (!IsOK) return false;
    // the refusals first: nothing has changed when one of them returns
    if (scale < GPUART_UPSCALE_MIN_SCALE || scale > GPUART_UPSCALE_MAX_SCALE) {
        std::cerr << "Renderer: ReadUpscaled: scale " << scale << " is not in 2..4." << std::endl;
        return false;
    }
    if (p && (!(p->normal_min >= -1) || !(p->normal_min <= 1) || !finite(p->plane_tol) || !(p->plane_tol >= 0))) {
        std::cerr << "Renderer: upscaler parameters out of range." << std::endl;
        return false;
    }
    if (source < GPUART_DISPLAY_RADIANCE || source > GPUART_DISPLAY_REFINED) {
        std::cerr << "Renderer: ReadUpscaled: no such source " << (int)source << std::endl;
        return false;
    }
    gpuart_tile_geom g;
    if (!Check(gpuart_hip_get_share(Backend, &g), "reading the tile")) return false;
    if (g.th > g.band_rows && g.band_stride != g.band_rows) {
        std::cerr << "Renderer: ReadUpscaled: the tile is interleaved with other renderers' (a share of several GPUs); its larger frame would "
                     "be no rectangle." << std::endl;
        return false;
    }
    if (!checkHip(hipSetDevice(Device), "hipSetDevice") || !Ensure(Upscaler, UP)) return false;
    const size_t lo = (size_t)Tile.w * Tile.h;
    n = lo * scale * scale;
    // the low plane, with edge resolve skipped for this call: the switch and its cache stay what they are
    if (!DisplayMem.Fit(lo, 16 + 4, "allocating the display stage's buffers")) return false;
    const bool edgeOn = EdgeOn;
    EdgeOn = false;
    const float *low;
    const bool staged = StageSource(source, lumFloor, nullptr, nullptr, nullptr, (float *)DisplayMem.mem, low);
    EdgeOn = edgeOn;
    if (!staged || !EnsureGBuffer()) return false;  // (RADIANCE and DIRECT stage no view)
    // the larger frame's G-buffer, of the view whose G-buffer is cached
    if (n != UpscaleMem.count || scale != UpscaleScale) UpscaleValid = false;
    if (!UpscaleMem.Fit(n, 32 + 16 + 4, "allocating the upscaler's buffers")) return false;
    gpuart_ray_hit *hiHits = (gpuart_ray_hit *)UpscaleMem.mem;
    float *out = (float *)((char *)UpscaleMem.mem + n * 32);
    int32_t *hiPrims = (int32_t *)((char *)UpscaleMem.mem + n * 48);
    if (!UpscaleValid) {
        if (!Check(gpuart_hip_gbuffer_scaled(Backend, scale, GBufferSphere, hiHits, hiPrims), "building the larger frame's G-buffer") ||
            !Check(gpuart_hip_finish(Backend), "waiting for the device"))
            return false;
        UpscaleScale = scale;
        UpscaleValid = true;
    }
    const ViewBuffers b(DenoiseMem.mem, lo);
    plane = out;
    return Run(gpuart_upscale_run(Upscaler, scale, low, b.hits, b.prims, Tile.w, Tile.h, hiHits, hiPrims, UserSphere.flags, p, out), Upscaler, UP,
               "upsampling the frame");
}

bool Renderer::ReadUpscaled(float *rgba, gpuart_display_source source, uint32_t scale, float lumFloor, const gpuart_upscale_params *p) {
    const float *plane;
    size_t n;
    return rgba && StageUpscaled(source, scale, lumFloor, p, plane, n) &&
           checkHip(hipMemcpy(rgba, plane, n * 16, hipMemcpyDeviceToHost), "reading the upsampled frame");
}

bool Renderer::ReadUpscaledDisplay(uint8_t *rgba8, gpuart_display_source source, uint32_t scale, const gpuart_display_params *dp, float lumFloor,
                                   const gpuart_upscale_params *p) {
    const float *plane;
    size_t n;
    if (!rgba8 || !IsOK || !checkHip(hipSetDevice(Device), "hipSetDevice") || !Ensure(Display, DP)) return false;
    if (!StageUpscaled(source, scale, lumFloor, p, plane, n) || !UpscaleWords.Fit(n, 4, "allocating the 8-bit frame")) return false;
    return Run(gpuart_display_run(Display, plane, (uint8_t *)UpscaleWords.mem, scale * Tile.w, scale * Tile.h, scale * Tile.x, scale * Tile.y, dp), Display,
               DP, "encoding the frame") &&
           checkHip(hipMemcpy(rgba8, UpscaleWords.mem, n * 4, hipMemcpyDeviceToHost), "reading the 8-bit frame");
}

// ---- checkpoint / resume ---------------------------------------------------------------------------------------------
namespace {
const char CK_MAGIC[8] = {'G', 'P', 'U', 'A', 'R', 'T', 'C', 'K'};
struct CkHeader {
    char magic[8];
    uint32_t version, width, height, tileX, tileY, tileW, tileH;
    uint32_t numPathsRendered, pathsPerPixel, pathsPerPass, maxPathSegments;
    float minWeight;
    uint32_t rngTextBytes;
};
}  // namespace

bool Renderer::SaveCheckpoint(const char *fileName) {
    if (!IsOK) return false;
    if (NonUniform) {
        std::cerr << "Renderer: SaveCheckpoint after adaptive sampling retired blocks: a checkpoint holds one path count." << std::endl;
        return false;
    }
    std::vector<float> acc((size_t)Tile.w * Tile.h * 4);
    if (!ReadRadiance(acc.data(), false)) return false;
    std::ostringstream rng;
    rng << RndGen;  // the full mt19937 state, as text
    const std::string rngText = rng.str();
    CkHeader h{};
    memcpy(h.magic, CK_MAGIC, 8);
    h.version = 1; h.width = Viewport.width; h.height = Viewport.height;
    h.tileX = Tile.x; h.tileY = Tile.y; h.tileW = Tile.w; h.tileH = Tile.h;
    h.numPathsRendered = PathTracing.numPathsRendered; h.pathsPerPixel = PathTracing.pathsPerPixel;
    h.pathsPerPass = PathTracing.pathsPerPass; h.maxPathSegments = MaxPathSegments; h.minWeight = MinWeight;
    h.rngTextBytes = (uint32_t)rngText.size();
    std::ofstream f(fileName, std::ios::binary);
    f.write((const char *)&h, sizeof h);
    f.write(rngText.data(), (std::streamsize)rngText.size());
    f.write((const char *)acc.data(), (std::streamsize)(acc.size() * sizeof(float)));
    return f.good();
}

bool Renderer::LoadCheckpoint(const char *fileName) {
    if (!IsOK) return false;
    std::ifstream f(fileName, std::ios::binary);
    CkHeader h{};
    f.read((char *)&h, sizeof h);
    if (!f.good() || memcmp(h.magic, CK_MAGIC, 8) != 0 || h.version != 1) {
        std::cerr << "Renderer: \"" << fileName << "\" is not a checkpoint." << std::endl;
        return false;
    }
    if (h.width != Viewport.width || h.height != Viewport.height || h.tileX != Tile.x || h.tileY != Tile.y ||
        h.tileW != Tile.w || h.tileH != Tile.h || h.rngTextBytes > (1u << 20)) {
        std::cerr << "Renderer: checkpoint does not match the current viewport / tile." << std::endl;
        return false;
    }
    std::string rngText(h.rngTextBytes, '\0');
    f.read(&rngText[0], (std::streamsize)rngText.size());
    std::vector<float> acc((size_t)Tile.w * Tile.h * 4);
    f.read((char *)acc.data(), (std::streamsize)(acc.size() * sizeof(float)));
    if (!f.good()) return false;
    std::istringstream rng(rngText);
    std::mt19937 gen;
    rng >> gen;
    if (rng.fail()) return false;
    // (the reset drops an active block list and the back end's block counts: the checkpoint's paths are CountBase from here on)
    if (!Check(gpuart_hip_pt_reset(Backend), "clearing the radiance accumulator") ||
        !Check(gpuart_hip_write(Backend, 1, acc.data()), "restoring the radiance accumulator")) return false;
    RndGen = gen;
    DropTemporalHistory();
    if (Converge) ResetConvergeNow();
    if (Adaptive) ResetAdaptiveNow();
    CountBase = h.numPathsRendered;
    PathTracing.numPathsRendered = h.numPathsRendered;
    PathTracing.pathsPerPixel = h.pathsPerPixel;
    PathTracing.pathsPerPass = h.pathsPerPass;
    MaxPathSegments = h.maxPathSegments;
    MinWeight = h.minWeight;
    return true;
}

bool Renderer::Finish() { return Backend && Check(gpuart_hip_finish(Backend), "waiting for the device"); }

}  // namespace gpuart
