// capi.cpp — flat C API over the C++ library (see capi.h).
#include "capi.h"

#include <system_error>
#include <thread>
#include "exact_sort.h"

#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>

#include "renderer.h"
#include "scenes.h"
#include "utils.h"

using namespace gpuart;

namespace {

Primitive *make_primitive(const gpuart_prim_desc &d) {
    const float *f = d.f;
    switch (d.type) {
    case SPHERE: return new Sphere(Vec3f(f[0], f[1], f[2]), f[3]);
    case DISC: return new Disc(Vec3f(f[0], f[1], f[2]), Vec3f(f[3], f[4], f[5]), f[6]);
    case TRIANGLE: return new Triangle(Vec3f(f[0], f[1], f[2]), Vec3f(f[3], f[4], f[5]), Vec3f(f[6], f[7], f[8]));
    case CONE: return new Cone(Vec3f(f[0], f[1], f[2]), Vec3f(f[3], f[4], f[5]), f[6], f[7]);
    }
    return nullptr;
}

/// (Python hands over descriptions, the C++ API wants objects: for large scenes they are made and freed by several threads —
/// this is harness work, not part of SetPrimitives.)
template <class F>
void in_parts(size_t n, F body) {
    const size_t parts = n >= 65536 ? 8 : 1;
    std::vector<std::thread> th;
    struct Joiner {  // joins whatever was started, also when a part throws
        std::vector<std::thread> &th;
        ~Joiner() { for (auto &t : th) if (t.joinable()) t.join(); }
    } joiner{th};
    th.reserve(parts);
    for (size_t k = 1; k < parts; k++) {
        const size_t a = n * k / parts, b = n * (k + 1) / parts;
        try {
            th.emplace_back(body, a, b);
        } catch (const std::system_error &) {
            body(a, b);  // no thread to be had (the GPU box's CPU share caps them): this part runs here
        }
    }
    body(0, n / parts);
}

bool make_list(const gpuart_prim_desc *prims, int n, std::vector<Primitive *> &out) {
    const size_t base = out.size();
    out.resize(base + (size_t)n, nullptr);
    in_parts((size_t)n, [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) out[base + i] = make_primitive(prims[i]); });
    for (size_t i = base; i < out.size(); i++)
        if (!out[i]) return false;
    return true;
}

void free_list(std::vector<Primitive *> &v) {
    in_parts(v.size(), [&](size_t a, size_t b) { for (size_t i = a; i < b; i++) delete v[i]; });
    v.clear();
}

double g_last_build_ms[2] = {0, 0};  ///< BoundingVolumesHierarchy's constructor, CompileTo — of the last compile_list (gpuart_last_build_ms)

int compile_list(std::vector<Primitive *> &list, unsigned maxLevels, unsigned minPrims, float **quads, size_t *nquads,
                 unsigned *depth) {
    const bool timing = std::getenv("GPUART_HOST_TIMING") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    BoundingVolumesHierarchy tree(list, maxLevels, minPrims);
    const auto t1 = std::chrono::steady_clock::now();
    const size_t floats = tree.CompiledFloats();
    *quads = (float *)malloc(floats * sizeof(float) + 16);
    if (!*quads) return -1;
    tree.CompileTo(*quads);
    {
        const auto t2 = std::chrono::steady_clock::now();
        g_last_build_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
        g_last_build_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
    }
    if (timing) {
        const auto t2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[gpuart] BVH of %zu primitives: build %.1f ms, compile %.1f ms\n", list.size(),
                std::chrono::duration<double, std::milli>(t1 - t0).count(),
                std::chrono::duration<double, std::milli>(t2 - t1).count());
    }
    *nquads = floats / RGBA_ELEMS;
    if (depth) *depth = tree.GetDepth();
    return 0;
}

Camera make_camera(const float pos[3], const float dir[3], const float up[3], float fovY, float screenDist) {
    Camera c;
    c.Pos = Vec3f(pos[0], pos[1], pos[2]);
    c.Dir = Vec3f(dir[0], dir[1], dir[2]);
    c.Up = Vec3f(up[0], up[1], up[2]);
    c.FovY = fovY;
    c.ScreenDist = screenDist;
    return c;
}

}  // namespace

struct gpuart_renderer {
    Renderer impl;
    /// After gpuart_renderer_set_primitives: descOf[k] = the index in the caller's `prims` of the primitive SetPrimitives left at position k
    /// (the build sorts its vector); empty for the scenes of the init_* calls, whose ordinals are returned as they are.
    std::vector<int32_t> descOf;
    gpuart_renderer(unsigned w, unsigned h, const Camera &c, int device) : impl(w, h, c, device) {}
};

namespace {
template <typename T>
void vec3_ops(const T av[3], const T bv[3], T s, T out[36]) {
    const Vec3<T> a(av[0], av[1], av[2]), b(bv[0], bv[1], bv[2]);
    out[0] = a.length(); out[1] = a.sqrlength(); out[2] = a * b;
    const Vec3<T> r[11] = {a.normalized(), a ^ b, a + b, a - b, a * s, s * a, a / s, a.vrotx(s), a.vroty(s), a.vrotz(s), -a};
    for (int i = 0; i < 11; i++) { out[3 + 3 * i] = r[i].x; out[4 + 3 * i] = r[i].y; out[5 + 3 * i] = r[i].z; }
}
}  // namespace

extern "C" {

int gpuart_compile_bvh(const gpuart_prim_desc *prims, int n, unsigned maxLevels, unsigned minPrims, float **quads,
                       size_t *nquads, unsigned *depth) {
    if (!prims || n < 0 || !quads || !nquads) return -1;
    std::vector<Primitive *> list;
    int rc = make_list(prims, n, list) ? compile_list(list, maxLevels, minPrims, quads, nquads, depth) : -1;
    free_list(list);
    return rc;
}

int gpuart_compile_bvh_from_file(int kind, const char *path, float magnification, const float t[3],
                                 const gpuart_prim_desc *extra, int nextra, float **quads, size_t *nquads,
                                 unsigned *depth, size_t *nloaded) {
    if (!path || !t || !quads || !nquads) return -1;
    std::vector<Primitive *> list;
    const Vec3f tr(t[0], t[1], t[2]);
    bool ok = kind == 0 ? Utils::LoadMeshFromPLY(list, path, magnification, tr) : Utils::LoadPrimitives(list, path, magnification, tr);
    if (nloaded) *nloaded = list.size();
    int rc = -1;
    if (ok && make_list(extra, extra ? nextra : 0, list)) rc = compile_list(list, 1024, 2, quads, nquads, depth);
    free_list(list);
    return rc;
}

void gpuart_sort_permutation(const float *keys, size_t n, unsigned threads, uint32_t *perm) {
    std::vector<gpuart::SortKey> v(n);
    for (size_t i = 0; i < n; i++) v[i] = gpuart::SortKey{keys[i], (uint32_t)i};
    gpuart::ExactSort::Sort(v.data(), v.data() + n, threads);
    for (size_t i = 0; i < n; i++) perm[i] = v[i].index;
}

void gpuart_free(void *p) { free(p); }

int gpuart_refit_tree(const float *quads, size_t nquads, const uint32_t *ordinals, const float *payloads, size_t n, float *out,
                      size_t *firstBad, int touchedOnly) {
    if (!quads || !out || (n && (!ordinals || !payloads))) return -1;
    BoundingVolumesHierarchy tree;
    if (!tree.Load(quads, nquads) || tree.CompiledFloats() != nquads * RGBA_ELEMS) return -1;
    if (!tree.Refit(ordinals, payloads, n, firstBad, touchedOnly != 0)) return -2;
    tree.CompileTo(out);
    return 0;
}

int gpuart_rebuild_tree(const float *quads, size_t nquads, const uint32_t *order, float **out, size_t *nout, uint32_t *newToOld) {
    if (!quads || !out || !nout) return -1;
    BoundingVolumesHierarchy tree;
    if (!tree.Load(quads, nquads) || tree.CompiledFloats() != nquads * RGBA_ELEMS) return -1;
    std::vector<uint32_t> perm;
    if (!tree.RebuildMorton(&perm, order)) return -2;
    const size_t floats = tree.CompiledFloats();
    float *q = (float *)malloc(floats * sizeof(float));
    if (!q) return -1;
    tree.CompileTo(q);
    *out = q;
    *nout = floats / RGBA_ELEMS;
    if (newToOld) std::copy(perm.begin(), perm.end(), newToOld);
    return 0;
}

int gpuart_adopt_tree(const float *quads, size_t nquads, const uint32_t *order, const uint32_t *refs, size_t nRecs, float **out, size_t *nout) {
    if (!quads || !out || !nout || !order) return -1;
    BoundingVolumesHierarchy tree;
    if (!tree.Load(quads, nquads) || tree.CompiledFloats() != nquads * RGBA_ELEMS) return -1;
    if (!tree.AdoptTopology(order, refs, nRecs)) return -2;
    const size_t floats = tree.CompiledFloats();
    float *q = (float *)malloc(floats * sizeof(float));
    if (!q) return -1;
    tree.CompileTo(q);
    *out = q;
    *nout = floats / RGBA_ELEMS;
    return 0;
}

void gpuart_last_build_ms(double out[2]) { out[0] = g_last_build_ms[0]; out[1] = g_last_build_ms[1]; }

void gpuart_camera_basis(const float pos[3], const float dir[3], const float up[3], float fovY, float screenDist,
                         unsigned width, unsigned height, float out[13]) {
    const Camera c = make_camera(pos, dir, up, fovY, screenDist);
    const Renderer::ScreenBasis s = Renderer::ComputeScreenBasis(c, width, height);
    s.Pos.storeIn(out); s.BottomLeft.storeIn(out + 3); s.DeltaHorz.storeIn(out + 6); s.DeltaVert.storeIn(out + 9);
    out[12] = Renderer::ComputePixelSize(c, height);
}

void gpuart_sun_direction(float azimuth, float altitude, float out[3]) {
    Renderer::ComputeSunDirection(azimuth, altitude).storeIn(out);
}

void gpuart_vec3f_ops(const float a[3], const float b[3], float s, float out[36]) { vec3_ops<float>(a, b, s, out); }
void gpuart_vec3d_ops(const double a[3], const double b[3], double s, double out[36]) { vec3_ops<double>(a, b, s, out); }

gpuart_renderer *gpuart_renderer_create(unsigned width, unsigned height, const float pos[3], const float dir[3],
                                        const float up[3], float fovY, float screenDist, int device) {
    return new gpuart_renderer(width, height, make_camera(pos, dir, up, fovY, screenDist), device);
}
void gpuart_renderer_destroy(gpuart_renderer *r) { delete r; }
int gpuart_renderer_is_ok(gpuart_renderer *r) { return r && r->impl.GetIsOK(); }

void gpuart_renderer_set_primitives(gpuart_renderer *r, const gpuart_prim_desc *prims, int n, int printInfo) {
    std::vector<Primitive *> list;
    r->descOf.clear();
    if (make_list(prims, n, list)) {
        // the permutation the build applies: each object's position in the caller's order, looked up after SetPrimitives sorted the list
        std::vector<std::pair<const Primitive *, int32_t>> pos(list.size());
        for (size_t i = 0; i < list.size(); i++) pos[i] = {list[i], (int32_t)i};
        std::sort(pos.begin(), pos.end());
        r->impl.SetPrimitives(list, printInfo != 0);
        r->descOf.resize(list.size());
        for (size_t k = 0; k < list.size(); k++)
            r->descOf[k] = std::lower_bound(pos.begin(), pos.end(), std::make_pair((const Primitive *)list[k], (int32_t)-1))->second;
    }
    free_list(list);
}
int gpuart_renderer_update_primitives(gpuart_renderer *r, const uint32_t *indices, const gpuart_prim_desc *descs, int n) {
    if (!r || n < 0 || (n && (!indices || !descs))) return 0;
    // the caller's numbering -> positions in the renderer's sorted vector, ascending
    std::vector<uint32_t> ordinalOf(r->descOf.size());
    for (size_t k = 0; k < r->descOf.size(); k++) ordinalOf[(size_t)r->descOf[k]] = (uint32_t)k;
    std::vector<std::pair<uint32_t, int>> order((size_t)n);
    for (int i = 0; i < n; i++) {
        if (!ordinalOf.empty() && indices[i] >= ordinalOf.size()) return 0;
        order[(size_t)i] = {ordinalOf.empty() ? indices[i] : ordinalOf[indices[i]], i};
    }
    std::sort(order.begin(), order.end());
    std::vector<uint32_t> sorted((size_t)n);
    std::vector<gpuart_prim_desc> moved((size_t)n);
    for (int i = 0; i < n; i++) {
        sorted[(size_t)i] = order[(size_t)i].first;
        moved[(size_t)i] = descs[order[(size_t)i].second];
    }
    std::vector<Primitive *> list;
    const bool ok = make_list(moved.data(), n, list) && r->impl.UpdatePrimitives(sorted.data(), list.data(), (size_t)n);
    free_list(list);
    return ok ? 1 : 0;
}
int gpuart_renderer_rebuild_tree(gpuart_renderer *r, uint32_t *newToOld) { return gpuart_renderer_rebuild_tree_mode(r, Renderer::TREE_MORTON, newToOld); }
int gpuart_renderer_rebuild_tree_mode(gpuart_renderer *r, int mode, uint32_t *newToOld) {
    if (!r) return 0;
    std::vector<uint32_t> perm;
    if (!r->impl.RebuildTree(&perm, mode)) return 0;
    if (!r->descOf.empty()) {  // the caller's numbering follows the primitives to their new positions
        std::vector<int32_t> moved(perm.size());
        for (size_t p = 0; p < perm.size(); p++) moved[p] = r->descOf[perm[p]];
        r->descOf.swap(moved);
    }
    if (newToOld) std::copy(perm.begin(), perm.end(), newToOld);
    return 1;
}
int gpuart_renderer_edit_primitives(gpuart_renderer *r, const uint32_t *remove, int nRemove, const gpuart_prim_desc *added, int nAdd, int mode,
                                    uint32_t *source, size_t *n_new) {
    if (!r || nRemove < 0 || nAdd < 0 || (nRemove && !remove) || (nAdd && !added)) return 0;
    // the caller's numbering -> device ordinals, ascending
    const size_t nOld = r->impl.GetBVH().GetNumPrimitives();
    std::vector<uint32_t> ordinalOf(r->descOf.size());
    for (size_t k = 0; k < r->descOf.size(); k++) ordinalOf[(size_t)r->descOf[k]] = (uint32_t)k;
    std::vector<uint32_t> sorted((size_t)nRemove);
    std::vector<bool> gone(std::max(nOld, r->descOf.size()), false);  // by the caller's index
    for (int i = 0; i < nRemove; i++) {
        if (remove[i] >= gone.size() || gone[remove[i]]) return 0;
        gone[remove[i]] = true;
        sorted[(size_t)i] = ordinalOf.empty() ? remove[i] : ordinalOf[remove[i]];
    }
    std::sort(sorted.begin(), sorted.end());
    std::vector<Primitive *> list;
    std::vector<uint32_t> from;
    const bool ok = make_list(added, nAdd, list) && r->impl.EditPrimitives(sorted.data(), (size_t)nRemove, list.data(), (size_t)nAdd, &from, mode);
    free_list(list);
    if (!ok) return 0;
    if (!r->descOf.empty() || nOld) {
        // a survivor's description keeps its rank among the survivors; the added ones follow
        std::vector<int32_t> rank(gone.size(), -1);
        int32_t next = 0;
        for (size_t d = 0; d < gone.size(); d++)
            if (!gone[d]) rank[d] = next++;
        std::vector<int32_t> now(from.size());
        for (size_t p = 0; p < from.size(); p++)
            now[p] = from[p] < nOld ? rank[r->descOf.empty() ? from[p] : (size_t)r->descOf[from[p]]] : next + (int32_t)(from[p] - nOld);
        r->descOf.swap(now);
    }
    if (source) std::copy(from.begin(), from.end(), source);
    if (n_new) *n_new = from.size();
    return 1;
}
int gpuart_edit_tree(const float *quads, size_t nquads, const uint32_t *remove, size_t nRemove, const uint32_t *addTypes, const float *addPayloads,
                     size_t nAdd, int adopt, const uint32_t *order, const uint32_t *refs, size_t nRecs, float **out, size_t *nout, uint32_t *newToOld,
                     size_t *firstBad) {
    if (!quads || !out || !nout || (adopt && !order)) return -1;
    BoundingVolumesHierarchy tree;
    if (!tree.Load(quads, nquads) || tree.CompiledFloats() != nquads * RGBA_ELEMS) return -1;
    if (!tree.EditPrimitives(remove, nRemove, addTypes, addPayloads, nAdd, firstBad)) return -2;
    std::vector<uint32_t> perm;
    if (adopt) {
        if (!tree.AdoptTopology(order, refs, nRecs)) return -3;
        perm.assign(order, order + tree.GetNumPrimitives());
    } else if (!tree.RebuildMorton(&perm, order)) return -3;
    const size_t floats = tree.CompiledFloats();
    float *q = (float *)malloc(floats * sizeof(float));
    if (!q) return -1;
    tree.CompileTo(q);
    *out = q;
    *nout = floats / RGBA_ELEMS;
    if (newToOld) std::copy(perm.begin(), perm.end(), newToOld);
    return 0;
}
int gpuart_renderer_tree_cost(gpuart_renderer *r, double *cost) { return r && r->impl.TreeCost(cost) ? 1 : 0; }
void gpuart_renderer_last_rebuild_ms(gpuart_renderer *r, double out[2]) {
    if (!r || !out) return;
    out[0] = r->impl.GetLastRebuildMs()[0]; out[1] = r->impl.GetLastRebuildMs()[1];
}
int gpuart_renderer_compile_bvh(gpuart_renderer *r, float **quads, size_t *nquads) {
    if (!r || !quads || !nquads) return -1;
    const BoundingVolumesHierarchy &t = r->impl.GetBVH();
    const size_t floats = t.CompiledFloats();
    float *q = (float *)malloc(floats * sizeof(float));
    if (!q) return -1;
    t.CompileTo(q);
    *quads = q;
    *nquads = floats / RGBA_ELEMS;
    return 0;
}
void gpuart_renderer_init_box(gpuart_renderer *r) { r->descOf.clear(); InitBox(r->impl); }
int gpuart_renderer_init_dragon(gpuart_renderer *r, const char *plyPath) { r->descOf.clear(); return InitDragon(r->impl, plyPath) ? 1 : 0; }
int gpuart_renderer_init_cluster(gpuart_renderer *r, const char *datPath) {
    r->descOf.clear();
    return (datPath ? InitCluster(r->impl, datPath) : InitCluster(r->impl)) ? 1 : 0;
}
int gpuart_renderer_init_tree(gpuart_renderer *r, const char *datPath) {
    r->descOf.clear();
    return (datPath ? InitTree(r->impl, datPath) : InitTree(r->impl)) ? 1 : 0;
}
namespace {
/// Device ordinals -> indices of the caller's descriptions (capi.h: gpuart_renderer_trace_rays).
void to_desc_index(const gpuart_renderer *r, int32_t *prims, size_t n) {
    if (!prims || r->descOf.empty()) return;
    for (size_t i = 0; i < n; i++)
        if (prims[i] >= 0 && (size_t)prims[i] < r->descOf.size()) prims[i] = r->descOf[(size_t)prims[i]];
}
}  // namespace
int gpuart_renderer_trace_rays(gpuart_renderer *r, const float *rays, size_t n, int occlusion, int withUserSphere, gpuart_ray_hit *hits,
                               int32_t *prims) {
    if (!r->impl.TraceRays(rays, n, occlusion != 0, withUserSphere != 0, hits, prims)) return 0;
    to_desc_index(r, prims, n);
    return 1;
}
int gpuart_renderer_pick(gpuart_renderer *r, const uint32_t *xy, size_t n, int withUserSphere, gpuart_ray_hit *hits, int32_t *prims) {
    if (!r->impl.Pick(xy, n, hits, prims, withUserSphere != 0)) return 0;
    to_desc_index(r, prims, n);
    return 1;
}
int gpuart_renderer_closest_points(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, gpuart_nearest_hit *hits) {
    return r->impl.ClosestPoints(points, n, withUserSphere != 0, hits) ? 1 : 0;
}

int gpuart_renderer_nearest_primitives(gpuart_renderer *r, const float *points, size_t n, size_t k, int withUserSphere, gpuart_nearest_hit *hits) {
    return r->impl.NearestPrimitives(points, n, k, withUserSphere != 0, hits) ? 1 : 0;
}

int gpuart_renderer_primitives_within(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, uint32_t *offsets,
                                      gpuart_nearest_hit *items, size_t capacity, uint64_t *total) {
    return r->impl.PrimitivesWithin(points, n, withUserSphere != 0, offsets, items, capacity, total) ? 1 : 0;
}

int gpuart_renderer_primitives_within_fill(gpuart_renderer *r, const float *points, size_t n, int withUserSphere, const uint32_t *offsets,
                                           gpuart_nearest_hit *items, size_t capacity) {
    return r->impl.FillPrimitivesWithin(points, n, withUserSphere != 0, offsets, items, capacity) ? 1 : 0;
}

int gpuart_renderer_primitives_overlapping(gpuart_renderer *r, const float *boxes, size_t n, float margin, int withUserSphere, uint32_t *offsets,
                                           int32_t *items, size_t capacity, uint64_t *total) {
    return r->impl.PrimitivesOverlapping(boxes, n, margin, withUserSphere != 0, offsets, items, capacity, total) ? 1 : 0;
}

int gpuart_renderer_primitives_overlapping_fill(gpuart_renderer *r, const float *boxes, size_t n, float margin, int withUserSphere, const uint32_t *offsets,
                                                int32_t *items, size_t capacity) {
    return r->impl.FillPrimitivesOverlapping(boxes, n, margin, withUserSphere != 0, offsets, items, capacity) ? 1 : 0;
}

int gpuart_renderer_overlapping_pairs(gpuart_renderer *r, float margin, uint32_t *offsets, int32_t *items, size_t capacity, uint64_t *total) {
    return r->impl.OverlappingPairs(margin, offsets, items, capacity, total) ? 1 : 0;
}

int gpuart_renderer_set_camera(gpuart_renderer *r, const float pos[3], const float dir[3], const float up[3], float fovY,
                               float screenDist) {
    return r->impl.SetCamera(make_camera(pos, dir, up, fovY, screenDist)) ? 1 : 0;
}
int gpuart_renderer_update_viewport(gpuart_renderer *r, unsigned w, unsigned h) { return r->impl.UpdateViewportSize(w, h) ? 1 : 0; }
int gpuart_renderer_set_tile(gpuart_renderer *r, unsigned x0, unsigned y0, unsigned w, unsigned h) {
    return r->impl.SetTile(x0, y0, w, h) ? 1 : 0;
}
int gpuart_renderer_set_interleaved_tile(gpuart_renderer *r, unsigned x0, unsigned y0, unsigned w, unsigned localRows,
                                         unsigned bandRows, unsigned bandStride) {
    return r->impl.SetInterleavedTile(x0, y0, w, localRows, bandRows, bandStride) ? 1 : 0;
}
void gpuart_renderer_set_sun(gpuart_renderer *r, float azimuth, float altitude, int directLighting) {
    r->impl.SetSunAzimuth(azimuth);
    r->impl.SetSunAltitude(altitude);
    r->impl.SetSunDirectLighting(directLighting != 0);
}
void gpuart_renderer_set_user_sphere(gpuart_renderer *r, const float pos[3], float radius, float emittance, int specular,
                                     int fuzzy) {
    r->impl.SetUserSphere(Vec3f(pos[0], pos[1], pos[2]), radius, emittance);
    r->impl.SetUserSphereSpecular(specular != 0);
    r->impl.SetUserSphereFuzzy(fuzzy != 0);
}
void gpuart_renderer_set_user_sphere_pos(gpuart_renderer *r, const float pos[3]) { r->impl.SetUserSpherePos(Vec3f(pos[0], pos[1], pos[2])); }
void gpuart_renderer_set_max_path_segments(gpuart_renderer *r, unsigned n) { r->impl.SetMaxPathSegments(n); }
void gpuart_renderer_set_seed(gpuart_renderer *r, uint32_t seed) { r->impl.SetSeed(seed); }
void gpuart_renderer_render_direct(gpuart_renderer *r) { r->impl.RenderDirectLighting(); }
void gpuart_renderer_restart_path_tracing(gpuart_renderer *r, unsigned perPass, unsigned perPixel) {
    r->impl.RestartPathTracing(perPass, perPixel);
}
unsigned gpuart_renderer_path_tracing_pass(gpuart_renderer *r) { return r->impl.RenderPathTracingPass(); }
int gpuart_renderer_read_direct(gpuart_renderer *r, float *rgba) { return r->impl.ReadDirectLighting(rgba) ? 1 : 0; }
int gpuart_renderer_read_radiance(gpuart_renderer *r, float *rgba, int normalized) {
    return r->impl.ReadRadiance(rgba, normalized != 0) ? 1 : 0;
}
int gpuart_renderer_read_denoised(gpuart_renderer *r, float *rgba, const gpuart_denoise_params *p) {
    return r->impl.ReadDenoised(rgba, p) ? 1 : 0;
}
void gpuart_renderer_set_min_weight(gpuart_renderer *r, float w) { r->impl.SetMinWeight(w); }
int gpuart_renderer_set_nearest_first(gpuart_renderer *r, uint32_t minPrims) { return r->impl.SetNearestFirst(minPrims) ? 1 : 0; }
int gpuart_renderer_set_temporal_history(gpuart_renderer *r, int on, const gpuart_temporal_params *tp) {
    return r->impl.SetTemporalHistory(on != 0, tp) ? 1 : 0;
}
int gpuart_renderer_read_preview(gpuart_renderer *r, float *rgba, const gpuart_denoise_params *dn, const gpuart_temporal_params *tp) {
    return r->impl.ReadPreview(rgba, dn, tp) ? 1 : 0;
}
int gpuart_renderer_render_until(gpuart_renderer *r, float threshold, float maxAboveShare, unsigned batchPaths, float lumFloor,
                                 gpuart_converge_summary *last) {
    return r->impl.RenderUntil(threshold, maxAboveShare, batchPaths, lumFloor, last);
}
int gpuart_renderer_read_error_map(gpuart_renderer *r, float *e, float lumFloor) { return r->impl.ReadErrorMap(e, lumFloor) ? 1 : 0; }
int gpuart_renderer_read_refined(gpuart_renderer *r, float *rgba, float lumFloor, const gpuart_refine_params *p) {
    return r->impl.ReadRefined(rgba, lumFloor, p) ? 1 : 0;
}
int gpuart_renderer_read_display(gpuart_renderer *r, uint8_t *rgba8, int source, const gpuart_display_params *dp, float lumFloor) {
    return r->impl.ReadDisplay(rgba8, (gpuart_display_source)source, dp, lumFloor) ? 1 : 0;
}
int gpuart_renderer_read_upscaled(gpuart_renderer *r, float *rgba, int source, uint32_t scale, float lumFloor, const gpuart_upscale_params *p) {
    return r->impl.ReadUpscaled(rgba, (gpuart_display_source)source, scale, lumFloor, p) ? 1 : 0;
}
int gpuart_renderer_read_upscaled_display(gpuart_renderer *r, uint8_t *rgba8, int source, uint32_t scale, const gpuart_display_params *dp,
                                          float lumFloor, const gpuart_upscale_params *p) {
    return r->impl.ReadUpscaledDisplay(rgba8, (gpuart_display_source)source, scale, dp, lumFloor, p) ? 1 : 0;
}
int gpuart_renderer_set_history_variance(gpuart_renderer *r, int on, const gpuart_moments_params *p) {
    return r->impl.SetHistoryVariance(on != 0, p) ? 1 : 0;
}
int gpuart_renderer_set_history_antilag(gpuart_renderer *r, int on, const gpuart_antilag_params *p) {
    return r->impl.SetHistoryAntiLag(on != 0, p) ? 1 : 0;
}
int gpuart_renderer_set_edge_resolve(gpuart_renderer *r, int on, const gpuart_edges_params *p) {
    return r->impl.SetEdgeResolve(on != 0, p) ? 1 : 0;
}
int gpuart_renderer_get_edge_resolve(gpuart_renderer *r) { return r->impl.GetEdgeResolve() ? 1 : 0; }
int gpuart_renderer_set_firefly_clamp(gpuart_renderer *r, int on, const gpuart_despeckle_params *p) {
    return r->impl.SetFireflyClamp(on != 0, p) ? 1 : 0;
}
int gpuart_renderer_get_firefly_clamp(gpuart_renderer *r) { return r->impl.GetFireflyClamp() ? 1 : 0; }
int gpuart_renderer_read_firefly_summary(gpuart_renderer *r, gpuart_despeckle_summary *out) {
    return r->impl.ReadFireflySummary(out) ? 1 : 0;
}
int gpuart_renderer_read_guided_preview(gpuart_renderer *r, float *rgba, float lumFloor, const gpuart_refine_params *rf,
                                        const gpuart_temporal_params *tp) {
    return r->impl.ReadGuidedPreview(rgba, lumFloor, rf, tp) ? 1 : 0;
}
int gpuart_renderer_render_adaptive(gpuart_renderer *r, float threshold, unsigned minPaths, unsigned batchPaths, float lumFloor,
                                    gpuart_adaptive_summary *last) {
    return r->impl.RenderAdaptive(threshold, minPaths, batchPaths, lumFloor, last);
}
int gpuart_renderer_read_sample_counts(gpuart_renderer *r, uint32_t *perPixel) { return r->impl.ReadSampleCounts(perPixel) ? 1 : 0; }
int gpuart_renderer_gather_radiance(gpuart_renderer *const *ranks, int n, int root, int normalized, float *fullFrame) {
    if (!ranks || n < 1) return 0;
    std::vector<Renderer *> impl((size_t)n);
    for (int k = 0; k < n; k++) impl[(size_t)k] = ranks[k] ? &ranks[k]->impl : nullptr;
    return Renderer::GatherRadiance(impl.data(), n, root, normalized != 0, fullFrame) ? 1 : 0;
}
int gpuart_renderer_finish(gpuart_renderer *r) { return r->impl.Finish() ? 1 : 0; }
int gpuart_renderer_save_checkpoint(gpuart_renderer *r, const char *path) { return r->impl.SaveCheckpoint(path) ? 1 : 0; }
int gpuart_renderer_load_checkpoint(gpuart_renderer *r, const char *path) { return r->impl.LoadCheckpoint(path) ? 1 : 0; }
gpuart_hip_ctx *gpuart_renderer_backend(gpuart_renderer *r) { return r->impl.GetBackend(); }
void gpuart_renderer_params(gpuart_renderer *r, gpuart_params *out) { *out = r->impl.MakeParams(); }
void gpuart_renderer_last_setprims_ms(gpuart_renderer *r, double out[4]) {
    for (int k = 0; k < 4; k++) out[k] = r->impl.GetLastSetPrimitivesMs()[k];
}

void gpuart_renderer_scene_info(gpuart_renderer *r, uint64_t *nodes, uint64_t *prims, unsigned *depth) {
    const BoundingVolumesHierarchy &t = r->impl.GetBVH();
    if (nodes) *nodes = t.GetNumNodes();
    if (prims) *prims = t.GetNumPrimitives();
    if (depth) *depth = t.GetDepth();
}

}  // extern "C"
