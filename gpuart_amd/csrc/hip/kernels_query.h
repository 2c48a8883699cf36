// kernels_query.h — the batched ray queries of libgpuart_hip.so (gpuart_hip_trace_rays / _trace_rays_host / _pick): closest hit and
// occlusion over the uploaded tree for rays the caller supplies, or for the camera rays of frame pixels. Included by gpuart_hip.hip only;
// DESIGN.md "Batched ray queries" describes the kernel and why its occlusion answer is exact.
#pragma once
#include "kernels_pipeline.h"

namespace {

enum { RQ_RAYS = 0, RQ_PIXELS = 1 };  ///< where a query's ray comes from (k_ray_query's template parameter)

/// One launch of k_ray_query: `n` queries, their sources and their results (device memory).
struct RayQuery {
    const float4 *rays;   ///< RQ_RAYS: per ray {origin.xyz, tmax}{dir.xyz, unused}
    const uint2 *xy;      ///< RQ_PIXELS: frame pixels (x, y), row 0 = bottom
    float4 *hits;         ///< per query two float4: {pos, p.xyz}{n.xyz, bits(type)} (gpuart_ray_hit)
    int32_t *prims;       ///< per query the primitive's ordinal, -1 none, -2 the user sphere; may be null
    uint32_t n;
    uint32_t occlusion;   ///< 1: is 0 < closest-hit pos < tmax? (RQ_RAYS only)
    uint32_t use_us;      ///< 1: the user sphere `us` takes part, as in CheckIntersectionInclUserSphere
    float us[4];
    // RQ_RAYS with sub_n != 0 (gpuart_hip_trace_subpixel): the launch walks nothing; it is the streaming pass that MAKES the n rays a
    // second, ordinary launch walks. Ray k * sub_n + e is the first segment path_begin makes for tile pixel sub_pixels[e] with the draws
    // sub_uv[2k], sub_uv[2k + 1], stored into sub_rays in the layout of `rays`
    const uint32_t *sub_pixels;  ///< local pixel indices ly * tw + lx
    const float *sub_uv;         ///< device memory: (rand1, rand2) per sub-sample
    float4 *sub_rays;
    uint32_t *sub_bad;           ///< set to 1 if an index lies outside the tile (its ray is pixel 0's: nothing is read out of bounds)
    uint32_t sub_n;
    float sub_pixel_size;
};

/// The record of query `i`: pos, point, normal, type and ordinal (the writes of replicas in a thin group are left to the first).
GD_FN void rq_store(const RayQuery &q, uint32_t i, float pos, F3 p, F3 n, int type, int32_t prim) {
    q.hits[2 * (size_t)i] = make_float4(pos, p.x, p.y, p.z);
    q.hits[2 * (size_t)i + 1] = make_float4(n.x, n.y, n.z, __int_as_float(type));
    if (q.prims) q.prims[i] = prim;
}

/// Persistent lanes over a batch of ray queries, on the loop it shares with k_direct_persistent (kernels_pipeline.h: ChunkCursor,
/// wide_rounds, thin_rounds): a wave takes chunks of queries from a cursor, a lane that has its answer stores it and takes the next query,
/// and once the cursor is dry a wave that is down to 32 (16) rays carries each by a pair (quad) of lanes. Every walk is the reference's closest-hit walk (lower child first, pruning on entry > closest: the order
/// of shaders/bvh_intersection.glsl:405-441), whatever order the context's render kernels use. An occlusion query walks the same walk
/// and stops at the first accepted hit whose parameter is below tmax: a prefix of the walk finds such a hit if and only if the minimum
/// over all primitives the full walk tests — the reference's closest hit — is below tmax.
template <int TYPES, int SOURCE>
__global__ void __launch_bounds__(BLOCK, GD_DIRECT_WAVES) k_ray_query(Scene sc, Frame f, RayQuery q, uint4 *spill, uint32_t *cursor,
                                                                  TraceTuning tune) {
    __shared__ uint2 ring_a[GD_RING * BLOCK];
    __shared__ float ring_b[GD_RING * BLOCK];
    if (SOURCE == RQ_RAYS && q.sub_n) {  // (launch-uniform) the generation pass of gpuart_hip_trace_subpixel: camera_ray and path_begin_at,
                                         // the very functions k_gen calls, one ray per thread and stride; no lane holds a walk here
        for (uint32_t idx = blockIdx.x * BLOCK + threadIdx.x; idx < q.n; idx += gridDim.x * BLOCK) {
            const uint32_t k = idx / q.sub_n, e = idx - k * q.sub_n;
            uint32_t p = q.sub_pixels[e];
            if (p >= (unsigned long long)f.tw * f.th) {
                *q.sub_bad = 1u;
                p = 0;
            }
            const uint32_t ly = p / f.tw, lx = p - ly * f.tw;
            F3 rs0, rd0, rs, rd;
            camera_ray(f, f.x0 + lx, frame_y(f, ly), rs0, rd0);
            path_begin_at(q.sub_pixel_size, f3(f.cam_pos[0], f.cam_pos[1], f.cam_pos[2]), q.sub_uv[2 * k], q.sub_uv[2 * k + 1], rs0, rd0, rs, rd);
            q.sub_rays[2 * (size_t)idx] = make_float4(rs.x, rs.y, rs.z, __builtin_inff());
            q.sub_rays[2 * (size_t)idx + 1] = make_float4(rd.x, rd.y, rd.z, 0.0f);
        }
        return;
    }
    TravStack st = make_stack(ring_a, ring_b, spill, gridDim.x * BLOCK);
    constexpr bool THIN_OK = GD_TRACE_THIN > 1 && GD_BOXES_OF(TYPES) == GD_BOXES_FAST;
    const bool occl = SOURCE == RQ_RAYS && q.occlusion != 0;  // wave-uniform
    uint32_t M = 1, sub = 0;                                  // M wave-uniform
    ChunkCursor cc(q.n, tune.chunk);
    uint32_t ray = SLOT_INVALID;  // the query this lane works on
    float tmax = __builtin_inff();
    F3 ro = f3(0, 0, 0), rd = f3(1, 0, 0), rdiv = f3(1, 1, 1);
    Trav t; t.state = TRAV_DONE; t.closest = 0; t.hit_prim = GD_NO_PRIM; t.node = 0; t.entry = 0; t.second = 0;

    for (;;) {
        // ---- idle lanes take the next queries
        unsigned long long idle = __ballot(ray == SLOT_INVALID);
        while (idle && !cc.exhausted) {
            bool served;
            const uint32_t i = cc.take(idle, ray == SLOT_INVALID, cursor, tune.chunk, served);
            if (i != SLOT_INVALID) {
                if (SOURCE == RQ_PIXELS) {
                    const uint2 px = q.xy[i];
                    camera_ray(f, px.x, px.y, ro, rd);
                    tmax = __builtin_inff();
                } else {
                    const float4 a = q.rays[2 * (size_t)i], b = q.rays[2 * (size_t)i + 1];
                    ro = xyz(a); rd = xyz(b);
                    tmax = a.w;
                }
                rdiv = f3(1 / rd.x, 1 / rd.y, 1 / rd.z);
                bool answered = false;
                if (occl) {
                    // decided without a walk: nothing lies in (0, tmax) when tmax <= 0 or NaN; the user sphere, when it is nearer than
                    // tmax, occludes whatever the tree holds (the reference's closest hit is then at most its parameter)
                    if (!(tmax > 0)) {
                        rq_store(q, i, -1.0f, f3(0, 0, 0), f3(0, 0, 0), -1, -1);
                        answered = true;
                    } else if (q.use_us) {
                        float usPos; F3 usP, usN;
                        sphere_hit(Ray{ro, rd}, f3(q.us[0], q.us[1], q.us[2]), q.us[3], usPos, usP, usN);
                        if (usPos > GD_VISIBILITY_OFFSET && usPos < tmax) {
                            rq_store(q, i, usPos, f3(0, 0, 0), f3(0, 0, 0), P_SPHERE, -2);
                            answered = true;
                        }
                    }
                }
                if (!answered) {
                    ray = i;
                    trav_init<GD_BOXES_OF(TYPES)>(sc, Ray{ro, rd}, rdiv, t, st, nullptr, false);
                }
            }
            idle = __ballot(ray == SLOT_INVALID);
            if (served) break;
        }
        const unsigned long long flying = __ballot(ray != SLOT_INVALID && sub == 0);
        if (flying == 0) {
            if (cc.exhausted) break;
            continue;
        }
        if (THIN_OK && cc.exhausted && M < (uint32_t)GD_TRACE_THIN) {
            const uint32_t left = (uint32_t)__popcll(flying);
            const uint32_t to = GD_THIN_WIDTH(left);
            if (to > M) {
                __shared__ uint32_t xfer[BLOCK];
                uint32_t tm = __float_as_uint(tmax);
                thin_regroup(to, flying, xfer, ring_a, ring_b, spill, ray, tm, ro, rd, rdiv, t, st);
                tmax = __uint_as_float(tm);
                if ((uint32_t)lane_id() / to >= left) ray = SLOT_INVALID;
                M = to;
                sub = (uint32_t)lane_id() & (M - 1);
            }
        }
        // ---- traverse until enough lanes have an answer, every walk in the reference's order. Occlusion: the first leaf after which the
        // walk holds an accepted hit below tmax ends it (closest only decreases, so this is the leaf that holds the first such hit of the walk)
        auto stop = [&] { return occl && t.hit_prim != GD_NO_PRIM && t.closest < tmax; };
        if (THIN_OK && M == 2) thin_rounds<2, TYPES, false>(sc, ro, rd, rdiv, t, st, sub, ray != SLOT_INVALID, tune, false, stop);
        else if (THIN_OK && M > 1) thin_rounds<4, TYPES, false>(sc, ro, rd, rdiv, t, st, sub, ray != SLOT_INVALID, tune, false, stop);
        else wide_rounds<TYPES, false>(sc, ro, rd, rdiv, t, st, tune, false, stop);
        // ---- lanes with an answer store it and go idle
        if (ray != SLOT_INVALID && t.state == TRAV_DONE) {
            if (sub == 0) {
                if (occl) {
                    const bool hit = t.hit_prim != GD_NO_PRIM && t.closest < tmax;
                    const int type = hit ? (int)(__float_as_uint(sc.prims[3 * (size_t)t.hit_prim].w) & 3u) : -1;
                    rq_store(q, ray, hit ? t.closest : -1.0f, f3(0, 0, 0), f3(0, 0, 0), type, hit ? (int32_t)t.hit_prim : -1);
                } else {
                    // reference CheckIntersectionInclUserSphere (resolve_hit), or CheckBVHIntersection alone
                    const Ray r{ro, rd};
                    Surface h; h.p = f3(0, 0, 0); h.n = f3(0, 0, 0);
                    bool ush = false;
                    if (q.use_us) resolve_hit(sc, r, t.closest, t.hit_prim, q.us, h, ush);
                    else if (t.hit_prim != GD_NO_PRIM) shade_prim(sc, r, t.hit_prim, h);
                    else { h.pos = -1; h.ptype = -1; }
                    if (h.ptype >= 0) rq_store(q, ray, h.pos, h.p, h.n, h.ptype, ush ? -2 : (int32_t)t.hit_prim);
                    else rq_store(q, ray, -1.0f, f3(0, 0, 0), f3(0, 0, 0), -1, -1);
                }
            }
            ray = SLOT_INVALID;
        }
    }
}

}  // namespace
