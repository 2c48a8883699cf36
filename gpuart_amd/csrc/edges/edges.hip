// edges.hip — libgpuart_edges.so (gfx950): the edge pixels of a G-buffer as an ordered list, and a filtered frame mended at those
// pixels from their sub-pixel records, as include/gpuart_edges.h states it operation by operation. Built without flushing fp32
// denormals, with IEEE '/' and no contraction, so that every value is the one tests/edges_ref.py computes in NumPy float32. DESIGN.md
// "Edge resolve" describes the kernels.
#include <cmath>

#include "../image/image_lib.h"
#include "../image/atrous.h"
#include "gpuart_edges.h"

namespace {

const char LIB[] = "edges";

#define ED_FN __device__ __forceinline__

enum { C_SKY = 0, C_SPHERE = 1, C_SURFACE = 2 };

/// A record as match() reads it.
struct Rec {
    float pos;
    float3 p, n;
    int type, cls;
    bool us;  ///< ordinal -2
};

ED_FN Rec load_rec(const float4 *hits, const int32_t *prims, size_t i, uint32_t us_flags) {
    const float4 h0 = hits[2 * i], h1 = hits[2 * i + 1];
    Rec r;
    r.pos = h0.x;
    r.p = make_float3(h0.y, h0.z, h0.w);
    r.n = make_float3(h1.x, h1.y, h1.z);
    r.type = __float_as_int(h1.w);
    r.us = false;
    r.cls = C_SKY;
    if (r.type >= 0) {  // (prims is read only where something was hit)
        r.us = prims[i] == -2;
        r.cls = r.us && (us_flags & (US_EM_NONZERO | US_SPECULAR)) ? C_SPHERE : C_SURFACE;
    }
    return r;
}

/// match(a, b) of the header: a record against a centre record.
ED_FN bool match(const Rec &a, const Rec &b, float normal_min, float plane_tol) {
    if (a.cls != b.cls) return false;
    if (a.cls != C_SURFACE) return true;
    if (a.type != b.type || a.us != b.us) return false;
    const float dn = (a.n.x * b.n.x + a.n.y * b.n.y) + a.n.z * b.n.z;
    if (!(dn > normal_min)) return false;
    const float dx = a.p.x - b.p.x, dy = a.p.y - b.p.y, dz = a.p.z - b.p.z;
    const float dist = fabsf((b.n.x * dx + b.n.y * dy) + b.n.z * dz);
    return dist <= plane_tol * gt_or(b.pos, 1e-6f);
}

// ---- mark -----------------------------------------------------------------------------------------------------------------------
// Three launches, no atomics. k_ed_flag: one thread per pixel in index order, a wave is 64 consecutive indices; every thread compares
// its 8 neighbours' centre records with its own (36-byte records its neighbours in the wave load too: L1 serves them) and the wave's
// ballot is stored, one 64-bit word per wave. k_ed_scan: one workgroup turns the words' popcounts into their exclusive prefix and the
// total. k_ed_list: every wave writes its edge pixels behind its prefix, a lane behind the lanes below it. The list is ascending
// because a wave's indices are and the prefix follows the waves' order.
constexpr int MARK_BLOCK = 256, SCAN_BLOCK = 1024;

__global__ void __launch_bounds__(MARK_BLOCK) k_ed_flag(const float4 *hits, const int32_t *prims, uint32_t us_flags, float normal_min,
                                                        float plane_tol, int w, int h, unsigned long long *ballots) {
    const size_t i = (size_t)blockIdx.x * MARK_BLOCK + threadIdx.x, n = (size_t)w * h;
    bool edge = false;
    if (i < n) {
        const int y = (int)(i / w), x = (int)(i - (size_t)y * w);
        const Rec own = load_rec(hits, prims, i, us_flags);
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++) {
                const int qx = x + dx, qy = y + dy;
                if ((dx == 0 && dy == 0) || qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                if (!match(load_rec(hits, prims, (size_t)qy * w + qx, us_flags), own, normal_min, plane_tol)) edge = true;
            }
    }
    const unsigned long long b = __ballot(edge);
    if ((threadIdx.x & 63) == 0 && i < n) ballots[i >> 6] = b;  // (a wave's first index is below n iff any of its indices is)
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_ed_scan(const unsigned long long *ballots, uint32_t words, uint32_t *prefix, uint32_t *count) {
    __shared__ uint32_t s_wave[SCAN_BLOCK / 64];
    __shared__ uint32_t s_carry;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t base = 0; base < words; base += SCAN_BLOCK) {
        const uint32_t k = base + threadIdx.x;
        const uint32_t c = k < words ? (uint32_t)__popcll(ballots[k]) : 0u;
        uint32_t incl = c;  // inclusive scan over the wave
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (int v = 0; v < wave; v++) before += s_wave[v];
        if (k < words) prefix[k] = before + incl - c;
        __syncthreads();
        if (threadIdx.x == SCAN_BLOCK - 1) s_carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = s_carry;
}

__global__ void __launch_bounds__(MARK_BLOCK) k_ed_list(const unsigned long long *ballots, const uint32_t *prefix, size_t n, uint32_t *list) {
    const size_t i = (size_t)blockIdx.x * MARK_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long b = ballots[i >> 6];
    const int lane = threadIdx.x & 63;
    if ((b >> lane) & 1ull) list[prefix[i >> 6] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull))] = (uint32_t)i;
}

// ---- resolve --------------------------------------------------------------------------------------------------------------------
// One thread per listed pixel: its n_sub sub-samples in turn, each against the centre records of the pixel and its 8 neighbours in
// the header's order (loaded on demand: most sub-samples match the pixel itself or its first neighbours). Unlisted pixels are the copy
// the launch follows.
__global__ void __launch_bounds__(256) k_ed_resolve(const float4 *filtered, const float4 *hits, const int32_t *prims, uint32_t us_flags,
                                                    int w, int h, const uint32_t *list, uint32_t n, const float4 *sub_hits,
                                                    const int32_t *sub_prims, uint32_t n_sub, float normal_min, float plane_tol, float4 *out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = list[i];
    if (p >= (size_t)w * h) return;
    const int y = (int)(p / (uint32_t)w), x = (int)(p - (uint32_t)y * (uint32_t)w);
    const float4 own = filtered[p];
    const int DY[9] = {0, 0, 0, 1, -1, 1, 1, -1, -1}, DX[9] = {0, 1, -1, 0, 0, 1, -1, 1, -1};
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (uint32_t k = 0; k < n_sub; k++) {
        const Rec s = load_rec(sub_hits, sub_prims, (size_t)k * n + i, us_flags);
        float cr = own.x, cg = own.y, cb = own.z;
        for (int c = 0; c < 9; c++) {
            const int qx = x + DX[c], qy = y + DY[c];
            if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
            const size_t q = (size_t)qy * w + qx;
            const Rec m = load_rec(hits, prims, q, us_flags);
            if (!match(s, m, normal_min, plane_tol)) continue;
            const float4 f = filtered[q];
            if (s.cls == C_SURFACE) {
                const float3 am = albedo(m.type & 3), as = albedo(s.type & 3);
                cr = (f.x / am.x) * as.x;
                cg = (f.y / am.y) * as.y;
                cb = (f.z / am.z) * as.z;
            } else {
                cr = f.x;
                cg = f.y;
                cb = f.z;
            }
            break;
        }
        sr += cr;
        sg += cg;
        sb += cb;
    }
    const float d = (float)n_sub;
    out[p] = make_float4(sr / d, sg / d, sb / d, own.w);
}

}  // namespace

struct gpuart_edges : ImageHandle {
    DeviceBuffer prefix;  ///< mark's: per 64 pixels the wave's ballot (8 bytes), then per 64 pixels its prefix (4)
};

namespace {

int check_params(const gpuart_edges_params *p) {
    if (!p) return 0;
    if (p->n_sub < 1 || p->n_sub > GPUART_EDGES_MAX_SUB)
        return fail(GPUART_HIP_ERR_ARG, "edges: n_sub must be in 1.." + std::to_string(GPUART_EDGES_MAX_SUB));
    if (!(p->normal_min >= -1) || !(p->normal_min <= 1)) return fail(GPUART_HIP_ERR_ARG, "edges: normal_min must be in -1..1");
    if (!std::isfinite(p->plane_tol) || !(p->plane_tol >= 0)) return fail(GPUART_HIP_ERR_ARG, "edges: plane_tol must be finite and >= 0");
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_edges_last_error(void) { return g_last_error.c_str(); }

int gpuart_edges_defaults(gpuart_edges_params *p) {
    if (!p) return fail(GPUART_HIP_ERR_ARG, "edges: params is NULL");
    p->n_sub = 8;
    p->normal_min = 0.95f;
    p->plane_tol = 0.02f;
    return 0;
}

int gpuart_edges_offsets(uint32_t n_sub, float *uv) {
    if (n_sub < 1 || n_sub > GPUART_EDGES_MAX_SUB) return fail(GPUART_HIP_ERR_ARG, "edges: n_sub must be in 1.." + std::to_string(GPUART_EDGES_MAX_SUB));
    if (!uv) return fail(GPUART_HIP_ERR_ARG, "edges: uv is NULL");
    for (uint32_t k = 0; k < n_sub; k++) {
        const uint32_t perm = n_sub == 4 ? GPUART_EDGES_RGSS[k] : (k * GPUART_EDGES_ROTATION[n_sub]) % n_sub;
        uv[2 * k] = ((float)k + 0.5f) / (float)n_sub;
        uv[2 * k + 1] = ((float)perm + 0.5f) / (float)n_sub;
    }
    return 0;
}

int gpuart_edges_create(int device, gpuart_edges **out) { return create_handle(LIB, device, out); }

int gpuart_edges_destroy(gpuart_edges *e) {
    if (!e) return 0;
    destroy_handle(e, {e->prefix.mem});
    delete e;
    return 0;
}

int gpuart_edges_finish(gpuart_edges *e) { return finish_handle(LIB, e); }

int gpuart_edges_mark(gpuart_edges *e, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags, uint32_t w, uint32_t h,
                      const gpuart_edges_params *p, uint32_t *list, uint32_t *count) {
    if (int rc = check_handle(LIB, e)) return rc;
    if (!hits || !prims || !list || !count) return fail(GPUART_HIP_ERR_ARG, "edges: hits, prims, list or count is NULL");
    if (misaligned({hits}, 16) || misaligned({prims, list, count}, 4))
        return fail(GPUART_HIP_ERR_ARG, "edges: misaligned pointer (hits needs 16 bytes, prims, list and count 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (int rc = check_params(p)) return rc;
    HIP_TRY(hipSetDevice(e->device));
    const gpuart_edges_params v = params_or_defaults(p, gpuart_edges_defaults);
    const size_t n = (size_t)w * h, words = (n + 63) / 64;
    if (int rc = ensure(e->stream, e->prefix, words * 12)) return rc;
    unsigned long long *ballots = (unsigned long long *)e->prefix.mem;
    uint32_t *prefix = (uint32_t *)(ballots + words);
    const dim3 grid((unsigned)((n + MARK_BLOCK - 1) / MARK_BLOCK));
    k_ed_flag<<<grid, MARK_BLOCK, 0, e->stream>>>((const float4 *)hits, prims, userSphereFlags, v.normal_min, v.plane_tol, (int)w, (int)h, ballots);
    HIP_TRY(hipGetLastError());
    k_ed_scan<<<1, SCAN_BLOCK, 0, e->stream>>>(ballots, (uint32_t)words, prefix, count);
    HIP_TRY(hipGetLastError());
    k_ed_list<<<grid, MARK_BLOCK, 0, e->stream>>>(ballots, prefix, n, list);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gpuart_edges_resolve(gpuart_edges *e, const float *filtered, const gpuart_ray_hit *hits, const int32_t *prims, uint32_t userSphereFlags,
                         uint32_t w, uint32_t h, const uint32_t *list, size_t n, const gpuart_ray_hit *sub_hits, const int32_t *sub_prims,
                         const gpuart_edges_params *p, float *out) {
    if (int rc = check_handle(LIB, e)) return rc;
    if (!filtered || !hits || !prims || !out) return fail(GPUART_HIP_ERR_ARG, "edges: filtered, hits, prims or out is NULL");
    if (n && (!list || !sub_hits || !sub_prims)) return fail(GPUART_HIP_ERR_ARG, "edges: list, sub_hits or sub_prims is NULL");
    if (misaligned({filtered, hits, sub_hits, out}, 16) || misaligned({prims, list, sub_prims}, 4))
        return fail(GPUART_HIP_ERR_ARG, "edges: misaligned pointer (filtered, hits, sub_hits and out need 16 bytes, prims, list and sub_prims 4)");
    if (int rc = check_size(LIB, w, h)) return rc;
    if (int rc = check_params(p)) return rc;
    const gpuart_edges_params v = params_or_defaults(p, gpuart_edges_defaults);
    if (n > GPUART_HIP_MAX_RAYS / v.n_sub) return fail(GPUART_HIP_ERR_ARG, "edges: n * n_sub exceeds GPUART_HIP_MAX_RAYS");
    const size_t bytes = (size_t)w * h * 16;
    if (overlaps(out, bytes, filtered, bytes)) return fail(GPUART_HIP_ERR_ARG, "edges: out overlaps filtered");
    HIP_TRY(hipSetDevice(e->device));
    HIP_TRY(hipMemcpyAsync(out, filtered, bytes, hipMemcpyDeviceToDevice, e->stream));
    if (n == 0) return 0;
    k_ed_resolve<<<dim3((unsigned)((n + 255) / 256)), 256, 0, e->stream>>>((const float4 *)filtered, (const float4 *)hits, prims, userSphereFlags,
                                                                            (int)w, (int)h, list, (uint32_t)n, (const float4 *)sub_hits, sub_prims,
                                                                            v.n_sub, v.normal_min, v.plane_tol, (float4 *)out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
