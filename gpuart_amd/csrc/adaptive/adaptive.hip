// adaptive.hip — libgpuart_adaptive.so (gfx950): the convergence estimate per 8x8 block, the decision which blocks still need paths and
// the normalisation by per-block path counts, include/gpuart_adaptive.h, which states every operation. Built like converge.hip — fp32
// denormals kept, IEEE '/' and sqrt, no contraction — so that every value is the one tests/adaptive_ref.py computes in NumPy float32.
// DESIGN.md "Adaptive sampling" describes the kernels.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../image/image_lib.h"
#include "../image/estimate.h"
#include "gpuart_adaptive.h"

namespace {

const char LIB[] = "adaptive";

constexpr int SEL_WAVES = 4;  ///< k_ad_select: 8x8 blocks (one wave each) per workgroup
constexpr int SEL_ABOVE_SHIFT = 1, SEL_NONFINITE_SHIFT = 8;  ///< k_ad_select's first word: bit 0 stays active, 7 bits for each count

__device__ __forceinline__ uint32_t block_of(int x, int y, int bw) { return (uint32_t)(y >> 3) * (uint32_t)bw + (uint32_t)(x >> 3); }

/// The convergence estimate's k_cv_update with the block's own batch weight and total: 32 bytes in, 16 out per pixel of a block that
/// moved, 8 bytes of block words (eight lanes share them) for the others.
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_ad_update(const float4 *accum, float4 *state, const uint32_t *paths, const uint4 *blk,
                                                             int w, int h, int bw) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const uint32_t t = block_of(x, y, bw);
    const uint32_t p = paths[t], seen = blk[t].x;
    if (p == seen) return;  // (p < seen was refused on the host)
    const float b = (float)(p - seen), Wn = (float)p;
    const float r = b / Wn;
    const size_t i = (size_t)y * w + x;
    state[i] = estimate_step(accum[i], state[i], b, r);
}

/// Behind k_ad_update on the same stream: no pixel reads a block word while it changes.
__global__ void __launch_bounds__(256) k_ad_blocks(const uint32_t *paths, uint4 *blk, uint32_t n) {
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    uint4 v = blk[t];
    const uint32_t p = paths[t];
    if (p != v.x) {
        v.x = p;
        v.y += 1;
        blk[t] = v;
    }
}

/// e of one pixel from its state and its block's words; +inf without an estimate (fewer than two batches).
__device__ __forceinline__ float error_of(const float4 s, const uint4 b, float lum_floor) {
    if (b.y < 2) return INFINITY;
    return estimate_error(s, (float)(b.y - 1), (float)b.x, lum_floor);
}

/// One wave per 8x8 block, a lane per pixel: a row of the block is one 128-byte line of the state. Ballot + popcount for the two counts,
/// a maximum over bit patterns (as k_cv_measure), then lane 0 writes the block's two words — the flag with both counts (at most 64 each)
/// packed above it, SEL_ABOVE_SHIFT and SEL_NONFINITE_SHIFT, and the max bits — and its active word.
template <bool MAP>
__global__ void __launch_bounds__(64 * SEL_WAVES) k_ad_select(const float4 *state, uint4 *blk, int w, int h, int bw, uint32_t n_blocks,
                                                              float threshold, float lum_floor, uint32_t min_paths, float *map, uint2 *out) {
    const uint32_t t = blockIdx.x * SEL_WAVES + (threadIdx.x >> 6);  // (wave-uniform)
    if (t >= n_blocks) return;
    const int lane = threadIdx.x & 63;
    const int x = (int)(t % (uint32_t)bw) * 8 + (lane & 7), y = (int)(t / (uint32_t)bw) * 8 + (lane >> 3);
    const uint4 b = blk[t];
    bool ab = false, nf = false;
    unsigned int mx = 0;
    if (x < w && y < h) {
        const size_t i = (size_t)y * w + x;
        const float e = error_of(state[i], b, lum_floor);
        if (MAP) map[i] = e;
        ab = !(e <= threshold);
        nf = !(fabsf(e) < INFINITY);
        if (!nf) mx = __float_as_uint(e);  // (e >= +0 here)
    }
    const uint32_t above = (uint32_t)__popcll(__ballot(ab)), non_finite = (uint32_t)__popcll(__ballot(nf));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)mx, o, 64);
        mx = other > mx ? other : mx;
    }
    if (lane == 0) {
        const uint32_t stays = (b.z && (b.x < min_paths || b.y < 2 || above)) ? 1u : 0u;
        out[t] = make_uint2(stays | above << SEL_ABOVE_SHIFT | non_finite << SEL_NONFINITE_SHIFT, mx);
        if (stays != b.z) blk[t] = make_uint4(b.x, b.y, stays, 0u);
    }
}

__global__ void __launch_bounds__(ROW_X * ROW_Y) k_ad_error_map(const float4 *state, const uint4 *blk, int w, int h, int bw, float lum_floor,
                                                                float *map) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    map[i] = error_of(state[i], blk[block_of(x, y, bw)], lum_floor);
}

/// k_scale_copy of libgpuart_hip.so with the divisor of the pixel's block.
__global__ void __launch_bounds__(ROW_X * ROW_Y) k_ad_normalize(const float4 *accum, const uint32_t *paths, float4 *out, int w, int h, int bw) {
    const int x = blockIdx.x * ROW_X + threadIdx.x, y = blockIdx.y * ROW_Y + threadIdx.y;
    if (x >= w || y >= h) return;
    const size_t i = (size_t)y * w + x;
    const uint32_t p = paths[block_of(x, y, bw)];
    const float d = (float)(p ? p : 1u);
    const float4 a = accum[i];
    out[i] = make_float4(a.x / d, a.y / d, a.z / d, a.w);
}

}  // namespace

struct gpuart_adaptive : ImageHandle {
    DeviceBuffer state;   ///< 16 bytes per pixel: {mean, m2, prevL, 0}
    DeviceBuffer blk;     ///< 16 bytes per block: {seen, batches, active, 0}
    DeviceBuffer out;     ///< 8 bytes per block: what k_ad_select writes
    DeviceBuffer stage;   ///< the host entry points' images and counts
    void *pinned = nullptr;   ///< host, pinned: the counts an update checks, the words a select reads
    size_t pinned_bytes = 0;
    uint32_t w = 0, h = 0;    ///< of the state; 0 after create and reset
    std::vector<uint32_t> seen;  ///< the host's copy of every block's seen: what an update checks and a summary reports
};

namespace {

uint32_t blocks_x(uint32_t w) { return (w + 7) / 8; }
size_t blocks_of(uint32_t w, uint32_t h) { return (size_t)blocks_x(w) * ((h + 7) / 8); }

int ensure_pinned(gpuart_adaptive *a, size_t bytes) {
    if (bytes <= a->pinned_bytes) return 0;
    HIP_TRY(hipStreamSynchronize(a->stream));
    if (a->pinned) (void)hipHostFree(a->pinned);
    a->pinned = nullptr;
    a->pinned_bytes = 0;
    HIP_TRY(hipHostMalloc(&a->pinned, bytes, hipHostMallocDefault));
    a->pinned_bytes = bytes;
    return 0;
}

int check_image(gpuart_adaptive *a, std::initializer_list<const void *> images, const void *paths, uint32_t w, uint32_t h, size_t align,
                bool state_size) {
    if (int r = check_handle(LIB, a)) return r;
    for (const void *p : images)
        if (!p) return fail(GPUART_HIP_ERR_ARG, "adaptive: an image pointer is NULL");
    if (!paths) return fail(GPUART_HIP_ERR_ARG, "adaptive: block_paths is NULL");
    if (misaligned(images, align) || misaligned({paths}, 4))
        return fail(GPUART_HIP_ERR_ARG, "adaptive: misaligned pointer (images need " + std::to_string(align) + " bytes, block_paths 4)");
    if (int r = check_size(LIB, w, h)) return r;
    if (state_size && a->w && (w != a->w || h != a->h))
        return fail(GPUART_HIP_ERR_ARG, "adaptive: size " + std::to_string(w) + " x " + std::to_string(h) + " is not the state's " + std::to_string(a->w) +
                                            " x " + std::to_string(a->h) + " (reset the handle first)");
    return 0;
}

/// One update on device memory: the counts come to the host and are checked, then the two kernels on the handle's stream.
int launch_update(gpuart_adaptive *a, const float4 *accum, const uint32_t *paths, uint32_t w, uint32_t h) {
    const size_t n = (size_t)w * h, nb = blocks_of(w, h);
    if (int r = ensure_pinned(a, nb * 4)) return r;
    uint32_t *hp = (uint32_t *)a->pinned;
    HIP_TRY(hipMemcpyAsync(hp, paths, nb * 4, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    const bool first = !a->w;
    for (size_t t = 0; t < nb; t++) {
        const uint32_t seen = first ? 0u : a->seen[t];
        if (hp[t] > GPUART_CONVERGE_MAX_PATHS)
            return fail(GPUART_HIP_ERR_ARG, "adaptive: block " + std::to_string(t) + " holds " + std::to_string(hp[t]) + " paths, above 2^24 (not exact in fp32)");
        if (hp[t] < seen)
            return fail(GPUART_HIP_ERR_ARG, "adaptive: block " + std::to_string(t) + " holds " + std::to_string(hp[t]) + " paths, below the " + std::to_string(seen) + " already seen");
    }
    if (first) {  // the first batch after create or reset: a state of zeros, every block active
        if (int r = ensure(a->stream, a->state, n * 16)) return r;
        if (int r = ensure(a->stream, a->blk, nb * 16)) return r;
        if (int r = ensure(a->stream, a->out, nb * 8)) return r;
        HIP_TRY(hipMemsetAsync(a->state.mem, 0, n * 16, a->stream));
        std::vector<uint4> init(nb, make_uint4(0u, 0u, 1u, 0u));
        HIP_TRY(hipMemcpyAsync(a->blk.mem, init.data(), nb * 16, hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipStreamSynchronize(a->stream));  // (init is freed on return)
    }
    const int bw = (int)blocks_x(w);
    k_ad_update<<<row_grid(w, h), row_block(), 0, a->stream>>>(accum, (float4 *)a->state.mem, paths, (const uint4 *)a->blk.mem, (int)w, (int)h, bw);
    HIP_TRY(hipGetLastError());
    k_ad_blocks<<<dim3((unsigned)((nb + 255) / 256)), 256, 0, a->stream>>>(paths, (uint4 *)a->blk.mem, (uint32_t)nb);
    HIP_TRY(hipGetLastError());
    a->seen.assign(hp, hp + nb);
    a->w = w;
    a->h = h;
    return 0;
}

int launch_normalize(gpuart_adaptive *a, const float4 *accum, const uint32_t *paths, float4 *out, uint32_t w, uint32_t h) {
    k_ad_normalize<<<row_grid(w, h), row_block(), 0, a->stream>>>(accum, paths, out, (int)w, (int)h, (int)blocks_x(w));
    HIP_TRY(hipGetLastError());
    return 0;
}

int check_floor(float lum_floor) {
    if (!std::isfinite(lum_floor) || !(lum_floor > 0)) return fail(GPUART_HIP_ERR_ARG, "adaptive: lum_floor must be finite and > 0");
    return 0;
}

}  // namespace

extern "C" {

const char *gpuart_adaptive_last_error(void) { return g_last_error.c_str(); }

int gpuart_adaptive_create(int device, gpuart_adaptive **out) { return create_handle(LIB, device, out); }

int gpuart_adaptive_destroy(gpuart_adaptive *a) {
    if (!a) return 0;
    destroy_handle(a, {a->state.mem, a->blk.mem, a->out.mem, a->stage.mem});
    if (a->pinned) (void)hipHostFree(a->pinned);
    delete a;
    return 0;
}

int gpuart_adaptive_reset(gpuart_adaptive *a) {
    if (int r = check_handle(LIB, a)) return r;
    a->w = a->h = 0;  // the next update zeroes the state it then has
    a->seen.clear();
    return 0;
}

int gpuart_adaptive_finish(gpuart_adaptive *a) { return finish_handle(LIB, a); }

int gpuart_adaptive_update(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, uint32_t w, uint32_t h) {
    if (int r = check_image(a, {accum}, block_paths, w, h, 16, true)) return r;
    HIP_TRY(hipSetDevice(a->device));
    return launch_update(a, (const float4 *)accum, block_paths, w, h);
}

int gpuart_adaptive_update_host(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, uint32_t w, uint32_t h) {
    if (int r = check_image(a, {accum}, block_paths, w, h, 4, true)) return r;
    HIP_TRY(hipSetDevice(a->device));
    const size_t n = (size_t)w * h, nb = blocks_of(w, h);
    if (int r = ensure(a->stream, a->stage, n * 32 + nb * 4)) return r;
    uint32_t *d_paths = (uint32_t *)((char *)a->stage.mem + n * 32);
    HIP_TRY(hipMemcpyAsync(a->stage.mem, accum, n * 16, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(d_paths, block_paths, nb * 4, hipMemcpyHostToDevice, a->stream));
    if (int r = launch_update(a, (const float4 *)a->stage.mem, d_paths, w, h)) return r;
    HIP_TRY(hipStreamSynchronize(a->stream));
    return 0;
}

int gpuart_adaptive_select(gpuart_adaptive *a, float threshold, float lum_floor, uint32_t min_paths, float *error_map, uint32_t *blocks_host,
                           gpuart_adaptive_summary *summary) {
    if (int r = check_handle(LIB, a)) return r;
    if (!summary) return fail(GPUART_HIP_ERR_ARG, "adaptive: summary is NULL");
    if (misaligned({error_map}, 4) || misaligned({blocks_host}, 4)) return fail(GPUART_HIP_ERR_ARG, "adaptive: misaligned pointer (error_map and blocks need 4 bytes)");
    if (!std::isfinite(threshold) || !(threshold >= 0)) return fail(GPUART_HIP_ERR_ARG, "adaptive: threshold must be finite and >= 0");
    if (int r = check_floor(lum_floor)) return r;
    if (!a->w) return fail(GPUART_HIP_ERR_ARG, "adaptive: select before the first update");
    HIP_TRY(hipSetDevice(a->device));
    const uint32_t w = a->w, h = a->h, bw = blocks_x(w);
    const size_t nb = blocks_of(w, h);
    if (int r = ensure_pinned(a, nb * 8)) return r;
    const dim3 grid((unsigned)((nb + SEL_WAVES - 1) / SEL_WAVES));
    if (error_map)
        k_ad_select<true><<<grid, 64 * SEL_WAVES, 0, a->stream>>>((const float4 *)a->state.mem, (uint4 *)a->blk.mem, (int)w, (int)h, (int)bw, (uint32_t)nb,
                                                                  threshold, lum_floor, min_paths, error_map, (uint2 *)a->out.mem);
    else
        k_ad_select<false><<<grid, 64 * SEL_WAVES, 0, a->stream>>>((const float4 *)a->state.mem, (uint4 *)a->blk.mem, (int)w, (int)h, (int)bw, (uint32_t)nb,
                                                                   threshold, lum_floor, min_paths, nullptr, (uint2 *)a->out.mem);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(a->pinned, a->out.mem, nb * 8, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    const uint2 *o = (const uint2 *)a->pinned;
    gpuart_adaptive_summary s{};
    s.pixels = (uint64_t)w * h;
    s.blocks = (uint32_t)nb;
    s.paths_min = 0xffffffffu;
    uint32_t mx = 0;
    for (size_t t = 0; t < nb; t++) {
        const uint32_t bx = (uint32_t)(t % bw), by = (uint32_t)(t / bw);
        const uint64_t inside = (uint64_t)std::min(8u, w - bx * 8) * std::min(8u, h - by * 8);
        if (o[t].x & 1u) {
            if (blocks_host) blocks_host[s.active_blocks] = (uint32_t)t;
            s.active_blocks++;
        }
        mx = std::max(mx, o[t].y);
        s.above += o[t].x >> SEL_ABOVE_SHIFT & 127u;
        s.non_finite += o[t].x >> SEL_NONFINITE_SHIFT & 127u;
        s.paths_sum += inside * a->seen[t];
        s.paths_min = std::min(s.paths_min, a->seen[t]);
        s.paths_max = std::max(s.paths_max, a->seen[t]);
    }
    static_assert(sizeof(float) == sizeof(uint32_t), "fp32");
    __builtin_memcpy(&s.max_error, &mx, 4);
    *summary = s;
    return 0;
}

int gpuart_adaptive_error_map(gpuart_adaptive *a, float lum_floor, float *error_map, uint32_t w, uint32_t h) {
    if (int r = check_handle(LIB, a)) return r;
    if (!error_map || misaligned({error_map}, 4)) return fail(GPUART_HIP_ERR_ARG, "adaptive: error_map is NULL or misaligned");
    if (int r = check_floor(lum_floor)) return r;
    if (!a->w) return fail(GPUART_HIP_ERR_ARG, "adaptive: no estimate before the first update");
    if (w != a->w || h != a->h)
        return fail(GPUART_HIP_ERR_ARG, "adaptive: size " + std::to_string(w) + " x " + std::to_string(h) + " is not the state's " + std::to_string(a->w) + " x " + std::to_string(a->h));
    HIP_TRY(hipSetDevice(a->device));
    k_ad_error_map<<<row_grid(w, h), row_block(), 0, a->stream>>>((const float4 *)a->state.mem, (const uint4 *)a->blk.mem, (int)w, (int)h, (int)blocks_x(w), lum_floor, error_map);
    HIP_TRY(hipGetLastError());
    return 0;
}

int gpuart_adaptive_normalize(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, float *out, uint32_t w, uint32_t h) {
    if (int r = check_image(a, {accum, out}, block_paths, w, h, 16, false)) return r;
    HIP_TRY(hipSetDevice(a->device));
    return launch_normalize(a, (const float4 *)accum, block_paths, (float4 *)out, w, h);
}

int gpuart_adaptive_normalize_host(gpuart_adaptive *a, const float *accum, const uint32_t *block_paths, float *out, uint32_t w, uint32_t h) {
    if (int r = check_image(a, {accum, out}, block_paths, w, h, 4, false)) return r;
    HIP_TRY(hipSetDevice(a->device));
    const size_t n = (size_t)w * h, nb = blocks_of(w, h);
    if (int r = ensure(a->stream, a->stage, n * 32 + nb * 4)) return r;
    float4 *d_out = (float4 *)((char *)a->stage.mem + n * 16);
    uint32_t *d_paths = (uint32_t *)((char *)a->stage.mem + n * 32);
    HIP_TRY(hipMemcpyAsync(a->stage.mem, accum, n * 16, hipMemcpyHostToDevice, a->stream));
    HIP_TRY(hipMemcpyAsync(d_paths, block_paths, nb * 4, hipMemcpyHostToDevice, a->stream));
    if (int r = launch_normalize(a, (const float4 *)a->stage.mem, d_paths, d_out, w, h)) return r;
    HIP_TRY(hipMemcpyAsync(out, d_out, n * 16, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return 0;
}

int gpuart_adaptive_read_state(gpuart_adaptive *a, float *state, uint32_t *block_state) {
    if (int r = check_handle(LIB, a)) return r;
    if (misaligned({state}, 4) || misaligned({block_state}, 4)) return fail(GPUART_HIP_ERR_ARG, "adaptive: misaligned pointer");
    if (!a->w) return fail(GPUART_HIP_ERR_ARG, "adaptive: no state before the first update");
    HIP_TRY(hipSetDevice(a->device));
    if (state) HIP_TRY(hipMemcpyAsync(state, a->state.mem, (size_t)a->w * a->h * 16, hipMemcpyDeviceToHost, a->stream));
    if (block_state) HIP_TRY(hipMemcpyAsync(block_state, a->blk.mem, blocks_of(a->w, a->h) * 16, hipMemcpyDeviceToHost, a->stream));
    HIP_TRY(hipStreamSynchronize(a->stream));
    return 0;
}

}  // extern "C"
