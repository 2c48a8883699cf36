// image_lib.h — the scaffold of the eleven image libraries (denoise/denoise.hip, temporal/temporal.hip, converge/converge.hip, refine/refine.hip,
// adaptive/adaptive.hip, moments/moments.hip, display/display.hip, antilag/antilag.hip, edges/edges.hip, despeckle/despeckle.hip, upscale/upscale.hip), private
// to them: the last-error string, the handle's device and stream with the shared parts of create / destroy / finish, the grow-only device
// buffer, the handle, size and overlap checks, the caller's parameters or the defaults, the 64 x 4 row block, the staging of a G-buffer
// for the _host entry points, and the two device functions more than one library states: the luminance and "what is a surface pixel".
// Each library is one translation unit that includes this once, so everything sits in an anonymous namespace and every library has its
// own copy (its own last error). The checks take the library's name: every message starts with it. DESIGN.md "The image libraries'
// scaffold" says what stays in each library. refit/refit.hip, treebuild/build.hip, ploc/ploc.hip and edit/edit.hip, which are no image
// libraries (they work on the uploaded tree), take the last error, HIP_TRY, the handle, the checks and the grow-only buffer from here too;
// what those four share beyond that is in tree/tree_lib.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <initializer_list>
#include <string>

#include "gpuart_hip.h"

namespace {

thread_local std::string g_last_error;

inline int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(GPUART_HIP_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

// ---- the handle ------------------------------------------------------------------------------------------------------------------
/// What every library's handle starts with; all of a handle's work is on its stream.
struct ImageHandle {
    int device = 0;
    hipStream_t stream = nullptr;
};

/// create: a new H (an ImageHandle) on `device`, made current, with a non-blocking stream. *out stays NULL on failure.
template <class H>
int create_handle(const char *lib, int device, H **out) {
    if (!out) return fail(GPUART_HIP_ERR_ARG, std::string(lib) + ": out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
        return fail(GPUART_HIP_ERR_NO_DEVICE, std::string(lib) + ": no HIP device " + std::to_string(device));
    HIP_TRY(hipSetDevice(device));
    H *h = new H;
    h->device = device;
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(GPUART_HIP_ERR_DEVICE, std::string(lib) + ": hipStreamCreateWithFlags failed");
    }
    *out = h;
    return 0;
}

/// destroy: waits for the handle's work, frees its device memory (NULL entries are skipped) and its stream. The caller deletes the handle.
inline void destroy_handle(ImageHandle *h, std::initializer_list<void *> device_mem) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *m : device_mem)
        if (m) (void)hipFree(m);
    if (h->stream) (void)hipStreamDestroy(h->stream);
}

inline int check_handle(const char *lib, const void *h) {
    if (!h) return fail(GPUART_HIP_ERR_ARG, std::string(lib) + ": handle is NULL");
    return 0;
}

/// finish: waits for everything the handle has been given.
inline int finish_handle(const char *lib, ImageHandle *h) {
    if (int r = check_handle(lib, h)) return r;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// ---- argument checks -------------------------------------------------------------------------------------------------------------
inline int check_size(const char *lib, uint32_t w, uint32_t h) {
    if (w == 0 || h == 0 || w > 65536 || h > 65536)
        return fail(GPUART_HIP_ERR_ARG, std::string(lib) + ": bad size " + std::to_string(w) + " x " + std::to_string(h));
    return 0;
}

/// Is one of the pointers not a multiple of `align`? (NULL is aligned: an optional pointer may be given.)
inline bool misaligned(std::initializer_list<const void *> ptrs, size_t align) {
    for (const void *p : ptrs)
        if ((uintptr_t)p % align) return true;
    return false;
}

/// Do the na bytes at a and the nb bytes at b share a byte?
inline bool overlaps(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}

/// The caller's parameters, or with p = NULL what the library's own gpuart_<name>_defaults fills in.
template <class P>
P params_or_defaults(const P *p, int (*defaults)(P *)) {
    P v;
    if (p) v = *p;
    else defaults(&v);
    return v;
}

// ---- device memory ---------------------------------------------------------------------------------------------------------------
/// A device buffer that only grows. Growing waits for the stream first (work in flight may use the old memory), frees and allocates
/// again: the content is lost.
struct DeviceBuffer {
    void *mem = nullptr;
    size_t bytes = 0;
};

inline int ensure(hipStream_t stream, DeviceBuffer &b, size_t bytes) {
    if (bytes <= b.bytes) return 0;
    if (b.mem) {
        HIP_TRY(hipStreamSynchronize(stream));
        (void)hipFree(b.mem);
        b.mem = nullptr;
        b.bytes = 0;
    }
    HIP_TRY(hipMalloc(&b.mem, bytes));
    b.bytes = bytes;
    return 0;
}

/// A tile's radiance and G-buffer in device memory for a _host entry point: per pixel the radiance (16 bytes; the entry points write
/// their result over it), the record (32) and the ordinal (4), plane after plane from `base`.
struct Staged {
    float4 *rgba, *hits;
    int32_t *prims;
};
constexpr size_t STAGED_BYTES = 16 + 32 + 4;  ///< per pixel

inline int stage_gbuffer(hipStream_t stream, void *base, size_t n, const void *rgba, const void *hits, const void *prims, Staged &s) {
    s.rgba = (float4 *)base;
    s.hits = (float4 *)((char *)base + n * 16);
    s.prims = (int32_t *)((char *)base + n * 48);
    HIP_TRY(hipMemcpyAsync(s.rgba, rgba, n * 16, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s.hits, hits, n * 32, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(s.prims, prims, n * 4, hipMemcpyHostToDevice, stream));
    return 0;
}

// ---- the row block ---------------------------------------------------------------------------------------------------------------
// A 64 x 4 block: a wave is 64 consecutive pixels of one row, so a per-pixel 16-byte access is 1 KiB per wave instruction and the
// neighbours of a wave's pixels are neighbours in memory. Pixel (blockIdx.x * ROW_X + threadIdx.x, blockIdx.y * ROW_Y + threadIdx.y).
constexpr int ROW_X = 64, ROW_Y = 4;

inline dim3 row_block() { return dim3(ROW_X, ROW_Y); }
inline dim3 row_grid(uint32_t w, uint32_t h) { return dim3((w + ROW_X - 1) / ROW_X, (h + ROW_Y - 1) / ROW_Y); }

// ---- device functions ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

constexpr uint32_t US_EM_NONZERO = 1u, US_SPECULAR = 2u;  // userSphereFlags bits that take a user-sphere pixel out of the surface pixels

/// The pixel classes' one rule: a pixel whose record has primitive type `type` and whose ordinal is `prim` is a surface pixel — filtered,
/// and given a history — unless nothing was hit (type < 0) or it shows an emissive or specular user sphere (ordinal -2).
/// k_tp_accumulate writes this expression out instead of calling it: the call moves the load of the ordinal out of the branch that
/// needs it, and the kernel's instructions are held to what they were (profiles/image_libs.txt). tests/denoise_ref.py `surface` is the
/// one restatement both libraries are compared with.
__device__ __forceinline__ bool is_surface(int type, int32_t prim, uint32_t us_flags) {
    return type >= 0 && !(prim == -2 && (us_flags & (US_EM_NONZERO | US_SPECULAR)));
}

}  // namespace
