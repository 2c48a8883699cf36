"""ctypes bindings of lib/libgpuart.so (C++ host library, capi.h) and lib/libgpuart_hip.so
(device back end, include/gpuart_hip.h). Plumbing only — no computation happens here.
GPUART_LIBDIR selects another build of the pair: gpuart_amd/lib_test (the product + the test hooks of include/gpuart_hip_test.h:
what tests/conftest.py chooses), or an A/B variant under gpuart_amd/lib_ab/."""
import ctypes as C
import os
import sys

os.environ.setdefault("GPU_MAX_HW_QUEUES", "32")  # see libgpuart_hip's request_hw_queues(); before any HIP initialisation

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.environ.get("GPUART_LIBDIR") or os.path.join(HERE, "lib")  # override: A/B runs of differently built libraries
HIP_LIB = os.path.join(LIBDIR, "libgpuart_hip.so")
HOST_LIB = os.path.join(LIBDIR, "libgpuart.so")


class NativeLibraryMissing(RuntimeError):
    pass


class PrimDesc(C.Structure):
    _fields_ = [("type", C.c_int32), ("f", C.c_float * 9)]


class Params(C.Structure):
    _fields_ = [("sunDirAlt", C.c_float * 4), ("sunEnabled", C.c_int32), ("userSphere", C.c_float * 4),
                ("userSphereEm", C.c_float * 3), ("userSphereFlags", C.c_uint32), ("pixelSize", C.c_float),
                ("cameraPos", C.c_float * 3), ("maxSegments", C.c_int32), ("minWeight", C.c_float)]


class Counters(C.Structure):
    _fields_ = [("rays", C.c_uint64), ("nodes", C.c_uint64), ("prim_tests", C.c_uint64 * 4), ("segments", C.c_uint64),
                ("box_steps", C.c_uint64), ("box_steps_top", C.c_uint64), ("rewalks", C.c_uint64)]

    def algorithmic_bytes(self):
        """48 B per distinct node + (16 + 16*len) B per tested primitive."""
        p = self.prim_tests
        return 48 * self.nodes + 32 * p[0] + 48 * p[1] + 64 * p[2] + 80 * p[3]

    def as_dict(self):
        return dict(rays=self.rays, nodes=self.nodes, prim_tests=list(self.prim_tests), segments=self.segments,
                    algorithmic_bytes=self.algorithmic_bytes())


class RayHit(C.Structure):
    """gpuart_ray_hit (include/gpuart_hip.h): one query's record, 32 bytes."""
    _fields_ = [("pos", C.c_float), ("p", C.c_float * 3), ("n", C.c_float * 3), ("type", C.c_int32)]


# the same record as a NumPy dtype: what trace_rays / pick return for host arrays (hits.view(np.float32).reshape(-1, 8): the raw words)
class HipScene(C.Structure):
    """gpuart_hip_scene (include/gpuart_hip.h)."""
    _fields_ = [("layout", C.c_uint32), ("exact_boxes", C.c_uint32), ("recs", C.c_void_p), ("n_recs", C.c_uint64), ("prims", C.c_void_p),
                ("n_prims", C.c_uint64), ("prim_boxes", C.c_void_p), ("root_min", C.c_float * 3), ("root_max", C.c_float * 3),
                ("root_ref", C.c_uint32), ("box_slack", C.c_float), ("max_depth", C.c_uint32), ("generation", C.c_uint64)]


class RefitResult(C.Structure):
    """gpuart_refit_result (include/gpuart_refit.h)."""
    _fields_ = [("status", C.c_int32), ("first_bad", C.c_uint32), ("subnormal", C.c_uint32), ("root_min", C.c_float * 3), ("root_max", C.c_float * 3)]


class BuildResult(C.Structure):
    """gpuart_build_result (include/gpuart_build.h)."""
    _fields_ = [("n_recs", C.c_uint64), ("root_ref", C.c_uint32), ("max_depth", C.c_uint32), ("subnormal", C.c_uint32), ("levels", C.c_uint32),
                ("root_min", C.c_float * 3), ("root_max", C.c_float * 3)]


class PlocResult(C.Structure):
    """gpuart_ploc_result (include/gpuart_ploc.h)."""
    _fields_ = [("n_recs", C.c_uint64), ("root_ref", C.c_uint32), ("max_depth", C.c_uint32), ("subnormal", C.c_uint32), ("iterations", C.c_uint32),
                ("root_min", C.c_float * 3), ("root_max", C.c_float * 3)]


class EditResult(C.Structure):
    """gpuart_edit_result (include/gpuart_edit.h)."""
    _fields_ = [("status", C.c_int32), ("first_bad", C.c_uint32), ("n_prims", C.c_uint64), ("type_mask", C.c_uint32),
                ("root_min", C.c_float * 3), ("root_max", C.c_float * 3)]


EDIT_STEPS = ("validate", "scan", "move", "reduce")  # gpuart_edit_step_ms
REFIT_PAYLOAD = 16  # GPUART_REFIT_PAYLOAD
PLOC_STEPS = ("keys", "sort", "iterations", "number", "emit", "permute")  # gpuart_ploc_step_ms
TREE_MODES = {"morton": 0, "clustered": 1}  # Renderer::TreeMode
BUILD_STEPS = ("keys", "sort", "permute", "hierarchy", "number", "emit", "levels")  # gpuart_build_step_ms
RAY_HIT = np.dtype([("pos", np.float32), ("p", np.float32, 3), ("n", np.float32, 3), ("type", np.int32)])
RAYS_OCCLUSION = 1  # GPUART_HIP_RAYS_OCCLUSION
# gpuart_nearest_hit (include/gpuart_nearest.h): prim -1 none, -2 the user sphere; type -1 none
NEAREST_HIT = np.dtype([("dist", np.float32), ("q", np.float32, 3), ("d2", np.float32), ("prim", np.int32), ("type", np.int32), ("zero", np.uint32)])
NEAREST_CHUNK = 64  # GPUART_NEAREST_CHUNK
NEAREST_RING = 8    # GPUART_NEAREST_RING
NEAREST_MAX_DEPTH = 1024  # GPUART_NEAREST_MAX_DEPTH
NEAREST_KNN_MAX = 32  # GPUART_NEAREST_KNN_MAX


def _params(cls, defaults, noun, params):
    """None (the library's defaults), a `cls`, or a dict of fields that replace `defaults` -> `cls` or None."""
    if params is None or isinstance(params, cls):
        return params
    unknown = set(params) - set(defaults)
    if unknown:
        raise ValueError("unknown %s parameters: %s" % (noun, sorted(unknown)))
    return cls(**dict(defaults, **params))


# the two filters' parameter records are one layout under two names (csrc/image/atrous.h checks both)
_FILTER_FIELDS = [("iterations", C.c_uint32), ("lum_k", C.c_float), ("normal_pow2", C.c_uint32), ("depth_sigma", C.c_float)]


class DenoiseParams(C.Structure):
    """gpuart_denoise_params (include/gpuart_denoise.h)."""
    _fields_ = _FILTER_FIELDS


DENOISE_DEFAULTS = dict(iterations=5, lum_k=4.0, normal_pow2=5, depth_sigma=0.05)


def denoise_params(params):
    """None (the library's defaults), a DenoiseParams, or a dict of fields that replace the defaults -> DenoiseParams or None."""
    return _params(DenoiseParams, DENOISE_DEFAULTS, "denoiser", params)


class RefineParams(C.Structure):
    """gpuart_refine_params (include/gpuart_refine.h)."""
    _fields_ = _FILTER_FIELDS


REFINE_DEFAULTS = dict(iterations=5, lum_k=1.0, normal_pow2=5, depth_sigma=0.05)


def refine_params(params):
    """None (the library's defaults), a RefineParams, or a dict of fields that replace the defaults -> RefineParams or None."""
    return _params(RefineParams, REFINE_DEFAULTS, "refine", params)


class MomentsParams(C.Structure):
    """gpuart_moments_params (include/gpuart_moments.h)."""
    _fields_ = [("min_batches", C.c_float), ("spatial_k", C.c_float)]


MOMENTS_DEFAULTS = dict(min_batches=8.0, spatial_k=4.0)


def moments_params(params):
    """None (the library's defaults), a MomentsParams, or a dict of fields that replace the defaults -> MomentsParams or None."""
    return _params(MomentsParams, MOMENTS_DEFAULTS, "moments", params)


class AntiLagParams(C.Structure):
    """gpuart_antilag_params (include/gpuart_antilag.h)."""
    _fields_ = [("fast_history", C.c_float), ("min_batches", C.c_float), ("min_votes", C.c_float), ("clip", C.c_float), ("z_lo", C.c_float),
                ("z_hi", C.c_float)]


ANTILAG_DEFAULTS = dict(fast_history=4.0, min_batches=8.0, min_votes=8.0, clip=3.0, z_lo=2.0, z_hi=4.0)


def antilag_params(params):
    """None (the library's defaults), an AntiLagParams, or a dict of fields that replace the defaults -> AntiLagParams or None."""
    return _params(AntiLagParams, ANTILAG_DEFAULTS, "anti-lag", params)


class EdgesParams(C.Structure):
    """gpuart_edges_params (include/gpuart_edges.h)."""
    _fields_ = [("n_sub", C.c_uint32), ("normal_min", C.c_float), ("plane_tol", C.c_float)]


EDGES_DEFAULTS = dict(n_sub=8, normal_min=0.95, plane_tol=0.02)
EDGES_MAX_SUB = 16  # GPUART_EDGES_MAX_SUB


def edges_params(params):
    """None (the library's defaults), an EdgesParams, or a dict of fields that replace the defaults -> EdgesParams or None."""
    return _params(EdgesParams, EDGES_DEFAULTS, "edge-resolve", params)


class UpscaleParams(C.Structure):
    """gpuart_upscale_params (include/gpuart_upscale.h)."""
    _fields_ = [("normal_min", C.c_float), ("plane_tol", C.c_float)]


UPSCALE_DEFAULTS = dict(normal_min=0.95, plane_tol=0.02)
UPSCALE_SCALES = (2, 3, 4)  # GPUART_UPSCALE_MIN_SCALE..GPUART_UPSCALE_MAX_SCALE


def upscale_params(params):
    """None (the library's defaults), an UpscaleParams, or a dict of fields that replace the defaults -> UpscaleParams or None."""
    return _params(UpscaleParams, UPSCALE_DEFAULTS, "upscaler", params)


class DespeckleParams(C.Structure):
    """gpuart_despeckle_params (include/gpuart_despeckle.h)."""
    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("k", C.c_float), ("floor", C.c_float), ("min_count", C.c_uint32)]


DESPECKLE_DEFAULTS = dict(radius=1, rank=3, k=2.0, floor=1e-3, min_count=4)


def despeckle_params(params):
    """None (the library's defaults), a DespeckleParams, or a dict of fields that replace the defaults -> DespeckleParams or None."""
    return _params(DespeckleParams, DESPECKLE_DEFAULTS, "firefly-clamp", params)


class DespeckleSummary(C.Structure):
    """gpuart_despeckle_summary (include/gpuart_despeckle.h): the counts of a handle's last run."""
    _fields_ = [("surface", C.c_uint64), ("clamped", C.c_uint64), ("too_few", C.c_uint64)]

    def as_dict(self):
        return dict(surface=int(self.surface), clamped=int(self.clamped), too_few=int(self.too_few))


class DisplayParams(C.Structure):
    """gpuart_display_params (include/gpuart_display.h)."""
    _fields_ = [("gain", C.c_float), ("auto_exposure", C.c_uint32), ("key", C.c_float), ("lo_share", C.c_float), ("hi_share", C.c_float),
                ("adapt", C.c_float), ("min_gain", C.c_float), ("max_gain", C.c_float), ("curve", C.c_uint32), ("white", C.c_float),
                ("transfer", C.c_uint32), ("dither", C.c_uint32)]


DISPLAY_DEFAULTS = dict(gain=1.0, auto_exposure=0, key=0.18, lo_share=0.5, hi_share=0.02, adapt=1.0, min_gain=2.0 ** -16, max_gain=2.0 ** 16,
                        curve=0, white=4.0, transfer=0, dither=0)
DISPLAY_CURVES = dict(clamp=0, reinhard=1, aces=2)      # GPUART_DISPLAY_CLAMP, _REINHARD, _ACES
DISPLAY_TRANSFERS = dict(linear=0, srgb=1)              # GPUART_DISPLAY_LINEAR, _SRGB
DISPLAY_SOURCES = dict(radiance=0, direct=1, denoised=2, preview=3, guided_preview=4, refined=5)   # gpuart_display_source


def display_params(params):
    """None (the library's defaults), a DisplayParams, or a dict of fields that replace the defaults -> DisplayParams or None. In a dict
    `curve` and `transfer` may be given by name (DISPLAY_CURVES, DISPLAY_TRANSFERS)."""
    if isinstance(params, dict):
        params = dict(params)
        if isinstance(params.get("curve"), str):
            params["curve"] = DISPLAY_CURVES[params["curve"]]
        if isinstance(params.get("transfer"), str):
            params["transfer"] = DISPLAY_TRANSFERS[params["transfer"]]
        for k in ("auto_exposure", "dither"):
            if k in params:
                params[k] = int(params[k])
    return _params(DisplayParams, DISPLAY_DEFAULTS, "display", params)


class DisplayState(C.Structure):
    """gpuart_display_state (include/gpuart_display.h)."""
    _fields_ = [("histogram", C.c_uint64 * 256), ("counted", C.c_uint64), ("skipped", C.c_uint64), ("gain", C.c_float), ("valid", C.c_uint32)]

    def as_dict(self):
        return dict(histogram=[int(v) for v in self.histogram], counted=int(self.counted), skipped=int(self.skipped),
                    gain=np.float32(self.gain), valid=int(self.valid))


class TemporalParams(C.Structure):
    """gpuart_temporal_params (include/gpuart_temporal.h)."""
    _fields_ = [("max_history", C.c_float), ("plane_tol", C.c_float), ("normal_min", C.c_float)]


TEMPORAL_DEFAULTS = dict(max_history=4.0, plane_tol=0.01, normal_min=0.8)


def temporal_params(params):
    """None (the library's defaults), a TemporalParams, or a dict of fields that replace the defaults -> TemporalParams or None."""
    return _params(TemporalParams, TEMPORAL_DEFAULTS, "temporal", params)


class ConvergeSummary(C.Structure):
    """gpuart_converge_summary (include/gpuart_converge.h): what a measure says about the frame."""
    _fields_ = [("pixels", C.c_uint64), ("above", C.c_uint64), ("non_finite", C.c_uint64), ("max_error", C.c_float),
                ("batches", C.c_uint32), ("total", C.c_uint32)]

    def as_dict(self):
        return dict(pixels=self.pixels, above=self.above, non_finite=self.non_finite, max_error=float(self.max_error),
                    batches=self.batches, total=self.total)


class AdaptiveSummary(C.Structure):
    """gpuart_adaptive_summary (include/gpuart_adaptive.h): what a select says about the frame and its blocks."""
    _fields_ = [("pixels", C.c_uint64), ("above", C.c_uint64), ("non_finite", C.c_uint64), ("paths_sum", C.c_uint64), ("blocks", C.c_uint32),
                ("active_blocks", C.c_uint32), ("paths_min", C.c_uint32), ("paths_max", C.c_uint32), ("max_error", C.c_float),
                ("reserved", C.c_uint32)]

    def as_dict(self):
        return dict(pixels=self.pixels, above=self.above, non_finite=self.non_finite, paths_sum=self.paths_sum, blocks=self.blocks,
                    active_blocks=self.active_blocks, paths_min=self.paths_min, paths_max=self.paths_max, max_error=float(self.max_error))


CONVERGE_MAX_PATHS = 1 << 24    # GPUART_CONVERGE_MAX_PATHS
CONVERGE_DEFAULT_BATCH = 64     # GPUART_CONVERGE_DEFAULT_BATCH
CONVERGE_DEFAULT_FLOOR = 1.0 / 256   # one step of an 8-bit output (gpuart_cli --until-floor)
ADAPTIVE_DEFAULT_MIN_PATHS = 8   # GPUART_ADAPTIVE_DEFAULT_MIN_PATHS (gpuart_cli --adaptive-min)


def _user_sphere(us):
    return None if us is None else (C.c_float * 4)(*[float(x) for x in us])


def _rays_array(rays):
    rays = np.ascontiguousarray(rays, np.float32)
    if rays.ndim != 2 or rays.shape[1] != 8:
        raise ValueError("rays must be (n, 8): origin.xyz, tmax, dir.xyz, unused")
    return rays


def _points_array(points):
    points = np.ascontiguousarray(points, np.float32)
    if points.ndim != 2 or points.shape[1] != 4:
        raise ValueError("points must be (n, 4): p.xyz, r")
    return points


def _pixels_array(xy):
    xy = np.asarray(xy)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("xy must be (n, 2) frame pixels (x, y), row 0 = bottom")
    if xy.size and (xy.min() < 0 or xy.max() > 0xffffffff):
        raise ValueError("pixel coordinates must be non-negative 32-bit values")
    return np.ascontiguousarray(xy, np.uint32)


_hip = None
_host = None
TEST_LIBDIR = os.path.join(HERE, "lib_test")  # the same sources + the hooks of include/gpuart_hip_test.h (csrc/Makefile)


class _HipLibrary(C.CDLL):
    """libgpuart_hip.so; says where the test hooks live when the product library is asked for one."""

    def __getattr__(self, name):
        try:
            return super().__getattr__(name)
        except AttributeError:
            if name.startswith("gpuart_hip_test_"):
                raise AttributeError("%s is a test hook (include/gpuart_hip_test.h): the product library %s has none — load the test build with "
                                     "GPUART_LIBDIR=%s" % (name, self._name, TEST_LIBDIR)) from None
            raise


def hip_lib():
    """libgpuart_hip.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB):
            raise NativeLibraryMissing("%s not found — run `python -c 'import __graft_entry__ as g; g.build()'` "
                                       "(make -C gpuart_amd/csrc); there is no CPU fallback" % HIP_LIB)
        L = _HipLibrary(HIP_LIB, mode=C.RTLD_GLOBAL)
        L.gpuart_hip_last_error.restype = C.c_char_p
        L.gpuart_hip_frame_row.restype = C.c_uint32
        _hip = L
    return _hip


_image_libs = {}


def _image_lib(name):
    """libgpuart_<name>.so, one of the image libraries; raises NativeLibraryMissing if it has not been built (no fallback)."""
    if name not in _image_libs:
        path = os.path.join(LIBDIR, "libgpuart_%s.so" % name)
        if not os.path.exists(path):
            raise NativeLibraryMissing("%s not found — run make -C gpuart_amd/csrc; there is no CPU fallback" % path)
        L = C.CDLL(path)
        getattr(L, "gpuart_%s_last_error" % name).restype = C.c_char_p
        _image_libs[name] = L
    return _image_libs[name]


def denoise_lib():
    """libgpuart_denoise.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("denoise")


def temporal_lib():
    """libgpuart_temporal.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("temporal")


def converge_lib():
    """libgpuart_converge.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("converge")


def refine_lib():
    """libgpuart_refine.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("refine")


def adaptive_lib():
    """libgpuart_adaptive.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("adaptive")


def moments_lib():
    """libgpuart_moments.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("moments")


def antilag_lib():
    """libgpuart_antilag.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("antilag")


def edges_lib():
    """libgpuart_edges.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("edges")


def despeckle_lib():
    """libgpuart_despeckle.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("despeckle")


def upscale_lib():
    """libgpuart_upscale.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("upscale")


def refit_lib():
    """libgpuart_refit.so (include/gpuart_refit.h), built by the image libraries' rule; raises NativeLibraryMissing if it has not been built
    (no fallback)."""
    return _image_lib("refit")


def build_lib():
    """libgpuart_build.so (include/gpuart_build.h), built by the image libraries' rule; raises NativeLibraryMissing if it has not been built
    (no fallback)."""
    return _image_lib("build")


def ploc_lib():
    """libgpuart_ploc.so (include/gpuart_ploc.h), built by the image libraries' rule; raises NativeLibraryMissing if it has not been built
    (no fallback)."""
    return _image_lib("ploc")


def edit_lib():
    """libgpuart_edit.so (include/gpuart_edit.h), built by the image libraries' rule; raises NativeLibraryMissing if it has not been built
    (no fallback)."""
    return _image_lib("edit")


def nearest_lib():
    """libgpuart_nearest.so (include/gpuart_nearest.h), built by the image libraries' rule; raises NativeLibraryMissing if it has not been built
    (no fallback)."""
    return _image_lib("nearest")


def display_lib():
    """libgpuart_display.so; raises NativeLibraryMissing if it has not been built (no fallback)."""
    return _image_lib("display")


def host_lib():
    global _host
    if _host is None:
        hip_lib()
        if not os.path.exists(HOST_LIB):
            raise NativeLibraryMissing("%s not found — run make -C gpuart_amd/csrc" % HOST_LIB)
        L = C.CDLL(HOST_LIB)
        L.gpuart_renderer_create.restype = C.c_void_p
        L.gpuart_renderer_backend.restype = C.c_void_p
        L.gpuart_renderer_path_tracing_pass.restype = C.c_uint
        for name in ["destroy", "is_ok", "set_primitives", "init_box", "init_dragon", "init_cluster", "init_tree", "set_camera", "update_viewport",
                     "set_tile", "set_interleaved_tile", "set_sun", "set_user_sphere", "set_max_path_segments", "set_seed", "render_direct",
                     "restart_path_tracing", "path_tracing_pass", "read_direct", "read_radiance", "finish", "backend",
                     "save_checkpoint", "load_checkpoint",
                     "params", "scene_info"]:
            getattr(L, "gpuart_renderer_" + name).argtypes = None
        _host = L
    return _host


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def make_prims(descs):
    arr = (PrimDesc * len(descs))()
    for i, (t, f) in enumerate(descs):
        arr[i].type = t
        for k, v in enumerate(f):
            arr[i].f[k] = v
    return arr


# ---- pure host functions ------------------------------------------------------------------------
def _take_quads(L, q, n):
    """The n quads the host library allocated at q, copied out as an (n, 4) float32 array and freed."""
    out = np.ctypeslib.as_array(q, shape=(n, 4)).copy()
    L.gpuart_free(q)
    return out


def compile_bvh(descs, max_levels=1024, min_prims=2):
    """BoundingVolumesHierarchy(prims, max_levels, min_prims).Compile() -> (quads (n,4) float32, depth)."""
    L = host_lib()
    arr = descs if isinstance(descs, C.Array) else make_prims(descs)
    q = C.POINTER(C.c_float)()
    nq = C.c_size_t(0)
    depth = C.c_uint(0)
    rc = L.gpuart_compile_bvh(arr, C.c_int(len(arr)), C.c_uint(max_levels), C.c_uint(min_prims), C.byref(q), C.byref(nq),
                              C.byref(depth))
    if rc != 0:
        raise RuntimeError("gpuart_compile_bvh failed")
    return _take_quads(L, q, nq.value), depth.value


def rebuild_tree(quads, order=None):
    """gpuart_rebuild_tree: BoundingVolumesHierarchy::RebuildMorton on the compiled tree `quads`, without a device -> (quads', new_to_old).
    `order`: the permutation to check instead of sorting. ValueError for a malformed tree (-1) or a refusal (-2)."""
    L = host_lib()
    q = np.ascontiguousarray(quads, np.float32).reshape(-1)
    o = None if order is None else np.ascontiguousarray(order, np.uint32).reshape(-1)
    out = C.POINTER(C.c_float)()
    nout = C.c_size_t(0)
    perm = np.zeros(max(1, q.size // 8), np.uint32)   # (a primitive takes at least two quads)
    rc = L.gpuart_rebuild_tree(_p(q), C.c_size_t(q.size // 4), _p(o) if o is not None else None, C.byref(out), C.byref(nout), _p(perm))
    if rc != 0:
        raise ValueError("gpuart_rebuild_tree: %d" % rc)
    res = _take_quads(L, out, nout.value)
    n = int(o.size) if o is not None else None
    if n is None:
        n = sum(1 for _ in _leaf_prims(res))
    return res, perm[:n].copy()


def adopt_tree(quads, order, refs):
    """gpuart_adopt_tree: BoundingVolumesHierarchy::AdoptTopology on the compiled tree `quads`, without a device -> quads'. `order`: the old
    ordinal of every new one; `refs`: two child refs per record in pre-order (include/gpuart_ploc.h). ValueError for a malformed tree
    (-1) or a refusal (-2)."""
    L = host_lib()
    q = np.ascontiguousarray(quads, np.float32).reshape(-1)
    o = np.ascontiguousarray(order, np.uint32).reshape(-1)
    r = np.ascontiguousarray(refs, np.uint32).reshape(-1)
    if r.size % 2:
        raise ValueError("adopt_tree: two refs per record")
    out = C.POINTER(C.c_float)()
    nout = C.c_size_t(0)
    rc = L.gpuart_adopt_tree(_p(q), C.c_size_t(q.size // 4), _p(o), _p(r) if r.size else None, C.c_size_t(r.size // 2), C.byref(out), C.byref(nout))
    if rc != 0:
        raise ValueError("gpuart_adopt_tree: %d" % rc)
    return _take_quads(L, out, nout.value)


def edit_tree(quads, remove, add_types, add_payload, order=None, refs=None):
    """gpuart_edit_tree: BoundingVolumesHierarchy::EditPrimitives on the compiled tree `quads`, without a device, followed by the Morton
    rebuild (refs None; `order` None or the permutation to check) or by AdoptTopology of `order` and `refs` -> (quads', new_to_old of
    the edited list). ValueError for a malformed tree (-1), a refused edit (-2; `first_bad`: the first offender, the removals counted
    first, or None) or a refused order or topology (-3)."""
    L = host_lib()
    q = np.ascontiguousarray(quads, np.float32).reshape(-1)
    rem = np.ascontiguousarray(remove, np.uint32).reshape(-1)
    typ = np.ascontiguousarray(add_types, np.uint32).reshape(-1)
    pay = np.ascontiguousarray(add_payload, np.float32).reshape(-1)
    if pay.size != 16 * typ.size:
        raise ValueError("edit_tree: add_payload must hold 16 floats per added primitive")
    o = None if order is None else np.ascontiguousarray(order, np.uint32).reshape(-1)
    r = None if refs is None else np.ascontiguousarray(refs, np.uint32).reshape(-1)
    ptr = lambda a: _p(a) if a is not None and a.size else None
    out = C.POINTER(C.c_float)()
    nout, bad = C.c_size_t(0), C.c_size_t(0)
    perm = np.zeros(q.size // 8 + typ.size + 1, np.uint32)   # (a primitive takes at least two quads)
    rc = L.gpuart_edit_tree(_p(q), C.c_size_t(q.size // 4), ptr(rem), C.c_size_t(rem.size), ptr(typ), ptr(pay), C.c_size_t(typ.size),
                            C.c_int(0 if r is None else 1), ptr(o), ptr(r), C.c_size_t(0 if r is None else r.size // 2), C.byref(out), C.byref(nout),
                            _p(perm), C.byref(bad))
    if rc != 0:
        e = ValueError("gpuart_edit_tree: %d" % rc)
        e.first_bad = int(bad.value) if rc == -2 and bad.value != C.c_size_t(-1).value else None
        raise e
    res = _take_quads(L, out, nout.value)
    return res, perm[:sum(1 for _ in _leaf_prims(res))].copy()


def _leaf_prims(quads):
    """The header quad address of every primitive of a canonical compiled tree, in the order the leaves are met."""
    bits = np.ascontiguousarray(quads, np.float32).view(np.uint32)
    stack = [0]
    while stack:
        a = stack.pop()
        flags = int(bits[a + 2, 0])
        if flags & 0x80000000:
            at = a + 3
            for _ in range(flags & 0x1fffffff):
                yield at
                at += 2 + int(bits[at, 0])
        else:
            stack.append(int(bits[a + 2, 2]))
            stack.append(int(bits[a + 2, 1]))


def last_build_ms():
    """(build ms, compile ms) the host library itself spent in the last compile_bvh / compile_bvh_from_file of this process."""
    out = (C.c_double * 2)()
    host_lib().gpuart_last_build_ms(out)
    return float(out[0]), float(out[1])


def compile_bvh_from_file(kind, path, magnification=1.0, translation=(0, 0, 0), extra=()):
    """kind: 'ply' or 'dat'. Returns (quads, depth, nloaded)."""
    L = host_lib()
    ex = make_prims(list(extra))
    q = C.POINTER(C.c_float)()
    nq = C.c_size_t(0)
    depth = C.c_uint(0)
    nl = C.c_size_t(0)
    rc = L.gpuart_compile_bvh_from_file(C.c_int(0 if kind == "ply" else 1), path.encode(), C.c_float(magnification),
                                        _f3(translation), ex, C.c_int(len(ex)), C.byref(q), C.byref(nq), C.byref(depth),
                                        C.byref(nl))
    if rc != 0:
        raise RuntimeError("loading %s failed" % path)
    return _take_quads(L, q, nq.value), depth.value, nl.value


def sort_permutation(keys, threads=8):
    """gpuart_sort_permutation: the BVH build's parallel exact sort (csrc/host/exact_sort.h) on `keys`."""
    k = np.ascontiguousarray(keys, np.float32)
    perm = np.zeros(len(k), np.uint32)
    host_lib().gpuart_sort_permutation(_p(k), C.c_size_t(len(k)), C.c_uint(threads), _p(perm))
    return perm


def camera_basis(pos, dir, up, fov_y, screen_dist, W, H):
    out = np.zeros(13, np.float32)
    host_lib().gpuart_camera_basis(_f3(pos), _f3(dir), _f3(up), C.c_float(fov_y), C.c_float(screen_dist), C.c_uint(W),
                                   C.c_uint(H), _p(out))
    return out


def sun_direction(az, alt):
    out = (C.c_float * 3)()
    host_lib().gpuart_sun_direction(C.c_float(az), C.c_float(alt), out)
    return np.array(list(out), np.float32)


def vec3_ops(a, b, s, dtype=np.float32):
    """Every Vec3 operation of csrc/host/math_types.h once (36 values; gpuart_vec3f_ops / gpuart_vec3d_ops)."""
    a = np.ascontiguousarray(a, dtype); b = np.ascontiguousarray(b, dtype)
    out = np.zeros(36, dtype)
    if dtype == np.float32:
        host_lib().gpuart_vec3f_ops(_p(a), _p(b), C.c_float(float(s)), _p(out))
    else:
        host_lib().gpuart_vec3d_ops(_p(a), _p(b), C.c_double(float(s)), _p(out))
    return out


# ---- device back end (include/gpuart_hip.h) -----------------------------------------------------------
class TileGeom(C.Structure):
    """gpuart_tile_geom (include/gpuart_hip.h): one rank's share of a frame sharded by rows."""
    _fields_ = [("W", C.c_uint32), ("H", C.c_uint32), ("x0", C.c_uint32), ("y0", C.c_uint32), ("tw", C.c_uint32),
                ("th", C.c_uint32), ("band_rows", C.c_uint32), ("band_stride", C.c_uint32)]

    def rows(self):
        """Frame rows of the share, in local row order."""
        L = hip_lib()
        return np.array([L.gpuart_hip_frame_row(C.byref(self), C.c_uint32(k)) for k in range(self.th)], np.int64)


class TemporalView(C.Structure):
    """gpuart_temporal_view (include/gpuart_temporal.h): the view a tile was rendered from."""
    _fields_ = [("pos", C.c_float * 3), ("bottomLeft", C.c_float * 3), ("deltaHorz", C.c_float * 3), ("deltaVert", C.c_float * 3),
                ("geom", TileGeom), ("userSphere", C.c_float * 4), ("userSphereFlags", C.c_uint32)]


def temporal_view(cam, geom, user_sphere=None, us_flags=0):
    """cam: the 12 floats given to Backend.set_camera (pos, bottomLeft, deltaHorz, deltaVert; more are ignored); geom: a TileGeom
    (Backend.get_share) or (W, H, x0, y0, tw, th, band_rows, band_stride); user_sphere: (x, y, z, radius) or None."""
    v = TemporalView()
    cam = [float(x) for x in cam[:12]]
    v.pos[:], v.bottomLeft[:], v.deltaHorz[:], v.deltaVert[:] = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    if isinstance(geom, TileGeom):
        C.memmove(C.byref(v.geom), C.byref(geom), C.sizeof(TileGeom))
    else:
        v.geom = TileGeom(*[int(g) for g in geom])
    v.userSphere[:] = [float(x) for x in (user_sphere if user_sphere is not None else (0, 0, 0, 0))]
    v.userSphereFlags = int(us_flags)
    return v


def share_of_rank(W, H, rank, nranks, band_rows=8):
    """gpuart_hip_share_of_rank: bands of band_rows rows dealt round-robin to the ranks (pure host code)."""
    g = TileGeom()
    rc = hip_lib().gpuart_hip_share_of_rank(C.c_uint32(W), C.c_uint32(H), rank, nranks, C.c_uint32(band_rows), C.byref(g))
    if rc:
        raise ValueError("gpuart_hip_share_of_rank(%d, %d, %d, %d, %d) -> %d" % (W, H, rank, nranks, band_rows, rc))
    return g


def scatter_rows_host(g, tile_rgba, full_rgba):
    """gpuart_hip_scatter_rows_host: rows of a share (th x tw x 4) into the full frame (H x W x 4), on the host."""
    tile = np.ascontiguousarray(tile_rgba, np.float32)
    assert tile.shape == (g.th, g.tw, 4) and full_rgba.shape == (g.H, g.W, 4) and full_rgba.flags["C_CONTIGUOUS"]
    rc = hip_lib().gpuart_hip_scatter_rows_host(C.byref(g), _p(tile), _p(full_rgba))
    if rc:
        raise ValueError("gpuart_hip_scatter_rows_host -> %d" % rc)
    return full_rgba


def tree_class(quads):
    """What the uploader decides about a compiled tree, without a device: dict(irregular, disorderly, type_mask); the fast kernels
    walk nearest-child-first iff neither flag is set."""
    L = hip_lib()
    q = np.ascontiguousarray(quads, np.float32)
    flags = C.c_uint32(0)
    rc = L.gpuart_hip_test_tree_class(_p(q), C.c_size_t(q.size // 4), C.byref(flags))
    if rc != 0:
        raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    return dict(irregular=bool(flags.value & 1), disorderly=bool(flags.value & 2), type_mask=(flags.value >> 8) & 15)


def convert_tree(quads, nquads=None, threads=1, top_depth=0):
    """The arrays the uploader would put on the device for a compiled tree (gpuart_hip_test_convert: its own Converter::convert, no device):
    dict(recs (R, 4, 4) float32, prims (P, 3, 4) float32, root_min, root_max (3,) float32, root_ref, num_nodes, max_depth, type_mask, irregular,
    disorderly, subnormal). nquads: how many of the quads the library is told of (default: all). A rejected tree raises HipError with the
    uploader's message."""
    L = hip_lib()
    q = np.ascontiguousarray(quads, np.float32)
    nq = C.c_size_t(q.size // 4 if nquads is None else int(nquads))
    assert nq.value <= q.size // 4
    info, box = (C.c_uint32 * 8)(), (C.c_float * 6)()
    rc = L.gpuart_hip_test_convert(_p(q), nq, C.c_uint32(threads), C.c_uint32(top_depth), None, C.c_size_t(0), None, C.c_size_t(0), info, box)
    if rc != 0:
        raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    recs, prims = np.empty((info[0], 4, 4), np.float32), np.empty((info[1], 3, 4), np.float32)
    rc = L.gpuart_hip_test_convert(_p(q), nq, C.c_uint32(threads), C.c_uint32(top_depth), _p(recs), C.c_size_t(info[0]), _p(prims),
                                   C.c_size_t(info[1]), info, box)
    if rc != 0:
        raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    return dict(recs=recs, prims=prims, root_min=np.array(box[0:3], np.float32), root_max=np.array(box[3:6], np.float32), root_ref=int(info[2]),
                num_nodes=int(info[3]), max_depth=int(info[4]), type_mask=int(info[5]), irregular=bool(info[6] & 1), disorderly=bool(info[6] & 2),
                subnormal=bool(info[6] & 4))


KERNEL_ENTRIES = ("direct", "run", "trace", "query")   # gpuart_hip_test_kernel_choice's `entry`


def kernel_choice(type_mask, exact_boxes, ref_order, lean, mode, entry):
    """The instantiation the library's launch sites would pick, without a device: (TYPES, COUNT, REFWORK); entry: one of KERNEL_ENTRIES."""
    L = hip_lib()
    out = (C.c_uint32 * 3)()
    rc = L.gpuart_hip_test_kernel_choice(C.c_uint32(type_mask), C.c_uint32(exact_boxes), C.c_uint32(ref_order), C.c_uint32(lean), int(mode),
                                         KERNEL_ENTRIES.index(entry), out)
    if rc != 0:
        raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    return int(out[0]), bool(out[1]), bool(out[2])


def tree_slack(quads):
    """(slack constant the upload would give the tree for its quick box answers — inf: none —, a box plane is subnormal), without a device."""
    L = hip_lib()
    q = np.ascontiguousarray(quads, np.float32)
    slack, flags = C.c_float(0), C.c_uint32(0)
    for rc in (L.gpuart_hip_test_tree_slack(_p(q), C.c_size_t(q.size // 4), C.byref(slack)),
               L.gpuart_hip_test_tree_class(_p(q), C.c_size_t(q.size // 4), C.byref(flags))):
        if rc != 0:
            raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    return float(slack.value), bool(flags.value & 4)


def comm_library():
    """Path of the RCCL library libgpuart_hip resolved its entry points from (dladdr of ncclCommInitRank)."""
    L = hip_lib()
    buf = C.create_string_buffer(4096)
    rc = L.gpuart_hip_comm_library(buf, C.c_size_t(len(buf)))
    if rc != 0:
        raise HipError("gpuart_hip error %d: %s" % (rc, L.gpuart_hip_last_error().decode()))
    return buf.value.decode()


def comm_unique_id():
    """gpuart_hip_comm_unique_id (ncclGetUniqueId): 128 bytes for rank 0 to hand to the other ranks."""
    buf = (C.c_ubyte * 128)()
    L = hip_lib()
    if L.gpuart_hip_comm_unique_id(buf):
        raise HipError(L.gpuart_hip_last_error().decode())
    return bytes(buf)


def phase_begin(name, timeout_ms):
    """gpuart_hip_phase_begin: names the phase the process enters and arms the library's watchdog (a native thread: it fires
    whatever the interpreter is doing) — a phase that outlives timeout_ms ends the process with exit code WATCHDOG_EXIT after
    printing the phase and the library's recent errors."""
    hip_lib().gpuart_hip_phase_begin(str(name).encode(), C.c_uint32(int(timeout_ms)))


def phase_end():
    hip_lib().gpuart_hip_phase_end()


def phase_log(on):
    """gpuart_hip_phase_log: phase lines on / off from now on (the watchdog stays armed either way); returns the previous setting."""
    return bool(hip_lib().gpuart_hip_phase_log(C.c_int(1 if on else 0)))


class phase:
    """with phase("communicator init", 120000): ...   (the phase ends when the block does, exception or not)"""

    def __init__(self, name, timeout_ms):
        self.name, self.timeout_ms = name, timeout_ms

    def __enter__(self):
        phase_begin(self.name, self.timeout_ms)

    def __exit__(self, *exc):
        phase_end()
        return False


WATCHDOG_EXIT = 86
ERR_TIMEOUT = -4


def comm_stuck():
    """True once an RCCL call of this process has outlived GPUART_HIP_COMM_TIMEOUT_MS (its thread is parked in it)."""
    return bool(hip_lib().gpuart_hip_comm_stuck())


def comm_init_all(backends):
    """gpuart_hip_comm_init_all: the contexts become the ranks 0..n-1 of one communicator (ncclCommInitAll)."""
    L = hip_lib()
    arr = (C.c_void_p * len(backends))(*[b.ctx for b in backends])
    backends[0]._chk(L.gpuart_hip_comm_init_all(arr, len(backends)))


def gather_all_read(backends, which, divide_by, root, W, H):
    """gpuart_hip_gather_all_read: the frame assembled on the root's device from every context's share, read back (H, W, 4)."""
    L = hip_lib()
    arr = (C.c_void_p * len(backends))(*[b.ctx for b in backends])
    out = np.empty((H, W, 4), np.float32)
    backends[0]._chk(L.gpuart_hip_gather_all_read(arr, len(backends), which, C.c_float(divide_by), root, _p(out)))
    return out


def _library_symbols(path):
    """{address: name} of a shared library's symbol table (nm; local symbols included)."""
    import subprocess
    out = subprocess.run(["nm", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {int(f[0], 16): f[2] for f in (line.split() for line in out.splitlines()) if len(f) == 3}


class HipError(RuntimeError):
    """A gpuart_hip_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*: -4 a bounded wait ran out)."""
    code = None


class Backend:
    """A gpuart_hip_ctx. Owns the context unless constructed from a borrowed pointer."""

    def __init__(self, device=0, borrowed=None):
        self.L = hip_lib()
        self.device = device
        self.owned = borrowed is None
        if borrowed is None:
            ctx = C.c_void_p()
            self._chk(self.L.gpuart_hip_create(C.c_int(device), C.byref(ctx)))
            self.ctx = ctx
        else:
            self.ctx = C.c_void_p(borrowed)
        self.tile = None

    def _chk(self, rc):
        if rc != 0:
            e = HipError("gpuart_hip error %d: %s" % (rc, self.L.gpuart_hip_last_error().decode()))
            e.code = rc
            raise e

    def close(self):
        for handle in (getattr(self, "_refit", None), getattr(self, "_build", None), getattr(self, "_ploc", None), getattr(self, "_edit", None),
                       getattr(self, "_nearest", None)):
            if handle is not None:
                handle.close()
        if self.owned and self.ctx:
            self.L.gpuart_hip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # frame / scene / camera
    def resize(self, W, H):
        self._chk(self.L.gpuart_hip_resize(self.ctx, C.c_uint32(W), C.c_uint32(H)))
        self.tile = (0, 0, W, H)

    def set_tile(self, x0, y0, tw, th):
        self._chk(self.L.gpuart_hip_set_tile(self.ctx, C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(tw), C.c_uint32(th)))
        self.tile = (x0, y0, tw, th)

    def set_tile_interleaved(self, x0, y0, tw, th_local, band_rows, band_stride):
        self._chk(self.L.gpuart_hip_set_tile_interleaved(self.ctx, C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(tw), C.c_uint32(th_local),
                                                         C.c_uint32(band_rows), C.c_uint32(band_stride)))
        self.tile = (x0, y0, tw, th_local)

    def upload_bvh(self, quads):
        quads = np.ascontiguousarray(quads, np.float32)
        self._chk(self.L.gpuart_hip_upload_bvh(self.ctx, _p(quads), C.c_size_t(quads.size // 4)))

    def set_camera(self, cam):
        cam = np.ascontiguousarray(cam, np.float32)
        self._chk(self.L.gpuart_hip_set_camera(self.ctx, _f3(cam[0:3]), _f3(cam[3:6]), _f3(cam[6:9]), _f3(cam[9:12])))

    # a refit in place (include/gpuart_refit.h)
    def scene_device(self):
        """gpuart_hip_scene_device: the uploaded scene's device arrays and what the context knows of its tree, as a HipScene (pointers as
        integers; valid until the next upload). Flushes and waits for every pass requested so far."""
        s = HipScene()
        self._chk(self.L.gpuart_hip_scene_device(self.ctx, C.byref(s)))
        return s

    def scene_refitted(self, root_min, root_max, subnormal):
        self._chk(self.L.gpuart_hip_scene_refitted(self.ctx, _f3(root_min), _f3(root_max), C.c_int(1 if subnormal else 0)))

    def refit(self, ordinals, payload):
        """Replaces the primitives `ordinals` (strictly ascending device ordinals, as trace_rays returns them) by `payload` (n x 16 floats:
        each primitive's canonical data quads, zero-padded) and refits the tree's boxes on the device; the context adopts the result.
        Both arguments torch tensors on this device (int32 / float32, contiguous: the call stays device to device) or both anything NumPy
        converts. Returns dict(root_min, root_max, subnormal, levels). A refused update raises HipError with code -1 (ERR_ARG), `first_bad`
        = the offending update's index, and nothing changed."""
        R = refit_lib()
        scene = self.scene_device()
        if getattr(self, "_refit", None) is None:
            self._refit = _RefitHandle(self.device)
        h = self._refit
        if h.generation != scene.generation:
            h._chk(R.gpuart_refit_bind(h, C.byref(scene)))
            h.generation = scene.generation
        res = RefitResult()
        if hasattr(ordinals, "data_ptr"):
            import torch
            if not (hasattr(payload, "data_ptr") and ordinals.is_cuda and payload.is_cuda and ordinals.is_contiguous() and payload.is_contiguous()
                    and ordinals.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and payload.dtype == torch.float32 and payload.numel() == 16 * ordinals.numel()):
                raise ValueError("refit: ordinals (int32) and payload (float32, n x 16) must both be contiguous tensors on the device")
            torch.cuda.synchronize(ordinals.device)   # (the handle's stream is its own: what wrote the tensors must be complete)
            n = ordinals.numel()
            rc = R.gpuart_refit_run(h, C.byref(scene), C.c_void_p(ordinals.data_ptr() if n else None),
                                    C.c_void_p(payload.data_ptr() if n else None), C.c_size_t(n), C.byref(res))
        else:
            o = np.ascontiguousarray(ordinals, np.uint32).reshape(-1)
            p = np.ascontiguousarray(payload, np.float32).reshape(-1)
            if p.size != 16 * o.size:
                raise ValueError("refit: payload must hold 16 floats per ordinal")
            rc = R.gpuart_refit_run_host(h, C.byref(scene), _p(o), _p(p), C.c_size_t(o.size), C.byref(res))
        h._chk(rc, res)
        self.scene_refitted(res.root_min[:], res.root_max[:], res.subnormal)
        levels = C.c_uint32()
        h._chk(R.gpuart_refit_levels(h, C.byref(levels)))
        return dict(root_min=np.array(res.root_min[:], np.float32), root_max=np.array(res.root_max[:], np.float32), subnormal=bool(res.subnormal),
                    levels=int(levels.value))

    # a rebuild on the device (include/gpuart_build.h)
    def scene_reserve(self, n_recs):
        """gpuart_hip_scene_reserve: the context's spare arrays, with room for n_recs records, as a HipScene."""
        s = HipScene()
        self._chk(self.L.gpuart_hip_scene_reserve(self.ctx, C.c_uint64(n_recs), C.byref(s)))
        return s

    def scene_rebuilt(self, built):
        self._chk(self.L.gpuart_hip_scene_rebuilt(self.ctx, C.byref(built)))

    def _build_handle(self):
        if getattr(self, "_build", None) is None:
            self._build = _BuildHandle(self.device)
        return self._build

    def _builder(self, clustered):
        """(handle, an empty result, run, run_host, step_ms, the steps' names) of the clustered or the Morton build."""
        if clustered:
            if getattr(self, "_ploc", None) is None:
                self._ploc = _PlocHandle(self.device)
            Bd = ploc_lib()
            return self._ploc, PlocResult(), Bd.gpuart_ploc_run, Bd.gpuart_ploc_run_host, Bd.gpuart_ploc_step_ms, PLOC_STEPS
        Bd = build_lib()
        return self._build_handle(), BuildResult(), Bd.gpuart_build_run, Bd.gpuart_build_run_host, Bd.gpuart_build_step_ms, BUILD_STEPS

    def _build_report(self, h, res, step_ms, steps, clustered):
        ms = (C.c_double * len(steps))()
        h._chk(step_ms(h, ms))
        report = dict(n_recs=int(res.n_recs), root_ref=int(res.root_ref), max_depth=int(res.max_depth), subnormal=bool(res.subnormal),
                      root_min=np.array(res.root_min[:], np.float32), root_max=np.array(res.root_max[:], np.float32),
                      step_ms=dict(zip(steps, [float(v) for v in ms])))
        if clustered:
            report["iterations"] = int(res.iterations)
        else:
            report["levels"] = int(res.levels)
        return report

    def _fill_spare(self, spare, res):
        """What a build reported (BuildResult or PlocResult), into the descriptor of the spare set it built into."""
        spare.n_recs, spare.root_ref, spare.max_depth = res.n_recs, res.root_ref, res.max_depth
        spare.root_min, spare.root_max = res.root_min, res.root_max
        spare.box_slack = float("inf") if res.subnormal else 0.0

    def _out_tensor(self, out, n, fn, count):
        """rebuild's `out` rule: the contiguous int32 tensor of n entries on the device that receives the result — `out` itself (else
        ValueError in `fn`'s name), a new one for True, and for None when the process has imported torch — or None: the result is a NumPy array."""
        if out is None:
            out = "torch" in sys.modules
        if out is False:
            return None
        import torch
        t = torch.empty((n,), dtype=torch.int32, device="cuda:%d" % self.device) if out is True else out
        if not (hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() and t.dtype == torch.int32 and t.numel() == n):
            raise ValueError("%s: out must be a contiguous int32 tensor of %s entries on the device" % (fn, count))
        return t

    def rebuild(self, out=None, mode="morton"):
        """Rebuilds the uploaded scene's tree on the device and has the context adopt it — `mode` "morton": in Morton order
        (include/gpuart_build.h), fast to build; "clustered": by locally-ordered clustering (include/gpuart_ploc.h), a tree of lower cost
        for more launches; `last_rebuild` then holds iterations in place of levels, and gpuart_ploc_step_ms's steps. The
        primitives are renumbered, new device ordinal p is the old new_to_old[p]. Returns new_to_old: when torch is in use (the process
        has imported it) an int32 tensor on this device, and nothing crosses the host; else a NumPy uint32 array. `out` overrides that:
        a contiguous int32 torch tensor of n_prims entries on this device is written in place and returned, True makes one, False asks
        for the NumPy array. What the build reported is kept in `last_rebuild`: dict(n_recs, root_ref, max_depth, subnormal, levels,
        root_min, root_max, step_ms). A refusal raises HipError with code -1 (ERR_ARG) and nothing changed. Passes requested before
        the call render the old tree."""
        if mode not in TREE_MODES:
            raise ValueError("rebuild: mode must be one of %s" % sorted(TREE_MODES))
        clustered = mode == "clustered"
        h, res, run, run_host, step_ms, steps = self._builder(clustered)
        scene = self.scene_device()
        n = int(scene.n_prims)
        spare = self.scene_reserve((n - 1 if clustered else (n + 1) // 2 - 1) if n else 0)
        perm = self._out_tensor(out, n, "rebuild", "n_prims")
        if perm is None:
            perm = np.zeros(n, np.uint32)
            rc = run_host(h, C.byref(scene), C.byref(spare), _p(perm), C.byref(res))
        else:
            import torch
            torch.cuda.synchronize(perm.device)
            rc = run(h, C.byref(scene), C.byref(spare), C.c_void_p(perm.data_ptr()), C.byref(res))
        h._chk(rc)
        self._fill_spare(spare, res)
        self.scene_rebuilt(spare)
        self.last_rebuild = self._build_report(h, res, step_ms, steps, clustered)
        return perm

    # an edit on the device (include/gpuart_edit.h)
    def scene_reserve_prims(self, n_recs, n_prims):
        """gpuart_hip_scene_reserve_prims: the context's spare arrays, with room for n_recs records and n_prims primitives, as a HipScene."""
        s = HipScene()
        self._chk(self.L.gpuart_hip_scene_reserve_prims(self.ctx, C.c_uint64(n_recs), C.c_uint64(n_prims), C.byref(s)))
        return s

    def scene_replaced(self, built, type_mask):
        self._chk(self.L.gpuart_hip_scene_replaced(self.ctx, C.byref(built), C.c_uint32(type_mask)))

    def _edit_handle(self):
        if getattr(self, "_edit", None) is None:
            self._edit = _EditHandle(self.device)
        return self._edit

    def edit(self, remove, add_types, add_payload, mode="clustered", out=None):
        """Removes the primitives `remove` (strictly ascending device ordinals) from the uploaded scene, appends primitives of the types
        `add_types` (0..3) with the data quads `add_payload` (n x 16 floats, zero-padded as for refit), builds the tree of the result on
        the device — `mode` as for rebuild — and has the context adopt it (include/gpuart_edit.h). The three arguments are contiguous
        tensors on this device (int32, int32, float32: nothing crosses the host) or anything NumPy converts. Returns the composed map,
        int32: per new device ordinal the old ordinal of a survivor, or n_old + k for the k-th addition — under rebuild's `out` rules (a
        tensor on the device when torch is in use, else a NumPy array; a tensor of n_new entries is written in place; True / False
        choose). `last_edit` keeps dict(n_prims, type_mask, root_min, root_max, step_ms, rebuild: what last_rebuild would hold). A
        refusal raises HipError with code -1 (ERR_ARG), `first_bad` where a removal (index i) or an addition (n_remove + k) is at
        fault, and nothing changed."""
        if mode not in TREE_MODES:
            raise ValueError("edit: mode must be one of %s" % sorted(TREE_MODES))
        clustered = mode == "clustered"
        E, h = edit_lib(), self._edit_handle()
        scene = self.scene_device()
        n_old = int(scene.n_prims)
        edited, res = HipScene(), EditResult()
        on_device = hasattr(remove, "data_ptr")
        if on_device:
            import torch
            ok = all(hasattr(t, "data_ptr") and t.is_cuda and t.is_contiguous() for t in (remove, add_types, add_payload))
            if not (ok and remove.dtype == torch.int32 and add_types.dtype == torch.int32 and add_payload.dtype == torch.float32 and
                    add_payload.numel() == 16 * add_types.numel()):
                raise ValueError("edit: remove (int32), add_types (int32) and add_payload (float32, n x 16) must all be contiguous tensors on the device")
            n_remove, n_add = remove.numel(), add_types.numel()
            n_new = n_old - n_remove + n_add
            source = torch.empty((max(n_new, 1),), dtype=torch.int32, device="cuda:%d" % self.device)
            torch.cuda.synchronize(source.device)   # (the handle's stream is its own: what wrote the tensors must be complete)
            ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)
            rc = E.gpuart_edit_run(h, C.byref(scene), ptr(remove), C.c_size_t(n_remove), ptr(add_types), ptr(add_payload), C.c_size_t(n_add),
                                   C.c_void_p(source.data_ptr()), C.byref(edited), C.byref(res))
        else:
            r = np.ascontiguousarray(remove, np.uint32).reshape(-1)
            t = np.ascontiguousarray(add_types, np.uint32).reshape(-1)
            p = np.ascontiguousarray(add_payload, np.float32).reshape(-1)
            if p.size != 16 * t.size:
                raise ValueError("edit: add_payload must hold 16 floats per added primitive")
            n_remove, n_add = r.size, t.size
            n_new = n_old - n_remove + n_add
            source = np.zeros(max(n_new, 1), np.int32)
            rc = E.gpuart_edit_run_host(h, C.byref(scene), _p(r), C.c_size_t(n_remove), _p(t), _p(p), C.c_size_t(n_add), _p(source), C.byref(edited),
                                        C.byref(res))
        h._chk(rc, res)
        bh, bres, run, run_host, step_ms, steps = self._builder(clustered)
        spare = self.scene_reserve_prims(n_new - 1 if clustered else (n_new + 1) // 2 - 1, n_new)
        if on_device:
            perm = torch.empty((n_new,), dtype=torch.int32, device=source.device)
            torch.cuda.synchronize(source.device)
            bh._chk(run(bh, C.byref(edited), C.byref(spare), C.c_void_p(perm.data_ptr()), C.byref(bres)))
            composed = self._out_tensor(True if out is False else out, n_new, "edit", "n_new")   # (False: a tensor first, copied to the host below)
            torch.cuda.synchronize(source.device)
            h._chk(E.gpuart_edit_compose(h, C.c_void_p(source.data_ptr()), C.c_void_p(perm.data_ptr()), C.c_size_t(n_new), C.c_void_p(composed.data_ptr())))
            if out is False:
                composed = composed.cpu().numpy()
        else:
            perm = np.zeros(n_new, np.uint32)
            bh._chk(run_host(bh, C.byref(edited), C.byref(spare), _p(perm), C.byref(bres)))
            composed = source[:n_new][perm]
            target = self._out_tensor(out, n_new, "edit", "n_new")
            if target is not None:
                import torch
                target.copy_(torch.from_numpy(composed))
                torch.cuda.synchronize(target.device)
                composed = target
        spare.n_prims = n_new
        self._fill_spare(spare, bres)
        self.scene_replaced(spare, int(res.type_mask))
        ms = (C.c_double * len(EDIT_STEPS))()
        h._chk(E.gpuart_edit_step_ms(h, ms))
        self.last_rebuild = self._build_report(bh, bres, step_ms, steps, clustered)
        self.last_edit = dict(n_prims=int(res.n_prims), type_mask=int(res.type_mask), root_min=np.array(res.root_min[:], np.float32),
                              root_max=np.array(res.root_max[:], np.float32), step_ms=dict(zip(EDIT_STEPS, [float(v) for v in ms])),
                              rebuild=self.last_rebuild)
        return composed

    def tree_cost(self):
        """gpuart_build_cost of the uploaded scene's tree: the sum over its records of both children's half-areas over the root's."""
        cost = C.c_double()
        scene = self.scene_device()
        h = self._build_handle()
        h._chk(build_lib().gpuart_build_cost(h, C.byref(scene), C.byref(cost)))
        return float(cost.value)

    # rendering
    def render_direct(self, params):
        self._chk(self.L.gpuart_hip_render_direct(self.ctx, C.byref(params)))

    def pt_reset(self):
        self._chk(self.L.gpuart_hip_pt_reset(self.ctx))

    def pt_plan(self, passes):
        self._chk(self.L.gpuart_hip_pt_plan(self.ctx, C.c_uint32(passes)))

    def flush(self):
        self._chk(self.L.gpuart_hip_flush(self.ctx))

    def pt_pass(self, params, rand_seed, npaths):
        rs = (C.c_float * 4)(*[float(x) for x in rand_seed])
        self._chk(self.L.gpuart_hip_pt_pass(self.ctx, C.byref(params), rs, C.c_int(npaths)))

    def read(self, which, divide_by=1.0):
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        self._chk(self.L.gpuart_hip_read(self.ctx, C.c_int(which), _p(out), C.c_float(divide_by)))
        return out

    def write(self, which, rgba):
        rgba = np.ascontiguousarray(rgba, np.float32)
        self._chk(self.L.gpuart_hip_write(self.ctx, C.c_int(which), _p(rgba)))

    def export(self, which, device_ptr, divide_by=1.0):
        self._chk(self.L.gpuart_hip_export(self.ctx, C.c_int(which), C.c_void_p(device_ptr), C.c_float(divide_by)))

    def n_blocks(self):
        """8x8 blocks of the tile, row-major: what an active list indexes and the block counts have one word for."""
        _, _, tw, th = self.tile
        return ((tw + 7) // 8) * ((th + 7) // 8)

    def set_active_blocks(self, blocks):
        """The blocks the passes to come render (gpuart_hip_set_active_blocks): a strictly ascending sequence of block indices, possibly
        empty; None: every block again."""
        if blocks is None:
            self._chk(self.L.gpuart_hip_set_active_blocks(self.ctx, None, C.c_size_t(0)))
            return
        b = np.ascontiguousarray(blocks, np.uint32).reshape(-1)
        keep = b if b.size else np.zeros(1, np.uint32)   # (an empty list is a non-NULL pointer with n = 0)
        self._chk(self.L.gpuart_hip_set_active_blocks(self.ctx, keep.ctypes.data_as(C.c_void_p), C.c_size_t(b.size)))

    def block_paths(self, device_ptr=None):
        """Paths per pixel accumulated into each block since the last pt_reset: a uint32 array (gpuart_hip_read_block_paths), or, given a
        device pointer, exported there on the context's stream (gpuart_hip_export_block_paths; finish() before use)."""
        if device_ptr is not None:
            self._chk(self.L.gpuart_hip_export_block_paths(self.ctx, C.c_void_p(device_ptr)))
            return None
        out = np.empty(self.n_blocks(), np.uint32)
        self._chk(self.L.gpuart_hip_read_block_paths(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out

    def set_share(self, g):
        self._chk(self.L.gpuart_hip_set_share(self.ctx, C.byref(g)))
        self.tile = (g.x0, g.y0, g.tw, g.th)

    def get_share(self):
        g = TileGeom()
        self._chk(self.L.gpuart_hip_get_share(self.ctx, C.byref(g)))
        return g

    def comm_init(self, nranks, rank, unique_id):
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        self._chk(self.L.gpuart_hip_comm_init(self.ctx, nranks, rank, buf))

    def comm_destroy(self):
        self._chk(self.L.gpuart_hip_comm_destroy(self.ctx))

    def gather(self, which, divide_by, root, full_frame_device_ptr):
        """Collective: assembles every rank's share on `root` (full_frame_device_ptr: W*H*4 floats on the root, else 0)."""
        self._chk(self.L.gpuart_hip_gather(self.ctx, which, C.c_float(divide_by), root, C.c_void_p(full_frame_device_ptr or None)))

    def comm_info(self):
        """(ranks, own rank) as the communicator itself reports them (ncclCommCount, ncclCommUserRank)."""
        n, me = C.c_int(0), C.c_int(0)
        self._chk(self.L.gpuart_hip_comm_info(self.ctx, C.byref(n), C.byref(me)))
        return n.value, me.value

    def finish(self):
        self._chk(self.L.gpuart_hip_finish(self.ctx))

    def wait(self, timeout_ms):
        """finish() with a bound: HipError with code ERR_TIMEOUT if the context's work is not complete after timeout_ms."""
        self._chk(self.L.gpuart_hip_wait(self.ctx, C.c_uint32(int(timeout_ms))))

    def test_tile_order(self, order):
        """Birth order of the paths of a pass: a permutation of the tile's 8x8 pixel blocks (None: row-major)."""
        if order is None:
            self._chk(self.L.gpuart_hip_test_tile_order(self.ctx, None, C.c_size_t(0)))
            return
        o = np.ascontiguousarray(order, np.uint32)
        self._chk(self.L.gpuart_hip_test_tile_order(self.ctx, o.ctypes.data_as(C.c_void_p), C.c_size_t(o.size)))

    def test_current_tile_order(self):
        """The birth order in use (None: row-major)."""
        g = self.get_share()
        out = np.empty(((g.tw + 7) // 8) * ((g.th + 7) // 8), np.uint32)
        rc = self.L.gpuart_hip_test_current_tile_order(self.ctx, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size))
        if rc < 0:
            self._chk(rc)
        return out if rc == 1 else None

    def test_sort_tiles(self, cost):
        """k_tile_order alone: per-block cost -> birth order (most expensive class first, row-major within a class)."""
        cst = np.ascontiguousarray(cost, np.uint32)
        out = np.empty(cst.size, np.uint32)
        self._chk(self.L.gpuart_hip_test_sort_tiles(self.ctx, cst.ctypes.data_as(C.c_void_p), C.c_size_t(cst.size), out.ctypes.data_as(C.c_void_p)))
        return out

    def test_stall(self, ms):
        """Keeps the context's primary stream busy for `ms` milliseconds (what a missing peer looks like to the bounded waits)."""
        self._chk(self.L.gpuart_hip_test_stall(self.ctx, C.c_uint32(int(ms))))

    def launched(self, reset=True):
        """Test build only: the set of product kernels launched on this context since the ledger was last reset (gpuart_hip_test_launches),
        by their code-object symbols (mangled, without ".kd"); reset=True empties the ledger."""
        n = C.c_size_t(0)
        self._chk(self.L.gpuart_hip_test_launches(self.ctx, None, C.c_size_t(0), C.byref(n), C.c_int(0)))
        buf = C.create_string_buffer(n.value + 1)
        self._chk(self.L.gpuart_hip_test_launches(self.ctx, buf, C.c_size_t(n.value + 1), C.byref(n), C.c_int(1 if reset else 0)))
        names = set(buf.value.decode().split())
        if any(x.startswith("@") for x in names):  # the runtime could not name a kernel: its host handle's symbol in this library
            syms = _library_symbols(self.L._name)
            names = {syms.get(int(x[1:], 16), x) if x.startswith("@") else x for x in names}
        return names

    MODE_WAVEFRONT, MODE_REFERENCE_WORK, MODE_MEGAKERNEL = 0, 1, 2

    def set_mode(self, mode):
        """0 wavefront (fast, default), 1 reference-work (exact counters), 2 megakernel."""
        self._chk(self.L.gpuart_hip_set_mode(self.ctx, C.c_int(int(mode))))

    def set_timing(self, level):
        self._chk(self.L.gpuart_hip_set_timing(self.ctx, C.c_int(int(level))))

    def counters(self, reset=False):
        c = Counters()
        self._chk(self.L.gpuart_hip_counters(self.ctx, C.byref(c), C.c_int(1 if reset else 0)))
        return c

    def kernel_time(self, cls=0, reset=False):
        """(total ms, count) of HIP-event-timed intervals: cls 0 = render calls, 1 = BVH-query kernels."""
        ms = C.c_double(0)
        n = C.c_uint64(0)
        self._chk(self.L.gpuart_hip_kernel_time(self.ctx, C.c_int(cls), C.byref(ms), C.byref(n), C.c_int(1 if reset else 0)))
        return ms.value, n.value

    def scene_info(self):
        nodes, prims, bytes_ = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        depth = C.c_uint32(0)
        self._chk(self.L.gpuart_hip_scene_info(self.ctx, C.byref(nodes), C.byref(prims), C.byref(depth), C.byref(bytes_)))
        return dict(nodes=nodes.value, prims=prims.value, max_depth=depth.value, device_bytes=bytes_.value)

    def set_nearest_first(self, min_prims):
        """gpuart_hip_set_nearest_first: trees of at least min_prims primitives are walked nearer child first (opt-in; 0xffffffff: never)."""
        self._chk(self.L.gpuart_hip_set_nearest_first(self.ctx, C.c_uint32(int(min_prims))))

    def scene_order(self):
        """0: nearer child first (certified); 1: the reference's order (small tree); 2: the reference's order, exact box tests."""
        o = C.c_int(-1)
        self._chk(self.L.gpuart_hip_scene_order(self.ctx, C.byref(o)))
        return o.value

    # batched ray queries (include/gpuart_hip.h gpuart_hip_trace_rays / _trace_rays_host / _pick)
    def trace_rays(self, rays, occlusion=False, user_sphere=None, want_prims=False, out=None, prims_out=None):
        """Closest hit (or, occlusion=True, "is 0 < closest-hit pos < tmax?") of rays (n, 8) = origin.xyz, tmax, dir.xyz, unused, as the
        reference answers it; user_sphere = (x, y, z, r) takes part, None = no user sphere.
        A NumPy array runs through host memory (synchronous) and returns a RAY_HIT record array. A torch tensor on this context's device
        runs in place, without a copy: torch's current stream is synchronised before, and the context (gpuart_hip_finish, which also
        launches collected passes) before returning; hits is an (n, 8) float32 tensor (column 7 holds the int32 type: .view(torch.int32)),
        written into `out` if given. With want_prims, also the primitive ordinals (int32; -1 none, -2 the user sphere)."""
        flags = C.c_uint32(RAYS_OCCLUSION if occlusion else 0)
        us = _user_sphere(user_sphere)
        if type(rays).__module__.startswith("torch"):
            import torch
            if rays.dtype != torch.float32 or rays.dim() != 2 or rays.shape[1] != 8 or not rays.is_contiguous() or rays.device.type != "cuda":
                raise ValueError("rays must be a contiguous (n, 8) float32 tensor on the GPU")
            n = rays.shape[0]
            hits = out if out is not None else torch.empty((n, 8), dtype=torch.float32, device=rays.device)
            if hits.dtype != torch.float32 or tuple(hits.shape) != (n, 8) or not hits.is_contiguous() or hits.device != rays.device:
                raise ValueError("out must be a contiguous (n, 8) float32 tensor on the rays' device")
            prims = None
            if want_prims:
                prims = prims_out if prims_out is not None else torch.empty((n,), dtype=torch.int32, device=rays.device)
                if prims.dtype != torch.int32 or tuple(prims.shape) != (n,) or not prims.is_contiguous() or prims.device != rays.device:
                    raise ValueError("prims_out must be a contiguous (n,) int32 tensor on the rays' device")
            torch.cuda.current_stream(rays.device).synchronize()
            self._chk(self.L.gpuart_hip_trace_rays(self.ctx, C.c_void_p(rays.data_ptr()), C.c_size_t(n), flags, us,
                                                   C.c_void_p(hits.data_ptr()), C.c_void_p(prims.data_ptr() if prims is not None else 0)))
            self.finish()
            return (hits, prims) if want_prims else hits
        rays = _rays_array(rays)
        n = rays.shape[0]
        hits = np.zeros(n, RAY_HIT)
        prims = np.zeros(n, np.int32) if want_prims else None
        self._chk(self.L.gpuart_hip_trace_rays_host(self.ctx, _p(rays), C.c_size_t(n), flags, us, _p(hits),
                                                    _p(prims) if prims is not None else None))
        return (hits, prims) if want_prims else hits

    def _nearest_handle(self, scene):
        """The context's gpuart_nearest, made at the first closest_points and bound to `scene` unless it is already (its generation: an
        upload, a rebuild and an edit raise it, a refit in place keeps it and the nesting the binding checked)."""
        if getattr(self, "_nearest", None) is None:
            self._nearest = _NearestHandle(self.device)
        h = self._nearest
        if h.generation != scene.generation:
            h.generation = None
            h._chk(h.L.gpuart_nearest_bind(h, C.byref(scene)))
            h.generation = scene.generation
        return h

    def closest_points(self, points, user_sphere=None, out=None):
        """Per query (p.xyz, r) of points (n, 4) the nearest surface point among the scene's primitives within r, as
        include/gpuart_nearest.h defines it; user_sphere = (x, y, z, R) takes part with ordinal -2, None = no user sphere.
        A NumPy array runs through host memory (synchronous) and returns a NEAREST_HIT record array. A contiguous (n, 4) float32 tensor
        on this context's device runs in place, without a copy: torch's current stream is synchronised before, the handle's stream
        before returning; the result is an (n, 8) float32 tensor — dist, q.xyz, d2, prim, type, 0; columns 5 and 6 hold int32:
        .view(torch.int32) — written into `out` if given. The scene's descriptor is fetched at every call, as Backend.refit does.
        A scene the uploader classified irregular or disorderly, and an empty one, raise HipError (code -1) with nothing written."""
        N = nearest_lib()
        us = _user_sphere(user_sphere)
        scene = self.scene_device()
        h = self._nearest_handle(scene)
        if type(points).__module__.startswith("torch"):
            import torch
            n = self._device_queries("points", points, 4)
            hits = out if out is not None else torch.empty((n, 8), dtype=torch.float32, device=points.device)
            if hits.dtype != torch.float32 or tuple(hits.shape) != (n, 8) or not hits.is_contiguous() or hits.device != points.device:
                raise ValueError("out must be a contiguous (n, 8) float32 tensor on the points' device")
            torch.cuda.current_stream(points.device).synchronize()
            h._chk(N.gpuart_nearest_run(h, C.byref(scene), C.c_void_p(points.data_ptr() if n else None), C.c_size_t(n), us,
                                        C.c_void_p(hits.data_ptr() if n else None)))
            h.finish()
            return hits
        points = _points_array(points)
        hits = np.zeros(points.shape[0], NEAREST_HIT)
        h._chk(N.gpuart_nearest_run_host(h, C.byref(scene), _p(points), C.c_size_t(points.shape[0]), us, _p(hits)))
        return hits

    def nearest_k(self, points, k, user_sphere=None, out=None):
        """Per query (p.xyz, r) of points (n, 4) the k nearest primitives within r (1 <= k <= NEAREST_KNN_MAX), as include/gpuart_nearest.h
        "k nearest" defines them: row i holds query i's candidates in ascending distance — equal distances by ordinal, the user sphere
        (ordinal -2) last —, each the record `within` lists for that primitive, and misses (prim -1) behind the last one found. A NumPy
        array runs through host memory (synchronous) and returns an (n, k) NEAREST_HIT array. A contiguous (n, 4) float32 tensor on this
        context's device runs in place and returns an (n, k, 8) float32 tensor, written into `out` if given; streams, checks and refusals
        as closest_points. k = 1 gives closest_points' records."""
        N = nearest_lib()
        us = _user_sphere(user_sphere)
        k = int(k)
        if not 1 <= k <= NEAREST_KNN_MAX:
            raise ValueError("k must be in 1 .. %d" % NEAREST_KNN_MAX)
        scene = self.scene_device()
        h = self._nearest_handle(scene)
        if type(points).__module__.startswith("torch"):
            import torch
            n = self._device_queries("points", points, 4)
            hits = out if out is not None else torch.empty((n, k, 8), dtype=torch.float32, device=points.device)
            if hits.dtype != torch.float32 or tuple(hits.shape) != (n, k, 8) or not hits.is_contiguous() or hits.device != points.device:
                raise ValueError("out must be a contiguous (n, k, 8) float32 tensor on the points' device")
            torch.cuda.current_stream(points.device).synchronize()
            h._chk(N.gpuart_nearest_knn_run(h, C.byref(scene), C.c_void_p(points.data_ptr() if n else None), C.c_size_t(n), C.c_size_t(k), us,
                                            C.c_void_p(hits.data_ptr() if n else None)))
            h.finish()
            return hits
        if out is not None:
            raise ValueError("out goes with device tensors")
        points = _points_array(points)
        hits = np.zeros((points.shape[0], k), NEAREST_HIT)
        h._chk(N.gpuart_nearest_knn_run_host(h, C.byref(scene), _p(points), C.c_size_t(points.shape[0]), C.c_size_t(k), us, _p(hits)))
        return hits

    def within(self, points, user_sphere=None, max_items=1 << 27, out=None):
        """Per query (p.xyz, r) of points (n, 4) the list of every primitive within r, as include/gpuart_nearest.h "Neighbour lists" defines
        it, in CSR form: (offsets, items), list i = items[offsets[i]:offsets[i + 1]] in the tree's order (the user sphere, ordinal -2,
        first). A NumPy array runs through host memory (synchronous) and returns (offsets uint32 (n + 1,), items NEAREST_HIT (total,)).
        A contiguous (n, 4) float32 tensor on this context's device runs in place: the count, one 8-byte read-back of the total, the
        fill; it returns (offsets int32 tensor (n + 1,), items float32 tensor (total, 8)), written into out = (offsets, items) if given
        (an items tensor with more rows than the total is returned whole, rows from the total on untouched). A total above max_items,
        and an `out` items tensor below the total, raise ValueError naming the total before anything is allocated or filled. Refusals
        as closest_points."""
        N = nearest_lib()
        us = _user_sphere(user_sphere)
        max_items = int(max_items)
        if max_items < 0:
            raise ValueError("max_items is negative")
        scene = self.scene_device()
        h = self._nearest_handle(scene)
        if type(points).__module__.startswith("torch"):
            import torch
            n = self._device_queries("points", points, 4)
            ptr = C.c_void_p(points.data_ptr())
            return self._lists_device(N.gpuart_nearest_within_total, h, n, max_items, out, points.device, "the points' device", (8,), torch.float32,
                                      lambda o: N.gpuart_nearest_within_count(h, C.byref(scene), ptr, C.c_size_t(n), us, o),
                                      lambda o, it, cap: N.gpuart_nearest_within_fill(h, C.byref(scene), ptr, C.c_size_t(n), us, o, it, cap))
        if out is not None:
            raise ValueError("out goes with device tensors")
        points = _points_array(points)
        args = (h, C.byref(scene), _p(points), C.c_size_t(points.shape[0]), us)
        return self._lists_host(h, points.shape[0], max_items, NEAREST_HIT,
                                lambda o, total: N.gpuart_nearest_within_host(*args, o, None, C.c_size_t(0), total),
                                lambda o, it, cap, total: N.gpuart_nearest_within_fill_host(*args, o, it, cap))

    def _device_queries(self, name, t, columns):
        """The queries of a device route: `t` is a contiguous (n, columns) float32 tensor on this context's device, or ValueError; n."""
        import torch
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != columns or not t.is_contiguous() or t.device.type != "cuda":
            raise ValueError("%s must be a contiguous (n, %d) float32 tensor on the GPU" % (name, columns))
        index = t.device.index if t.device.index is not None else torch.cuda.current_device()
        if index != self.device:
            raise ValueError("%s is on cuda:%d, this context on device %d: the kernel reads the tensor's memory in place" % (name, index, self.device))
        return t.shape[0]

    def _lists_device(self, total_of, h, n, max_items, out, device, where, trailing, dtype, count, fill):
        """The device route of within, overlaps and overlapping_pairs: count(offsets_ptr), the 8-byte total through the entry `total_of`,
        fill(offsets_ptr, items_ptr, capacity). offsets: int32 (n + 1,); items: `dtype` (total, *trailing) — float32 records of 8 words,
        or int32 ordinals —, both on `device`, which the messages call `where`; out = (offsets, items) or None."""
        import torch
        total = C.c_uint64(0)
        offsets, items = out if out is not None else (None, None)
        if offsets is None:
            offsets = torch.zeros((n + 1,), dtype=torch.int32, device=device)
        if offsets.dtype != torch.int32 or tuple(offsets.shape) != (n + 1,) or not offsets.is_contiguous() or offsets.device != device:
            raise ValueError("out[0] must be a contiguous (n + 1,) int32 tensor on " + where)
        if items is not None and (items.dtype != dtype or items.dim() != 1 + len(trailing) or tuple(items.shape[1:]) != trailing or not items.is_contiguous() or
                                  items.device != device):
            raise ValueError("out[1] must be a contiguous (capacity%s) %s tensor on %s" % ("".join(", %d" % d for d in trailing) or ",", str(dtype).split(".")[-1], where))
        torch.cuda.current_stream(device).synchronize()
        if n == 0:
            offsets.zero_()
            return offsets, items if items is not None else torch.empty((0, *trailing), dtype=dtype, device=device)
        h._chk(count(C.c_void_p(offsets.data_ptr())))
        rc = total_of(h, C.byref(total))
        if total.value > max_items:
            raise ValueError("the lists hold %d items, more than max_items = %d" % (total.value, max_items))
        h._chk(rc)
        if items is None:
            items = torch.empty((total.value, *trailing), dtype=dtype, device=device)
        elif items.shape[0] < total.value:
            raise ValueError("out[1] has room for %d items, the lists hold %d" % (items.shape[0], total.value))
        cap = items.shape[0]
        h._chk(fill(C.c_void_p(offsets.data_ptr()), C.c_void_p(items.data_ptr() if cap else None), C.c_size_t(cap)))
        h.finish()
        return offsets, items

    @staticmethod
    def _lists_host(h, n, max_items, item_dtype, count, fill):
        """The host route of the same three: count(offsets_p, total_ref) with no items, a total above max_items refused, the items
        allocated, fill(offsets_p, items_p, capacity, total_ref) unless there are none: (offsets uint32 (n + 1,), items)."""
        offsets = np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        rc = count(_p(offsets), C.byref(total))
        if total.value > max_items:
            raise ValueError("the lists hold %d items, more than max_items = %d" % (total.value, max_items))
        h._chk(rc)
        items = np.zeros(total.value, item_dtype)
        if total.value:     # (the fill alone where the library has one: the offsets are the count's of a moment ago)
            h._chk(fill(_p(offsets), _p(items), C.c_size_t(total.value), C.byref(total)))
        return offsets, items

    @staticmethod
    def _margin(margin):
        margin = float(np.float32(margin))
        if not (0.0 <= margin < float("inf")):
            raise ValueError("margin must be finite and not negative")
        return margin

    def overlaps(self, boxes, margin=0.0, user_sphere=None, max_items=1 << 27, out=None):
        """Per query box (lo.xyz, hi.xyz) of boxes (n, 6), inflated by `margin` on every side, the ordinals of every primitive whose own box
        meets it, as include/gpuart_nearest.h "Box overlap" defines them, in CSR form: (offsets, items), list i =
        items[offsets[i]:offsets[i + 1]] in the tree's order (the user sphere, ordinal -2, first). A NumPy array runs through host memory
        (synchronous) and returns (offsets uint32 (n + 1,), items int32 (total,)). A contiguous (n, 6) float32 tensor on this context's
        device runs in place and returns int32 tensors, written into out = (offsets, items) if given; streams, max_items and refusals as
        `within`. A margin that is NaN, infinite or negative raises ValueError."""
        N = nearest_lib()
        us = _user_sphere(user_sphere)
        margin = self._margin(margin)
        max_items = int(max_items)
        if max_items < 0:
            raise ValueError("max_items is negative")
        scene = self.scene_device()
        h = self._nearest_handle(scene)
        m = C.c_float(margin)
        if type(boxes).__module__.startswith("torch"):
            import torch
            n = self._device_queries("boxes", boxes, 6)
            ptr = C.c_void_p(boxes.data_ptr() if n else None)
            return self._lists_device(N.gpuart_nearest_overlap_total, h, n, max_items, out, boxes.device, "the context's device", (), torch.int32,
                                      lambda o: N.gpuart_nearest_overlap_count(h, C.byref(scene), ptr, C.c_size_t(n), m, us, o),
                                      lambda o, it, cap: N.gpuart_nearest_overlap_fill(h, C.byref(scene), ptr, C.c_size_t(n), m, us, o, it, cap))
        if out is not None:
            raise ValueError("out goes with device tensors")
        boxes = np.ascontiguousarray(boxes, np.float32)
        if boxes.ndim != 2 or boxes.shape[1] != 6:
            raise ValueError("boxes must be (n, 6): lo.xyz, hi.xyz")
        args = (h, C.byref(scene), _p(boxes), C.c_size_t(boxes.shape[0]), m, us)
        return self._lists_host(h, boxes.shape[0], max_items, np.int32,
                                lambda o, total: N.gpuart_nearest_overlap_host(*args, o, None, C.c_size_t(0), total),
                                lambda o, it, cap, total: N.gpuart_nearest_overlap_fill_host(*args, o, it, cap))

    def overlapping_pairs(self, margin=0.0, max_items=1 << 27, device=False, out=None, as_pairs=False):
        """The overlapping pairs of the scene's own primitives (include/gpuart_nearest.h "Box overlap", pairs): list i holds the ordinals
        j > i whose box meets primitive i's box inflated by `margin`, in the tree's order; nothing is uploaded. Returns (offsets uint32
        (n_prims + 1,), items int32 (total,)) as NumPy arrays, or with device=True int32 tensors on the context's device (written into
        out = (offsets, items) if given; only the 8-byte total crosses the host). as_pairs=True returns instead the (total, 2) int32
        array or tensor of (i, j), i < j, expanded from the CSR. Adjacent triangles of a mesh share vertices and always overlap:
        filtering topological neighbours is the caller's."""
        N = nearest_lib()
        margin = self._margin(margin)
        max_items = int(max_items)
        if max_items < 0:
            raise ValueError("max_items is negative")
        scene = self.scene_device()
        h = self._nearest_handle(scene)
        m = C.c_float(margin)
        n = int(scene.n_prims)
        if device:
            import torch
            dev = torch.device("cuda", self.device)
            offsets, items = self._lists_device(N.gpuart_nearest_overlap_total, h, n, max_items, out, dev, "the context's device", (), torch.int32,
                                                lambda o: N.gpuart_nearest_pairs_count(h, C.byref(scene), m, o),
                                                lambda o, it, cap: N.gpuart_nearest_pairs_fill(h, C.byref(scene), m, o, it, cap))
            if not as_pairs:
                return offsets, items
            total = int(offsets[-1].item())
            i = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev), torch.diff(offsets).to(torch.int64), output_size=total)
            return torch.stack([i, items[:total]], 1)
        if out is not None:
            raise ValueError("out goes with device=True")
        offsets, items = self._lists_host(h, n, max_items, np.int32,
                                          lambda o, total: N.gpuart_nearest_pairs_host(h, C.byref(scene), m, o, None, C.c_size_t(0), total),
                                          lambda o, it, cap, total: N.gpuart_nearest_pairs_host(h, C.byref(scene), m, o, it, cap, total))
        if not as_pairs:
            return offsets, items
        i = np.repeat(np.arange(n, dtype=np.int32), np.diff(offsets.astype(np.int64)))
        return np.stack([i, items], 1).reshape(-1, 2)

    def pick(self, xy, user_sphere=None, want_prims=False):
        """Closest hit of the camera rays of frame pixels xy (n, 2) = (x, y), row 0 = bottom, any pixel of the frame: a RAY_HIT record
        array (and the primitive ordinals)."""
        xy = _pixels_array(xy)
        n = xy.shape[0]
        hits = np.zeros(n, RAY_HIT)
        prims = np.zeros(n, np.int32) if want_prims else None
        self._chk(self.L.gpuart_hip_pick(self.ctx, _p(xy), C.c_size_t(n), _user_sphere(user_sphere), _p(hits),
                                         _p(prims) if prims is not None else None))
        return (hits, prims) if want_prims else hits

    def gbuffer(self, user_sphere=None, out=None, prims_out=None):
        """gpuart_hip_gbuffer: the record and ordinal pick returns for every pixel of the context's tile, in the tile's local order
        (row 0 = bottom) -> (hits, prims). With torch tensors `out` ((th, tw, 8) float32) and `prims_out` ((th, tw) int32) on this
        context's device they are written in place (torch's current stream is synchronised first, the context before returning); the
        returned hits are then that tensor. Otherwise a RAY_HIT record array (th, tw) and an int32 array (th, tw), written into the
        NumPy arrays `out` / `prims_out` when given."""
        _, _, tw, th = self.tile
        return self._gbuffer(tw, th, out, prims_out,
                             lambda hits, prims: self.L.gpuart_hip_gbuffer(self.ctx, _user_sphere(user_sphere), hits, prims))

    def gbuffer_scaled(self, scale, user_sphere=None, out=None, prims_out=None):
        """gpuart_hip_gbuffer_scaled: the G-buffer of the frame `scale` (2..4) times larger in each direction, for the tile scaled alike:
        what gbuffer() returns on a context resized to scale*W x scale*H with the tile (scale*x0, scale*y0, scale*tw, scale*th), bit for
        bit -> (hits, prims) of (scale*th, scale*tw) pixels. `out` and `prims_out` as gbuffer's, at that size."""
        _, _, tw, th = self.tile
        s = int(scale)
        return self._gbuffer(tw * max(s, 0), th * max(s, 0), out, prims_out,
                             lambda hits, prims: self.L.gpuart_hip_gbuffer_scaled(self.ctx, C.c_uint32(s & 0xffffffff), _user_sphere(user_sphere), hits, prims))

    def _gbuffer(self, tw, th, out, prims_out, call):
        """What gbuffer and gbuffer_scaled share: the (th, tw) outputs checked or made, `call(hits, prims)` on their device pointers, the
        wait, and the copy into NumPy arrays where no tensors were given."""
        import torch
        dev = torch.device("cuda", self.device)
        on_device = out is not None and type(out).__module__.startswith("torch")
        if on_device:
            if out.dtype != torch.float32 or tuple(out.shape) != (th, tw, 8) or not out.is_contiguous() or out.device != dev:
                raise ValueError("out must be a contiguous (%d, %d, 8) float32 tensor on %s" % (th, tw, dev))
            hits = out
            prims = prims_out if prims_out is not None else torch.empty((th, tw), dtype=torch.int32, device=dev)
            if prims.dtype != torch.int32 or tuple(prims.shape) != (th, tw) or not prims.is_contiguous() or prims.device != dev:
                raise ValueError("prims_out must be a contiguous (%d, %d) int32 tensor on %s" % (th, tw, dev))
        else:
            hits = torch.empty((th, tw, 8), dtype=torch.float32, device=dev)
            prims = torch.empty((th, tw), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(call(C.c_void_p(hits.data_ptr()), C.c_void_p(prims.data_ptr())))
        self.finish()
        if on_device:
            return hits, prims
        h = np.ascontiguousarray(hits.cpu().numpy()).view(RAY_HIT).reshape(th, tw)
        p = prims.cpu().numpy()
        if out is not None:
            out.reshape(-1).view(np.uint8)[:] = h.reshape(-1).view(np.uint8)
            h = out
        if prims_out is not None:
            prims_out[...] = p
            p = prims_out
        return h, p

    def trace_subpixel(self, pixels, uv, pixel_size, user_sphere=None, want_prims=True, out=None, prims_out=None):
        """gpuart_hip_trace_subpixel: the closest hits of the sub-pixel camera rays of listed tile pixels. pixels: a contiguous (n,) int32
        tensor on this context's device holding local pixel indices ly * tw + lx (the bits of uint32 indices; any order, repeats
        allowed); uv: (n_sub, 2) values in [0, 1), (rand1, rand2) of sub-sample k; pixel_size: gpuart_params.pixelSize. -> hits, an
        (n_sub, n, 8) float32 tensor (column 7 holds the int32 type), and with want_prims the (n_sub, n) int32 ordinals (-1 none, -2 the
        user sphere), written into `out` / `prims_out` if given. torch's current stream is synchronised before, and the context
        (gpuart_hip_finish, which also launches collected passes) before returning."""
        import torch
        uv = np.ascontiguousarray(uv, np.float32)
        if uv.ndim != 2 or uv.shape[1] != 2:
            raise ValueError("uv must be (n_sub, 2): rand1, rand2 of every sub-sample")
        if pixels.dtype != torch.int32 or pixels.dim() != 1 or not pixels.is_contiguous() or pixels.device.type != "cuda":
            raise ValueError("pixels must be a contiguous (n,) int32 tensor on the GPU")
        n, k = pixels.shape[0], uv.shape[0]
        hits = out if out is not None else torch.empty((k, n, 8), dtype=torch.float32, device=pixels.device)
        if hits.dtype != torch.float32 or tuple(hits.shape) != (k, n, 8) or not hits.is_contiguous() or hits.device != pixels.device:
            raise ValueError("out must be a contiguous (n_sub, n, 8) float32 tensor on the pixels' device")
        prims = None
        if want_prims:
            prims = prims_out if prims_out is not None else torch.empty((k, n), dtype=torch.int32, device=pixels.device)
            if prims.dtype != torch.int32 or tuple(prims.shape) != (k, n) or not prims.is_contiguous() or prims.device != pixels.device:
                raise ValueError("prims_out must be a contiguous (n_sub, n) int32 tensor on the pixels' device")
        torch.cuda.current_stream(pixels.device).synchronize()
        self._chk(self.L.gpuart_hip_trace_subpixel(self.ctx, C.c_void_p(pixels.data_ptr() if n else 0), C.c_size_t(n), _p(uv), C.c_uint32(k),
                                                   C.c_float(pixel_size), _user_sphere(user_sphere), C.c_void_p(hits.data_ptr() if n else 0),
                                                   C.c_void_p(prims.data_ptr() if prims is not None and n else 0)))
        self.finish()
        return (hits, prims) if want_prims else hits

    # test hooks
    def _hook(self, name, ins, nout, *extra):
        ins = [np.ascontiguousarray(a, np.float32) for a in ins]
        n = ins[0].shape[0]
        outs = [np.zeros((n, 4), np.float32) for _ in range(nout)]
        self._chk(getattr(self.L, name)(self.ctx, *[_p(a) for a in ins], *extra, C.c_int(n), *[_p(o) for o in outs]))
        return outs

    def test_random(self, x): return self._hook("gpuart_hip_test_random", [x], 1)[0]
    def test_math(self, x): return self._hook("gpuart_hip_test_math", [x], 1)[0]
    def test_hemisphere(self, v, ri): return self._hook("gpuart_hip_test_hemisphere", [v, ri], 1)[0]

    def test_inside_cone(self, v, nrm, ri, half_angle):
        return self._hook("gpuart_hip_test_inside_cone", [v, nrm, ri], 1, C.c_float(half_angle))[0]

    def test_sky(self, dirs, sun_dir_alt):
        return self._hook("gpuart_hip_test_sky", [dirs], 1, (C.c_float * 4)(*[float(x) for x in sun_dir_alt]))[0]

    def test_intersect(self, ptype, rs, rd, quads16):
        rs = np.ascontiguousarray(rs, np.float32)
        rd = np.ascontiguousarray(rd, np.float32)
        q = np.ascontiguousarray(quads16, np.float32).reshape(rs.shape[0], 16)
        n = rs.shape[0]
        o0, o1 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        self._chk(self.L.gpuart_hip_test_intersect(self.ctx, C.c_int(ptype), _p(rs), _p(rd), _p(q), C.c_int(n), _p(o0), _p(o1)))
        return o0, o1

    def test_aabb(self, rs, rd, bmin, bmax): return self._hook("gpuart_hip_test_aabb", [rs, rd, bmin, bmax], 1)[0]

    def test_traverse(self, rs, rd, user_sphere, any_hit=False, nearest_first=False):
        """any_hit: only "anything hit?"; nearest_first: the closest-hit query in the order of the fast kernels (nearer child first)."""
        rs = np.ascontiguousarray(rs, np.float32)
        rd = np.ascontiguousarray(rd, np.float32)
        n = rs.shape[0]
        o0, o1 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        us = (C.c_float * 4)(*[float(x) for x in user_sphere])
        self._chk(self.L.gpuart_hip_test_traverse(self.ctx, _p(rs), _p(rd), us, C.c_int(n), C.c_int(2 if nearest_first else 1 if any_hit else 0),
                                                  _p(o0), _p(o1)))
        return o0, o1

    def test_cam_rays(self):
        _, _, tw, th = self.tile
        rs, rd = np.zeros((th, tw, 4), np.float32), np.zeros((th, tw, 4), np.float32)
        self._chk(self.L.gpuart_hip_test_cam_rays(self.ctx, _p(rs), _p(rd)))
        return rs, rd


# ---- gpuart::Renderer ------------------------------------------------------------------------------
class Renderer:
    """Python handle of the C++ gpuart::Renderer (reference API, src/renderer.h:183-296)."""

    def __init__(self, W, H, cam, device=0):
        self.L = host_lib()
        self.W, self.H = W, H
        self.tile = (0, 0, W, H)
        self.h = C.c_void_p(self.L.gpuart_renderer_create(C.c_uint(W), C.c_uint(H), _f3(cam["pos"]), _f3(cam["dir"]),
                                                          _f3(cam["up"]), C.c_float(cam["fov_y"]),
                                                          C.c_float(cam["screen_dist"]), C.c_int(device)))
        if not self.L.gpuart_renderer_is_ok(self.h):
            msg = hip_lib().gpuart_hip_last_error().decode()
            self.L.gpuart_renderer_destroy(self.h)
            self.h = None
            raise HipError("Renderer initialisation failed: " + msg)
        self.backend = Backend(device=device, borrowed=self.L.gpuart_renderer_backend(self.h))
        self.backend.tile = self.tile

    def close(self):
        if self.h:
            self.L.gpuart_renderer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def is_ok(self): return bool(self.L.gpuart_renderer_is_ok(self.h))

    def set_primitives(self, descs, print_info=False):
        arr = descs if isinstance(descs, C.Array) else make_prims(descs)
        self.L.gpuart_renderer_set_primitives(self.h, arr, C.c_int(len(arr)), C.c_int(1 if print_info else 0))

    def update_primitives(self, indices, descs):
        """Renderer::UpdatePrimitives: the primitives `indices` — distinct, numbering the descriptions set_primitives was given, as the
        ordinals of trace_rays do — become `descs` (the same types); the tree is refitted on the device and the temporal history kept.
        False, with nothing changed, on any refusal."""
        arr = descs if isinstance(descs, C.Array) else make_prims(descs)
        idx = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        if idx.size != len(arr):
            raise ValueError("update_primitives: one description per index")
        return bool(self.L.gpuart_renderer_update_primitives(self.h, _p(idx), arr, C.c_int(len(arr))))

    def rebuild_tree(self, mode="morton"):
        """Renderer::RebuildTree: the tree rebuilt on the device — `mode` "morton": in Morton order; "clustered": by locally-ordered
        clustering (Renderer::TREE_CLUSTERED: slower to build, cheaper to walk) —, the temporal history kept. Returns new_to_old (per new
        device ordinal the old one; the indices of update_primitives and the ordinals of trace_rays keep numbering the descriptions
        set_primitives was given), or None — nothing changed — on a refusal."""
        n = C.c_uint64()
        self.L.gpuart_renderer_scene_info(self.h, None, C.byref(n), None)
        perm = np.zeros(int(n.value), np.uint32)
        if mode not in TREE_MODES:
            raise ValueError("rebuild_tree: mode must be one of %s" % sorted(TREE_MODES))
        return perm if self.L.gpuart_renderer_rebuild_tree_mode(self.h, C.c_int(TREE_MODES[mode]), _p(perm)) else None

    def edit_primitives(self, remove, descs, mode="clustered"):
        """Renderer::EditPrimitives: the descriptions `remove` — distinct indices, numbered as for update_primitives — leave the scene,
        `descs` (any types) join it and the tree is built on the device in `mode`, the temporal history kept. Afterwards the caller's
        descriptions are the ones not removed, in their order, followed by `descs`: update_primitives and trace_rays number that list.
        Returns source (per new device ordinal the old device ordinal, or n_old + k for descs[k]), or None — nothing changed — on a
        refusal."""
        if mode not in TREE_MODES:
            raise ValueError("edit_primitives: mode must be one of %s" % sorted(TREE_MODES))
        arr = descs if isinstance(descs, C.Array) else make_prims(descs)
        idx = np.ascontiguousarray(remove, np.uint32).reshape(-1)
        n = C.c_uint64()
        self.L.gpuart_renderer_scene_info(self.h, None, C.byref(n), None)
        source = np.zeros(int(n.value) + len(arr), np.uint32)
        n_new = C.c_size_t(0)
        ok = self.L.gpuart_renderer_edit_primitives(self.h, _p(idx), C.c_int(idx.size), arr, C.c_int(len(arr)), C.c_int(TREE_MODES[mode]), _p(source),
                                                    C.byref(n_new))
        return source[:n_new.value].copy() if ok else None

    def tree_cost(self):
        """Renderer::TreeCost, or None on failure."""
        cost = C.c_double()
        return float(cost.value) if self.L.gpuart_renderer_tree_cost(self.h, C.byref(cost)) else None

    def last_rebuild_ms(self):
        out = (C.c_double * 2)()
        self.L.gpuart_renderer_last_rebuild_ms(self.h, out)
        return float(out[0]), float(out[1])

    def compile_bvh(self):
        """GetBVH().Compile() -> quads (n, 4) float32."""
        q = C.POINTER(C.c_float)()
        nq = C.c_size_t(0)
        if self.L.gpuart_renderer_compile_bvh(self.h, C.byref(q), C.byref(nq)) != 0:
            raise RuntimeError("gpuart_renderer_compile_bvh failed")
        return _take_quads(self.L, q, nq.value)

    def init_box(self): self.L.gpuart_renderer_init_box(self.h)
    def init_dragon(self, path): return bool(self.L.gpuart_renderer_init_dragon(self.h, path.encode()))
    def init_cluster(self, path): return bool(self.L.gpuart_renderer_init_cluster(self.h, path.encode()))
    def init_tree(self, path): return bool(self.L.gpuart_renderer_init_tree(self.h, path.encode()))

    def set_camera(self, cam):
        return bool(self.L.gpuart_renderer_set_camera(self.h, _f3(cam["pos"]), _f3(cam["dir"]), _f3(cam["up"]),
                                                      C.c_float(cam["fov_y"]), C.c_float(cam["screen_dist"])))

    def update_viewport(self, W, H):
        ok = bool(self.L.gpuart_renderer_update_viewport(self.h, C.c_uint(W), C.c_uint(H)))
        self.W, self.H = W, H
        self.tile = self.backend.tile = (0, 0, W, H)
        return ok

    def set_tile(self, x0, y0, w, h):
        ok = bool(self.L.gpuart_renderer_set_tile(self.h, C.c_uint(x0), C.c_uint(y0), C.c_uint(w), C.c_uint(h)))
        if ok:
            self.tile = self.backend.tile = (x0, y0, w, h)
        return ok

    def set_interleaved_tile(self, x0, y0, w, local_rows, band_rows, band_stride):
        ok = bool(self.L.gpuart_renderer_set_interleaved_tile(self.h, C.c_uint(x0), C.c_uint(y0), C.c_uint(w), C.c_uint(local_rows),
                                                              C.c_uint(band_rows), C.c_uint(band_stride)))
        if ok:
            self.tile = self.backend.tile = (x0, y0, w, local_rows)
        return ok

    def set_sun(self, az, alt, direct=True):
        self.L.gpuart_renderer_set_sun(self.h, C.c_float(az), C.c_float(alt), C.c_int(1 if direct else 0))

    def set_user_sphere(self, pos, radius, emittance=0.0, specular=False, fuzzy=False):
        self.L.gpuart_renderer_set_user_sphere(self.h, _f3(pos), C.c_float(radius), C.c_float(emittance),
                                               C.c_int(int(specular)), C.c_int(int(fuzzy)))

    def set_user_sphere_pos(self, pos):
        """Renderer::SetUserSpherePos: moves the user sphere alone; with set_temporal_history on, the view is committed and the history
        kept (set_user_sphere also sets emittance and flags, which drops it)."""
        self.L.gpuart_renderer_set_user_sphere_pos(self.h, _f3(pos))

    def set_max_path_segments(self, n): self.L.gpuart_renderer_set_max_path_segments(self.h, C.c_uint(n))
    def set_seed(self, seed): self.L.gpuart_renderer_set_seed(self.h, C.c_uint32(seed))
    def set_min_weight(self, w): self.L.gpuart_renderer_set_min_weight(self.h, C.c_float(w))
    def set_nearest_first(self, min_prims): return bool(self.L.gpuart_renderer_set_nearest_first(self.h, C.c_uint32(min_prims)))
    def render_direct(self): self.L.gpuart_renderer_render_direct(self.h)

    def restart_path_tracing(self, per_pass, per_pixel):
        self.L.gpuart_renderer_restart_path_tracing(self.h, C.c_uint(per_pass), C.c_uint(per_pixel))

    def path_tracing_pass(self): return int(self.L.gpuart_renderer_path_tracing_pass(self.h))

    def read_direct(self):
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        if not self.L.gpuart_renderer_read_direct(self.h, _p(out)):
            raise HipError("read_direct failed")
        return out

    def read_radiance(self, normalized=False):
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        if not self.L.gpuart_renderer_read_radiance(self.h, _p(out), C.c_int(1 if normalized else 0)):
            raise HipError("read_radiance failed")
        return out

    def read_denoised(self, params=None):
        """Renderer::ReadDenoised: the denoised preview of the normalised accumulator, (th, tw, 4) float32; params as Denoiser.run."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        p = denoise_params(params)
        if not self.L.gpuart_renderer_read_denoised(self.h, _p(out), C.byref(p) if p is not None else None):
            raise HipError("read_denoised failed: %s / %s" % (hip_lib().gpuart_hip_last_error().decode(),
                                                              denoise_lib().gpuart_denoise_last_error().decode()))
        return out

    def set_temporal_history(self, on=True, params=None):
        """Renderer::SetTemporalHistory: carry path-traced history across set_camera (and user-sphere moves made through the C++
        API's SetUserSpherePos / SetUserSphereRadius; set_user_sphere also sets emittance and flags, which drops the history);
        params as Temporal.accumulate, used by the commits."""
        p = temporal_params(params)
        if not self.L.gpuart_renderer_set_temporal_history(self.h, C.c_int(1 if on else 0), C.byref(p) if p is not None else None):
            raise ValueError("temporal parameters out of range")

    def read_preview(self, denoise=None, temporal=None):
        """Renderer::ReadPreview: the history blended with the accumulator, then denoised, (th, tw, 4) float32; read_denoised while
        there is no history. denoise as read_denoised's params; temporal as Temporal.accumulate's (None: set_temporal_history's)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        dn, tp = denoise_params(denoise), temporal_params(temporal)
        if not self.L.gpuart_renderer_read_preview(self.h, _p(out), C.byref(dn) if dn is not None else None,
                                                   C.byref(tp) if tp is not None else None):
            raise HipError("read_preview failed: %s / %s / %s" % (hip_lib().gpuart_hip_last_error().decode(),
                                                                  denoise_lib().gpuart_denoise_last_error().decode(),
                                                                  temporal_lib().gpuart_temporal_last_error().decode()))
        return out

    def set_history_variance(self, on=True, params=None):
        """Renderer::SetHistoryVariance: while on, every commit of set_temporal_history also carries the luminance's moments through a
        second history (include/gpuart_moments.h); turning it on or off drops the temporal history. params = None (the defaults), a
        MomentsParams or a dict of fields that replace the defaults: read_guided_preview's error map."""
        p = moments_params(params)
        if not self.L.gpuart_renderer_set_history_variance(self.h, C.c_int(1 if on else 0), C.byref(p) if p is not None else None):
            raise ValueError("moments parameters out of range")

    def set_history_antilag(self, on=True, params=None):
        """Renderer::SetHistoryAntiLag: while on (and set_temporal_history and set_history_variance are), every commit also carries the
        radiance through a third, short history, and read_guided_preview follows it where the lighting has changed
        (include/gpuart_antilag.h); turning it on or off drops the temporal history. params = None (the defaults), an AntiLagParams or
        a dict of fields that replace the defaults."""
        p = antilag_params(params)
        if not self.L.gpuart_renderer_set_history_antilag(self.h, C.c_int(1 if on else 0), C.byref(p) if p is not None else None):
            raise ValueError("anti-lag parameters out of range")

    def set_edge_resolve(self, on=True, params=None):
        """Renderer::SetEdgeResolve: while on, read_denoised, read_preview, read_guided_preview and read_refined (and read_display of
        them) end in mark, the sub-pixel rays and resolve (include/gpuart_edges.h); nothing else sees a resolved value. params = None
        (the defaults), an EdgesParams or a dict of fields that replace the defaults."""
        p = edges_params(params)
        if not self.L.gpuart_renderer_set_edge_resolve(self.h, C.c_int(1 if on else 0), C.byref(p) if p is not None else None):
            raise ValueError("edge-resolve parameters out of range")

    def get_edge_resolve(self): return bool(self.L.gpuart_renderer_get_edge_resolve(self.h))

    def set_firefly_clamp(self, on=True, params=None):
        """Renderer::SetFireflyClamp: while on, the view every filtered read (read_denoised, read_preview, read_guided_preview,
        read_refined, and read_display of them) and every temporal commit stages is clamped in place first
        (include/gpuart_despeckle.h); read_radiance, the accumulator and the estimates never see a clamped value. Biased: it removes
        energy. Changing the switch or its parameters drops the temporal history. params = None (the defaults), a DespeckleParams or a
        dict of fields that replace the defaults."""
        p = despeckle_params(params)
        if not self.L.gpuart_renderer_set_firefly_clamp(self.h, C.c_int(1 if on else 0), C.byref(p) if p is not None else None):
            raise ValueError("firefly-clamp parameters out of range")

    def get_firefly_clamp(self): return bool(self.L.gpuart_renderer_get_firefly_clamp(self.h))

    def firefly_summary(self):
        """Renderer::ReadFireflySummary: the counts of the last clamp a read or a commit ran, as a dict (DespeckleSummary.as_dict); None
        before the first."""
        s = DespeckleSummary()
        if not self.L.gpuart_renderer_read_firefly_summary(self.h, C.byref(s)):
            return None
        return s.as_dict()

    def read_guided_preview(self, lum_floor=CONVERGE_DEFAULT_FLOOR, refine=None, temporal=None):
        """Renderer::ReadGuidedPreview: the history blended with the accumulator, then filtered by the variance-guided filter with the
        error map of the history's measured variance, (th, tw, 4) float32. refine as Refine.run's params; temporal as
        Temporal.accumulate's (None: set_temporal_history's). None while set_history_variance or set_temporal_history is off and
        before the view's first path."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        rf, tp = refine_params(refine), temporal_params(temporal)
        if not self.L.gpuart_renderer_read_guided_preview(self.h, _p(out), C.c_float(lum_floor), C.byref(rf) if rf is not None else None,
                                                          C.byref(tp) if tp is not None else None):
            return None
        return out

    def render_until(self, threshold, max_above_share=0.0, batch_paths=CONVERGE_DEFAULT_BATCH, lum_floor=CONVERGE_DEFAULT_FLOOR):
        """Renderer::RenderUntil: continue the current accumulation (restart_path_tracing's target is the cap) in batches of at least
        batch_paths paths per pixel until at most max_above_share of the tile's pixels have a relative standard error of their
        luminance above threshold (include/gpuart_converge.h). Returns (converged, summary): converged is False when the cap was
        reached first; summary is the last measure as a dict (ConvergeSummary.as_dict; `total` = the paths rendered), None if none ran."""
        if not (threshold >= 0 and threshold < float("inf")):
            raise ValueError("threshold must be finite and >= 0")
        if not max_above_share >= 0:
            raise ValueError("max_above_share must be >= 0")
        if int(batch_paths) != batch_paths or not 1 <= batch_paths <= 0xffffffff:
            raise ValueError("batch_paths must be an integer >= 1")
        if not (lum_floor > 0 and lum_floor < float("inf")):
            raise ValueError("lum_floor must be finite and > 0")
        s = ConvergeSummary()
        rc = self.L.gpuart_renderer_render_until(self.h, C.c_float(threshold), C.c_float(max_above_share), C.c_uint(int(batch_paths)),
                                                 C.c_float(lum_floor), C.byref(s))
        if rc < 0:
            raise HipError("render_until failed: %s / %s" % (hip_lib().gpuart_hip_last_error().decode(),
                                                             converge_lib().gpuart_converge_last_error().decode()))
        return rc == 1, (s.as_dict() if s.batches else None)

    def render_adaptive(self, threshold, min_paths=ADAPTIVE_DEFAULT_MIN_PATHS, batch_paths=CONVERGE_DEFAULT_BATCH, lum_floor=CONVERGE_DEFAULT_FLOOR):
        """Renderer::RenderAdaptive: render_until's loop with the estimate kept per 8x8 block (include/gpuart_adaptive.h): a block whose
        pixels all have a relative standard error of at most threshold, and which holds at least min_paths paths and two batches, is
        retired, and the passes that follow render the remaining blocks only. Returns (converged, summary): converged is True when no
        block is active any more, False when the cap was reached first; summary is the last select as a dict (AdaptiveSummary.as_dict),
        None if none ran. Raises HipError for arguments out of range, while temporal history is on, and on errors."""
        s = AdaptiveSummary()
        rc = self.L.gpuart_renderer_render_adaptive(self.h, C.c_float(threshold), C.c_uint(int(min_paths)), C.c_uint(int(batch_paths)),
                                                    C.c_float(lum_floor), C.byref(s))
        if rc < 0:
            raise HipError("render_adaptive failed (arguments out of range, temporal history on, or: %s / %s)" % (
                hip_lib().gpuart_hip_last_error().decode(), adaptive_lib().gpuart_adaptive_last_error().decode()))
        return rc == 1, (s.as_dict() if s.blocks else None)

    def read_sample_counts(self):
        """Renderer::ReadSampleCounts: the paths accumulated into every tile pixel (its 8x8 block's count), (th, tw) uint32."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw), np.uint32)
        if not self.L.gpuart_renderer_read_sample_counts(self.h, out.ctypes.data_as(C.c_void_p)):
            raise HipError("read_sample_counts failed: %s" % hip_lib().gpuart_hip_last_error().decode())
        return out

    def read_error_map(self, lum_floor=CONVERGE_DEFAULT_FLOOR):
        """Renderer::ReadErrorMap: the relative standard error per tile pixel as of render_until's last batch, (th, tw) float32; None
        before its second batch (and after anything that restarted the accumulation)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw), np.float32)
        if not self.L.gpuart_renderer_read_error_map(self.h, _p(out), C.c_float(lum_floor)):
            return None
        return out

    def read_refined(self, lum_floor=CONVERGE_DEFAULT_FLOOR, params=None):
        """Renderer::ReadRefined: the normalised accumulator filtered by the error map of render_until's last batch
        (include/gpuart_refine.h), (th, tw, 4) float32; params as Refine.run. None where read_error_map gives None: before render_until's
        second batch (and after anything that restarted the accumulation)."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.float32)
        p = refine_params(params)
        if not self.L.gpuart_renderer_read_refined(self.h, _p(out), C.c_float(lum_floor), C.byref(p) if p is not None else None):
            return None
        return out

    def read_display(self, source="radiance", params=None, lum_floor=CONVERGE_DEFAULT_FLOOR):
        """Renderer::ReadDisplay: the frame `source` names (DISPLAY_SOURCES: what read_radiance(True), read_direct, read_denoised,
        read_preview, read_guided_preview or read_refined returns, the filters with their defaults) encoded on the device as 8-bit RGBA
        (include/gpuart_display.h), (th, tw, 4) uint8, row 0 at the bottom; params as Display.run. None wherever the matching read
        fails or gives None; ValueError for parameters out of range."""
        _, _, tw, th = self.tile
        out = np.empty((th, tw, 4), np.uint8)
        p = display_params(params)
        src = DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)
        if not self.L.gpuart_renderer_read_display(self.h, _p(out), C.c_int(src), C.byref(p) if p is not None else None, C.c_float(lum_floor)):
            return None
        return out

    def read_upscaled(self, source="denoised", scale=2, lum_floor=CONVERGE_DEFAULT_FLOOR, params=None):
        """Renderer::ReadUpscaled: the frame `source` names (DISPLAY_SOURCES) upsampled `scale` (2..4) times under the guidance of a
        G-buffer of the larger frame (include/gpuart_upscale.h), (scale*th, scale*tw, 4) float32, row 0 at the bottom; params as
        Upscaler.run. None for a scale out of range, an interleaved tile, parameters out of range and wherever the matching read fails
        or gives None (the message is on stderr)."""
        _, _, tw, th = self.tile
        s = int(scale)
        out = np.empty((th * max(s, 1), tw * max(s, 1), 4), np.float32)
        p = upscale_params(params)
        src = DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)
        if not self.L.gpuart_renderer_read_upscaled(self.h, _p(out), C.c_int(src), C.c_uint32(s & 0xffffffff), C.c_float(lum_floor),
                                                    C.byref(p) if p is not None else None):
            return None
        return out

    def read_upscaled_display(self, source="denoised", scale=2, params=None, lum_floor=CONVERGE_DEFAULT_FLOOR, upscale=None):
        """Renderer::ReadUpscaledDisplay: read_upscaled's plane encoded on the device as 8-bit RGBA through the renderer's display handle
        (params as Display.run, upscale as Upscaler.run), (scale*th, scale*tw, 4) uint8. None where read_upscaled gives None."""
        _, _, tw, th = self.tile
        s = int(scale)
        out = np.empty((th * max(s, 1), tw * max(s, 1), 4), np.uint8)
        p = display_params(params)
        u = upscale_params(upscale)
        src = DISPLAY_SOURCES[source] if isinstance(source, str) else int(source)
        if not self.L.gpuart_renderer_read_upscaled_display(self.h, _p(out), C.c_int(src), C.c_uint32(s & 0xffffffff),
                                                            C.byref(p) if p is not None else None, C.c_float(lum_floor),
                                                            C.byref(u) if u is not None else None):
            return None
        return out

    def finish(self): return bool(self.L.gpuart_renderer_finish(self.h))

    def trace_rays(self, rays, occlusion=False, user_sphere=True, want_prims=False):
        """Renderer::TraceRays: rays (n, 8) in host memory; user_sphere = include the renderer's current user sphere. Returns a RAY_HIT
        record array (and, with want_prims, per ray the index of the hit primitive in the list given to set_primitives — in the
        caller's order —, -1 none, -2 the user sphere)."""
        rays = _rays_array(rays)
        n = rays.shape[0]
        hits = np.zeros(n, RAY_HIT)
        prims = np.zeros(n, np.int32) if want_prims else None
        if not self.L.gpuart_renderer_trace_rays(self.h, _p(rays), C.c_size_t(n), C.c_int(1 if occlusion else 0), C.c_int(1 if user_sphere else 0),
                                                 _p(hits), _p(prims) if prims is not None else None):
            raise HipError("trace_rays failed: " + hip_lib().gpuart_hip_last_error().decode())
        return (hits, prims) if want_prims else hits

    def pick(self, xy, user_sphere=True, want_prims=False):
        """Renderer::Pick: what lies under frame pixels xy (n, 2) = (x, y), row 0 = bottom. As trace_rays."""
        xy = _pixels_array(xy)
        n = xy.shape[0]
        hits = np.zeros(n, RAY_HIT)
        prims = np.zeros(n, np.int32) if want_prims else None
        if not self.L.gpuart_renderer_pick(self.h, _p(xy), C.c_size_t(n), C.c_int(1 if user_sphere else 0), _p(hits),
                                           _p(prims) if prims is not None else None):
            raise HipError("pick failed: " + hip_lib().gpuart_hip_last_error().decode())
        return (hits, prims) if want_prims else hits

    def closest_points(self, points, user_sphere=True):
        """Renderer::ClosestPoints: points (n, 4) = p.xyz, r in host memory; user_sphere = include the renderer's current user sphere.
        Returns a NEAREST_HIT record array; a hit's prim is the device ordinal (-2: the user sphere)."""
        points = _points_array(points)
        hits = np.zeros(points.shape[0], NEAREST_HIT)
        if not self.L.gpuart_renderer_closest_points(self.h, _p(points), C.c_size_t(points.shape[0]), C.c_int(1 if user_sphere else 0), _p(hits)):
            raise HipError("closest_points refused or failed: Renderer::ClosestPoints says why on stderr (an empty scene and a tree with irregular "
                           "boxes are not queried)")
        return hits

    def nearest_primitives(self, points, k, user_sphere=True):
        """Renderer::NearestPrimitives: points (n, 4) = p.xyz, r in host memory; user_sphere = include the renderer's current user sphere.
        Returns an (n, k) NEAREST_HIT array: row i holds query i's k nearest in ascending distance, misses behind them."""
        points = _points_array(points)
        k = int(k)
        if not 1 <= k <= NEAREST_KNN_MAX:
            raise ValueError("k must be in 1 .. %d" % NEAREST_KNN_MAX)
        hits = np.zeros((points.shape[0], k), NEAREST_HIT)
        if not self.L.gpuart_renderer_nearest_primitives(self.h, _p(points), C.c_size_t(points.shape[0]), C.c_size_t(k), C.c_int(1 if user_sphere else 0), _p(hits)):
            raise HipError("nearest_primitives refused or failed: Renderer::NearestPrimitives says why on stderr (an empty scene and a tree with "
                           "irregular boxes are not queried)")
        return hits

    def primitives_within(self, points, with_user_sphere=True):
        """Renderer::PrimitivesWithin: points (n, 4) = p.xyz, r in host memory -> (offsets uint32 (n + 1,), items NEAREST_HIT (total,)),
        list i = items[offsets[i]:offsets[i + 1]]; ordinals as closest_points reports them."""
        points = _points_array(points)
        n = points.shape[0]
        offsets = np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        us = C.c_int(1 if with_user_sphere else 0)
        ok = self.L.gpuart_renderer_primitives_within(self.h, _p(points), C.c_size_t(n), us, _p(offsets), None, C.c_size_t(0), C.byref(total))
        items = np.zeros(total.value if ok else 0, NEAREST_HIT)
        if ok and total.value:
            ok = self.L.gpuart_renderer_primitives_within_fill(self.h, _p(points), C.c_size_t(n), us, _p(offsets), _p(items), C.c_size_t(len(items)))
        if not ok:
            raise HipError("primitives_within refused or failed: Renderer::PrimitivesWithin says why on stderr (an empty scene and a tree with "
                           "irregular boxes are not queried)")
        return offsets, items

    def primitives_overlapping(self, boxes, margin=0.0, with_user_sphere=True):
        """Renderer::PrimitivesOverlapping: boxes (n, 6) = lo.xyz, hi.xyz in host memory, inflated by margin -> (offsets uint32 (n + 1,),
        items int32 (total,)), list i = items[offsets[i]:offsets[i + 1]]; ordinals as closest_points reports them."""
        boxes = np.ascontiguousarray(boxes, np.float32)
        if boxes.ndim != 2 or boxes.shape[1] != 6:
            raise ValueError("boxes must be (n, 6): lo.xyz, hi.xyz")
        n = boxes.shape[0]
        offsets = np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        us, m = C.c_int(1 if with_user_sphere else 0), C.c_float(float(margin))
        ok = self.L.gpuart_renderer_primitives_overlapping(self.h, _p(boxes), C.c_size_t(n), m, us, _p(offsets), None, C.c_size_t(0), C.byref(total))
        items = np.zeros(total.value if ok else 0, np.int32)
        if ok and total.value:
            ok = self.L.gpuart_renderer_primitives_overlapping_fill(self.h, _p(boxes), C.c_size_t(n), m, us, _p(offsets), _p(items), C.c_size_t(len(items)))
        if not ok:
            raise HipError("primitives_overlapping refused or failed: Renderer::PrimitivesOverlapping says why on stderr (an empty scene, a tree "
                           "with irregular boxes and a margin that is NaN, infinite or negative are refused)")
        return offsets, items

    def overlapping_pairs(self, margin=0.0):
        """Renderer::OverlappingPairs: (offsets uint32 (n_prims + 1,), items int32 (total,)): list i holds the ordinals j > i whose box meets
        primitive i's box inflated by margin."""
        n = int(self.backend.scene_device().n_prims)
        offsets = np.zeros(n + 1, np.uint32)
        total = C.c_uint64(0)
        m = C.c_float(float(margin))
        ok = self.L.gpuart_renderer_overlapping_pairs(self.h, m, _p(offsets), None, C.c_size_t(0), C.byref(total))
        items = np.zeros(total.value if ok else 0, np.int32)
        if ok and total.value:
            ok = self.L.gpuart_renderer_overlapping_pairs(self.h, m, _p(offsets), _p(items), C.c_size_t(len(items)), C.byref(total))
        if not ok:
            raise HipError("overlapping_pairs refused or failed: Renderer::OverlappingPairs says why on stderr")
        return offsets, items

    def last_setprims_ms(self):
        """(whole call, BVH build, compilation, re-layout + upload) of the last set_primitives, ms, as the library timed them."""
        out = (C.c_double * 4)()
        self.L.gpuart_renderer_last_setprims_ms(self.h, out)
        return tuple(float(x) for x in out)

    def save_checkpoint(self, path): return bool(self.L.gpuart_renderer_save_checkpoint(self.h, path.encode()))
    def load_checkpoint(self, path): return bool(self.L.gpuart_renderer_load_checkpoint(self.h, path.encode()))

    def params(self):
        p = Params()
        self.L.gpuart_renderer_params(self.h, C.byref(p))
        return p

    @staticmethod
    def gather_radiance(ranks, root=0, normalized=True):
        """Renderer::GatherRadiance: the shares of the renderers `ranks` (rank k of len(ranks)) as one full frame (H, W, 4) float32; None
        on error, and while a rank's path counts are not uniform (render_adaptive retired blocks): the message is on stderr."""
        r0 = ranks[root]
        out = np.empty((r0.H, r0.W, 4), np.float32)
        handles = (C.c_void_p * len(ranks))(*[r.h.value for r in ranks])
        if not r0.L.gpuart_renderer_gather_radiance(handles, C.c_int(len(ranks)), C.c_int(root), C.c_int(1 if normalized else 0), _p(out)):
            return None
        return out


# ---- the image libraries: what their handles share ----------------------------------------------------------------------------
class _ImageHandle:
    """A handle of one of the image libraries on one device. A subclass names its library (NAME: gpuart_<NAME>_create, _destroy,
    _finish, _last_error) and the error its failed calls raise (Error)."""
    NAME = Error = None

    def __init__(self, device=0):
        self.L = _image_lib(self.NAME)
        self.device = device
        h = C.c_void_p()
        self._chk(self._fn("create")(C.c_int(device), C.byref(h)))
        self.h = h

    _as_parameter_ = property(lambda self: self.h)  # what ctypes passes where a call is given the object

    def _fn(self, what):
        return getattr(self.L, "gpuart_%s_%s" % (self.NAME, what))

    def _chk(self, rc):
        if rc != 0:
            e = self.Error("gpuart_%s error %d: %s" % (self.NAME, rc, self._fn("last_error")().decode()))
            e.code = rc
            raise e

    def close(self):
        if getattr(self, "h", None):
            self._fn("destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def finish(self):
        self._chk(self._fn("finish")(self.h))


class _RefitHandle(_ImageHandle):
    """Backend.refit's gpuart_refit, made at the first refit; `generation`: that of the upload it is bound to."""
    NAME, Error = "refit", HipError
    generation = None

    def _chk(self, rc, res=None):  # res: the run's RefitResult, whose refused update becomes the error's first_bad
        try:
            super()._chk(rc)
        except HipError as e:
            e.first_bad = int(res.first_bad) if res is not None and res.status else None
            raise


class _BuildHandle(_ImageHandle):
    """Backend.rebuild's and tree_cost's gpuart_build, made at the first of them."""
    NAME, Error = "build", HipError


class _PlocHandle(_ImageHandle):
    """Backend.rebuild(mode="clustered")'s gpuart_ploc, made at the first of them."""
    NAME, Error = "ploc", HipError


class _EditHandle(_RefitHandle):
    """Backend.edit's gpuart_edit, made at the first edit; a refused edit's error carries `first_bad` as a refused refit's does."""
    NAME, Error = "edit", HipError


class _NearestHandle(_ImageHandle):
    """Backend.closest_points' gpuart_nearest, made at the first call; `generation`: that of the scene it is bound to."""
    NAME, Error = "nearest", HipError
    generation = None


def _gbuffer_args(device, rgba, hits, prims, out):
    """What the filters' run and Temporal.accumulate check of a tile's radiance, G-buffer and result: torch tensors on cuda:<device>, or
    NumPy arrays (made contiguous). -> (dev, rgba, hits, prims, res, h, w): dev is the tensors' torch device, None for NumPy arrays;
    res is `out`, or a new image like rgba."""
    if type(rgba).__module__.startswith("torch"):
        import torch
        dev = torch.device("cuda", device)
        if rgba.dtype != torch.float32 or rgba.dim() != 3 or rgba.shape[2] != 4 or not rgba.is_contiguous() or rgba.device != dev:
            raise ValueError("rgba must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
        h, w = rgba.shape[0], rgba.shape[1]
        if hits.dtype != torch.float32 or hits.numel() != h * w * 8 or not hits.is_contiguous() or hits.device != dev:
            raise ValueError("hits must be a contiguous (h, w, 8) float32 tensor on %s" % dev)
        if prims.dtype != torch.int32 or prims.numel() != h * w or not prims.is_contiguous() or prims.device != dev:
            raise ValueError("prims must be a contiguous (h, w) int32 tensor on %s" % dev)
        res = out if out is not None else torch.empty_like(rgba)
        if res.dtype != torch.float32 or tuple(res.shape) != (h, w, 4) or not res.is_contiguous() or res.device != dev:
            raise ValueError("out must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
        return dev, rgba, hits, prims, res, h, w
    rgba = np.ascontiguousarray(rgba, np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4:
        raise ValueError("rgba must be (h, w, 4) float32")
    h, w = rgba.shape[:2]
    hits = np.ascontiguousarray(hits)
    prims = np.ascontiguousarray(prims, np.int32)
    if hits.nbytes != h * w * 32 or prims.size != h * w:
        raise ValueError("hits must hold h*w 32-byte records and prims h*w ordinals")
    res = out if out is not None else np.empty_like(rgba)
    if res.dtype != np.float32 or res.shape != (h, w, 4) or not res.flags.c_contiguous:
        raise ValueError("out must be a contiguous (h, w, 4) float32 array")
    return None, rgba, hits, prims, res, h, w


def _dp(t):
    return C.c_void_p(t.data_ptr())


# ---- the two filters: the denoiser (include/gpuart_denoise.h) and the variance-guided one (include/gpuart_refine.h) ---------
class _Filter(_ImageHandle):
    """What the two filters' run methods share: gpuart_<NAME>_run for torch tensors, gpuart_<NAME>_run_host for NumPy arrays."""

    def _run(self, p, rgba, hits, prims, us_flags, out, more=lambda dev, h, w, ptr: []):
        """`more` checks the arguments a library takes between us_flags and the size and returns them, pointers made by ptr."""
        pp = C.byref(p) if p is not None else None
        dev, rgba, hits, prims, res, h, w = _gbuffer_args(self.device, rgba, hits, prims, out)
        ptr = _p if dev is None else _dp
        args = [self.h, ptr(rgba), ptr(hits), ptr(prims), C.c_uint32(us_flags)] + more(dev, h, w, ptr) + [C.c_uint32(w), C.c_uint32(h), pp, ptr(res)]
        if dev is None:
            self._chk(self._fn("run_host")(*args))
            return res
        import torch
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._fn("run")(*args))
        self.finish()
        return res


class DenoiseError(RuntimeError):
    """A gpuart_denoise_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Denoiser(_Filter):
    """A gpuart_denoise handle on one device."""
    NAME, Error = "denoise", DenoiseError

    def run(self, rgba, hits, prims, us_flags=0, params=None, out=None):
        """Filters radiance rgba (h, w, 4) float32 guided by a G-buffer: hits = the (h, w) RAY_HIT records or their (h, w, 8) float32 words,
        prims (h, w) int32 (Backend.gbuffer gives both); us_flags = the user sphere's flags (1 emissive, 2 specular); params = None (the
        defaults), a DenoiseParams or a dict of fields that replace the defaults. torch tensors on this handle's device run in place
        through gpuart_denoise_run (torch's current stream is synchronised first, the handle before returning) and the result is `out`
        or a new tensor; NumPy arrays run through gpuart_denoise_run_host and the result is `out` or a new array."""
        return self._run(denoise_params(params), rgba, hits, prims, us_flags, out)


class UpscaleError(RuntimeError):
    """A gpuart_upscale_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Upscaler(_ImageHandle):
    """A gpuart_upscale handle on one device."""
    NAME, Error = "upscale", UpscaleError

    def run(self, scale, filtered, hits, prims, hi_hits, hi_prims, us_flags=0, params=None, out=None):
        """Upsamples the filtered frame (h, w, 4) float32 `scale` times guided by its G-buffer (hits, prims: Backend.gbuffer) and the
        larger frame's (hi_hits, hi_prims: Backend.gbuffer_scaled) -> (scale*h, scale*w, 4) float32; us_flags and params as
        Denoiser.run (an UpscaleParams). torch tensors on this handle's device run in place through gpuart_upscale_run (torch's current
        stream is synchronised first, the handle before returning); NumPy arrays run through gpuart_upscale_run_host. The result is
        `out` or a new tensor or array."""
        p = upscale_params(params)
        s = int(scale)
        k = max(s, 1)
        if type(filtered).__module__.startswith("torch"):
            import torch
            dev, filtered, hits, prims, _, h, w = _gbuffer_args(self.device, filtered, hits, prims, None)
            if hi_hits.dtype != torch.float32 or hi_hits.numel() != k * k * h * w * 8 or not hi_hits.is_contiguous() or hi_hits.device != dev:
                raise ValueError("hi_hits must be a contiguous (scale*h, scale*w, 8) float32 tensor on %s" % dev)
            if hi_prims.dtype != torch.int32 or hi_prims.numel() != k * k * h * w or not hi_prims.is_contiguous() or hi_prims.device != dev:
                raise ValueError("hi_prims must be a contiguous (scale*h, scale*w) int32 tensor on %s" % dev)
            res = out if out is not None else torch.empty((k * h, k * w, 4), dtype=torch.float32, device=dev)
            if res.dtype != torch.float32 or tuple(res.shape) != (k * h, k * w, 4) or not res.is_contiguous() or res.device != dev:
                raise ValueError("out must be a contiguous (scale*h, scale*w, 4) float32 tensor on %s" % dev)
            ptr, fn = _dp, "run"
            torch.cuda.current_stream(dev).synchronize()
        else:
            _, filtered, hits, prims, _, h, w = _gbuffer_args(self.device, filtered, hits, prims, None)
            hi_hits = np.ascontiguousarray(hi_hits)
            hi_prims = np.ascontiguousarray(hi_prims, np.int32)
            if hi_hits.nbytes != k * k * h * w * 32 or hi_prims.size != k * k * h * w:
                raise ValueError("hi_hits must hold scale*h * scale*w 32-byte records and hi_prims as many ordinals")
            res = out if out is not None else np.empty((k * h, k * w, 4), np.float32)
            if res.dtype != np.float32 or res.shape != (k * h, k * w, 4) or not res.flags.c_contiguous:
                raise ValueError("out must be a contiguous (scale*h, scale*w, 4) float32 array")
            ptr, fn = _p, "run_host"
        self._chk(self._fn(fn)(self.h, C.c_uint32(s & 0xffffffff), ptr(filtered), ptr(hits), ptr(prims), C.c_uint32(w), C.c_uint32(h),
                               ptr(hi_hits), ptr(hi_prims), C.c_uint32(us_flags), C.byref(p) if p is not None else None, ptr(res)))
        if fn == "run":
            self.finish()
        return res


class RefineError(RuntimeError):
    """A gpuart_refine_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Refine(_Filter):
    """A gpuart_refine handle on one device."""
    NAME, Error = "refine", RefineError

    def run(self, rgba, hits, prims, error, lum_floor, us_flags=0, params=None, out=None):
        """Filters radiance rgba (h, w, 4) float32 guided by a G-buffer (hits, prims, us_flags as Denoiser.run) and by error (h, w) float32,
        the map Converge.measure / Renderer.read_error_map give for the same lum_floor; params = None (the defaults), a RefineParams or
        a dict of fields that replace the defaults. torch tensors on this handle's device run in place through gpuart_refine_run
        (torch's current stream is synchronised first, the handle before returning) and the result is `out` or a new tensor; NumPy
        arrays run through gpuart_refine_run_host and the result is `out` or a new array."""
        def more(dev, h, w, ptr):
            e = error
            if dev is None:
                e = np.ascontiguousarray(e, np.float32)
                if e.size != h * w:
                    raise ValueError("error must hold h*w floats")
            else:
                import torch
                if not type(e).__module__.startswith("torch") or e.dtype != torch.float32 or e.numel() != h * w or not e.is_contiguous() or \
                        e.device != dev:
                    raise ValueError("error must be a contiguous (h, w) float32 tensor on %s" % dev)
            return [ptr(e), C.c_float(lum_floor)]

        return self._run(refine_params(params), rgba, hits, prims, us_flags, out, more)


# ---- temporal accumulation (include/gpuart_temporal.h) --------------------------------------------------------------------
class TemporalError(RuntimeError):
    """A gpuart_temporal_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Temporal(_ImageHandle):
    """A gpuart_temporal handle on one device: it owns the history."""
    NAME, Error = "temporal", TemporalError

    def reset(self):
        """Drops the history."""
        self._chk(self.L.gpuart_temporal_reset(self.h))

    def accumulate(self, rgba, spp, hits, prims, view, params=None, commit=True, out=None, out_len=None):
        """Blends the history, re-sampled into `view` (a TemporalView: temporal_view()), with rgba (h, w, 4) float32, the mean of spp
        paths, guided by the G-buffer of the same tile and view (hits, prims as Denoiser.run); with commit the blend becomes the
        history. params = None (the defaults), a TemporalParams or a dict of fields that replace the defaults. Returns (blend, len):
        len (h, w) float32 is the effective sample count behind each pixel. torch tensors on this handle's device run through
        gpuart_temporal_accumulate (torch's current stream is synchronised first, the handle before returning); NumPy arrays through
        gpuart_temporal_accumulate_host. out / out_len: where to put the results (new ones otherwise)."""
        p = temporal_params(params)
        pp = C.byref(p) if p is not None else None
        dev, rgba, hits, prims, res, h, w = _gbuffer_args(self.device, rgba, hits, prims, out)
        if dev is not None:
            import torch
            ln = out_len if out_len is not None else torch.empty((h, w), dtype=torch.float32, device=dev)
            if ln.dtype != torch.float32 or tuple(ln.shape) != (h, w) or not ln.is_contiguous() or ln.device != dev:
                raise ValueError("out_len must be a contiguous (h, w) float32 tensor on %s" % dev)
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_temporal_accumulate(self.h, _dp(rgba), C.c_uint32(spp), _dp(hits), _dp(prims), C.c_uint32(w), C.c_uint32(h),
                                                        C.byref(view), pp, C.c_int(1 if commit else 0), _dp(res), _dp(ln)))
            self.finish()
            return res, ln
        ln = out_len if out_len is not None else np.empty((h, w), np.float32)
        if ln.dtype != np.float32 or ln.shape != (h, w) or not ln.flags.c_contiguous:
            raise ValueError("out_len must be a contiguous (h, w) float32 array")
        self._chk(self.L.gpuart_temporal_accumulate_host(self.h, _p(rgba), C.c_uint32(spp), _p(hits), _p(prims), C.c_uint32(w), C.c_uint32(h),
                                                         C.byref(view), pp, C.c_int(1 if commit else 0), _p(res), _p(ln)))
        return res, ln


# ---- the history's measured variance (include/gpuart_moments.h) -------------------------------------------------------------
class MomentsError(RuntimeError):
    """A gpuart_moments_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Moments(_ImageHandle):
    """A gpuart_moments handle on one device."""
    NAME, Error = "moments", MomentsError

    def pack(self, rgba, spp, out=None):
        """rgba (h, w, 4) float32, the mean of spp paths -> {L, L*L, 1/spp, a}, the image a second Temporal handle carries. A torch
        tensor on this handle's device runs through gpuart_moments_pack (torch's current stream is synchronised first, the handle
        before returning; out may be rgba itself); a NumPy array through gpuart_moments_pack_host. The result is `out` or a new image."""
        if type(rgba).__module__.startswith("torch"):
            import torch
            dev = torch.device("cuda", self.device)
            if rgba.dtype != torch.float32 or rgba.dim() != 3 or rgba.shape[2] != 4 or not rgba.is_contiguous() or rgba.device != dev:
                raise ValueError("rgba must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
            res = out if out is not None else torch.empty_like(rgba)
            if res.dtype != torch.float32 or res.shape != rgba.shape or not res.is_contiguous() or res.device != dev:
                raise ValueError("out must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_moments_pack(self.h, _dp(rgba), C.c_uint32(spp), C.c_uint32(rgba.shape[1]), C.c_uint32(rgba.shape[0]), _dp(res)))
            self.finish()
            return res
        rgba = np.ascontiguousarray(rgba, np.float32)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be (h, w, 4) float32")
        res = out if out is not None else np.empty_like(rgba)
        if res.dtype != np.float32 or res.shape != rgba.shape or not res.flags.c_contiguous:
            raise ValueError("out must be a contiguous (h, w, 4) float32 array")
        self._chk(self.L.gpuart_moments_pack_host(self.h, _p(rgba), C.c_uint32(spp), C.c_uint32(rgba.shape[1]), C.c_uint32(rgba.shape[0]), _p(res)))
        return res

    def error(self, rgba, length, moments, hits, prims, lum_floor=CONVERGE_DEFAULT_FLOOR, us_flags=0, params=None, out=None):
        """The error map (h, w) float32 of a pair of blends: rgba and length are what Temporal.accumulate returned for the radiance,
        moments what a second handle returned for the packed image; hits, prims, us_flags as Denoiser.run; params = None (the
        defaults), a MomentsParams or a dict of fields that replace the defaults. torch tensors on this handle's device run through
        gpuart_moments_error, NumPy arrays through gpuart_moments_error_host. The result is `out` or a new map."""
        p = moments_params(params)
        pp = C.byref(p) if p is not None else None
        dev, rgba, hits, prims, _, h, w = _gbuffer_args(self.device, rgba, hits, prims, None)
        if dev is not None:
            import torch
            for name, a, shape in (("length", length, (h, w)), ("moments", moments, (h, w, 4))):
                if not type(a).__module__.startswith("torch") or a.dtype != torch.float32 or tuple(a.shape) != shape or not a.is_contiguous() or \
                        a.device != dev:
                    raise ValueError("%s must be a contiguous %s float32 tensor on %s" % (name, shape, dev))
            res = out if out is not None else torch.empty((h, w), dtype=torch.float32, device=dev)
            if res.dtype != torch.float32 or tuple(res.shape) != (h, w) or not res.is_contiguous() or res.device != dev:
                raise ValueError("out must be a contiguous (h, w) float32 tensor on %s" % dev)
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_moments_error(self.h, _dp(rgba), _dp(length), _dp(moments), _dp(hits), _dp(prims), C.c_uint32(us_flags),
                                                  C.c_float(lum_floor), C.c_uint32(w), C.c_uint32(h), pp, _dp(res)))
            self.finish()
            return res
        length = np.ascontiguousarray(length, np.float32)
        moments = np.ascontiguousarray(moments, np.float32)
        if length.shape != (h, w) or moments.shape != (h, w, 4):
            raise ValueError("length must be (h, w) and moments (h, w, 4) float32")
        res = out if out is not None else np.empty((h, w), np.float32)
        if res.dtype != np.float32 or res.shape != (h, w) or not res.flags.c_contiguous:
            raise ValueError("out must be a contiguous (h, w) float32 array")
        self._chk(self.L.gpuart_moments_error_host(self.h, _p(rgba), _p(length), _p(moments), _p(hits), _p(prims), C.c_uint32(us_flags),
                                                   C.c_float(lum_floor), C.c_uint32(w), C.c_uint32(h), pp, _p(res)))
        return res


# ---- a fast history where the lighting changed (include/gpuart_antilag.h) ----------------------------------------------------
class AntiLagError(RuntimeError):
    """A gpuart_antilag_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class AntiLag(_ImageHandle):
    """A gpuart_antilag handle on one device."""
    NAME, Error = "antilag", AntiLagError

    def mix(self, slow, slow_len, fast, fast_len, moments, hits, prims, us_flags=0, params=None, out=None, out_len=None, want_alpha=True):
        """Moves the slow blend and its len towards the fast one where they disagree by more than the measured variance explains:
        slow, slow_len and fast, fast_len are what two Temporal handles returned for the radiance with a long and a short window,
        moments what the long window's second handle returned for the packed image; hits, prims, us_flags as Denoiser.run; params =
        None (the defaults), an AntiLagParams or a dict of fields that replace the defaults. torch tensors on this handle's device run
        through gpuart_antilag_mix (out may be slow itself, out_len slow_len itself), NumPy arrays through gpuart_antilag_mix_host.
        -> (out, out_len, alpha); alpha is None without want_alpha."""
        p = antilag_params(params)
        pp = C.byref(p) if p is not None else None
        dev, slow, hits, prims, res, h, w = _gbuffer_args(self.device, slow, hits, prims, out)
        planes = (("slow_len", slow_len, (h, w)), ("fast", fast, (h, w, 4)), ("fast_len", fast_len, (h, w)), ("moments", moments, (h, w, 4)))
        if dev is not None:
            import torch
            for name, a, shape in planes:
                if not type(a).__module__.startswith("torch") or a.dtype != torch.float32 or tuple(a.shape) != shape or not a.is_contiguous() or \
                        a.device != dev:
                    raise ValueError("%s must be a contiguous %s float32 tensor on %s" % (name, shape, dev))
            ln = out_len if out_len is not None else torch.empty((h, w), dtype=torch.float32, device=dev)
            if ln.dtype != torch.float32 or tuple(ln.shape) != (h, w) or not ln.is_contiguous() or ln.device != dev:
                raise ValueError("out_len must be a contiguous (h, w) float32 tensor on %s" % dev)
            al = torch.empty((h, w), dtype=torch.float32, device=dev) if want_alpha else None
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_antilag_mix(self.h, _dp(slow), _dp(slow_len), _dp(fast), _dp(fast_len), _dp(moments), _dp(hits), _dp(prims),
                                                C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h), pp, _dp(res), _dp(ln),
                                                _dp(al) if al is not None else None))
            self.finish()
            return res, ln, al
        slow_len, fast, fast_len, moments = (np.ascontiguousarray(a, np.float32) for _, a, _ in planes)
        for (name, _, shape), a in zip(planes, (slow_len, fast, fast_len, moments)):
            if a.shape != shape:
                raise ValueError("%s must be %s float32" % (name, shape))
        ln = out_len if out_len is not None else np.empty((h, w), np.float32)
        if ln.dtype != np.float32 or ln.shape != (h, w) or not ln.flags.c_contiguous:
            raise ValueError("out_len must be a contiguous (h, w) float32 array")
        al = np.empty((h, w), np.float32) if want_alpha else None
        self._chk(self.L.gpuart_antilag_mix_host(self.h, _p(slow), _p(slow_len), _p(fast), _p(fast_len), _p(moments), _p(hits), _p(prims),
                                                 C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h), pp, _p(res), _p(ln),
                                                 _p(al) if al is not None else None))
        return res, ln, al


# ---- geometric edges resolved from a sub-pixel G-buffer (include/gpuart_edges.h) ----------------------------------------------
class EdgesError(RuntimeError):
    """A gpuart_edges_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Edges(_ImageHandle):
    """A gpuart_edges handle on one device. Device memory only: torch tensors on this handle's device (torch's current stream is
    synchronised before a call, the handle before it returns)."""
    NAME, Error = "edges", EdgesError

    @staticmethod
    def offsets(n_sub):
        """gpuart_edges_offsets: the (n_sub, 2) sub-pixel offsets (rand1, rand2) of the header's rotated grid, what Backend.trace_subpixel
        is given."""
        if not 1 <= n_sub <= EDGES_MAX_SUB:
            raise ValueError("n_sub must be in 1..%d" % EDGES_MAX_SUB)
        uv = np.zeros((n_sub, 2), np.float32)
        if edges_lib().gpuart_edges_offsets(C.c_uint32(n_sub), _p(uv)) != 0:
            raise EdgesError(edges_lib().gpuart_edges_last_error().decode())
        return uv

    def _gbuffer(self, hits, prims):
        import torch
        dev = torch.device("cuda", self.device)
        if not type(prims).__module__.startswith("torch") or prims.dtype != torch.int32 or prims.dim() != 2 or not prims.is_contiguous() or \
                prims.device != dev:
            raise ValueError("prims must be a contiguous (h, w) int32 tensor on %s" % dev)
        h, w = prims.shape
        if not type(hits).__module__.startswith("torch") or hits.dtype != torch.float32 or hits.numel() != h * w * 8 or \
                not hits.is_contiguous() or hits.device != dev:
            raise ValueError("hits must be a contiguous (h, w, 8) float32 tensor on %s" % dev)
        return torch, dev, h, w

    def mark(self, hits, prims, us_flags=0, params=None):
        """The edge pixels of a G-buffer (Backend.gbuffer's tensors): -> an (n,) int32 tensor of pixel indices y * w + x in ascending
        order (the bits of uint32 indices), what Backend.trace_subpixel and resolve take. params = None (the defaults), an EdgesParams
        or a dict of fields that replace the defaults."""
        p = edges_params(params)
        torch, dev, h, w = self._gbuffer(hits, prims)
        lst = torch.empty((h * w,), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.L.gpuart_edges_mark(self.h, _dp(hits), _dp(prims), C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h),
                                           C.byref(p) if p is not None else None, _dp(lst), _dp(count)))
        self.finish()
        return lst[:int(count.item())].clone()

    def resolve(self, filtered, hits, prims, lst, sub_hits, sub_prims, us_flags=0, params=None, out=None):
        """The filtered frame (h, w, 4) mended at the listed pixels from their sub-pixel records (Backend.trace_subpixel's (n_sub, n, 8)
        and (n_sub, n) tensors; n_sub must be params'): -> `out` or a new tensor; out must not be `filtered`."""
        p = edges_params(params)
        torch, dev, h, w = self._gbuffer(hits, prims)
        n_sub = p.n_sub if p is not None else EDGES_DEFAULTS["n_sub"]
        if filtered.dtype != torch.float32 or tuple(filtered.shape) != (h, w, 4) or not filtered.is_contiguous() or filtered.device != dev:
            raise ValueError("filtered must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
        res = out if out is not None else torch.empty_like(filtered)
        if res.dtype != torch.float32 or tuple(res.shape) != (h, w, 4) or not res.is_contiguous() or res.device != dev:
            raise ValueError("out must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
        if lst.dtype != torch.int32 or lst.dim() != 1 or not lst.is_contiguous() or lst.device != dev:
            raise ValueError("lst must be a contiguous (n,) int32 tensor on %s" % dev)
        n = lst.shape[0]
        if sub_hits.dtype != torch.float32 or tuple(sub_hits.shape) != (n_sub, n, 8) or not sub_hits.is_contiguous() or sub_hits.device != dev:
            raise ValueError("sub_hits must be a contiguous (%d, %d, 8) float32 tensor on %s" % (n_sub, n, dev))
        if sub_prims.dtype != torch.int32 or tuple(sub_prims.shape) != (n_sub, n) or not sub_prims.is_contiguous() or sub_prims.device != dev:
            raise ValueError("sub_prims must be a contiguous (%d, %d) int32 tensor on %s" % (n_sub, n, dev))
        ptr = lambda t: C.c_void_p(t.data_ptr() if n else 0)
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self.L.gpuart_edges_resolve(self.h, _dp(filtered), _dp(hits), _dp(prims), C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h),
                                              ptr(lst), C.c_size_t(n), ptr(sub_hits), ptr(sub_prims), C.byref(p) if p is not None else None,
                                              _dp(res)))
        self.finish()
        return res


# ---- the convergence estimate (include/gpuart_converge.h) -----------------------------------------------------------------
# ---- the display stage (include/gpuart_display.h) ----------------------------------------------------------------------------------
class DisplayError(RuntimeError):
    """A gpuart_display_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


def srgb_table():
    """gpuart_display_srgb_table: E[0..255] as float32; needs no device."""
    out = np.empty(256, np.float32)
    rc = display_lib().gpuart_display_srgb_table(_p(out))
    if rc != 0:
        raise DisplayError("gpuart_display_srgb_table error %d" % rc)
    return out


class Display(_ImageHandle):
    """A gpuart_display handle on one device: it keeps the adapted exposure between runs."""
    NAME, Error = "display", DisplayError

    def reset(self):
        """Forgets the adapted exposure."""
        self._chk(self._fn("reset")(self.h))

    def run(self, rgba, params=None, origin=(0, 0), out=None):
        """Encodes radiance rgba (h, w, 4) float32 as 8-bit RGBA (h, w, 4) uint8; params = None (the defaults), a DisplayParams or a dict
        of fields that replace the defaults; origin = (x, y) of pixel (0, 0) in the dither pattern. torch tensors on this handle's
        device run through gpuart_display_run (torch's current stream is synchronised first, the handle before returning) and the
        result is `out` or a new tensor; NumPy arrays run through gpuart_display_run_host and the result is `out` or a new array."""
        p = display_params(params)
        pp = C.byref(p) if p is not None else None
        if type(rgba).__module__.startswith("torch"):
            import torch
            dev = torch.device("cuda", self.device)
            if rgba.dtype != torch.float32 or rgba.dim() != 3 or rgba.shape[2] != 4 or not rgba.is_contiguous() or rgba.device != dev:
                raise ValueError("rgba must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
            h, w = rgba.shape[0], rgba.shape[1]
            res = out if out is not None else torch.empty((h, w, 4), dtype=torch.uint8, device=dev)
            if res.dtype != torch.uint8 or tuple(res.shape) != (h, w, 4) or not res.is_contiguous() or res.device != dev:
                raise ValueError("out must be a contiguous (h, w, 4) uint8 tensor on %s" % dev)
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self._fn("run")(self.h, _dp(rgba), _dp(res), C.c_uint32(w), C.c_uint32(h), C.c_uint32(origin[0]), C.c_uint32(origin[1]), pp))
            self.finish()
            return res
        rgba = np.ascontiguousarray(rgba, np.float32)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be (h, w, 4) float32")
        h, w = rgba.shape[:2]
        res = out if out is not None else np.empty((h, w, 4), np.uint8)
        if res.dtype != np.uint8 or res.shape != (h, w, 4) or not res.flags.c_contiguous:
            raise ValueError("out must be a contiguous (h, w, 4) uint8 array")
        self._chk(self._fn("run_host")(self.h, _p(rgba), _p(res), C.c_uint32(w), C.c_uint32(h), C.c_uint32(origin[0]), C.c_uint32(origin[1]), pp))
        return res

    def state(self):
        """gpuart_display_read_state as a dict: histogram (256 ints), counted, skipped, gain (float32), valid."""
        s = DisplayState()
        self._chk(self._fn("read_state")(self.h, C.byref(s)))
        return s.as_dict()

    @staticmethod
    def srgb_table():
        return srgb_table()


# ---- the firefly clamp (include/gpuart_despeckle.h) ------------------------------------------------------------------------------
class DespeckleError(RuntimeError):
    """A gpuart_despeckle_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Despeckle(_ImageHandle):
    """A gpuart_despeckle handle on one device: it keeps the counts of its last run."""
    NAME, Error = "despeckle", DespeckleError

    def run(self, rgba, hits, prims, us_flags=0, params=None, out=None, want_scale=False):
        """gpuart_despeckle_run: clamps radiance rgba (h, w, 4) float32 by its G-buffer (hits, prims, us_flags as Denoiser.run), torch
        tensors on this handle's device (torch's current stream is synchronised first, the handle before returning). out = None (a new
        tensor), a tensor of rgba's shape, or rgba itself (in place). params = None (the defaults), a DespeckleParams or a dict of
        fields that replace the defaults. -> out, or with want_scale (out, scale (h, w) float32: s where clamped, 1 elsewhere)."""
        import torch
        p = despeckle_params(params)
        dev, rgba, hits, prims, res, h, w = _gbuffer_args(self.device, rgba, hits, prims, out)
        if dev is None:
            raise ValueError("run takes torch tensors on cuda:%d; NumPy arrays go through run_host" % self.device)
        scale = torch.empty((h, w), dtype=torch.float32, device=dev) if want_scale else None
        torch.cuda.current_stream(dev).synchronize()
        self._chk(self._fn("run")(self.h, _dp(rgba), _dp(hits), _dp(prims), C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h),
                                  C.byref(p) if p is not None else None, _dp(res), _dp(scale) if want_scale else None))
        self.finish()
        return (res, scale) if want_scale else res

    def run_host(self, rgba, hits, prims, us_flags=0, params=None, out=None, want_scale=False):
        """gpuart_despeckle_run_host: the same for NumPy arrays, staged through the handle's memory; the result is `out` or a new array."""
        p = despeckle_params(params)
        dev, rgba, hits, prims, res, h, w = _gbuffer_args(self.device, rgba, hits, prims, out)
        if dev is not None:
            raise ValueError("run_host takes NumPy arrays; torch tensors go through run")
        scale = np.empty((h, w), np.float32) if want_scale else None
        self._chk(self._fn("run_host")(self.h, _p(rgba), _p(hits), _p(prims), C.c_uint32(us_flags), C.c_uint32(w), C.c_uint32(h),
                                       C.byref(p) if p is not None else None, _p(res), _p(scale) if want_scale else None))
        return (res, scale) if want_scale else res

    def summary(self):
        """gpuart_despeckle_read_summary as a dict: surface, clamped, too_few of the last run."""
        s = DespeckleSummary()
        self._chk(self._fn("read_summary")(self.h, C.byref(s)))
        return s.as_dict()


class ConvergeError(RuntimeError):
    """A gpuart_converge_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


class Converge(_ImageHandle):
    """A gpuart_converge handle on one device: it owns the per-pixel state {mean, m2, prevL, 0}."""
    NAME, Error = "converge", ConvergeError

    def __init__(self, device=0):
        super().__init__(device)
        self.shape = None   # (h, w) of the state; None after reset

    def reset(self):
        """Forgets every batch: the next update may have any size."""
        self._chk(self.L.gpuart_converge_reset(self.h))
        self.shape = None

    def update(self, accum, paths_total):
        """Shows the estimator the raw accumulator accum (h, w, 4) float32, the sum over paths_total paths per pixel: one more batch.
        A torch tensor on this handle's device runs through gpuart_converge_update (torch's current stream is synchronised first, the
        handle before returning); a NumPy array through gpuart_converge_update_host."""
        if int(paths_total) != paths_total or not 0 < paths_total <= CONVERGE_MAX_PATHS:
            raise ValueError("paths_total must be an integer in 1..2^24")
        if type(accum).__module__.startswith("torch"):
            import torch
            dev = torch.device("cuda", self.device)
            if accum.dtype != torch.float32 or accum.dim() != 3 or accum.shape[2] != 4 or not accum.is_contiguous() or accum.device != dev:
                raise ValueError("accum must be a contiguous (h, w, 4) float32 tensor on %s" % dev)
            h, w = accum.shape[0], accum.shape[1]
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_converge_update(self.h, C.c_void_p(accum.data_ptr()), C.c_uint32(int(paths_total)), C.c_uint32(w), C.c_uint32(h)))
            self.finish()
        else:
            accum = np.ascontiguousarray(accum, np.float32)
            if accum.ndim != 3 or accum.shape[2] != 4:
                raise ValueError("accum must be (h, w, 4) float32")
            h, w = accum.shape[:2]
            self._chk(self.L.gpuart_converge_update_host(self.h, _p(accum), C.c_uint32(int(paths_total)), C.c_uint32(w), C.c_uint32(h)))
        self.shape = (h, w)

    def measure(self, threshold, lum_floor=CONVERGE_DEFAULT_FLOOR, error_map=False):
        """The frame's summary (a dict: ConvergeSummary.as_dict) for a threshold on e = standard error / max(mean, lum_floor), after at
        least two updates. error_map: False (none), True (a new (h, w) float32 NumPy array), a NumPy array to fill, or a torch tensor on
        this handle's device to fill through gpuart_converge_measure. Returns the summary, or (summary, map) when a map was asked for."""
        if self.shape is None:
            raise ValueError("measure before the first update")
        s = ConvergeSummary()
        if error_map is not False and error_map is not None and type(error_map).__module__.startswith("torch"):
            import torch
            dev = torch.device("cuda", self.device)
            if error_map.dtype != torch.float32 or tuple(error_map.shape) != self.shape or not error_map.is_contiguous() or error_map.device != dev:
                raise ValueError("error_map must be a contiguous %s float32 tensor on %s" % (self.shape, dev))
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_converge_measure(self.h, C.c_float(threshold), C.c_float(lum_floor), C.c_void_p(error_map.data_ptr()), C.byref(s)))
            return s.as_dict(), error_map
        if error_map is False or error_map is None:
            self._chk(self.L.gpuart_converge_measure_host(self.h, C.c_float(threshold), C.c_float(lum_floor), None, C.byref(s)))
            return s.as_dict()
        m = np.empty(self.shape, np.float32) if error_map is True else error_map
        if not isinstance(m, np.ndarray) or m.dtype != np.float32 or m.shape != self.shape or not m.flags.c_contiguous:
            raise ValueError("error_map must be a contiguous %s float32 array" % (self.shape,))
        self._chk(self.L.gpuart_converge_measure_host(self.h, C.c_float(threshold), C.c_float(lum_floor), _p(m), C.byref(s)))
        return s.as_dict(), m

    def state(self):
        """The per-pixel state (h, w, 4) float32 = {mean, m2, prevL, 0}."""
        if self.shape is None:
            raise ValueError("no state before the first update")
        out = np.empty(self.shape + (4,), np.float32)
        self._chk(self.L.gpuart_converge_read_state(self.h, _p(out)))
        return out


# ---- adaptive sampling: the estimate per 8x8 block (include/gpuart_adaptive.h) --------------------------------------------------
class AdaptiveError(RuntimeError):
    """A gpuart_adaptive_* call returned an error; `code` is the library's (GPUART_HIP_ERR_*)."""
    code = None


def _blocks_of(h, w):
    return ((w + 7) // 8) * ((h + 7) // 8)


class Adaptive(_ImageHandle):
    """A gpuart_adaptive handle on one device: it owns the per-pixel state {mean, m2, prevL, 0} and the per-block words
    {seen, batches, active, 0}."""
    NAME, Error = "adaptive", AdaptiveError

    def __init__(self, device=0):
        super().__init__(device)
        self.shape = None   # (h, w) of the state; None after reset

    def reset(self):
        """Forgets every batch: every block is active again and the next update may have any size."""
        self._chk(self.L.gpuart_adaptive_reset(self.h))
        self.shape = None

    def _images(self, images, block_paths, what):
        """torch tensors on this handle's device (-> their torch device) or NumPy arrays (-> None), checked; the arrays made contiguous."""
        first = images[0]
        if type(first).__module__.startswith("torch"):
            import torch
            dev = torch.device("cuda", self.device)
            h, w = first.shape[0], first.shape[1]
            for t in images:
                if t.dtype != torch.float32 or tuple(t.shape) != (h, w, 4) or not t.is_contiguous() or t.device != dev:
                    raise ValueError("%s must be contiguous (h, w, 4) float32 tensors on %s" % (what, dev))
            if not type(block_paths).__module__.startswith("torch") or block_paths.element_size() != 4 or block_paths.is_floating_point() or \
                    block_paths.numel() != _blocks_of(h, w) or not block_paths.is_contiguous() or block_paths.device != dev:
                raise ValueError("block_paths must be a contiguous 32-bit integer tensor of one word per 8x8 block on %s" % dev)
            return dev, list(images), block_paths, h, w
        images = [a if k else np.ascontiguousarray(a, np.float32) for k, a in enumerate(images)]
        h, w = images[0].shape[:2]
        for a in images:
            if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.shape != (h, w, 4) or not a.flags.c_contiguous:
                raise ValueError("%s must be contiguous (h, w, 4) float32 arrays" % what)
        block_paths = np.ascontiguousarray(block_paths, np.uint32).reshape(-1)
        if block_paths.size != _blocks_of(h, w):
            raise ValueError("block_paths must hold one word per 8x8 block")
        return None, images, block_paths, h, w

    def update(self, accum, block_paths):
        """Shows the estimator the raw accumulator accum (h, w, 4) float32 and the paths per pixel each 8x8 block holds (one 32-bit word per
        block, row-major: Backend.block_paths): one more batch for every block whose count moved. torch tensors on this handle's device
        run through gpuart_adaptive_update (torch's current stream is synchronised first, the handle before returning); NumPy arrays
        through gpuart_adaptive_update_host."""
        dev, (accum,), block_paths, h, w = self._images([accum], block_paths, "accum")
        if dev is not None:
            import torch
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_adaptive_update(self.h, _dp(accum), _dp(block_paths), C.c_uint32(w), C.c_uint32(h)))
            self.finish()
        else:
            self._chk(self.L.gpuart_adaptive_update_host(self.h, _p(accum), block_paths.ctypes.data_as(C.c_void_p), C.c_uint32(w), C.c_uint32(h)))
        self.shape = (h, w)

    def select(self, threshold, lum_floor=CONVERGE_DEFAULT_FLOOR, min_paths=1, error_map=None):
        """Retires the blocks whose pixels all have e <= threshold, hold at least min_paths paths and two batches. Returns (blocks, summary):
        the ascending uint32 array of the blocks that stay active and a dict (AdaptiveSummary.as_dict). error_map: None, or a contiguous
        (h, w) float32 torch tensor on this handle's device that receives e per pixel."""
        if self.shape is None:
            raise ValueError("select before the first update")
        mp = None
        if error_map is not None:
            import torch
            dev = torch.device("cuda", self.device)
            if not type(error_map).__module__.startswith("torch") or error_map.dtype != torch.float32 or tuple(error_map.shape) != self.shape or \
                    not error_map.is_contiguous() or error_map.device != dev:
                raise ValueError("error_map must be a contiguous %s float32 tensor on %s" % (self.shape, dev))
            torch.cuda.current_stream(dev).synchronize()
            mp = _dp(error_map)
        s = AdaptiveSummary()
        blocks = np.empty(_blocks_of(*self.shape), np.uint32)
        self._chk(self.L.gpuart_adaptive_select(self.h, C.c_float(threshold), C.c_float(lum_floor), C.c_uint32(int(min_paths)), mp,
                                                blocks.ctypes.data_as(C.c_void_p), C.byref(s)))
        return blocks[:s.active_blocks].copy(), s.as_dict()

    def error_map(self, lum_floor=CONVERGE_DEFAULT_FLOOR):
        """e per pixel, (h, w) float32 (+inf where the block has fewer than two batches), as a torch tensor on this handle's device."""
        if self.shape is None:
            raise ValueError("no estimate before the first update")
        import torch
        m = torch.empty(self.shape, dtype=torch.float32, device=torch.device("cuda", self.device))
        self._chk(self.L.gpuart_adaptive_error_map(self.h, C.c_float(lum_floor), _dp(m), C.c_uint32(self.shape[1]), C.c_uint32(self.shape[0])))
        self.finish()
        return m

    def normalize(self, accum, block_paths, out=None):
        """accum / its block's path count (a block without paths: / 1), alpha copied. torch tensors on this handle's device run through
        gpuart_adaptive_normalize (torch's current stream is synchronised first, the handle before returning); NumPy arrays through
        gpuart_adaptive_normalize_host. The result is `out` or a new image."""
        if out is None:
            if type(accum).__module__.startswith("torch"):
                import torch
                out = torch.empty_like(accum)
            else:
                out = np.empty(np.shape(accum), np.float32)
        dev, (accum, out), block_paths, h, w = self._images([accum, out], block_paths, "accum and out")
        if dev is not None:
            import torch
            torch.cuda.current_stream(dev).synchronize()
            self._chk(self.L.gpuart_adaptive_normalize(self.h, _dp(accum), _dp(block_paths), _dp(out), C.c_uint32(w), C.c_uint32(h)))
            self.finish()
        else:
            self._chk(self.L.gpuart_adaptive_normalize_host(self.h, _p(accum), block_paths.ctypes.data_as(C.c_void_p), _p(out), C.c_uint32(w), C.c_uint32(h)))
        return out

    def state(self):
        """(state, block_state): (h, w, 4) float32 {mean, m2, prevL, 0} and (blocks, 4) uint32 {seen, batches, active, 0}."""
        if self.shape is None:
            raise ValueError("no state before the first update")
        out = np.empty(self.shape + (4,), np.float32)
        blk = np.empty((_blocks_of(*self.shape), 4), np.uint32)
        self._chk(self.L.gpuart_adaptive_read_state(self.h, _p(out), blk.ctypes.data_as(C.c_void_p)))
        return out, blk
