#!/usr/bin/env python3
"""Time of the denoiser (libgpuart_denoise.so: k_dn_prepare + one k_dn_atrous per level) at 1920x1080 and 3840x2160, on cfg3's scene
(Scene D) and camera with the G-buffer of gpuart_hip_gbuffer and seeded random radiance; inputs and output resident on the GPU.

   python3 tools/denoise_time.py [--repeats R] [--calls K]

Per frame size and iteration count (0 = the copy alone, 1 = prepare + one level, ..., 8): K back-to-back gpuart_denoise_run calls
between two synchronisations, host clock around them, median of R repeats, settings alternating; the per-level figure is the slope
between iterations 1 and 5. The G-buffer itself (one k_ray_query launch) is timed the same way. Before timing, the device result is
checked against the host entry point."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    be.upload_bvh(quads)
    dn = B.Denoiser(0)
    L = dn.L
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    print("# libraries: %s" % B.LIBDIR)
    for W, H in ((1920, 1080), (3840, 2160)):
        basis = np.zeros(13, np.float32)
        B.host_lib().gpuart_camera_basis(B._f3(cam["pos"]), B._f3(cam["dir"]), B._f3(cam["up"]), C.c_float(cam["fov_y"]),
                                         C.c_float(cam["screen_dist"]), C.c_uint(W), C.c_uint(H), B._p(basis))
        be.resize(W, H)
        be.set_camera(basis)
        dev = torch.device("cuda", 0)
        hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        prims = torch.empty((H, W), dtype=torch.int32, device=dev)
        be.gbuffer(user_sphere=S.USER_SPHERE, out=hits, prims_out=prims)
        rgba = torch.from_numpy(np.random.default_rng(3).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)
        out = torch.empty_like(rgba)
        surface = float((hits[..., 7].view(torch.int32) >= 0).float().mean())
        ref = dn.run(rgba.cpu().numpy(), hits.cpu().numpy(), prims.cpu().numpy())
        dn.run(rgba, hits, prims, out=out)
        assert (out.cpu().numpy().view(np.uint32) == ref.view(np.uint32)).all(), "device and host entry points differ"

        def filt(it):
            p = B.denoise_params(dict(iterations=it))
            def fn():
                for _ in range(a.calls):
                    L.gpuart_denoise_run(dn.h, C.c_void_p(rgba.data_ptr()), C.c_void_p(hits.data_ptr()), C.c_void_p(prims.data_ptr()),
                                         C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), C.byref(p), C.c_void_p(out.data_ptr()))
                dn.finish()
            return fn

        def gbuf():
            for _ in range(a.calls):
                be.L.gpuart_hip_gbuffer(be.ctx, None, C.c_void_p(hits.data_ptr()), C.c_void_p(prims.data_ptr()))
            be.finish()

        methods = [("gbuffer", gbuf)] + [("iterations %d" % it, filt(it)) for it in (0, 1, 2, 3, 5, 8)]
        for _, fn in methods:
            fn()
        ms = {name: [] for name, _ in methods}
        for _ in range(a.repeats):
            for name, fn in methods:
                t0 = time.perf_counter()
                fn()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
        print("%dx%d: %.1f %% surface pixels; %d calls per timing, %d repeats, alternating" % (W, H, 100 * surface, a.calls, a.repeats))
        med = {}
        for name, _ in methods:
            v = np.array(ms[name])
            med[name] = float(np.median(v))
            print("  %-14s median %7.3f ms per call  (min %7.3f, max %7.3f)" % (name, med[name], v.min(), v.max()))
        level = (med["iterations 5"] - med["iterations 1"]) / 4
        print("  per level (slope 1 -> 5): %.3f ms; %.0f GB/s of compulsory traffic (48 B per pixel: state + guide in, state out)"
              % (level, 48.0 * W * H / level / 1e6))
    be.close()
    dn.close()


if __name__ == "__main__":
    main()
