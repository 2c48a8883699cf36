#!/usr/bin/env python3
"""Time of the variance-guided filter (libgpuart_refine.so: k_rf_prepare + one k_rf_level per level) beside the denoiser's
(libgpuart_denoise.so: k_dn_prepare + one k_dn_atrous per level), in one process on the same inputs: 1920x1080 and 3840x2160, cfg3's
scene (Scene D) and camera with the G-buffer of gpuart_hip_gbuffer, seeded random radiance and a seeded random error map; inputs and
output resident on the GPU.

   python3 tools/refine_time.py [--repeats R] [--calls K]

Per frame size, library and iteration count (0 = the copy alone, 1 = prepare + one level, 2, 3, 5, 8): K back-to-back run calls
between two synchronisations, host clock around them; every method runs once untimed first, then R timed repeats with the methods
alternating; printed are the median, the minimum and the maximum. The per-level figure is the slope between iterations 1 and 5, and
prepare is iterations 1 less one level and the copy-free launch. Before timing, each library's device result is checked against its
host entry point."""
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

LUM_FLOOR = 1.0 / 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    be.upload_bvh(quads)
    dn, rf = B.Denoiser(0), B.Refine(0)
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    print("# libraries: %s" % B.LIBDIR)
    for W, H in ((1920, 1080), (3840, 2160)):
        be.resize(W, H)
        be.set_camera(B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H))
        dev = torch.device("cuda", 0)
        hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        prims = torch.empty((H, W), dtype=torch.int32, device=dev)
        be.gbuffer(user_sphere=S.USER_SPHERE, out=hits, prims_out=prims)
        rng = np.random.default_rng(3)
        rgba = torch.from_numpy(rng.uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)
        err = torch.from_numpy(rng.uniform(0.01, 0.3, (H, W)).astype(np.float32)).to(dev)
        out = torch.empty_like(rgba)
        surface = float((hits[..., 7].view(torch.int32) >= 0).float().mean())
        host = [t.cpu().numpy() for t in (rgba, hits, prims, err)]
        dn.run(rgba, hits, prims, out=out)
        assert (out.cpu().numpy().view(np.uint32) == dn.run(*host[:3]).view(np.uint32)).all(), "denoise: device and host entry points differ"
        rf.run(rgba, hits, prims, err, LUM_FLOOR, out=out)
        assert (out.cpu().numpy().view(np.uint32) == rf.run(host[0], host[1], host[2], host[3], LUM_FLOOR).view(np.uint32)).all(), \
            "refine: device and host entry points differ"
        ptr = lambda t: C.c_void_p(t.data_ptr())

        def denoise(it):
            p = B.denoise_params(dict(iterations=it))
            def fn():
                for _ in range(a.calls):
                    dn.L.gpuart_denoise_run(dn.h, ptr(rgba), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), C.byref(p), ptr(out))
                dn.finish()
            return fn

        def refine(it):
            p = B.refine_params(dict(iterations=it))
            def fn():
                for _ in range(a.calls):
                    rf.L.gpuart_refine_run(rf.h, ptr(rgba), ptr(hits), ptr(prims), C.c_uint32(0), ptr(err), C.c_float(LUM_FLOOR), C.c_uint32(W),
                                           C.c_uint32(H), C.byref(p), ptr(out))
                rf.finish()
            return fn

        its = (0, 1, 2, 3, 5, 8)
        methods = [("%s %d" % (lib, it), make(it)) for it in its for lib, make in (("denoise", denoise), ("refine", refine))]
        for _, fn in methods:
            fn()
        ms = {name: [] for name, _ in methods}
        for _ in range(a.repeats):
            for name, fn in methods:
                t0 = time.perf_counter()
                fn()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.calls)
        print("%dx%d: %.1f %% surface pixels; %d calls per timing, %d repeats, alternating; ms per call: median (min .. max)"
              % (W, H, 100 * surface, a.calls, a.repeats))
        med = {}
        print("  %-12s %-28s %-28s" % ("iterations", "denoise", "refine"))
        for it in its:
            cells = []
            for lib in ("denoise", "refine"):
                v = np.array(ms["%s %d" % (lib, it)])
                med[(lib, it)] = float(np.median(v))
                cells.append("%7.3f (%7.3f .. %7.3f)" % (med[(lib, it)], v.min(), v.max()))
            print("  %-12d %-28s %-28s" % (it, cells[0], cells[1]))
        for lib in ("denoise", "refine"):
            level = (med[(lib, 5)] - med[(lib, 1)]) / 4
            print("  %s: per level (slope 1 -> 5) %.3f ms, %.0f GB/s of compulsory traffic (48 B per pixel: state + guide in, state out); "
                  "prepare + launch overhead (iterations 1 less one level) %.3f ms" % (lib, level, 48.0 * W * H / level / 1e6, med[(lib, 1)] - level))
    be.close()
    dn.close()
    rf.close()


if __name__ == "__main__":
    main()
