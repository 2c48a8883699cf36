#!/usr/bin/env python3
"""What the firefly clamp costs on the GPU (libgpuart_despeckle.so: k_ds_clamp), beside the denoiser's time from the same run:
1920x1080 and 3840x2160, cfg3's scene (Scene D) from the benchmark's camera with the G-buffer of gpuart_hip_gbuffer and a seeded random
frame with 1 % outliers of 50 times their value; everything resident on the GPU; the library's defaults.

   python3 tools/despeckle_time.py [--repeats R] [--calls K]

Per frame size: K back-to-back calls between two synchronisations, host clock around them, every method once untimed first, then R
timed repeats with the methods alternating; printed are the median, the minimum and the maximum in ms per call:
  clamp          gpuart_despeckle_run with separate buffers (the memset of the counts and one launch)
  clamp + scale  the same with the scale plane written
  in place       gpuart_despeckle_run with out == rgba (the copy into the handle's memory, 16 B per pixel each way, then the same launch)
  denoise        gpuart_denoise_run with its defaults, for scale
and the clamp's share of the 8 TB/s peak over its 68 compulsory bytes per pixel (16 + 32 + 4 in, 16 out). Then Renderer::ReadDenoised
end to end through the Python binding (the read-back of 16 bytes per pixel included) with the switch off - the launches the renderer
made before the switch existed - and on. Before timing, the device result is checked against the host entry point and in place against
separate buffers."""
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

PEAK_GBS = 8000.0
BYTES = 68.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    prims_desc = S.scene_d()
    quads, _ = B.compile_bvh(prims_desc)
    be = B.Backend(0)
    be.upload_bvh(quads)
    ds, dn = B.Despeckle(0), B.Denoiser(0)
    dev = torch.device("cuda", 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    print("# libraries: %s; %s" % (B.LIBDIR, B.DESPECKLE_DEFAULTS))
    for W, H in ((1920, 1080), (3840, 2160)):
        be.resize(W, H)
        be.set_camera(B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H))
        hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        prims = torch.empty((H, W), dtype=torch.int32, device=dev)
        be.gbuffer(user_sphere=None, out=hits, prims_out=prims)
        rng = np.random.default_rng(3)
        host = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
        host[rng.random((H, W)) < 0.01, :3] *= np.float32(50)
        rgba = torch.from_numpy(host).to(dev)
        out, work = torch.empty_like(rgba), rgba.clone()
        scale = torch.empty((H, W), dtype=torch.float32, device=dev)
        ds.run(rgba, hits, prims, out=out)
        summary = ds.summary()
        assert (out.cpu().numpy().view(np.uint32) == ds.run_host(host, hits.cpu().numpy(), prims.cpu().numpy()).view(np.uint32)).all(), \
            "device and host entry points differ"
        ds.run(work, hits, prims, out=work)
        assert torch.equal(work.view(torch.int32), out.view(torch.int32)), "in place and separate buffers differ"

        def clamp(src, dst, sc):
            def once():
                assert ds.L.gpuart_despeckle_run(ds.h, ptr(src), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), None, ptr(dst),
                                                 ptr(sc) if sc is not None else None) == 0
            return once

        def denoise():
            assert dn.L.gpuart_denoise_run(dn.h, ptr(rgba), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), None, ptr(out)) == 0

        def timed(once, finish):
            def fn():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    once()
                finish()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        methods = [("clamp", timed(clamp(rgba, out, None), ds.finish)), ("clamp + scale", timed(clamp(rgba, out, scale), ds.finish)),
                   ("in place", timed(clamp(work, work, None), ds.finish)), ("denoise", timed(denoise, dn.finish))]
        results = {name: [] for name, _ in methods}
        for _, fn in methods:
            fn()
        for _ in range(a.repeats):
            for name, fn in methods:
                results[name].append(fn())
        print("%dx%d: %d surface pixels of %d, %d clamped (%.2f %%), %d with too few neighbours; %d calls per timing, %d repeats, alternating; "
              "ms per call: median (min .. max)" % (W, H, summary["surface"], W * H, summary["clamped"], 100.0 * summary["clamped"] / max(1, summary["surface"]),
                                                    summary["too_few"], a.calls, a.repeats))
        med = {}
        for name, _ in methods:
            v = np.array(results[name])
            med[name] = float(np.median(v))
            print("  %-14s %7.4f (%7.4f .. %7.4f)" % (name, med[name], v.min(), v.max()))
        gbs = BYTES * W * H / med["clamp"] / 1e6
        print("  clamp: %.0f GB/s over %g compulsory bytes per pixel, %.1f %% of the %g TB/s peak; %.2f of the denoiser's time"
              % (gbs, BYTES, 100.0 * gbs / PEAK_GBS, PEAK_GBS / 1000, med["clamp"] / med["denoise"]))

        # Renderer::ReadDenoised end to end
        for on in (False, True):
            r = B.Renderer(W, H, cam)
            try:
                r.set_primitives(prims_desc)
                r.set_firefly_clamp(on)
                r.restart_path_tracing(1, 1)
                r.path_tracing_pass()
                r.finish()
                ms = []
                for _ in range(1 + a.repeats):
                    t0 = time.perf_counter()
                    r.read_denoised()
                    ms.append((time.perf_counter() - t0) * 1e3)
                print("  ReadDenoised, switch %-3s: %7.2f ms (median of %d cached reads; the first read of the view: %.2f)"
                      % ("on" if on else "off", float(np.median(ms[1:])), len(ms) - 1, ms[0]))
            finally:
                r.close()
    be.close()
    ds.close()
    dn.close()


if __name__ == "__main__":
    main()
