#!/usr/bin/env python3
"""What the G-buffer-guided upscaler costs on the GPU: 960x540 -> 1920x1080 and 1920x1080 -> 3840x2160 (scale 2), cfg3's scene (Scene
D) from the benchmark's camera, the G-buffers of gpuart_hip_gbuffer and gpuart_hip_gbuffer_scaled and a seeded random low frame,
everything resident on the GPU; the library's defaults.

   python3 tools/upscale_time.py [--repeats R] [--calls K] [--out profiles/upscale.txt]      (appends section B to that file)

Per pair of sizes: K back-to-back calls between two synchronisations, host clock around them, every method once untimed first, then R
timed repeats with the methods alternating; printed are the median, the minimum and the maximum in ms per call:
  gbuffer         gpuart_hip_gbuffer of the low tile, for scale
  gbuffer_scaled  gpuart_hip_gbuffer_scaled of the same context (the table of the scaled tile's pixels is made by the untimed call)
  upscale         gpuart_upscale_run alone, and its rate over the compulsory bytes - per output pixel 36 B of record and ordinal in and
                  16 B out, plus 52 / scale^2 B of the low tile - as a share of the 8 TB/s HBM peak
Then end to end, through the Python binding, on the same device in the same run, alternating: a 1920x1080 render shown at 3840x2160 -
set_camera, one pass of one path per pixel, ReadUpscaledDisplay(PREVIEW, 2) - against a 3840x2160 render of the same paths per pixel
shown as it is - set_camera, one pass, ReadDisplay(PREVIEW) -, temporal history on in both, a new view every time (so every read
builds its G-buffers); the 4 bytes per output pixel that leave the device are in both."""
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

PEAK = 8.0e12   # HBM3E, bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    prims_desc = S.scene_d()
    quads, _ = B.compile_bvh(prims_desc)
    be = B.Backend(0)
    be.upload_bvh(quads)
    up = B.Upscaler(0)
    dev = torch.device("cuda", 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    scale = 2
    say("B. tools/upscale_time.py on %s: scale %d, normal_min %g, plane_tol %g; libraries %s"
        % (torch.cuda.get_device_name(0), scale, B.UPSCALE_DEFAULTS["normal_min"], B.UPSCALE_DEFAULTS["plane_tol"], os.path.relpath(B.LIBDIR, ROOT)))
    for W, H in ((960, 540), (1920, 1080)):
        be.resize(W, H)
        be.set_camera(B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H))
        hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        prims = torch.empty((H, W), dtype=torch.int32, device=dev)
        hi_hits = torch.empty((scale * H, scale * W, 8), dtype=torch.float32, device=dev)
        hi_prims = torch.empty((scale * H, scale * W), dtype=torch.int32, device=dev)
        be.gbuffer(user_sphere=None, out=hits, prims_out=prims)
        be.gbuffer_scaled(scale, user_sphere=None, out=hi_hits, prims_out=hi_prims)
        frame = torch.from_numpy(np.random.default_rng(3).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)
        out = torch.empty((scale * H, scale * W, 4), dtype=torch.float32, device=dev)

        def gbuffer():
            assert be.L.gpuart_hip_gbuffer(be.ctx, None, ptr(hits), ptr(prims)) == 0

        def gbuffer_scaled():
            assert be.L.gpuart_hip_gbuffer_scaled(be.ctx, C.c_uint32(scale), None, ptr(hi_hits), ptr(hi_prims)) == 0

        def upscale():
            assert up.L.gpuart_upscale_run(up.h, C.c_uint32(scale), ptr(frame), ptr(hits), ptr(prims), C.c_uint32(W), C.c_uint32(H), ptr(hi_hits),
                                           ptr(hi_prims), C.c_uint32(0), None, ptr(out)) == 0

        def timed(once, finish):
            def fn():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    once()
                finish()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        methods = [("gbuffer", timed(gbuffer, be.finish)), ("gbuffer_scaled", timed(gbuffer_scaled, be.finish)), ("upscale", timed(upscale, up.finish))]
        results = {name: [] for name, _ in methods}
        for _, fn in methods:
            fn()
        for _ in range(a.repeats):
            for name, fn in methods:
                results[name].append(fn())
        plain = torch.nn.functional.interpolate(frame.permute(2, 0, 1)[None], scale_factor=scale, mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
        differ = float((out[..., :3] != plain[..., :3]).any(-1).float().mean())
        say("%dx%d -> %dx%d: %d calls per timing, %d repeats, alternating; ms per call: median (min .. max); %.1f %% of the output pixels differ from "
            "plain bilinear upsampling" % (W, H, scale * W, scale * H, a.calls, a.repeats, 100 * differ))
        med = {}
        for name, _ in methods:
            v = np.array(results[name])
            med[name] = float(np.median(v))
            say("  %-15s %7.3f (%7.3f .. %7.3f)" % (name, med[name], v.min(), v.max()))
        per_pixel = 36 + 16 + 52.0 / scale ** 2
        rate = per_pixel * scale * W * scale * H / (med["upscale"] * 1e-3)
        say("  upscale: %.0f GB/s over %g compulsory bytes per output pixel, %.1f %% of the %g TB/s peak; gbuffer_scaled / gbuffer = %.2f for %d times the pixels"
            % (rate / 1e9, per_pixel, 100 * rate / PEAK, PEAK / 1e12, med["gbuffer_scaled"] / med["gbuffer"], scale * scale))
        del hits, prims, hi_hits, hi_prims, frame, out, plain
    be.close()
    up.close()

    # end to end: a 1080p render shown at 4K against a 4K render, one path per pixel and view
    low, full = B.Renderer(1920, 1080, cam), B.Renderer(3840, 2160, cam)
    try:
        for r in (low, full):
            r.set_primitives(prims_desc)
            r.set_temporal_history(True)

        def view(r, k, read):
            c2 = dict(cam, pos=(cam["pos"][0] + 0.01 * k,) + tuple(cam["pos"][1:]))
            c2["dir"] = S.camera_dir(c2)
            r.finish()
            t0 = time.perf_counter()
            r.set_camera(c2)
            r.restart_path_tracing(1, 1)
            r.path_tracing_pass()
            img = read()
            ms = (time.perf_counter() - t0) * 1e3
            assert img is not None and img.shape == (2160, 3840, 4)
            return ms

        t_low, t_full = [], []
        for k in range(a.views + 2):
            t_low.append(view(low, k, lambda: low.read_upscaled_display("preview", 2)))
            t_full.append(view(full, k, lambda: full.read_display("preview")))
        lo, fu = np.array(t_low[2:]), np.array(t_full[2:])   # (the first two views of a renderer make its handles and its first history)
        say("end to end per view (set_camera, one pass of 1 path per pixel, the read; %d views after two untimed, alternating), ms: median (min .. max)" % a.views)
        say("  1920x1080 render, ReadUpscaledDisplay(PREVIEW, 2) -> 3840x2160: %7.2f (%7.2f .. %7.2f)" % (np.median(lo), lo.min(), lo.max()))
        say("  3840x2160 render, ReadDisplay(PREVIEW)                       : %7.2f (%7.2f .. %7.2f)" % (np.median(fu), fu.min(), fu.max()))
        say("  ratio of the medians: %.2f" % (np.median(lo) / np.median(fu)))
    finally:
        low.close()
        full.close()
    with open(a.out, "a") as f:
        f.write("\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
