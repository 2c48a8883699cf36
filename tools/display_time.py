#!/usr/bin/env python3
"""Time of the display stage (libgpuart_display.so: k_dp_histogram + k_dp_exposure + k_dp_encode) and of the 8-bit read-back it makes
possible, at 1920x1080 and 3840x2160 on cfg3's scene (Scene D) and camera, by the protocol of tools/refine_time.py.

   python3 tools/display_time.py [--repeats R] [--calls K] [--skip-renderer]

(a) gpuart_display_run alone on seeded radiance resident on the GPU (log-uniform over 1e-4..1e2): K back-to-back calls between two
    synchronisations, host clock around them; linear and sRGB, with and without auto exposure, the sRGB one also with a curve and the
    dither. The kernels: the encode is a run without auto exposure; histogram + exposure is what auto exposure adds; the exposure
    kernel alone is what auto exposure adds on a 64 x 4 frame, where the histogram is one block.
(b) Renderer::ReadPreview against ReadDisplay(PREVIEW), and ReadRadiance(normalized) against ReadDisplay(RADIANCE), through the C API
    into buffers made once: K calls each, end to end including the copy into the caller's buffer. The view has a committed history and
    two paths per pixel.
(c) The read-back of the 8-bit frame alone (torch copies): device to pageable memory in one copy, against device to pinned memory and
    a host copy from there into the pageable buffer: what Renderer::ReadDisplay's last step chooses between.
Every method runs once untimed first, then R timed repeats with the methods alternating; printed are the median, the minimum and the
maximum. Before timing, the device entry point is checked against the host one, and ReadDisplay against the restatement's defaults
(gpuart_cli --ppm's bytes) of the float read."""
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

HBM_PEAK = 8e12   # bytes/s


def timed(methods, repeats, calls):
    """-> {name: [ms per call] * repeats}: one untimed round, then the methods alternating."""
    for _, fn in methods:
        fn()
    ms = {name: [] for name, _ in methods}
    for _ in range(repeats):
        for name, fn in methods:
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3 / calls)
    return ms


def show(ms, names):
    med = {}
    for name in names:
        v = np.array(ms[name])
        med[name] = float(np.median(v))
        print("  %-34s %8.4f (%8.4f .. %8.4f)" % (name, med[name], v.min(), v.max()))
    return med


def library(a, dp, W, H):
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    rgba = torch.from_numpy(np.exp(rng.uniform(np.log(1e-4), np.log(1e2), (H, W, 4))).astype(np.float32)).to(dev)
    small = rgba[:4, :64].contiguous()
    out = torch.empty((H, W, 4), dtype=torch.uint8, device=dev)
    every = dict(auto_exposure=1, curve="reinhard", transfer="srgb", dither=1)
    dp.run(rgba, every, out=out)
    assert (out.cpu().numpy() == dp.run(rgba.cpu().numpy(), every)).all(), "display: device and host entry points differ"
    dp.reset()
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def run(params, img=rgba):
        p = B.display_params(params)
        h, w = img.shape[:2]

        def fn():
            for _ in range(a.calls):
                dp.L.gpuart_display_run(dp.h, ptr(img), ptr(out), C.c_uint32(w), C.c_uint32(h), C.c_uint32(0), C.c_uint32(0), C.byref(p))
            dp.finish()
        return fn

    methods = [("linear", run({})), ("sRGB", run(dict(transfer="srgb"))), ("linear, auto exposure", run(dict(auto_exposure=1))),
               ("sRGB, auto exposure", run(dict(transfer="srgb", auto_exposure=1))), ("sRGB, reinhard, dither, auto", run(every)),
               ("64 x 4: linear", run({}, small)), ("64 x 4: linear, auto exposure", run(dict(auto_exposure=1), small))]
    ms = timed(methods, a.repeats, a.calls)
    print("%dx%d, gpuart_display_run: %d calls per timing, %d repeats, alternating; ms per call: median (min .. max)" % (W, H, a.calls, a.repeats))
    med = show(ms, [n for n, _ in methods])
    n = W * H
    for name in ("linear", "sRGB"):
        print("  k_dp_encode, %s: %.4f ms, %.0f GB/s of compulsory traffic (20 B per pixel: 16 in, 4 out), %.1f %% of the 8 TB/s HBM peak"
              % (name, med[name], 20.0 * n / med[name] / 1e6, 100 * 20.0 * n / (med[name] * 1e-3) / HBM_PEAK))
    hist = med["linear, auto exposure"] - med["linear"]
    expo = med["64 x 4: linear, auto exposure"] - med["64 x 4: linear"]
    print("  k_dp_histogram + k_dp_exposure (what auto exposure adds): %.4f ms; k_dp_exposure and the clearing of the histogram (what it adds at "
          "64 x 4): %.4f ms; k_dp_histogram (the difference): %.4f ms, %.0f GB/s of its 16 B per pixel, %.1f %% of the peak"
          % (hist, expo, hist - expo, 16.0 * n / max(hist - expo, 1e-9) / 1e6, 100 * 16.0 * n / (max(hist - expo, 1e-9) * 1e-3) / HBM_PEAK))


def readback(a, W, H):
    dev = torch.device("cuda", 0)
    src = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
    pageable, pinned = torch.empty((H, W, 4), dtype=torch.uint8), torch.empty((H, W, 4), dtype=torch.uint8).pin_memory()

    def direct():
        for _ in range(a.calls):
            pageable.copy_(src)

    def staged():
        for _ in range(a.calls):
            pinned.copy_(src)
            pageable.copy_(pinned)

    ms = timed([("device -> pageable", direct), ("device -> pinned -> pageable", staged)], a.repeats, a.calls)
    print("%dx%d, read-back of %d bytes: %d calls per timing, %d repeats, alternating; ms per call: median (min .. max)" % (W, H, W * H * 4, a.calls, a.repeats))
    show(ms, ["device -> pageable", "device -> pinned -> pageable"])


def renderer(a, r, W, H):
    from tests import display_ref as R
    r.update_viewport(W, H)
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r.set_temporal_history(True)
    r.restart_path_tracing(1, 2)
    r.path_tracing_pass()
    cam2 = dict(cam, pos=tuple(np.add(cam["pos"], (0.01, 0.0, 0.0))))
    cam2["dir"] = S.camera_dir(cam2)
    r.set_camera(cam2)    # commits the view
    r.path_tracing_pass()
    r.path_tracing_pass()
    r.finish()
    f32, u8 = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.uint8)
    for source, floats in (("preview", r.read_preview()), ("radiance", r.read_radiance(True))):
        assert (r.read_display(source)[..., :3] == R.cli_bytes(floats[..., :3])).all(), source
    L, h = r.L, r.h
    pf, p8 = f32.ctypes.data_as(C.c_void_p), u8.ctypes.data_as(C.c_void_p)
    floor = C.c_float(B.CONVERGE_DEFAULT_FLOOR)

    def loop(call):
        def fn():
            for _ in range(a.calls):
                assert call()
        return fn

    methods = [("ReadPreview", loop(lambda: L.gpuart_renderer_read_preview(h, pf, None, None))),
               ("ReadDisplay(PREVIEW)", loop(lambda: L.gpuart_renderer_read_display(h, p8, C.c_int(3), None, floor))),
               ("ReadRadiance(normalized)", loop(lambda: L.gpuart_renderer_read_radiance(h, pf, C.c_int(1)))),
               ("ReadDisplay(RADIANCE)", loop(lambda: L.gpuart_renderer_read_display(h, p8, C.c_int(0), None, floor)))]
    ms = timed(methods, a.repeats, a.calls)
    print("%dx%d, Renderer, end to end into the caller's buffer: %d calls per timing, %d repeats, alternating; ms per call: median (min .. max)"
          % (W, H, a.calls, a.repeats))
    med = show(ms, [n for n, _ in methods])
    print("  ReadDisplay(PREVIEW) / ReadPreview: %.3f; ReadDisplay(RADIANCE) / ReadRadiance(normalized): %.3f"
          % (med["ReadDisplay(PREVIEW)"] / med["ReadPreview"], med["ReadDisplay(RADIANCE)"] / med["ReadRadiance(normalized)"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--skip-renderer", action="store_true")
    a = ap.parse_args()
    print("# libraries: %s" % B.LIBDIR)
    dp = B.Display(0)
    for W, H in ((1920, 1080), (3840, 2160)):
        library(a, dp, W, H)
    dp.close()
    for W, H in ((1920, 1080), (3840, 2160)):
        readback(a, W, H)
    if a.skip_renderer:
        return
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(1920, 1080, cam)
    r.set_primitives(S.scene_d())
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0)
    for W, H in ((1920, 1080), (3840, 2160)):
        renderer(a, r, W, H)
    r.close()


if __name__ == "__main__":
    main()
