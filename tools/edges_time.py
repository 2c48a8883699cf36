#!/usr/bin/env python3
"""What resolving geometric edges costs on the GPU: 1920x1080 and 3840x2160, cfg3's scene (Scene D) from the benchmark's camera, the
G-buffer of gpuart_hip_gbuffer and a seeded random frame, everything resident on the GPU; the library's defaults.

   python3 tools/edges_time.py [--repeats R] [--calls K]

Per frame size: the edge share (listed pixels / tile pixels), then K back-to-back calls between two synchronisations, host clock around
them, every method once untimed first, then R timed repeats with the methods alternating; printed are the median, the minimum and the
maximum in ms per call:
  gbuffer   gpuart_hip_gbuffer of the tile, for scale (n_sub x edge share x this is what the sub-pixel rays were expected to cost)
  mark      gpuart_edges_mark (three launches)
  subpixel  gpuart_hip_trace_subpixel for the list (the generation pass, the wait for its verdict, the walk)
  resolve   gpuart_edges_resolve (the copy of the frame and the launch)
Then Renderer::ReadDenoised end to end through the Python binding (the read-back of 16 bytes per pixel included), with the switch off
- the launches the renderer made before the switch existed - and on: the first read of a view (the G-buffer, and with the switch the
list and the sub-pixel records, are built) and a cached one. Before timing, the list is checked to be ascending and complete against
a second mark."""
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
    prims_desc = S.scene_d()
    quads, _ = B.compile_bvh(prims_desc)
    be = B.Backend(0)
    be.upload_bvh(quads)
    ed = B.Edges(0)
    dev = torch.device("cuda", 0)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    n_sub = B.EDGES_DEFAULTS["n_sub"]
    uv = B.Edges.offsets(n_sub)
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    print("# libraries: %s; n_sub %d, normal_min %g, plane_tol %g" % (B.LIBDIR, n_sub, B.EDGES_DEFAULTS["normal_min"], B.EDGES_DEFAULTS["plane_tol"]))
    for W, H in ((1920, 1080), (3840, 2160)):
        be.resize(W, H)
        basis = B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
        be.set_camera(basis)
        pixel_size = float(basis[12])
        hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
        prims = torch.empty((H, W), dtype=torch.int32, device=dev)
        be.gbuffer(user_sphere=None, out=hits, prims_out=prims)
        frame = torch.from_numpy(np.random.default_rng(3).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)
        out = torch.empty_like(frame)
        lst = ed.mark(hits, prims)
        again = ed.mark(hits, prims)
        n = lst.shape[0]
        assert torch.equal(lst, again) and bool((lst[1:] > lst[:-1]).all())
        sub_hits = torch.empty((n_sub, n, 8), dtype=torch.float32, device=dev)
        sub_prims = torch.empty((n_sub, n), dtype=torch.int32, device=dev)
        full = torch.empty((H * W,), dtype=torch.int32, device=dev)
        count = torch.zeros((1,), dtype=torch.int32, device=dev)

        def gbuffer():
            assert be.L.gpuart_hip_gbuffer(be.ctx, None, ptr(hits), ptr(prims)) == 0

        def mark():
            assert ed.L.gpuart_edges_mark(ed.h, ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), None, ptr(full), ptr(count)) == 0

        def subpixel():
            assert be.L.gpuart_hip_trace_subpixel(be.ctx, ptr(lst), C.c_size_t(n), uv.ctypes.data_as(C.c_void_p), C.c_uint32(n_sub), C.c_float(pixel_size),
                                                  None, ptr(sub_hits), ptr(sub_prims)) == 0

        def resolve():
            assert ed.L.gpuart_edges_resolve(ed.h, ptr(frame), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), ptr(lst), C.c_size_t(n),
                                             ptr(sub_hits), ptr(sub_prims), None, ptr(out)) == 0

        def timed(once, finish):
            def fn():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    once()
                finish()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        methods = [("gbuffer", timed(gbuffer, be.finish)), ("mark", timed(mark, ed.finish)), ("subpixel", timed(subpixel, be.finish)),
                   ("resolve", timed(resolve, ed.finish))]
        results = {name: [] for name, _ in methods}
        for _, fn in methods:
            fn()
        for _ in range(a.repeats):
            for name, fn in methods:
                results[name].append(fn())
        sky = float((hits[..., 7].view(torch.int32) < 0).float().mean())
        print("%dx%d: %d of %d pixels are edge pixels: %.2f %% (sky %.1f %%); %d calls per timing, %d repeats, alternating; ms per call: median (min .. max)"
              % (W, H, n, W * H, 100.0 * n / (W * H), 100 * sky, a.calls, a.repeats))
        med = {}
        for name, _ in methods:
            v = np.array(results[name])
            med[name] = float(np.median(v))
            print("  %-10s %7.3f (%7.3f .. %7.3f)" % (name, med[name], v.min(), v.max()))
        print("  mark + subpixel + resolve = %.3f ms; expected for subpixel, n_sub x edge share x gbuffer: %.3f ms; %.1f M sub-pixel rays/s"
              % (med["mark"] + med["subpixel"] + med["resolve"], n_sub * n / (W * H) * med["gbuffer"], n_sub * n / med["subpixel"] / 1e3))

        # Renderer::ReadDenoised end to end
        for on in (False, True):
            r = B.Renderer(W, H, cam)
            try:
                r.set_primitives(prims_desc)
                r.set_edge_resolve(on)
                first, cached = [], []
                for k in range(3):
                    c2 = dict(cam, pos=(cam["pos"][0] + 0.01 * k,) + tuple(cam["pos"][1:]))
                    c2["dir"] = S.camera_dir(c2)
                    r.set_camera(c2)
                    r.restart_path_tracing(1, 1)
                    r.path_tracing_pass()
                    r.finish()
                    for dst in (first, cached, cached):
                        t0 = time.perf_counter()
                        r.read_denoised()
                        dst.append((time.perf_counter() - t0) * 1e3)
                print("  ReadDenoised, switch %-3s: first read of a view %7.2f ms (views 2 and 3; the first view of a renderer: %.2f), cached %7.2f ms (median of %d)"
                      % ("on" if on else "off", float(np.median(first[1:])), first[0], float(np.median(cached[2:])), len(cached) - 2))
            finally:
                r.close()
    be.close()
    ed.close()


if __name__ == "__main__":
    main()
