#!/usr/bin/env python3
"""Time of the temporal accumulation (libgpuart_temporal.so: one k_tp_accumulate launch per call) at 1920x1080 and 3840x2160, on cfg3's
scene (Scene D) after a real camera move: two views of the benchmark camera 0.1 apart sideways, the G-buffers of gpuart_hip_gbuffer and
seeded random radiance; inputs, history and outputs resident on the GPU.

   python3 tools/temporal_time.py [--repeats R] [--calls K]

Per frame size: K back-to-back gpuart_temporal_accumulate calls between two synchronisations, host clock around them (the handle's stream
is its own: no event can be recorded on it from outside; `rocprofv3 --kernel-trace --stats -- python3 tools/temporal_time.py` in a run of
its own gives the kernel's time without the launch path), median of R repeats, the two methods alternating:
  preview  commit = 0: view B against the history of view A, again and again;
  commit   commit = 1, views A and B in turn, so that every call re-samples the other view's history and writes a new one.
Beside each the compulsory traffic over the time, as a share of the 8 TB/s HBM peak. Bytes per pixel, from the layout: colour 16 + record
32 + ordinal 4 in; history colour + guide + point 48 in, once, for surface pixels; blend 16 + length 4 out; history 48 out on commit.
Before timing, the device result is checked against the host entry point."""
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

HBM_PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    be.upload_bvh(quads)
    tp, chk = B.Temporal(0), B.Temporal(0)
    L = tp.L
    dev = torch.device("cuda", 0)
    print("# libraries: %s" % B.LIBDIR)
    for W, H in ((1920, 1080), (3840, 2160)):
        be.resize(W, H)
        views = []
        for k, dx in enumerate((0.0, 0.1)):
            cam = dict(S.BENCH_CAMERA)
            cam["pos"] = (cam["pos"][0] + dx,) + tuple(cam["pos"][1:])
            cam["dir"] = S.camera_dir(cam)
            basis = B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
            be.set_camera(basis)
            hits = torch.empty((H, W, 8), dtype=torch.float32, device=dev)
            prims = torch.empty((H, W), dtype=torch.int32, device=dev)
            be.gbuffer(user_sphere=None, out=hits, prims_out=prims)
            rgba = torch.from_numpy(np.random.default_rng(3 + k).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)
            views.append((rgba, hits, prims, B.temporal_view(basis, be.get_share())))
        out = torch.empty((H, W, 4), dtype=torch.float32, device=dev)
        ln = torch.empty((H, W), dtype=torch.float32, device=dev)
        surface = float((views[1][1][..., 7].view(torch.int32) >= 0).float().mean())

        # the two entry points agree, and the move is a real one: most surface pixels find history, few at their own pixel
        for t in (tp, chk):
            t.reset()
        tp.accumulate(*views[0][:1], 4, *views[0][1:], commit=True, out=out, out_len=ln)
        tp.accumulate(*views[1][:1], 1, *views[1][1:], commit=False, out=out, out_len=ln)
        h = [tuple(x.cpu().numpy() for x in v[:3]) + (v[3],) for v in views]
        chk.accumulate(h[0][0], 4, h[0][1], h[0][2], h[0][3], commit=True)
        ref, ref_len = chk.accumulate(h[1][0], 1, h[1][1], h[1][2], h[1][3], commit=False)
        assert (out.cpu().numpy().view(np.uint32) == ref.view(np.uint32)).all() and (ln.cpu().numpy() == ref_len).all(), "device and host entry points differ"
        found = float((ref_len > 1).mean())

        def call(v, spp, commit):
            rgba, hits, prims, view = v
            rc = L.gpuart_temporal_accumulate(tp.h, C.c_void_p(rgba.data_ptr()), C.c_uint32(spp), C.c_void_p(hits.data_ptr()),
                                              C.c_void_p(prims.data_ptr()), C.c_uint32(W), C.c_uint32(H), C.byref(view), None, C.c_int(commit),
                                              C.c_void_p(out.data_ptr()), C.c_void_p(ln.data_ptr()))
            assert rc == 0, L.gpuart_temporal_last_error()

        def preview():
            call(views[0], 4, 1)
            tp.finish()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(views[1], 1, 0)
            tp.finish()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        def commit():
            call(views[0], 4, 1)
            tp.finish()
            t0 = time.perf_counter()
            for k in range(a.calls):
                call(views[(k + 1) & 1], 1, 1)
            tp.finish()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        methods = [("preview (commit 0)", preview, 52 + 48 * surface + 20), ("commit  (commit 1)", commit, 52 + 48 * surface + 20 + 48)]
        for _, fn, _ in methods:
            fn()
        ms = {name: [] for name, _, _ in methods}
        for _ in range(a.repeats):
            for name, fn, _ in methods:
                ms[name].append(fn())
        print("%dx%d: %.1f %% surface pixels, %.1f %% of all pixels found history after the move; %d calls per timing, %d repeats, alternating"
              % (W, H, 100 * surface, 100 * found, a.calls, a.repeats))
        for name, _, bytes_pp in methods:
            v = np.array(ms[name])
            med = float(np.median(v))
            rate = bytes_pp * W * H / (med * 1e-3)
            print("  %-18s median %7.3f ms per call  (min %7.3f, max %7.3f); %.0f B per pixel compulsory: %.0f GB/s, %.1f %% of the 8 TB/s peak"
                  % (name, med, v.min(), v.max(), bytes_pp, rate / 1e9, 100 * rate / HBM_PEAK))
    be.close()
    tp.close()
    chk.close()


if __name__ == "__main__":
    main()
