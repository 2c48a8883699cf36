#!/usr/bin/env python3
"""Time of the convergence estimate (libgpuart_converge.so) and what stopping costs a render.

   python3 tools/converge_time.py [--repeats R] [--calls K] [--paths T] [--skip-kernels] [--skip-stopping]

1. Kernels, at 1920x1080 and 3840x2160, on seeded random accumulators resident on the GPU: K back-to-back gpuart_converge_update calls
   between two synchronisations, host clock around them; K gpuart_converge_measure calls, each of which is synchronous (words zeroed,
   kernel, the words back through pinned memory, wait), with and without an error map. Median of R repeats, the methods alternating.
   Beside each the compulsory traffic over the time as a share of the 8 TB/s HBM peak: update 48 B per pixel (accumulator 16 and state 16
   in, state 16 out), measure 16 B (+ 4 with a map). `rocprofv3 --kernel-trace --stats -- python3 tools/converge_time.py --skip-stopping`
   in a run of its own gives the kernels' times without the launch path. Before timing, the device result is checked against the host
   entry point.
2. Cost of stopping: cfg3 (Scene D, the benchmark camera, 8 segments) at 1920x1080, T paths per pixel in one-path passes: the plain
   RenderPathTracingPass loop against Renderer::RenderUntil with a threshold nothing reaches, for batches of 8, 16, 32 and 64 paths;
   the five alternate, R repeats, median with min and max. A batch ends in an export and a wait that drain the render pipeline."""
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


def kernels(a):
    dev = torch.device("cuda", 0)
    cv, chk = B.Converge(0), B.Converge(0)
    L = cv.L
    for W, H in ((1920, 1080), (3840, 2160)):
        rng = np.random.default_rng(5)
        base = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
        accs = [torch.from_numpy(base * np.float32(k + 1) + rng.uniform(0, 1, (H, W, 4)).astype(np.float32)).to(dev) for k in range(2)]
        emap = torch.empty((H, W), dtype=torch.float32, device=dev)
        summary = B.ConvergeSummary()
        for c in (cv, chk):
            c.reset()
        for k in range(2):
            cv.update(accs[k], 4 * (k + 1))
            chk.update(accs[k].cpu().numpy(), 4 * (k + 1))
        s1, m1 = cv.measure(0.05, error_map=emap)
        s2, m2 = chk.measure(0.05, error_map=True)
        assert s1 == s2 and (m1.cpu().numpy().view(np.uint32) == m2.view(np.uint32)).all(), "device and host entry points differ"
        torch.cuda.synchronize()
        state = {"total": 8}

        def update():
            cv.finish()
            t0 = time.perf_counter()
            for k in range(a.calls):
                state["total"] += 1
                rc = L.gpuart_converge_update(cv.h, C.c_void_p(accs[k & 1].data_ptr()), C.c_uint32(state["total"]), C.c_uint32(W), C.c_uint32(H))
                assert rc == 0, L.gpuart_converge_last_error()
            cv.finish()
            return (time.perf_counter() - t0) * 1e3 / a.calls

        def measure(with_map):
            def fn():
                cv.finish()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    rc = L.gpuart_converge_measure(cv.h, C.c_float(0.05), C.c_float(1.0 / 256), C.c_void_p(emap.data_ptr()) if with_map else None,
                                                   C.byref(summary))
                    assert rc == 0, L.gpuart_converge_last_error()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        methods = [("update", update, 48), ("measure", measure(False), 16), ("measure + map", measure(True), 20)]
        for _, fn, _ in methods:
            fn()
        ms = {name: [] for name, _, _ in methods}
        for _ in range(a.repeats):
            for name, fn, _ in methods:
                ms[name].append(fn())
        print("%dx%d: %d calls per timing, %d repeats, alternating; last summary %s" % (W, H, a.calls, a.repeats, summary.as_dict()))
        for name, _, bytes_pp in methods:
            v = np.array(ms[name])
            med = float(np.median(v))
            rate = bytes_pp * W * H / (med * 1e-3)
            print("  %-14s median %7.3f ms per call  (min %7.3f, max %7.3f); %d B per pixel compulsory: %.0f GB/s, %.1f %% of the 8 TB/s peak"
                  % (name, med, v.min(), v.max(), bytes_pp, rate / 1e9, 100 * rate / HBM_PEAK))
        del accs, emap
    cv.close()
    chk.close()


def stopping(a):
    W, H, T = 1920, 1080, a.paths
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(W, H, cam, device=0)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_primitives(B.make_prims(S.scene_d()))
    r.set_max_path_segments(8)
    assert r.is_ok()

    def plain():
        r.set_seed(5489)
        r.restart_path_tracing(1, T)
        r.finish()
        t0 = time.perf_counter()
        for _ in range(T):
            r.path_tracing_pass()
        r.finish()
        return (time.perf_counter() - t0) * 1e3

    def until(batch):
        def fn():
            r.set_seed(5489)
            r.restart_path_tracing(1, T)
            r.finish()
            t0 = time.perf_counter()
            converged, s = r.render_until(0.0, 0.0, batch)
            r.finish()
            ms = (time.perf_counter() - t0) * 1e3
            assert not converged and s["total"] == T and s["batches"] == (T + batch - 1) // batch, s
            return ms
        return fn

    methods = [("plain loop", plain)] + [("until, batch %d" % b, until(b)) for b in (8, 16, 32, 64)]
    frames = {}
    for name, fn in methods:   # warm-up, and the frames must be the same
        fn()
        frames[name] = r.read_radiance(False)
    for name in frames:
        assert (frames[name].view(np.uint32) == frames["plain loop"].view(np.uint32)).all(), name
    ms = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            ms[name].append(fn())
    print("cfg3 %dx%d, %d paths per pixel in one-path passes; %d repeats, alternating; the accumulators are bit-identical" % (W, H, T, a.repeats))
    base = float(np.median(ms["plain loop"]))
    for name, _ in methods:
        v = np.array(ms[name])
        med = float(np.median(v))
        print("  %-16s median %8.2f ms  (min %8.2f, max %8.2f)  %.3f ms per path  %+6.2f %% against the plain loop"
              % (name, med, v.min(), v.max(), med / T, 100 * (med / base - 1)))
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-stopping", action="store_true")
    a = ap.parse_args()
    print("# libraries: %s" % B.LIBDIR)
    if not a.skip_kernels:
        kernels(a)
    if not a.skip_stopping:
        stopping(a)


if __name__ == "__main__":
    main()
