#!/usr/bin/env python3
"""Time of adaptive sampling on an MI355X: what retiring blocks saves a render, and what its kernels cost.

   python3 tools/adaptive_time.py [--repeats R] [--calls K] [--paths T] [--batch B] [--threshold E] [--min-paths N] [--skip-kernels] [--skip-render] [--write]

--write: the output becomes section 2 of profiles/adaptive.txt, whose prose stays.

1. The render: cfg3 (Scene D, the benchmark camera, 8 segments) at 1920x1080, a cap of T paths per pixel in one-path passes, batches of B:
   Renderer::RenderAdaptive against Renderer::RenderUntil with share 0 at the same threshold, alternating, R repeats, medians with min
   and max. Beside the wall time the paths spent: paths_sum of the adaptive render, pixels x paths rendered of the uniform one. A run has
   a fixed part that a sparse list does not shrink, so the time saved is expected to be smaller than the paths saved; both are printed.
   A third method renders the plain pass loop to the cap (the time of a render that stops nowhere).
2. The kernels, at 1920x1080 on seeded random accumulators resident on the GPU: K back-to-back gpuart_adaptive_update calls (each waits
   for the copy of the block counts it checks; the K growing count arrays are made before the clock starts, so the timed loop holds
   nothing but the calls), K gpuart_adaptive_select calls (synchronous) and K gpuart_adaptive_normalize calls between
   two synchronisations, host clock around them, median of R repeats, alternating. And k_accumulate's plain form: the time per pass of
   the plain loop above is what a change of it would show in; bench.py measures the same."""
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
from tools.profile_section import section  # noqa: E402


def stats(name, v, extra=""):
    v = np.array(v)
    print("  %-22s median %9.3f ms  (min %9.3f, max %9.3f)%s" % (name, float(np.median(v)), v.min(), v.max(), extra), flush=True)
    return float(np.median(v))


def render(a):
    W, H, T = 1920, 1080, a.paths
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(W, H, cam, device=0)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_primitives(B.make_prims(S.scene_d()))
    r.set_max_path_segments(8)
    assert r.is_ok()
    info = {}

    def start():
        r.set_seed(5489)
        r.restart_path_tracing(1, T)
        r.finish()
        return time.perf_counter()

    def plain():
        t0 = start()
        for _ in range(T):
            r.path_tracing_pass()
        r.finish()
        return (time.perf_counter() - t0) * 1e3

    def until():
        t0 = start()
        converged, s = r.render_until(a.threshold, 0.0, a.batch)
        r.finish()
        ms = (time.perf_counter() - t0) * 1e3
        info["until"] = (converged, s["total"], s["total"] * W * H, s["above"])
        return ms

    def adaptive():
        t0 = start()
        converged, s = r.render_adaptive(a.threshold, a.min_paths, a.batch)
        r.finish()
        ms = (time.perf_counter() - t0) * 1e3
        info["adaptive"] = (converged, s["paths_max"], s["paths_sum"], s["active_blocks"], s["blocks"], s["paths_min"])
        return ms

    methods = [("plain loop to the cap", plain), ("RenderUntil, share 0", until), ("RenderAdaptive", adaptive)]
    for _, fn in methods:
        fn()   # warm-up
    ms = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            ms[name].append(fn())
    print("cfg3 %dx%d, cap %d paths per pixel in one-path passes, batches of %d, threshold %g, min_paths %d; %d repeats, alternating" % (
        W, H, T, a.batch, a.threshold, a.min_paths, a.repeats))
    p = stats("plain loop to the cap", ms["plain loop to the cap"], "  %.4f ms per pass" % (float(np.median(ms["plain loop to the cap"])) / T))
    u = stats("RenderUntil, share 0", ms["RenderUntil, share 0"], "  converged %s at %d paths: %d paths spent, %d pixels above" % info["until"])
    d = stats("RenderAdaptive", ms["RenderAdaptive"], "  converged %s, %d paths issued: %d paths spent, %d of %d blocks active, fewest paths %d" % info["adaptive"])
    print("  RenderAdaptive against RenderUntil: %.1f %% of the paths, %.1f %% of the time (against the plain loop to the cap: %.1f %% of the time)" % (
        100.0 * info["adaptive"][2] / info["until"][2], 100.0 * d / u, 100.0 * d / p))
    r.close()


def kernels(a):
    dev = torch.device("cuda", 0)
    W, H = 1920, 1080
    ad = B.Adaptive(0)
    L = ad.L
    rng = np.random.default_rng(5)
    nb = ((W + 7) // 8) * ((H + 7) // 8)
    base = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
    accs = [torch.from_numpy(base * np.float32(k + 1) + rng.uniform(0, 1, (H, W, 4)).astype(np.float32)).to(dev) for k in range(2)]
    out = torch.empty_like(accs[0])
    paths = torch.zeros(nb, dtype=torch.int32, device=dev)
    summary = B.AdaptiveSummary()
    blocks = np.empty(nb, np.uint32)
    state = {"total": 0}
    torch.cuda.synchronize()

    counts = [torch.empty(nb, dtype=torch.int32, device=dev) for _ in range(a.calls)]   # (K x 130 KB)

    def update():
        for c in counts:   # every call sees counts that moved by 4 paths since the one before, also across the repeats
            state["total"] += 4
            c.fill_(state["total"])
        paths.fill_(state["total"])   # (what normalize divides by)
        torch.cuda.synchronize()
        ad.finish()
        t0 = time.perf_counter()
        for k, c in enumerate(counts):
            rc = L.gpuart_adaptive_update(ad.h, C.c_void_p(accs[k & 1].data_ptr()), C.c_void_p(c.data_ptr()), C.c_uint32(W), C.c_uint32(H))
            assert rc == 0, L.gpuart_adaptive_last_error()
        ad.finish()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def select():
        ad.finish()
        t0 = time.perf_counter()
        for _ in range(a.calls):   # (threshold 0 and min_paths 2^24: nothing retires, every call does the same work)
            rc = L.gpuart_adaptive_select(ad.h, C.c_float(0.0), C.c_float(1.0 / 256), C.c_uint32(1 << 24), None, blocks.ctypes.data_as(C.c_void_p), C.byref(summary))
            assert rc == 0, L.gpuart_adaptive_last_error()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    def normalize():
        ad.finish()
        t0 = time.perf_counter()
        for k in range(a.calls):
            rc = L.gpuart_adaptive_normalize(ad.h, C.c_void_p(accs[k & 1].data_ptr()), C.c_void_p(paths.data_ptr()), C.c_void_p(out.data_ptr()), C.c_uint32(W), C.c_uint32(H))
            assert rc == 0, L.gpuart_adaptive_last_error()
        ad.finish()
        return (time.perf_counter() - t0) * 1e3 / a.calls

    methods = [("update", update), ("select", select), ("normalize", normalize)]
    for _, fn in methods:
        fn()
    ms = {name: [] for name, _ in methods}
    for _ in range(a.repeats):
        for name, fn in methods:
            ms[name].append(fn())
    print("%dx%d (%d blocks): %d calls per timing, %d repeats, alternating; per call:" % (W, H, nb, a.calls, a.repeats))
    for name, _ in methods:
        stats(name, ms[name])
    ad.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--paths", type=int, default=256)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--threshold", type=float, default=0.1)
    ap.add_argument("--min-paths", type=int, default=B.ADAPTIVE_DEFAULT_MIN_PATHS)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-render", action="store_true")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    print("# libraries: %s" % B.LIBDIR)
    with section(os.path.join(ROOT, "profiles", "adaptive.txt") if a.write else None, 2):
        if not a.skip_render:
            render(a)
        if not a.skip_kernels:
            kernels(a)


if __name__ == "__main__":
    main()
