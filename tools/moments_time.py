#!/usr/bin/env python3
"""Time of Renderer::ReadGuidedPreview's device sequence beside Renderer::ReadPreview's, without the read-back, in one process on the same
inputs, after tools/refine_time.py's protocol: 1920x1080 and 3840x2160, cfg3's scene (Scene D) after a sideways camera move of 0.1 (the
two views of tools/temporal_time.py), the G-buffers of gpuart_hip_gbuffer and seeded random radiance; inputs, histories and outputs
resident on the GPU.

   python3 tools/moments_time.py [--repeats R] [--calls K]

The histories: view A committed eight times at one path each, to both temporal handles (the radiance, and the packed moments of
gpuart_moments_pack), with max_history 32; then view B is previewed. Where B's pixels find history the effective number of batches is
9 and gpuart_moments_error takes the measured branch; the disoccluded pixels take the 7x7 window. "short" is the same after a single
commit: no pixel has 8 batches, so every block stages its window.

Per frame size, K back-to-back calls between two synchronisations, host clock around them; every method runs once untimed first, then
R timed repeats with the methods alternating; printed are the median, the minimum and the maximum:
  preview   blend (commit 0), wait, denoiser, wait: what ReadPreview issues
  guided    blend with out_len, wait, pack, wait, blend of the moments, wait, error, wait, variance-guided filter, wait
  blend     one gpuart_temporal_accumulate (commit 0) alone
  pack      gpuart_moments_pack alone
  error     gpuart_moments_error alone, and the same with the short history
  denoise / refine   the two filters alone
  pack, a wait per call   pack and gpuart_moments_finish K times: less pack alone, what one wait between libraries costs
Before timing, pack and error are checked against their host entry points."""
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
WINDOW = 32.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    a = ap.parse_args()
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    be.upload_bvh(quads)
    tx, tm, mo, dn, rf = B.Temporal(0), B.Temporal(0), B.Moments(0), B.Denoiser(0), B.Refine(0)
    dev = torch.device("cuda", 0)
    tparams = B.temporal_params(dict(max_history=WINDOW))
    ptr = lambda t: C.c_void_p(t.data_ptr())
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
            views.append((hits, prims, B.temporal_view(basis, be.get_share())))
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        packed, x, m, ln, e, out = f32(H, W, 4), f32(H, W, 4), f32(H, W, 4), f32(H, W), f32(H, W), f32(H, W, 4)
        frame = lambda seed: torch.from_numpy(np.random.default_rng(seed).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)

        def histories(commits):
            for t in (tx, tm):
                t.reset()
            for k in range(commits):
                f = frame(10 + k)
                tx.accumulate(f, 1, *views[0], params=tparams, commit=True, out=x, out_len=ln)
                tm.accumulate(mo.pack(f, 1, out=packed), 1, *views[0], params=tparams, commit=True, out=m)

        rgba = frame(3)
        hits, prims, view = views[1]

        def blend(t, src, dst, length):
            rc = t.L.gpuart_temporal_accumulate(t.h, ptr(src), C.c_uint32(1), ptr(hits), ptr(prims), C.c_uint32(W), C.c_uint32(H), C.byref(view),
                                                C.byref(tparams), C.c_int(0), ptr(dst), ptr(length) if length is not None else None)
            assert rc == 0, t.L.gpuart_temporal_last_error()

        def pack():
            assert mo.L.gpuart_moments_pack(mo.h, ptr(rgba), C.c_uint32(1), C.c_uint32(W), C.c_uint32(H), ptr(packed)) == 0

        def error():
            assert mo.L.gpuart_moments_error(mo.h, ptr(x), ptr(ln), ptr(m), ptr(hits), ptr(prims), C.c_uint32(0), C.c_float(LUM_FLOOR), C.c_uint32(W),
                                             C.c_uint32(H), None, ptr(e)) == 0

        def denoise(src):
            assert dn.L.gpuart_denoise_run(dn.h, ptr(src), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H), None, ptr(out)) == 0

        def refine(src):
            assert rf.L.gpuart_refine_run(rf.h, ptr(src), ptr(hits), ptr(prims), C.c_uint32(0), ptr(e), C.c_float(LUM_FLOOR), C.c_uint32(W), C.c_uint32(H),
                                          None, ptr(out)) == 0

        def guided_once():
            blend(tx, rgba, x, ln); tx.finish()
            pack(); mo.finish()
            blend(tm, packed, m, None); tm.finish()
            error(); mo.finish()
            refine(x); rf.finish()

        def preview_once():
            blend(tx, rgba, x, None); tx.finish()
            denoise(x); dn.finish()

        def timed(once, finish=None):
            def fn():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    once()
                if finish is not None:
                    finish()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        # the short history first: its error map's time, and the check of the entry points on inputs that take the window everywhere
        shares = {}
        results = {}
        for name, commits in (("short", 1), ("steady", 8)):
            histories(commits)
            guided_once()
            host = [t.cpu().numpy() for t in (x, ln, m, hits, prims)]
            assert (e.cpu().numpy().view(np.uint32) == mo.error(*host, LUM_FLOOR).view(np.uint32)).all(), "error: device and host entry points differ"
            assert (packed.cpu().numpy().view(np.uint32) == mo.pack(rgba.cpu().numpy(), 1).view(np.uint32)).all(), "pack: device and host entry points differ"
            surf = hits[..., 7].view(torch.int32) >= 0
            shares[name] = (float(surf.float().mean()), float(((ln * m[..., 2] >= 8) & surf).float().mean()))
            if name == "short":
                fn = timed(error, mo.finish)
                fn()
                results["error, short history"] = [fn() for _ in range(a.repeats)]
        methods = [("preview", timed(preview_once)), ("guided", timed(guided_once)), ("blend", timed(lambda: blend(tx, rgba, x, ln), tx.finish)),
                   ("pack", timed(pack, mo.finish)), ("error", timed(error, mo.finish)), ("denoise", timed(lambda: denoise(x), dn.finish)),
                   ("refine", timed(lambda: refine(x), rf.finish)), ("pack, a wait per call", timed(lambda: (pack(), mo.finish())))]
        for _, fn in methods:
            fn()
        for name, _ in methods:
            results[name] = []
        for _ in range(a.repeats):
            for name, fn in methods:
                results[name].append(fn())
        print("%dx%d: %.1f %% surface pixels; measured branch at %.1f %% of all pixels with the steady history, %.1f %% with the short one; "
              "%d calls per timing, %d repeats, alternating; ms per call: median (min .. max)"
              % (W, H, 100 * shares["steady"][0], 100 * shares["steady"][1], 100 * shares["short"][1], a.calls, a.repeats))
        med = {}
        for name in [n for n, _ in methods] + ["error, short history"]:
            v = np.array(results[name])
            med[name] = float(np.median(v))
            print("  %-22s %7.3f (%7.3f .. %7.3f)" % (name, med[name], v.min(), v.max()))
        parts = med["blend"] + med["pack"] + med["error"] + med["refine"] - med["denoise"]
        wait = med["pack, a wait per call"] - med["pack"]
        print("  guided - preview = %.3f ms; the parts: blend %.3f + pack %.3f + error %.3f + (refine - denoise) %.3f = %.3f ms; not in the parts: %.3f ms"
              % (med["guided"] - med["preview"], med["blend"], med["pack"], med["error"], med["refine"] - med["denoise"], parts,
                 med["guided"] - med["preview"] - parts))
        print("  a wait after a call, from pack with a wait per call less pack back to back: %.3f ms; guided has three more than preview: %.3f ms"
              % (wait, 3 * wait))
        # what error must move at the least: the record's second half and e for every pixel, the ordinal, the moments and len for a surface
        # pixel; the windows of the blocks that stage one come on top and are not counted
        surface = shares["steady"][0]
        bytes_error = 20.0 + 24.0 * surface
        print("  pack: %.0f GB/s of its 32 B per pixel; error: at least %.1f B per pixel (20 + 24 for a surface pixel; staged windows not counted): %.0f GB/s nominal"
              % (32.0 * W * H / med["pack"] / 1e6, bytes_error, bytes_error * W * H / med["error"] / 1e6))
    be.close()
    for h in (tx, tm, mo, dn, rf):
        h.close()


if __name__ == "__main__":
    main()
