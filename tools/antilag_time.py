#!/usr/bin/env python3
"""Time of Renderer::ReadGuidedPreview's device sequence with anti-lag on beside the same with it off, without the read-back, in one
process on the same inputs, after tools/moments_time.py's protocol: 1920x1080 and 3840x2160, cfg3's scene (Scene D) after a sideways
camera move of 0.1, the G-buffers of gpuart_hip_gbuffer and seeded random radiance; inputs, histories and outputs resident on the GPU.

   python3 tools/antilag_time.py [--repeats R] [--calls K]

The histories: view A committed eight times at one path each to three temporal handles (the radiance with max_history 32, the packed
moments with 32, the radiance again with fast_history 4); then view B is previewed. Where B's pixels find history B is 9 and fast_len
is 5: they vote, and every block that holds one sums its windows. "short" is the same after a single commit: no pixel has 8 batches,
nobody votes, and every block writes the slow blend through.

Per frame size, K back-to-back calls between two synchronisations, host clock around them; every method runs once untimed first, then R
timed repeats with the methods alternating; printed are the median, the minimum and the maximum:
  off       blend with out_len, wait, pack, wait, blend of the moments, wait, error, wait, variance-guided filter, wait
  on        the same with the fast blend (with out_len), wait, and mix in place, wait, before error
  blend     one gpuart_temporal_accumulate (commit 0) of the fast history alone
  mix       gpuart_antilag_mix alone, into separate buffers; in place (with the copy of slow and slow_len); and with the short history
Before timing, mix is checked against its host entry point."""
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
    tx, tm, tf, mo, al, rf = B.Temporal(0), B.Temporal(0), B.Temporal(0), B.Moments(0), B.AntiLag(0), B.Refine(0)
    dev = torch.device("cuda", 0)
    tparams = B.temporal_params(dict(max_history=WINDOW))
    fparams = B.temporal_params(dict(max_history=B.ANTILAG_DEFAULTS["fast_history"]))
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
        fx, fl, alpha, mixed, mixed_len = f32(H, W, 4), f32(H, W), f32(H, W), f32(H, W, 4), f32(H, W)
        frame = lambda seed: torch.from_numpy(np.random.default_rng(seed).uniform(0, 2, (H, W, 4)).astype(np.float32)).to(dev)

        def histories(commits):
            for t in (tx, tm, tf):
                t.reset()
            for k in range(commits):
                f = frame(10 + k)
                tx.accumulate(f, 1, *views[0], params=tparams, commit=True, out=x, out_len=ln)
                tm.accumulate(mo.pack(f, 1, out=packed), 1, *views[0], params=tparams, commit=True, out=m)
                tf.accumulate(f, 1, *views[0], params=fparams, commit=True, out=fx, out_len=fl)

        rgba = frame(3)
        hits, prims, view = views[1]

        def blend(t, src, dst, length, params=tparams):
            rc = t.L.gpuart_temporal_accumulate(t.h, ptr(src), C.c_uint32(1), ptr(hits), ptr(prims), C.c_uint32(W), C.c_uint32(H), C.byref(view),
                                                C.byref(params), C.c_int(0), ptr(dst), ptr(length) if length is not None else None)
            assert rc == 0, t.L.gpuart_temporal_last_error()

        def pack():
            assert mo.L.gpuart_moments_pack(mo.h, ptr(rgba), C.c_uint32(1), C.c_uint32(W), C.c_uint32(H), ptr(packed)) == 0

        def error(src, length):
            assert mo.L.gpuart_moments_error(mo.h, ptr(src), ptr(length), ptr(m), ptr(hits), ptr(prims), C.c_uint32(0), C.c_float(LUM_FLOOR),
                                             C.c_uint32(W), C.c_uint32(H), None, ptr(e)) == 0

        def refine(src):
            assert rf.L.gpuart_refine_run(rf.h, ptr(src), ptr(hits), ptr(prims), C.c_uint32(0), ptr(e), C.c_float(LUM_FLOOR), C.c_uint32(W), C.c_uint32(H),
                                          None, ptr(out)) == 0

        def mix(dst, dst_len):
            rc = al.L.gpuart_antilag_mix(al.h, ptr(x), ptr(ln), ptr(fx), ptr(fl), ptr(m), ptr(hits), ptr(prims), C.c_uint32(0), C.c_uint32(W), C.c_uint32(H),
                                         None, ptr(dst), ptr(dst_len), ptr(alpha))
            assert rc == 0, al.L.gpuart_antilag_last_error()

        def off_once():
            blend(tx, rgba, x, ln); tx.finish()
            pack(); mo.finish()
            blend(tm, packed, m, None); tm.finish()
            error(x, ln); mo.finish()
            refine(x); rf.finish()

        def on_once():
            blend(tx, rgba, x, ln); tx.finish()
            pack(); mo.finish()
            blend(tm, packed, m, None); tm.finish()
            blend(tf, rgba, fx, fl, fparams); tf.finish()
            mix(x, ln); al.finish()
            error(x, ln); mo.finish()
            refine(x); rf.finish()

        def timed(once, finish=None):
            def fn():
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    once()
                if finish is not None:
                    finish()
                return (time.perf_counter() - t0) * 1e3 / a.calls
            return fn

        shares = {}
        results = {}
        for name, commits in (("short", 1), ("steady", 8)):
            histories(commits)
            off_once()
            blend(tf, rgba, fx, fl, fparams); tf.finish()
            mix(mixed, mixed_len); al.finish()
            host = [t.cpu().numpy() for t in (x, ln, fx, fl, m, hits, prims)]
            for got, exp in zip((mixed, mixed_len, alpha), al.mix(*host)):
                assert (got.cpu().numpy().view(np.uint32) == exp.view(np.uint32)).all(), "mix: device and host entry points differ"
            surf = hits[..., 7].view(torch.int32) >= 0
            shares[name] = (float(surf.float().mean()), float(((ln * m[..., 2] >= 8) & (fl < ln) & surf).float().mean()), float((alpha > 0).float().mean()))
            if name == "short":
                fn = timed(lambda: mix(mixed, mixed_len), al.finish)
                fn()
                results["mix, short history"] = [fn() for _ in range(a.repeats)]
        # (mix follows off: it sees the slow blend, not what on's mix in place left in its stead)
        methods = [("off", timed(off_once)), ("mix", timed(lambda: mix(mixed, mixed_len), al.finish)),
                   ("blend", timed(lambda: blend(tf, rgba, fx, fl, fparams), tf.finish)), ("on", timed(on_once))]
        for _, fn in methods:
            fn()
        for name, _ in methods:
            results[name] = []
        for _ in range(a.repeats):
            for name, fn in methods:
                results[name].append(fn())
        # mix in place: single calls with the host clock around call and wait, the slow blend restored before each, outside the clock
        blend(tx, rgba, x, ln); tx.finish()
        x0, ln0 = x.clone(), ln.clone()
        results["mix, in place"] = []
        for _ in range(a.repeats + 1):
            x.copy_(x0); ln.copy_(ln0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mix(x, ln); al.finish()
            results["mix, in place"].append((time.perf_counter() - t0) * 1e3)
        results["mix, in place"] = results["mix, in place"][1:]
        print("%dx%d: %.1f %% surface pixels; voting pixels %.1f %% of all with the steady history (alpha > 0 at %.2f %%), %.1f %% with the short one; "
              "%d calls per timing, %d repeats, alternating; ms per call: median (min .. max)"
              % (W, H, 100 * shares["steady"][0], 100 * shares["steady"][1], 100 * shares["steady"][2], 100 * shares["short"][1], a.calls, a.repeats))
        med = {}
        for name in ["off", "on", "blend", "mix", "mix, short history", "mix, in place"]:
            v = np.array(results[name])
            med[name] = float(np.median(v))
            print("  %-22s %7.3f (%7.3f .. %7.3f)%s" % (name, med[name], v.min(), v.max(), "   (single calls, each with its wait)" if name == "mix, in place" else ""))
        print("  on - off = %.3f ms; the parts: blend %.3f + mix %.3f = %.3f ms; not in the parts (two waits, the in-place copy): %.3f ms"
              % (med["on"] - med["off"], med["blend"], med["mix"], med["blend"] + med["mix"], med["on"] - med["off"] - med["blend"] - med["mix"]))
        # what mix must move at the least: slow, slow_len, the record's second half, out, out_len and alpha for every pixel (60 B), the
        # ordinal, the moments, fast and fast_len for a surface pixel (40 B); the aprons come on top and are not counted
        surface = shares["steady"][0]
        b = 60.0 + 40.0 * surface
        print("  mix: at least %.1f B per pixel (60 + 40 for a surface pixel; aprons not counted): %.0f GB/s nominal" % (b, b * W * H / med["mix"] / 1e6))
    be.close()
    for h in (tx, tm, tf, mo, al, rf):
        h.close()


if __name__ == "__main__":
    main()
