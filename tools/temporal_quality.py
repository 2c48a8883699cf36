"""What the temporal history is worth, on the CPU: the oracle renders a camera track, the two NumPy restatements (tests/temporal_ref.py,
tests/denoise_ref.py) accumulate and filter it. No GPU is involved; the kernels equal the restatements bit for bit (tests/test_temporal.py),
and the product's frames equal the oracle's, so these are the figures the GPU reproduces.

The track is the one tests/test_temporal.py::test_history_helps_the_preview renders: eight views, camera x = 0.10, 0.15 ... 0.45 (looking
at (0, 0, 0.95) like the default camera), one path per pixel each from one seed sequence (seed 1234), 160 x 120, the Sun on, no user
sphere; the reference is 512 paths per pixel at the last view from another seed (2), rendered as 512 passes of one path. Errors are
RMSE over the surface pixels of the last view. How much the reference's own noise matters is shown at the end: the same ratios against
a reference of 8 passes of 64 paths from the same seed.

Printed: per view raw / spatial filter / history / history + spatial filter with the defaults; the sweep of max_history, plane_tol and
normal_min at the last view; what the rule picks; the ratios and bounds the test asserts.

The rule by which the defaults were chosen. The figure of merit is the product's: the geometric mean over the two scenes of
(history + spatial) / (spatial alone), since Renderer::ReadPreview always filters the blend. Among the windows (max_history) whose best
figure is within 2 % of the best of all, the longest is taken: a track of eight views cannot reward a window longer than eight, and the
blend itself — what a caller sees who filters differently or not at all — keeps improving with the window. Within that window the
figures of the plane_tol / normal_min pairs lie within 0.6 % of each other, which two scenes cannot resolve, except that normal_min 0.9
is consistently the worst on scene P (curved surfaces); so the strictest pair that is not the worst is taken: plane_tol 0.01,
normal_min 0.8.

    python tools/temporal_quality.py > profiles/temporal_quality.txt
"""
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import denoise_ref as R  # noqa: E402
from tests import temporal_ref as T  # noqa: E402
from tests.util import scene  # noqa: E402

W, H = 160, 120
NT = min(16, os.cpu_count() or 1)
XS = [0.10 + 0.05 * i for i in range(8)]


def cam_of(x):
    cam = dict(S.DEFAULT_CAMERA, pos=(x, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def render(tree, c, seeds):
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, 1, acc, nthreads=NT)
    return acc / np.float32(len(seeds))


def gbuffer(tree, c):
    """(H, W, 8) record words of the camera rays' closest hits, as gpuart_hip_gbuffer lays them out."""
    rs, rd = O.cam_rays(c, W, H)
    o0, o1 = O.traverse(tree, rs.reshape(-1, 4), rd.reshape(-1, 4), None)
    words = np.concatenate([o0, o1], 1).astype(np.float32)
    words[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
    return words.reshape(H, W, 8)


def rmse(a, b, m):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d[m] ** 2).mean()))


def chain(frames, gs, views, **params):
    """The blends of the track, every view committed."""
    hist, outs = None, []
    prims = np.zeros((H, W), np.int32)
    for f, g, c in zip(frames, gs, views):
        out, ln, hist = T.accumulate(hist, f, 1, g, prims, T.view(c, T.full_frame(W, H)), **params)
        outs.append((out, ln))
    return outs


def main():
    prims = np.zeros((H, W), np.int32)
    data, other_ref = {}, {}
    for name in ("box", "scene_p"):
        tree = O.build_bvh(scene(name))[0]
        views = [cam_of(x) for x in XS]
        t0 = time.time()
        ref = render(tree, views[-1], O.randseeds(512, seed=2))
        print("%s: 512-path reference in %.1f s" % (name, time.time() - t0))
        seeds = O.randseeds(len(XS), seed=1234)
        frames = [render(tree, v, seeds[i:i + 1]) for i, v in enumerate(views)]
        gs = [gbuffer(tree, v) for v in views]
        mask = np.ascontiguousarray(gs[-1][..., 7]).view(np.int32) >= 0
        raw = rmse(frames[-1], ref, mask)
        sp = rmse(R.denoise(frames[-1], gs[-1], prims, 0), ref, mask)
        ref2 = np.zeros((H, W, 4), np.float32)
        P = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(views[-1][12]),
                          views[-1][0:3], 5, 0.01)
        for s in O.randseeds(8, seed=2):
            O.pt_pass(tree, views[-1], W, H, P, s, 64, ref2, nthreads=NT)
        other_ref[name] = ref2 / np.float32(512)
        data[name] = (frames, gs, views, ref, mask, raw, sp)
        print("%s: last view, surface RMSE raw %.5f, spatial filter %.5f (%.3fx raw)" % (name, raw, sp, sp / raw))

    print("\nsweep at the last view: history / raw, (history + spatial) / spatial, mean length; box | scene_p | geometric mean")
    results = {}
    for mh, tol, nmin in itertools.product((2.0, 4.0, 8.0, 16.0, 32.0), (0.005, 0.01, 0.02, 0.05), (0.5, 0.8, 0.9)):
        row = []
        for name in ("box", "scene_p"):
            frames, gs, views, ref, mask, raw, sp = data[name]
            out, ln = chain(frames, gs, views, max_history=mh, plane_tol=tol, normal_min=nmin)[-1]
            t = rmse(out, ref, mask)
            ts = rmse(R.denoise(out, gs[-1], prims, 0), ref, mask)
            row.append((t / raw, ts / sp, float(ln[mask].mean())))
        gm = float(np.sqrt(row[0][1] * row[1][1]))
        results[(mh, tol, nmin)] = (row, gm)
        print("  max_history %4.0f plane_tol %.3f normal_min %.1f: %.3f %.3f %5.2f | %.3f %.3f %5.2f | %.4f"
              % ((mh, tol, nmin) + row[0] + row[1] + (gm,)))
    best = min(results, key=lambda k: results[k][1])
    print("\nthe best figure: max_history %.0f plane_tol %.3f normal_min %.1f (geometric mean %.4f)" % (best + (results[best][1],)))
    per_window = {}
    for (mh, tol, nmin), (_, gm) in results.items():
        per_window[mh] = min(per_window.get(mh, 9.0), gm)
    print("best figure per window: " + ", ".join("%.0f: %.4f" % kv for kv in sorted(per_window.items())))
    window = max(mh for mh, gm in per_window.items() if gm <= 1.02 * results[best][1])
    print("the longest window within 2 %% of the best: max_history %.0f" % window)
    d = (T.DEFAULTS["max_history"], T.DEFAULTS["plane_tol"], T.DEFAULTS["normal_min"])
    print("the defaults:    max_history %.0f plane_tol %.3f normal_min %.1f (geometric mean %.4f)" % (d + (results[d][1],)))

    print("\nthe defaults, view by view: mean length and share of the surface pixels that found history; then the last view's errors")
    for name in ("box", "scene_p"):
        frames, gs, views, ref, mask, raw, sp = data[name]
        outs = chain(frames, gs, views, **T.DEFAULTS)
        for i, (out, ln) in enumerate(outs):
            m = np.ascontiguousarray(gs[i][..., 7]).view(np.int32) >= 0
            print("  %s view %d (x = %.2f): mean length %.2f, found history %.4f" % (name, i, XS[i], float(ln[m].mean()), float((ln[m] > 1).mean())))
        out, ln = outs[-1]
        t = rmse(out, ref, mask)
        ts = rmse(R.denoise(out, gs[-1], prims, 0), ref, mask)
        ratio = ts / sp
        print("  %s last view: raw %.5f spatial %.5f history %.5f (%.3fx raw) history + spatial %.5f" % (name, raw, sp, t, t / raw, ts))
        print("  %s: (history + spatial) / spatial = %.4f; the test's bound = ratio + (1 - ratio)/4 = %.4f" % (name, ratio, ratio + (1 - ratio) / 4))
        ref2 = other_ref[name]
        print("  %s: against a reference of 8 passes of 64 paths (same seed; RMSE between the two references %.5f): %.4f"
              % (name, rmse(ref, ref2, mask), rmse(R.denoise(out, gs[-1], prims, 0), ref2, mask) / rmse(R.denoise(frames[-1], gs[-1], prims, 0), ref2, mask)))


if __name__ == "__main__":
    main()
