"""What the history's measured variance is worth to the preview, on the CPU: the oracle renders two camera tracks, the NumPy
restatements blend (tests/temporal_ref.py), measure (tests/moments_ref.py) and filter (tests/refine_ref.py, tests/denoise_ref.py). No
GPU is involved; the kernels equal the restatements bit for bit (tests/test_moments.py), and the product's frames equal the oracle's,
so these are the figures the GPU reproduces.

The protocol: the box and scene P, 160 x 120, the Sun on, no user sphere, one path per pixel and view from one seed sequence
(O.randseeds(n, seed=1234)), every view committed. Track A is tools/temporal_quality.py's: 8 views, camera x = 0.10 + 0.05*i. Track B
has 24 views, x = 0.10 + 0.015*i. Every view has a reference of 256 paths (256 passes of one path, O.randseeds(256, seed=2)); the last
view of a track also one of 512 (O.randseeds(512, seed=2): the 256 are its first half). Errors are RMSE over the surface pixels.

"product" is today's Renderer::ReadPreview: the blend with the temporal defaults (max_history 4), then the denoiser with its defaults.
"guided" is Renderer::ReadGuidedPreview: the radiance and the packed moments blended with max_history mh, gpuart_moments_error with
(min_batches, spatial_k) and lum_floor 1/256, then the variance-guided filter with lum_k and its other defaults. Swept: mh 4, 8, 16,
32; min_batches 2, 4, 8; spatial_k 1, 2, 4; lum_k 1, 2.

The rules. (1) The defaults of gpuart_moments_defaults follow profiles/refine.txt's rule: the (min_batches, spatial_k) pair whose worst
ratio guided / product is smallest, the worst being over all views of both tracks and both scenes and over the four windows (a caller
may pick any), at lum_k 1. (2) The window recommended with the guided preview is the one with the smallest geometric mean of the four
last-view ratios against the 512-path references (two tracks, two scenes) for that pair at lum_k 1.

Printed last: what tests/test_moments.py asserts on track A with the recommended window and the defaults: per scene R = guided /
product at the last view against 512 paths, and the ratio at view 1 against its 256 paths.

    python tools/moments_quality.py      (its output is kept as section 1 of profiles/moments.txt)
"""
import itertools
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import denoise_ref as D  # noqa: E402
from tests import moments_ref as M  # noqa: E402
from tests import refine_ref as R  # noqa: E402
from tests import temporal_ref as T  # noqa: E402
from tests.util import scene  # noqa: E402

W, H = 160, 120
NT = min(16, os.cpu_count() or 1)
FLOOR = 1.0 / 256
TRACKS = {"A": [0.10 + 0.05 * i for i in range(8)], "B": [0.10 + 0.015 * i for i in range(24)]}
WINDOWS = (4.0, 8.0, 16.0, 32.0)
PAIRS = list(itertools.product((2.0, 4.0, 8.0), (1.0, 2.0, 4.0)))   # (min_batches, spatial_k)
LUM_KS = (1.0, 2.0)
PRIMS = np.zeros((H, W), np.int32)


def cam_of(x):
    cam = dict(S.DEFAULT_CAMERA, pos=(x, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def render(tree, c, seeds, also_at=None):
    """The mean of len(seeds) passes of one path; with also_at, (the mean of the first also_at, the mean of all)."""
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    acc = np.zeros((H, W, 4), np.float32)
    first = None
    for k, s in enumerate(seeds):
        O.pt_pass(tree, c, W, H, P, s, 1, acc, nthreads=NT)
        if k + 1 == also_at:
            first = acc / np.float32(also_at)
    full = acc / np.float32(len(seeds))
    return (first, full) if also_at else full


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


def chains(frames, gs, views, max_history):
    """Per view the blends (radiance, len, moments) of two histories that commit every view with the same parameters."""
    hx = hm = None
    out = []
    for f, g, c in zip(frames, gs, views):
        v = T.view(c, T.full_frame(W, H))
        kw = dict(T.DEFAULTS, max_history=max_history)
        x, ln, hx = T.accumulate(hx, f, 1, g, PRIMS, v, **kw)
        m, _, hm = T.accumulate(hm, M.pack(f, 1), 1, g, PRIMS, v, **kw)
        out.append((x, ln, m))
    return out


def view_job(job):
    """One view of one track: the product's errors and every guided setting's. -> (key, product, {(mh, mb, sk, lk): error})."""
    key, g, refs, blends = job
    mask = np.ascontiguousarray(g[..., 7]).view(np.int32) >= 0
    score = lambda img: tuple(rmse(img, r, mask) for r in refs)
    product = score(D.denoise(blends[4.0][0], g, PRIMS, 0))
    guided = {}
    for mh in WINDOWS:
        x, ln, m = blends[mh]
        for mb, sk in PAIRS:
            e = M.error(x, ln, m, g, PRIMS, FLOOR, 0, min_batches=mb, spatial_k=sk)
            for lk in LUM_KS:
                guided[(mh, mb, sk, lk)] = score(R.refine(x, g, PRIMS, e, FLOOR, 0, **dict(R.DEFAULTS, lum_k=lk)))
    return key, product, guided


def main():
    jobs = []
    for name in ("box", "scene_p"):
        tree = O.build_bvh(scene(name))[0]
        for track, xs in TRACKS.items():
            t0 = time.time()
            views = [cam_of(x) for x in xs]
            seeds = O.randseeds(len(xs), seed=1234)
            frames = [render(tree, v, seeds[i:i + 1]) for i, v in enumerate(views)]
            gs = [gbuffer(tree, v) for v in views]
            refs = [(render(tree, v, O.randseeds(256, seed=2)),) for v in views[:-1]]
            refs.append(render(tree, views[-1], O.randseeds(512, seed=2), also_at=256))
            per_window = {mh: chains(frames, gs, views, mh) for mh in WINDOWS}
            for i in range(len(xs)):
                jobs.append(((name, track, i), gs[i], refs[i], {mh: per_window[mh][i] for mh in WINDOWS}))
            print("%s, track %s: %d views, their references and blends in %.1f s" % (name, track, len(xs), time.time() - t0), flush=True)
    with multiprocessing.Pool(min(NT, len(jobs))) as pool:
        res = {key: (product, guided) for key, product, guided in pool.imap_unordered(view_job, jobs)}

    # ---- every setting's worst ratio over the views (256-path references) and its last-view ratios (512-path references)
    keys = sorted(res)
    last = [k for k in keys if k[2] == len(TRACKS[k[1]]) - 1]
    ratio = lambda k, s, ref=0: res[k][1][s][ref] / res[k][0][ref]
    print("\nper setting: the worst ratio guided / product over all %d views (256 paths), and the geometric mean of the last views'"
          " ratios (512 paths)" % len(keys))
    worst, gm = {}, {}
    for s in itertools.product(WINDOWS, PAIRS, LUM_KS):
        s = (s[0],) + s[1] + (s[2],)
        wk = max(keys, key=lambda k: ratio(k, s))
        worst[s] = ratio(wk, s)
        gm[s] = float(np.exp(np.mean([np.log(ratio(k, s, 1)) for k in last])))
        print("  max_history %2.0f min_batches %.0f spatial_k %.0f lum_k %.0f: worst %.4f (%s, track %s, view %d)  last views %.4f"
              % (s + (worst[s],) + wk + (gm[s],)))
    print("\nrule 1: per (min_batches, spatial_k) the worst ratio over the views and the four windows, lum_k 1")
    pair_worst = {p: max(worst[(mh,) + p + (1.0,)] for mh in WINDOWS) for p in PAIRS}
    for p in PAIRS:
        print("  min_batches %.0f spatial_k %.0f: %.4f" % (p + (pair_worst[p],)))
    best = min(PAIRS, key=lambda p: pair_worst[p])
    print("the pair whose worst ratio is smallest: min_batches %.0f spatial_k %.0f; the library's defaults: min_batches %.0f spatial_k %.0f"
          % (best + (M.DEFAULTS["min_batches"], M.DEFAULTS["spatial_k"])))
    print("\nrule 2: per window the geometric mean of the last views' ratios with that pair, lum_k 1")
    for mh in WINDOWS:
        print("  max_history %2.0f: %.4f" % (mh, gm[(mh,) + best + (1.0,)]))
    window = min(WINDOWS, key=lambda mh: gm[(mh,) + best + (1.0,)])
    print("the window recommended with the guided preview: max_history %.0f (gpuart_temporal_defaults stays %.0f)" % (window, T.DEFAULTS["max_history"]))

    d = (window, M.DEFAULTS["min_batches"], M.DEFAULTS["spatial_k"], R.DEFAULTS["lum_k"])
    print("\nwith max_history %.0f and the defaults (min_batches %.0f, spatial_k %.0f, lum_k %.0f): surface RMSE, product | guided | ratio" % d)
    for name in ("box", "scene_p"):
        for track, xs in TRACKS.items():
            for i in range(len(xs)):
                k = (name, track, i)
                print("  %s, track %s, view %2d (256 paths): %.5f | %.5f | %.4f" % (k + (res[k][0][0], res[k][1][d][0], ratio(k, d))))
            k = (name, track, len(xs) - 1)
            print("  %s, track %s, last view (512 paths): %.5f | %.5f | %.4f" % (name, track, res[k][0][1], res[k][1][d][1], ratio(k, d, 1)))
    print("\nwhat tests/test_moments.py asserts on track A (max_history %.0f, the defaults):" % window)
    for name in ("box", "scene_p"):
        r_last, r_1 = ratio((name, "A", 7), d, 1), ratio((name, "A", 1), d)
        print("  %s: R = %.4f at the last view (512 paths), the bound R + (1 - R)/4 = %.4f; at view 1 (256 paths) %.4f"
              % (name, r_last, r_last + (1 - r_last) / 4, r_1))


if __name__ == "__main__":
    main()
