#!/usr/bin/env python3
"""What adaptive sampling (Renderer::RenderAdaptive, include/gpuart_adaptive.h) is worth, on the CPU: the oracle renders the passes, the
NumPy restatement (tests/adaptive_ref.py) runs RenderAdaptive's loop on them. No GPU is involved; the kernels equal the restatement bit
for bit and the product's frames equal the oracle's (tests/test_adaptive.py), so these are the figures the GPU reproduces for the same
RandSeeds.

The protocol: the box and scene P, 160 x 120, the default camera, the Sun on, no user sphere, 256 one-path passes from
O.randseeds(256, seed=31) as the cap; batches of 4 and 16 paths; thresholds 0.05, 0.1 and 0.2; lum_floor 1/256; min_paths 8, 16, 32 and
64. The reference is 512 paths per pixel, 64 passes of 8 from O.randseeds(64, seed=977). Errors are RMSE over the surface pixels.

Printed per scene, batch size, threshold and min_paths: whether the loop converged, the paths issued, the paths per pixel (min, mean,
max over the blocks), paths_sum, the adaptive frame's RMSE, and the RMSE of the UNIFORM render of the same pass colours stopped at the
adaptive frame's mean paths per pixel, rounded up — the same work spent evenly. ratio = adaptive / uniform: below 1 the adaptive frame
is the better use of the paths.

Then the rule for the default min_paths (gpuart_cli --adaptive-min, GPUART_ADAPTIVE_DEFAULT_MIN_PATHS): the smallest candidate whose
worst ratio over the table is within 2 % of the best candidate's worst ratio — the estimate of a block with few paths is itself noisy,
and a block retired by a lucky estimate is never looked at again; a larger minimum protects against that and costs paths on the blocks
that were finished anyway. What the rule can and cannot decide: the ratio compares the whole frame's RMSE at equal work, and a larger
minimum spends paths on blocks that were finished anyway, so wherever early retirement does no visible harm the ratio rises with
min_paths and the rule takes the smallest candidate. It would pick a larger one only if blocks retired on a lucky estimate hurt the
frame's RMSE by more than 2 %; harm to a few blocks that the frame's RMSE averages away (a single noisy block, a seam) it cannot weigh.

    python tools/adaptive_quality.py [--write]      (--write: the output becomes section 1 of profiles/adaptive.txt, whose prose stays)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import adaptive_ref as AR  # noqa: E402
from tests.util import scene  # noqa: E402
from tools.profile_section import section  # noqa: E402

W, H = 160, 120
NT = min(16, os.cpu_count() or 1)
FLOOR = 1.0 / 256
CAP = 256
BATCHES = (4, 16)
THRESHOLDS = (0.05, 0.1, 0.2)
MIN_PATHS = (8, 16, 32, 64)
F = np.float32


def rmse(a, b, m):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d[m] ** 2).mean()))


INTRO = """The box and scene P, 160 x 120, the default camera, 256 one-path passes from O.randseeds(256, seed=31) as the cap, lum_floor 1/256, against
512 oracle paths of another seed; RMSE over the surface pixels. "uniform at ceil(mean)" is the uniform render of the same pass colours
stopped at the adaptive frame's mean paths per pixel, rounded up: the same work spent evenly. ratio = adaptive / uniform.
"""


def main():
    with section(os.path.join(ROOT, "profiles", "adaptive.txt") if "--write" in sys.argv[1:] else None, 1):
        print(INTRO)
        sweep()


def sweep():
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    nb = len(AR.block_pixels(H, W))
    pb = AR.pixel_blocks(H, W)
    table = {}   # (scene, batch, threshold, min_paths) -> ratio
    for name in ("box", "scene_p"):
        tree = O.build_bvh(scene(name))[0]
        t0 = time.time()
        ref = np.zeros((H, W, 4), F)
        for s in O.randseeds(64, seed=977):
            O.pt_pass(tree, c, W, H, P, s, 8, ref, nthreads=NT)
        ref /= F(512)
        rs, rd = O.cam_rays(c, W, H)
        o0, o1 = O.traverse(tree, rs.reshape(-1, 4), rd.reshape(-1, 4), None)
        mask = (np.floor(o1[:, 3]).astype(np.int32) >= 0).reshape(H, W)
        colours, uniform = [], [np.zeros((H, W, 4), F)]
        for s in O.randseeds(CAP, seed=31):
            a = np.zeros((H, W, 4), F)
            O.pt_pass(tree, c, W, H, P, s, 1, a, nthreads=NT)
            colours.append(a)
            uniform.append(uniform[-1] + a)
        print("%s: 512-path reference and %d pass colours in %.1f s; %d of %d pixels are surface pixels" % (name, CAP, time.time() - t0, int(mask.sum()), W * H), flush=True)
        print("  uniform RMSE at 8, 16, 32, 64, 128, 256 paths: %s" % "  ".join("%.5f" % rmse(uniform[n] / F(n), ref, mask) for n in (8, 16, 32, 64, 128, 256)))
        for b in BATCHES:
            for thr in THRESHOLDS:
                print("%s, batches of %d, threshold %g: min_paths | converged, issued | paths min / mean / max | paths_sum | RMSE adaptive, uniform at ceil(mean) | ratio" % (name, b, thr))
                for mp in MIN_PATHS:
                    rc, s, accum, counts, issued, active = AR.render_adaptive(AR.Estimator(), lambda k, n: colours[k], np.zeros((H, W, 4), F), np.zeros(nb, np.int64),
                                                                              0, CAP, 1, b, thr, mp, FLOOR)
                    mean = s["paths_sum"] / s["pixels"]
                    n_uni = int(np.ceil(mean))
                    ra = rmse(AR.normalize(accum, counts), ref, mask)
                    ru = rmse(uniform[n_uni] / F(n_uni), ref, mask)
                    table[(name, b, thr, mp)] = ra / ru
                    print("  %3d | %d, %3d | %3d / %6.2f / %3d | %8d | %.5f, %.5f (%d paths) | %.3f" % (
                        mp, rc, issued, s["paths_min"], mean, s["paths_max"], s["paths_sum"], ra, ru, n_uni, ra / ru), flush=True)
    print("\nthe worst ratio over the table (2 scenes x 2 batch sizes x 3 thresholds), per min_paths:")
    worst = {}
    for mp in MIN_PATHS:
        key = max((k for k in table if k[3] == mp), key=lambda k: table[k])
        worst[mp] = table[key]
        print("  min_paths %3d: %.3f  (%s, batches of %d, threshold %g)" % ((mp, table[key]) + key[:3]))
    best = min(worst.values())
    rule = min(mp for mp in MIN_PATHS if worst[mp] <= 1.02 * best)
    print("the rule: the smallest min_paths whose worst ratio is within 2 %% of the best (%.3f): %d" % (best, rule))
    if all(worst[a] <= worst[b] for a, b in zip(MIN_PATHS, MIN_PATHS[1:])):
        print("(the worst ratio rises with min_paths over the whole table: the rule had nothing to weigh and takes the smallest candidate;\n"
              " a block retired on a lucky estimate would have to cost the frame's RMSE more than 2 % to show here)")


if __name__ == "__main__":
    main()
