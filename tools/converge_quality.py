#!/usr/bin/env python3
"""What the convergence estimate (include/gpuart_converge.h) means on real, heavy-tailed paths: calibration against a reference render.

   python3 tools/converge_quality.py [--threads N]

The box scene and scene P at 160x120, the default camera, the Sun on: 16 batches of 4 one-path passes through the Renderer, the raw
accumulator shown to the estimator after each. Against the mean luminance of a 512-path render of the CPU oracle with other RandSeeds,
per pixel z = |mean - reference| / se, se = sqrt(m2 / (batches - 1) / total): the share of pixels with a spread (se > 0) within 1 and
within 2 standard errors (a Gaussian mean would give 68.3 % and 95.4 %; the reference's own error, 1/8 of the estimate's variance, is
not taken out), and how the frame's `above` count falls as batches are added, for three thresholds. Nothing is asserted."""
import argparse
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

W, H, BATCHES, PER, REF_PATHS = 160, 120, 16, 4, 512
THRESHOLDS = (0.2, 0.1, 0.05)
FLOOR = 1.0 / 256


def lum(a):
    a = a.astype(np.float64)
    return 0.2126 * a[..., 0] + 0.7152 * a[..., 1] + 0.0722 * a[..., 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    cv = B.Converge(0)
    for name, descs in (("box", S.box_scene()), ("scene_p", S.scene_p())):
        tree, _ = O.build_bvh(descs)
        ref = np.zeros((H, W, 4), np.float32)
        for sd in O.randseeds(REF_PATHS // 8, seed=977):
            O.pt_pass(tree, c, W, H, P, sd, 8, ref, nthreads=a.threads)
        ref_l = lum(ref) / REF_PATHS
        r = B.Renderer(W, H, cam)
        r.set_primitives(B.make_prims(descs))
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.restart_path_tracing(1, BATCHES * PER)
        cv.reset()
        print("%s %dx%d, %d batches of %d paths; reference: %d oracle paths per pixel" % (name, W, H, BATCHES, PER, REF_PATHS))
        print("  batch paths  " + "  ".join("above(%.2f)" % t for t in THRESHOLDS) + "  max_error  within 1 se  within 2 se")
        for k in range(BATCHES):
            for _ in range(PER):
                r.path_tracing_pass()
            total = PER * (k + 1)
            cv.update(r.read_radiance(False), total)
            if k == 0:
                continue
            sums = [cv.measure(t, FLOOR) for t in THRESHOLDS]
            st = cv.state().astype(np.float64)
            se = np.sqrt(np.maximum(st[..., 1], 0) / k / total)
            spread = se > 0
            z = np.abs(st[..., 0] - ref_l)[spread] / se[spread]
            print("  %5d %5d  %s  %9.4f  %10.1f %%  %10.1f %%" % (k + 1, total, "  ".join("%11d" % s["above"] for s in sums), sums[0]["max_error"],
                                                              100 * (z <= 1).mean(), 100 * (z <= 2).mean()))
        print("  %d of %d pixels have a spread; non-finite: %d" % (int(spread.sum()), W * H, sums[0]["non_finite"]))
        r.close()
    cv.close()


if __name__ == "__main__":
    main()
