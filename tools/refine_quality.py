"""What the variance-guided filter (include/gpuart_refine.h) is worth, on the CPU: the oracle renders in batches, the NumPy restatements
estimate the error (tests/converge_ref.py) and filter (tests/refine_ref.py, tests/denoise_ref.py). No GPU is involved; the kernels equal
the restatements bit for bit (tests/test_refine.py), and the product's frames equal the oracle's, so these are the figures the GPU
reproduces for the same RandSeeds.

The protocol: the box and scene P, 160 x 120, the default camera, the Sun on, no user sphere. 16 batches of 1, 4 and 16 paths per
pixel, RandSeeds O.randseeds(16, seed=31), the estimator shown the accumulator after every batch; after 2, 4, 8 and 16 batches the
frame is filtered with the error map of that moment (lum_floor 1/256). The reference is 512 paths per pixel, 64 passes of 8 from
O.randseeds(64, seed=977). Errors are RMSE over the surface pixels; the residual noise of the reference pushes the ratios of the
well-sampled frames towards 1.

Printed: per scene, batch size and path count the raw RMSE, and relative to it the denoiser with its defaults (dn) and this filter
with lum_k 1, 2, 3 and 4 and, for comparison, without the 3x3 variance prefilter (a variant only the restatement has). Then the rule:
the default lum_k is the value whose worst ratio over the whole table is smallest. Then the bound B that
tests/test_refine.py::test_refining_never_hurts asserts at 8 paths: half-way between the ratio measured here for batches of 4 paths and 1,
since the product draws other RandSeeds than the oracle.

    python tools/refine_quality.py > profiles/refine_quality.txt      (its output is section 1 of profiles/refine.txt)
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import converge_ref  # noqa: E402
from tests import denoise_ref as D  # noqa: E402
from tests import refine_ref as R  # noqa: E402
from tests.util import scene  # noqa: E402

W, H = 160, 120
NT = min(16, os.cpu_count() or 1)
FLOOR = 1.0 / 256
LUM_KS = (1.0, 2.0, 3.0, 4.0)
BATCHES = (1, 4, 16)
POINTS = (2, 4, 8, 16)   # batches after which the frame is filtered


def camera():
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


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


def main():
    c = camera()
    prims = np.zeros((H, W), np.int32)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    cols = ["dn"] + ["k=%g" % k for k in LUM_KS] + ["k=%g, no prefilter" % k for k in LUM_KS]
    table = {}   # (scene, batch, paths) -> ratios in the order of cols
    for name in ("box", "scene_p"):
        tree = O.build_bvh(scene(name))[0]
        t0 = time.time()
        ref = np.zeros((H, W, 4), np.float32)
        for s in O.randseeds(64, seed=977):
            O.pt_pass(tree, c, W, H, P, s, 8, ref, nthreads=NT)
        ref /= np.float32(512)
        print("%s: 512-path reference in %.1f s" % (name, time.time() - t0), flush=True)
        words = gbuffer(tree, c)
        mask = np.ascontiguousarray(words[..., 7]).view(np.int32) >= 0
        for b in BATCHES:
            est = converge_ref.Estimator()
            acc = np.zeros((H, W, 4), np.float32)
            print("%s, 16 batches of %d path%s: paths, raw RMSE, then RMSE / raw: %s" % (name, b, "s" if b > 1 else "", " | ".join(cols)))
            for k, s in enumerate(O.randseeds(16, seed=31)):
                O.pt_pass(tree, c, W, H, P, s, b, acc, nthreads=NT)
                total = (k + 1) * b
                est.update(acc, total)
                if k + 1 not in POINTS:
                    continue
                frame = acc / np.float32(total)
                e = est.error(FLOOR)
                raw = rmse(frame, ref, mask)
                row = [rmse(D.denoise(frame, words, prims, 0), ref, mask) / raw]
                for pf in (True, False):
                    for lk in LUM_KS:
                        row.append(rmse(R.refine(frame, words, prims, e, FLOOR, 0, **dict(R.DEFAULTS, lum_k=lk), prefilter=pf), ref, mask) / raw)
                table[(name, b, total)] = row
                print("  %4d  %.5f   %s" % (total, raw, "  ".join("%.3f" % v for v in row)), flush=True)
    print("\nthe worst ratio over the table (2 scenes x 3 batch sizes x 4 path counts), per column:")
    worst = {}
    for j, col in enumerate(cols):
        key = max(table, key=lambda q: table[q][j])
        worst[col] = table[key][j]
        print("  %-20s %.3f  (%s, batches of %d, %d paths)" % ((col, table[key][j]) + key))
    best = min(LUM_KS, key=lambda k: worst["k=%g" % k])
    print("the rule: the lum_k whose worst ratio is smallest: %g; the library's default: %g" % (best, R.DEFAULTS["lum_k"]))
    print("\nthe bound B of tests/test_refine.py at 8 paths (batches of 4 paths, lum_k %g): B = (measured ratio + 1) / 2" % R.DEFAULTS["lum_k"])
    j = cols.index("k=%g" % R.DEFAULTS["lum_k"])
    for name in ("box", "scene_p"):
        m = table[(name, 4, 8)][j]
        print("  %s: measured %.3f, B = %.3f" % (name, m, (m + 1) / 2))


if __name__ == "__main__":
    main()
