"""What the G-buffer-guided upscaler buys, on the CPU: the oracle renders and answers the camera rays, the NumPy restatements filter
(tests/denoise_ref.py) and upsample (tests/upscale_ref.py). No GPU is involved; the kernel equals the restatement bit for bit, and
gpuart_hip_gbuffer_scaled the G-buffer of the larger frame (tests/test_upscale.py), so these are the figures the GPU reproduces.

The box and scene P from the camera of tests/edges_protocol.py, rendered at 80 x 60 and shown at 160 x 120 (scale 2): one pass of 1, 4,
16 or 64 paths from O.randseeds(1, seed=1234), denoised with the denoiser's defaults. Three frames are measured against the protocol's
160 x 120 reference of 1024 paths, as RMSE over the surface pixels, and split into the protocol's edge pixels and the interior as
profiles/edges.txt splits them:
  (a) the upscaled frame (tests/upscale_ref.py upscale);
  (b) plain bilinear upsampling of the same low frame (tests/upscale_ref.py bilinear: the same taps and weights, no guidance);
  (c) a 160 x 120 render of a quarter of the paths per pixel - the same number of paths, so about the same tracing work - denoised.
      There is no quarter of one path: (c) has no entry at 1 path.

The sweep: normal_min 0.8 / 0.9 / 0.95 and plane_tol 0.01 / 0.02 / 0.05. The rule, stated before the sweep was run: a setting's score
is its worst (a)/(b) over the two scenes and the four path counts; the defaults are the setting with the smallest score, and among
settings within 1 % of it edge resolve's defaults (normal_min 0.95, plane_tol 0.02) if they are among them - one statement of "the
same surface" for both libraries - else the smallest score.

    python tools/upscale_quality.py [--out profiles/upscale.txt]      (section A of that file; tools/upscale_time.py appends section B)
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gpuart_amd import synth_scenes as S  # noqa: E402
from tests import antilag_tracks as K  # noqa: E402
from tests import denoise_ref as D  # noqa: E402
from tests import edges_protocol as P  # noqa: E402
from tests import upscale_ref as U  # noqa: E402

SCALE = 2
LW, LH = P.W // SCALE, P.H // SCALE
NORMAL_MIN = (0.8, 0.9, 0.95)
PLANE_TOL = (0.01, 0.02, 0.05)


def low_camera():
    cam = K.cam_of(P.CAMERA_X)
    return K.oracle().camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], LW, LH)


def low_frame(name, paths):
    O, c = K.oracle(), low_camera()
    Pm = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    acc = np.zeros((LH, LW, 4), np.float32)
    O.pt_pass(K.tree(name), c, LW, LH, Pm, O.randseeds(1, seed=1234)[0], paths, acc, nthreads=K.NT)
    return acc / np.float32(paths)


def low_gbuffer(name):
    O = K.oracle()
    rs, rd = O.cam_rays(low_camera(), LW, LH)
    o0, o1 = O.traverse(K.tree(name), rs.reshape(-1, 4), rd.reshape(-1, 4), None)
    words = np.concatenate([o0, o1], 1).astype(np.float32)
    words[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
    return words.reshape(LH, LW, 8), np.zeros((LH, LW), np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale.txt"))
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    t0 = time.time()
    say("A. tools/upscale_quality.py: the upscaler on the CPU oracle (the restatements; no GPU)")
    say("protocol: %s rendered at %d x %d, shown at %d x %d (scale %d), camera x = %.2f, reference %d paths at %d x %d, frames of %s paths"
        % (", ".join(P.SCENES), LW, LH, P.W, P.H, SCALE, P.CAMERA_X, P.REF_PATHS, P.W, P.H, P.PATHS))
    settings = list(itertools.product(NORMAL_MIN, PLANE_TOL))
    ratio = {}   # (setting, scene, paths) -> (a)/(b)
    rows = {}
    for name in P.SCENES:
        surf, edge, ref = P.surface_mask(name), P.edge_mask(name), P.reference(name)
        parts = (("surface", surf), ("edge", edge), ("interior", surf & ~edge))
        hw, hp = P.gbuffer(name)
        lw, lp = low_gbuffer(name)
        say("\n%s: %d surface pixels of %d, %.1f %% of them edge pixels" % (name, surf.sum(), surf.size, 100.0 * edge.sum() / surf.sum()))
        for paths in P.PATHS:
            den = D.denoise(low_frame(name, paths), lw, lp, 0, **D.DEFAULTS)
            plain = U.bilinear(den, SCALE)
            same_work = P.denoised(name, paths // 4) if paths >= 4 else None
            for nm, pt in settings:
                up, led = U.upscale(den, lw, lp, hw, hp, SCALE, 0, nm, pt, want_ledger=True)
                ratio[(nm, pt), name, paths] = P.rmse(up, ref, surf) / P.rmse(plain, ref, surf)
                if (nm, pt) == (U.DEFAULTS["normal_min"], U.DEFAULTS["plane_tol"]):
                    rows[name, paths] = (up, plain, same_work, led)
            up, plain, same_work, led = rows[name, paths]
            say("  %2d paths, the defaults: %.2f %% of the output pixels took the fallback, %.2f %% found no candidate"
                % (paths, 100.0 * (up[..., 0].size - led["weighted"]) / up[..., 0].size, 100.0 * led["fallback_none"] / up[..., 0].size))
            for what, mask in parts:
                ea, eb = P.rmse(up, ref, mask), P.rmse(plain, ref, mask)
                if same_work is None:
                    say("    %-8s RMSE (a) upscaled %.4f  (b) bilinear %.4f  (c) -       (a)/(b) %.3f" % (what, ea, eb, ea / eb))
                else:
                    ec = P.rmse(same_work, ref, mask)
                    say("    %-8s RMSE (a) upscaled %.4f  (b) bilinear %.4f  (c) %d paths at %d x %d %.4f   (a)/(b) %.3f  (a)/(c) %.3f%s"
                        % (what, ea, eb, paths // 4, P.W, P.H, ec, ea / eb, ea / ec, "   (c) wins" if ec < ea else ""))
        say("  (%.0f s)" % (time.time() - t0))

    say("\nthe sweep: (a)/(b) on the surface pixels per scene at 1 / 4 / 16 / 64 paths, and the score (the worst of them)")
    score = {}
    for s in settings:
        rs = [ratio[s, name, paths] for name in P.SCENES for paths in P.PATHS]
        score[s] = max(rs)
        say("  normal_min %.2f plane_tol %.2f: %s  score %.4f"
            % (s + ("  ".join("%s %s" % (name, " ".join("%.3f" % ratio[s, name, p] for p in P.PATHS)) for name in P.SCENES), score[s])))
    best = min(score.values())
    tied = [s for s in settings if score[s] <= 1.01 * best]
    d = (U.DEFAULTS["normal_min"], U.DEFAULTS["plane_tol"])
    shared = (0.95, 0.02)
    chosen = shared if shared in tied else min(tied, key=lambda s: score[s])
    say("\nbest score %.4f; within 1 %%: %s; chosen by the rule: normal_min %.2f, plane_tol %.2f (score %.4f)"
        % ((best, ", ".join("%.2f/%.2f" % s for s in tied)) + chosen + (score[chosen],)))
    say("the library's defaults: normal_min %.2f, plane_tol %.2f (score %.4f)%s" % (d + (score[d], "" if d == chosen else "  -- NOT the rule's choice")))
    say("(%.0f s in all)" % (time.time() - t0))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
