"""What the firefly clamp buys the filtered frames, on the CPU: the oracle renders the protocol of tests/despeckle_cases.py (which states
it), the NumPy restatements clamp and filter (tests/despeckle_ref.py, tests/denoise_ref.py). No GPU is involved; the kernel equals the
restatement bit for bit (tests/test_despeckle.py) and the product's frames equal the oracle's, so these are the figures the GPU
reproduces.

Section 1: the four scenes at 1 / 4 / 16 / 64 paths with the library's defaults: the denoised frame's surface RMSE without and with the
clamp ahead of the denoiser, and the share of the surface pixels the clamp touched.
Section 2, the sweep: R = clamped-then-denoised / denoised surface RMSE, both against the 1024-path reference, for radius 1 / 2, rank
1..4 and k 1 / 2 / 4 (floor and min_count the defaults).

The rule, stated before the sweep was run. A setting's score is the geometric mean of R over the four scenes and the four path counts.
A setting is admissible if its worst R on the two scenes without a sphere is at most 1.02 (the clamp must not cost anything where
there is nothing to clamp). The defaults are the admissible setting with the best score.

Section 3: what tests/test_despeckle.py asserts with the shipped defaults: r on the firefly scene at 1 and 4 paths with the bound
r + (1 - r)/4, and R on the two scenes without a sphere at 1 and 64 paths against 1.02.
Section 4: the guided preview (tests/antilag_tracks.py `preview`, window 32) of 16 views of one path each from track `emissive`'s
fixed camera with the firefly scene's sphere: every view clamped before the chains, against the unclamped chain, at the last view.

    python tools/despeckle_quality.py      (its output is kept as section A of profiles/despeckle.txt)
"""
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import antilag_tracks as K  # noqa: E402
from tests import denoise_ref as D  # noqa: E402
from tests import despeckle_cases as P  # noqa: E402
from tests import despeckle_ref as DS  # noqa: E402
from tests import moments_ref as M  # noqa: E402
from tests import temporal_ref as T  # noqa: E402

RADIUS = (1, 2)
RANK = (1, 2, 3, 4)
KS = (1.0, 2.0, 4.0)
NO_SPHERE = ("scene_p", "box")


def main():
    t0 = time.time()
    print("protocol: %d x %d, camera x = %.2f, reference %d paths, frames of %s paths" % (P.W, P.H, P.CAMERA_X, P.REF_PATHS, P.PATHS))
    for name, (scene, us, em, flags) in P.SCENES.items():
        print("  %-16s %s, user sphere %s, emittance %g, flags %d" % (name, scene, us, em, flags))
    print("\n1. the defaults %s: denoised surface RMSE, no clamp -> clamp (clamped share of the surface pixels)" % (DS.DEFAULTS,))
    for name in P.SCENES:
        cells = []
        for paths in P.PATHS:
            e, s = P.clamped_error(name, paths)
            cells.append("%.4f -> %.4f (%.2f %%)" % (P.denoised_error(name, paths), e, 100.0 * s["clamped"] / s["surface"]))
        print("  %-16s %s" % (name, "   ".join(cells)))
    print("  (%.0f s)" % (time.time() - t0), flush=True)

    print("\n2. the sweep: R per scene at 1 / 4 / 16 / 64 paths, the score, the worst R without a sphere")
    settings = list(itertools.product(RADIUS, RANK, KS))
    ratios, score, worst = {}, {}, {}
    for s in settings:
        for name in P.SCENES:
            for paths in P.PATHS:
                ratios[s + (name, paths)] = P.ratio(name, paths, radius=s[0], rank=s[1], k=s[2])
        rs = [ratios[s + (name, paths)] for name in P.SCENES for paths in P.PATHS]
        score[s] = float(np.exp(np.mean(np.log(rs))))
        worst[s] = max(ratios[s + (name, paths)] for name in NO_SPHERE for paths in P.PATHS)
        print("  radius %d rank %d k %g: %s  score %.4f  worst %.4f%s"
              % (s + ("  ".join("%s %s" % (name, " ".join("%.3f" % ratios[s + (name, p)] for p in P.PATHS)) for name in P.SCENES), score[s], worst[s],
                      "" if worst[s] <= 1.02 else "  (not admissible)")), flush=True)
    ok = [s for s in settings if worst[s] <= 1.02]
    chosen = min(ok, key=lambda s: score[s])
    d = (DS.DEFAULTS["radius"], DS.DEFAULTS["rank"], DS.DEFAULTS["k"])
    print("\n%d of %d settings are admissible; chosen by the rule: radius %d, rank %d, k %g (score %.4f)" % ((len(ok), len(settings)) + chosen + (score[chosen],)))
    print("the library's defaults: radius %d, rank %d, k %g (score %.4f, worst %.4f)%s"
          % (d + (score[d], worst[d], "" if d == chosen else "  -- NOT the rule's choice")))

    print("\n3. what tests/test_despeckle.py asserts (the defaults)")
    for paths in (1, 4):
        r = ratios[d + ("scene_p_firefly", paths)]
        print("  scene_p_firefly, %2d paths: r = %.4f, the bound r + (1 - r)/4 = %.4f" % (paths, r, r + (1 - r) / 4))
    for name in NO_SPHERE:
        for paths in (1, 64):
            print("  %s, %2d paths: R = %.4f, the bound 1.02" % (name, paths, ratios[d + (name, paths)]))

    print("\n4. the guided preview, 16 views of one path, window 32, the firefly scene from the fixed camera, the defaults")
    name = "scene_p_firefly"
    scene, us, em, flags = P.SCENES[name]
    c = P.camera()
    words, prims = P.gbuffer(name)
    seeds = K.oracle().randseeds(K.N_CHANGE, seed=1234)
    views = [(K.render(scene, c, us, em, flags, seeds[i], 1), words, prims, T.view(c, T.full_frame(P.W, P.H), us, flags), flags) for i in range(K.N_CHANGE)]
    mask, ref = P.surface_mask(name), P.reference(name)
    errs = []
    for clamp in (False, True):
        images = [DS.clamp(v[0], words, prims, flags, **DS.DEFAULTS)[0] if clamp else v[0] for v in views]
        x = K.chain_of(images, views, K.WINDOW)
        m = K.chain_of([M.pack(img, 1) for img in images], views, K.WINDOW)
        i = len(views) - 1
        errs.append(K.rmse(K.preview(views[i], (x[i][0], x[i][1], m[i][0])), ref, mask))
    print("  surface RMSE of the last view's guided preview: %.5f unclamped, %.5f with every view clamped, ratio %.4f" % (errs[0], errs[1], errs[1] / errs[0]))
    print("\n(%.0f s in all)" % (time.time() - t0))


if __name__ == "__main__":
    main()
