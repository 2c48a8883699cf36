"""What resolving geometric edges from a sub-pixel G-buffer buys the filtered frames, on the CPU: the oracle renders the protocol of
tests/edges_protocol.py (which states it) and answers the sub-pixel rays, the NumPy restatements filter and resolve
(tests/denoise_ref.py, tests/edges_ref.py). No GPU is involved; the kernels equal the restatements bit for bit (tests/test_edges.py)
and the product's frames equal the oracle's, so these are the figures the GPU reproduces.

Section 1, the bias: how much of the denoised frame's squared error the measurement's edge pixels hold at 1, 4, 16 and 64 paths.
Section 2, the sweep on ReadDenoised's chain: R = surface RMSE of the resolved frame / surface RMSE of the denoised frame, both against
the 1024-path reference, for n_sub 4 / 8 / 16, four offset tables — the header's rotated grid (RGSS for 4, the lattices k*3 mod 8 and k*7 mod 16), stratified
cell centres (2x2, 4x2, 4x4), the prototype's pseudo-random set (O.random of O.randseeds(n_sub, seed=77)) and the prefixes of the
Halton points of bases 2 and 3 (the header's table before the first run of this tool, which chose the rotated grid) —, normal_min 0.8 / 0.9 / 0.95 and plane_tol 0.01 / 0.02 / 0.05.

The rule, stated before the sweep was run. A setting's score is the geometric mean of R over the two scenes and the four path counts.
Among the settings within 2 % of the best score the defaults are: the smallest n_sub (the cost is n_sub rays per edge pixel); among
those the header's table if one of them uses it, else the best-scoring table; among those
the best score.

Section 3: what tests/test_edges.py asserts with the shipped defaults, r at 1 and 16 paths per scene and the bound r + (1 - r)/4.
Section 4: the same resolve on the guided preview (tests/antilag_tracks.py `preview`, window 32) of track B's last view, against a
1024-path reference of that view.
Section 5, not shipped (out of scope): what taking the edge pixels out of the à-trous levels' sources would buy — the denoiser with
the mark's edge pixels masked out as sources is not expressible through the library's interface, so the figure is the surface RMSE of
the interior alone, before and after, which bounds what cleaner sources could give the interior.

    python tools/edges_quality.py      (its output is kept as section A of profiles/edges.txt)
"""
import itertools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import antilag_tracks as K  # noqa: E402
from tests import edges_protocol as P  # noqa: E402
from tests import edges_ref as E  # noqa: E402

N_SUB = (4, 8, 16)
NORMAL_MIN = (0.8, 0.9, 0.95)
PLANE_TOL = (0.01, 0.02, 0.05)
TABLES = ("rotated", "stratified", "random", "halton")


def table(kind, n):
    if kind == "rotated":
        return E.offsets(n)
    if kind == "halton":
        radical = lambda i, b: sum(int(d) * float(b) ** -(j + 1) for j, d in enumerate(reversed(np.base_repr(i, b))))
        return np.array([[radical(i, 2), radical(i, 3)] for i in range(1, n + 1)], np.float32)
    if kind == "stratified":
        nx, ny = {4: (2, 2), 8: (4, 2), 16: (4, 4)}[n]
        return np.array([[(i + 0.5) / nx, (j + 0.5) / ny] for j in range(ny) for i in range(nx)], np.float32)
    O = K.oracle()
    seeds = O.randseeds(n, seed=77)
    x, y = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    x[:, 0], y[:, 0] = seeds[:, 0], seeds[:, 1]
    return np.stack([O.random(x)[:, 0], O.random(y)[:, 0]], 1).astype(np.float32)


def main():
    t0 = time.time()
    all_pixels = np.arange(P.W * P.H)
    print("protocol: %s at %d x %d, camera x = %.2f, reference %d paths, frames of %s paths" % (", ".join(P.SCENES), P.W, P.H, P.CAMERA_X, P.REF_PATHS, P.PATHS))
    print("\n1. the bias: the measurement's edge pixels in the denoised frame")
    for name in P.SCENES:
        surf, edge = P.surface_mask(name), P.edge_mask(name)
        ref = P.reference(name)
        print("  %s: edge pixels are %.1f %% of the %d surface pixels" % (name, 100.0 * edge.sum() / surf.sum(), surf.sum()))
        for paths in P.PATHS:
            d = P.denoised(name, paths)
            se = ((d[..., :3].astype(np.float64) - ref[..., :3]) ** 2).sum(-1)
            print("    %2d paths: surface RMSE %.4f, edge %.4f, interior %.4f; the edge pixels hold %.0f %% of the squared error"
                  % (paths, P.rmse(d, ref, surf), P.rmse(d, ref, edge), P.rmse(d, ref, surf & ~edge), 100.0 * se[edge].sum() / se[surf].sum()))
    print("  (%.0f s)" % (time.time() - t0), flush=True)

    # every pixel's sub-pixel records per (scene, table, n_sub): a setting's list selects from them
    ratios = {}
    for name in P.SCENES:
        words, prims = P.gbuffer(name)
        surf, ref = P.surface_mask(name), P.reference(name)
        base = {paths: P.rmse(P.denoised(name, paths), ref, surf) for paths in P.PATHS}
        lists = {(nm, pt): E.mark(words, prims, 0, nm, pt) for nm, pt in itertools.product(NORMAL_MIN, PLANE_TOL)}
        for kind, n in itertools.product(TABLES, N_SUB):
            sw, sp = P.subpixel_records(name, all_pixels, table(kind, n))
            for (nm, pt), lst in lists.items():
                for paths in P.PATHS:
                    out = E.resolve(P.denoised(name, paths), words, prims, lst, sw[:, lst], sp[:, lst], 0, n, nm, pt)
                    ratios[(n, kind, nm, pt, name, paths)] = P.rmse(out, ref, surf) / base[paths]
            print("  %s, %s, n_sub %d done (%.0f s)" % (name, kind, n, time.time() - t0), flush=True)
        for (nm, pt), lst in lists.items():
            print("  %s: normal_min %.2f plane_tol %.2f marks %d pixels, %.1f %% of the tile" % (name, nm, pt, lst.size, 100.0 * lst.size / (P.W * P.H)))

    print("\n2. the sweep: R per scene at 1 / 4 / 16 / 64 paths, and the score")
    settings = list(itertools.product(N_SUB, TABLES, NORMAL_MIN, PLANE_TOL))
    score = {}
    for s in settings:
        rs = [ratios[s + (name, paths)] for name in P.SCENES for paths in P.PATHS]
        score[s] = float(np.exp(np.mean(np.log(rs))))
        print("  n_sub %2d %-10s normal_min %.2f plane_tol %.2f: %s  score %.4f"
              % (s + ("  ".join("%s %s" % (name, " ".join("%.3f" % ratios[s + (name, p)] for p in P.PATHS)) for name in P.SCENES), score[s])))
    best = min(score.values())
    ok = [s for s in settings if score[s] <= 1.02 * best]
    n = min(s[0] for s in ok)
    ok = [s for s in ok if s[0] == n]
    if any(s[1] == "rotated" for s in ok):
        ok = [s for s in ok if s[1] == "rotated"]
    chosen = min(ok, key=lambda s: score[s])
    print("\nbest score %.4f; within 2 %%: smallest n_sub %d; chosen by the rule: n_sub %d, table %s, normal_min %.2f, plane_tol %.2f (score %.4f)"
          % ((best, n) + chosen + (score[chosen],)))
    d = (E.DEFAULTS["n_sub"], "rotated", E.DEFAULTS["normal_min"], E.DEFAULTS["plane_tol"])
    print("the library's defaults: n_sub %d, table %s, normal_min %.2f, plane_tol %.2f (score %.4f)%s"
          % (d + (score.get(d, float("nan")), "" if d == chosen else "  -- NOT the rule's choice")))

    print("\n3. what tests/test_edges.py asserts (the defaults): r = resolved / denoised surface RMSE against the reference")
    for name in P.SCENES:
        for paths in (1, 16):
            r = ratios[d + (name, paths)]
            print("  %s, %2d paths: r = %.4f, the bound r + (1 - r)/4 = %.4f" % (name, paths, r, r + (1 - r) / 4))

    print("\n4. the guided preview of track B's last view (window 32), the defaults")
    for name in P.SCENES:
        views = K.track_views(name, "B")
        slow = K.slow_chains(views)
        i = len(views) - 1
        xs = K.TRACKS["B"][0]
        c = K.cpu_camera(xs[i])
        ref = K.render(name, c, None, 0.0, 0, K.oracle().randseeds(1, seed=2)[0], P.REF_PATHS)
        pre = K.preview(views[i], slow[i])
        _, words, prims, _, _ = views[i]
        lst = E.mark(words, prims, 0, d[2], d[3])
        rs, rd = P.subpixel_rays(c, E.offsets(d[0]))
        k = d[0]
        rs, rd = rs.reshape(k, -1, 4)[:, lst].reshape(-1, 4), rd.reshape(k, -1, 4)[:, lst].reshape(-1, 4)
        o0, o1 = K.oracle().traverse(K.tree(name), rs, rd, None)
        sw = np.concatenate([o0, o1], 1).astype(np.float32)
        sw[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
        out = E.resolve(pre, words, prims, lst, sw.reshape(k, -1, 8), np.zeros((k, lst.size), np.int32), 0, k, d[2], d[3])
        mask = K.surface_mask(views[i])
        a, b = K.rmse(pre, ref, mask), K.rmse(out, ref, mask)
        print("  %s: surface RMSE of the guided preview %.5f, resolved %.5f, ratio %.4f (%.0f s)" % (name, a, b, b / a, time.time() - t0), flush=True)

    print("\n5. not shipped: the interior alone (what cleaner sources inside the levels could at most address)")
    for name in P.SCENES:
        surf, edge, ref = P.surface_mask(name), P.edge_mask(name), P.reference(name)
        words, prims = P.gbuffer(name)
        for paths in (1, 16):
            den = P.denoised(name, paths)
            out = P.resolved(name, den, E.offsets(d[0]), d[2], d[3])
            print("  %s, %2d paths: interior RMSE %.4f denoised, %.4f resolved; edge RMSE %.4f denoised, %.4f resolved"
                  % (name, paths, P.rmse(den, ref, surf & ~edge), P.rmse(out, ref, surf & ~edge), P.rmse(den, ref, edge), P.rmse(out, ref, edge)))
    print("\n(%.0f s in all)" % (time.time() - t0))


if __name__ == "__main__":
    main()
