"""What the fast history buys the guided preview, and what it costs, on the CPU: the oracle renders the tracks of
tests/antilag_tracks.py (which states the protocol), the NumPy restatements blend, measure, mix (tests/antilag_ref.py) and filter. No
GPU is involved; the kernel equals the restatement bit for bit (tests/test_antilag.py) and the product's frames equal the oracle's, so
these are the figures the GPU reproduces.

"without" is today's Renderer::ReadGuidedPreview with window 32 and every default; "with" is the same with SetHistoryAntiLag on.
Swept: fast_history 2, 4, 8 and (z_lo, z_hi) over (1.5, 3), (2, 4), (2, 6), (3, 6), (4, 8), (6, 12); min_votes 8 and clip 3 stay.
min_batches is swept over 4 and 8 (gpuart_moments_defaults'): a first sweep with 8 alone showed the reason, the lighting-change tracks
have 16 views and with 8 no pixel votes before the ninth.

The rule, stated before the sweep was run. Only settings qualify whose ratio with / without of the surface RMSE is at most 1.02 at every
view of the static-lighting tracks A and B on both scenes (the 2 % tools/moments_quality.py grants). Among those the defaults are the
setting with the smallest surface RMSE summed over all views of the lighting-change tracks on both scenes. If no qualifying setting
improves that sum, the tool says so.

Printed last: what tests/test_antilag.py asserts with the defaults: per scene and lighting-change track R = with / without at the last
view, and per scene the share of voting pixels with alpha > 0 over the 24 views of the static track B.

    python tools/antilag_quality.py [--cache DIR]      (its output is kept as section 1 of profiles/antilag.txt)
--cache keeps the oracle's frames and references as .npz files in DIR and reads them from there when they exist.
"""
import argparse
import itertools
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import antilag_ref as A  # noqa: E402
from tests import antilag_tracks as K  # noqa: E402

FAST = (2.0, 4.0, 8.0)
MIN_BATCHES = (4.0, 8.0)
ZS = ((1.5, 3.0), (2.0, 4.0), (2.0, 6.0), (3.0, 6.0), (4.0, 8.0), (6.0, 12.0))
SETTINGS = [(fh, mb, z_lo, z_hi) for fh, mb, (z_lo, z_hi) in itertools.product(FAST, MIN_BATCHES, ZS)]


def load_track(name, track, cache):
    """(views, references) of one track, from the cache where it holds them."""
    path = os.path.join(cache, "%s_%s.npz" % (name, track)) if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return K.track_views(name, track, (z["frames"], z["words"], z["prims"])), list(z["refs"])
    views = K.track_views(name, track)
    refs = [K.reference(name, track, i) for i in range(len(views))]
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, frames=np.stack([v[0] for v in views]), words=np.stack([v[1] for v in views]), prims=np.stack([v[2] for v in views]),
                 refs=np.stack(refs))
    return views, refs


def view_job(job):
    """One view: the RMSE without, every setting's RMSE with, and per setting (voting pixels, those with alpha > 0)."""
    key, view, ref, slow, fasts = job
    mask = K.surface_mask(view)
    without = K.rmse(K.preview(view, slow), ref, mask)
    res = {}
    for fh, mb, z_lo, z_hi in SETTINGS:
        p = dict(fast_history=fh, min_batches=mb, z_lo=z_lo, z_hi=z_hi)
        out, (_, _, alpha) = K.preview(view, slow, fasts[fh], p, want_mix=True)
        votes, _, _ = A.statistic(slow[0], slow[1], fasts[fh][0], fasts[fh][1], slow[2], mask, mb, A.DEFAULTS["clip"])
        res[(fh, mb, z_lo, z_hi)] = (K.rmse(out, ref, mask), int(votes.sum()), int((votes & (alpha > 0)).sum()))
    return key, without, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    args = ap.parse_args()
    jobs = []
    for name in K.SCENES:
        for track in K.TRACKS:
            t0 = time.time()
            views, refs = load_track(name, track, args.cache)
            slow = K.slow_chains(views)
            fasts = {fh: K.fast_chain(views, fh) for fh in FAST}
            for i in range(len(views)):
                jobs.append(((name, track, i), views[i], refs[i], slow[i], {fh: fasts[fh][i] for fh in FAST}))
            print("%s, track %s: %d views, their references and blends in %.1f s" % (name, track, len(views), time.time() - t0), flush=True)
    with multiprocessing.Pool(min(K.NT, len(jobs))) as pool:
        res = {key: (without, r) for key, without, r in pool.imap_unordered(view_job, jobs)}

    keys = sorted(res)
    static = [k for k in keys if k[1] in K.STATIC]
    change = [k for k in keys if k[1] in K.CHANGE]
    ratio = lambda k, s: res[k][1][s][0] / res[k][0]
    base = sum(res[k][0] for k in change)
    print("\nmin_votes %g, clip %g; window %g" % (A.DEFAULTS["min_votes"], A.DEFAULTS["clip"], K.WINDOW))
    print("per setting: the worst ratio with / without over the %d static views, the surface RMSE summed over the %d lighting-change views"
          " (without: %.5f), and the share of voting pixels with alpha > 0 on the static views" % (len(static), len(change), base))
    worst, total = {}, {}
    for s in SETTINGS:
        wk = max(static, key=lambda k: ratio(k, s))
        worst[s] = ratio(wk, s)
        total[s] = sum(res[k][1][s][0] for k in change)
        votes, fired = sum(res[k][1][s][1] for k in static), sum(res[k][1][s][2] for k in static)
        print("  fast_history %g min_batches %g z_lo %3g z_hi %2g: worst static %.4f (%s, track %s, view %d) %s  change sum %.5f (%.4f of without)  fired %.5f"
              % (s + (worst[s],) + wk + ("qualifies" if worst[s] <= 1.02 else "         ", total[s], total[s] / base, fired / max(votes, 1))))
    ok = [s for s in worst if worst[s] <= 1.02]
    if not ok:
        print("\nno setting qualifies")
        return
    best = min(ok, key=lambda s: total[s])
    print("\nthe qualifying setting with the smallest sum: fast_history %g min_batches %g z_lo %g z_hi %g (%.4f of without%s); the library's defaults: "
          "fast_history %g min_batches %g z_lo %g z_hi %g" % (best + (total[best] / base, "" if total[best] < base else ": NO qualifying setting improves the lighting-change tracks",
                                                A.DEFAULTS["fast_history"], A.DEFAULTS["min_batches"], A.DEFAULTS["z_lo"], A.DEFAULTS["z_hi"])))
    d = (A.DEFAULTS["fast_history"], A.DEFAULTS["min_batches"], A.DEFAULTS["z_lo"], A.DEFAULTS["z_hi"])
    if d not in worst:
        print("the library's defaults are not in the sweep")
        return
    print("\nwith the defaults (fast_history %g, min_batches %g, z_lo %g, z_hi %g): surface RMSE, without | with | ratio" % d)
    for k in keys:
        print("  %s, track %s, view %2d: %.5f | %.5f | %.4f" % (k + (res[k][0], res[k][1][d][0], ratio(k, d))))
    print("\nwhat tests/test_antilag.py asserts (the defaults):")
    for name in K.SCENES:
        for track in K.CHANGE:
            r = ratio((name, track, K.N_CHANGE - 1), d)
            print("  %s, %s: R = %.4f at the last view, the bound R + (1 - R)/4 = %.4f" % (name, track, r, r + (1 - r) / 4))
        b = [k for k in keys if k[0] == name and k[1] == "B"]
        votes, fired = sum(res[k][1][d][1] for k in b), sum(res[k][1][d][2] for k in b)
        print("  %s, static track B: %d of %d voting pixels have alpha > 0: %.5f; the bound, one half more: %.5f; the worst static ratio %.4f"
              % (name, fired, votes, fired / max(votes, 1), 1.5 * fired / max(votes, 1), max(ratio(k, d) for k in static if k[0] == name)))


if __name__ == "__main__":
    main()
