"""The oracle tracks the anti-lag's defaults were chosen on and its tests measure (tools/antilag_quality.py, tests/test_antilag.py), on
the CPU alone: the oracle renders, the NumPy restatements blend (tests/temporal_ref.py), measure (tests/moments_ref.py), mix
(tests/antilag_ref.py) and filter (tests/refine_ref.py).

The protocol: the box and scene P at 160 x 120, the Sun on, one path per pixel and view from one seed sequence (O.randseeds(n,
seed=1234)), every view committed, window 32; every view's reference is one pass of 256 paths of another seed (O.randseeds(1, seed=2)).
Errors are RMSE over the surface pixels of the view. The static-lighting tracks are tools/moments_quality.py's A and B (no user sphere);
the lighting-change tracks have 16 views and a user sphere of radius 0.25 that moves 0.06 per view along x: diffuse with the camera
fixed, diffuse with the camera of track B, and emissive (emittance 3) with the camera fixed."""
import functools
import os

import numpy as np

from gpuart_amd import synth_scenes as S
from tests import antilag_ref as A
from tests import denoise_ref as D
from tests import moments_ref as M
from tests import refine_ref as R
from tests import temporal_ref as T
from tests.util import scene

W, H = 160, 120
FLOOR = 1.0 / 256
WINDOW = 32.0
NT = min(8, os.cpu_count() or 1)
SCENES = ("box", "scene_p")
N_CHANGE = 16
EMITTANCE = 3.0


def sphere_at(i):
    return (-0.6 + 0.06 * i, 0.0, 0.2, 0.25)


# name -> (camera x per view, user sphere per view or None, emittance, userSphereFlags)
STATIC = {"A": ([0.10 + 0.05 * i for i in range(8)], None, 0.0, 0), "B": ([0.10 + 0.015 * i for i in range(24)], None, 0.0, 0)}
CHANGE = {"diffuse_fixed": ([0.10] * N_CHANGE, [sphere_at(i) for i in range(N_CHANGE)], 0.0, 0),
          "diffuse_moving": ([0.10 + 0.015 * i for i in range(N_CHANGE)], [sphere_at(i) for i in range(N_CHANGE)], 0.0, 0),
          "emissive": ([0.10] * N_CHANGE, [sphere_at(i) for i in range(N_CHANGE)], EMITTANCE, D.EM_NONZERO)}
TRACKS = dict(STATIC, **CHANGE)


def oracle():
    from oracle import oracle as O
    return O


@functools.lru_cache(maxsize=None)
def tree(name):
    return oracle().build_bvh(scene(name))[0]


def cam_of(x):
    cam = dict(S.DEFAULT_CAMERA, pos=(x, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    return cam


def cpu_camera(x):
    cam = cam_of(x)
    return oracle().camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def render(name, c, us, em, flags, seed, paths):
    """The oracle's mean of one pass of `paths` paths."""
    O = oracle()
    P = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, us or (0, 0, 0, 0), em, flags, float(c[12]), c[0:3], 5, 0.01)
    acc = np.zeros((H, W, 4), np.float32)
    O.pt_pass(tree(name), c, W, H, P, seed, paths, acc, nthreads=NT)
    return acc / np.float32(paths)


def gbuffer(name, c, us):
    """(words (H, W, 8), ordinals (H, W)) of the camera rays' closest hits as gpuart_hip_gbuffer lays them out: ordinal -2 on the user sphere."""
    O = oracle()
    rs, rd = O.cam_rays(c, W, H)
    rs, rd = rs.reshape(-1, 4), rd.reshape(-1, 4)
    o0, o1 = O.traverse(tree(name), rs, rd, us)
    prims = np.zeros(W * H, np.int32)
    if us is not None:
        b0, _ = O.traverse(tree(name), rs, rd, None)
        prims[(o0.view(np.uint32) != b0.view(np.uint32)).any(1)] = -2
    words = np.concatenate([o0, o1], 1).astype(np.float32)
    words[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
    return words.reshape(H, W, 8), prims.reshape(H, W)


def track_views(name, track, stored=None):
    """Per view of the track (frame of one path, words, prims, the temporal view, userSphereFlags). stored: (frames, words, prims) that an
    earlier call made, to be used instead of the oracle."""
    xs, spheres, em, flags = TRACKS[track]
    seeds = oracle().randseeds(len(xs), seed=1234)
    out = []
    for i, x in enumerate(xs):
        us = spheres[i] if spheres else None
        c = cpu_camera(x)
        if stored is None:
            words, prims = gbuffer(name, c, us)
            frame = render(name, c, us, em, flags, seeds[i], 1)
        else:
            frame, words, prims = (a[i] for a in stored)
        out.append((frame, words, prims, T.view(c, T.full_frame(W, H), us or (0, 0, 0, 0), flags), flags))
    return out


def reference(name, track, i):
    """View i's reference: one pass of 256 paths of another seed."""
    xs, spheres, em, flags = TRACKS[track]
    return render(name, cpu_camera(xs[i]), spheres[i] if spheres else None, em, flags, oracle().randseeds(1, seed=2)[0], 256)


def chain(views, max_history):
    """Per view the blend and its len of a history that commits every view of `views`."""
    return chain_of([v[0] for v in views], views, max_history)


def chain_of(images, views, max_history):
    """The same for images[i] in place of the frame of view i."""
    hist = None
    out = []
    kw = dict(T.DEFAULTS, max_history=max_history)
    for img, (_, words, prims, v, _) in zip(images, views):
        x, ln, hist = T.accumulate(hist, img, 1, words, prims, v, **kw)
        out.append((x, ln))
    return out


def slow_chains(views, window=WINDOW):
    """Per view (slow blend, slow len, moments blend) with the long window."""
    x = chain(views, window)
    m = chain_of([M.pack(v[0], 1) for v in views], views, window)
    return [(a, ln, b) for (a, ln), (b, _) in zip(x, m)]


def fast_chain(views, fast_history, window=WINDOW):
    """Per view (fast blend, fast len): the window is min(fast_history, window), as Renderer::BlendFast caps it."""
    return chain(views, fast_history if fast_history < window else window)


def preview(view, slow, fast=None, params=None, want_mix=False):
    """The guided preview of one view from its blends: without `fast` today's sequence (error, refine), with it mix, error, refine."""
    _, words, prims, _, flags = view
    x, ln, m = slow
    mixed = None
    if fast is not None:
        mixed = A.mix(x, ln, fast[0], fast[1], m, words, prims, flags, **dict(A.DEFAULTS, **(params or {})))
        x, ln = mixed[0], mixed[1]
    e = M.error(x, ln, m, words, prims, FLOOR, flags, **M.DEFAULTS)
    out = R.refine(x, words, prims, e, FLOOR, flags, **R.DEFAULTS)
    return (out, mixed) if want_mix else out


def surface_mask(view):
    return D.surface(view[1], view[2], view[4])[0]


def rmse(a, b, mask):
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return float(np.sqrt((d[mask] ** 2).mean()))
