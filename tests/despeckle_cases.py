"""The planted frames the firefly clamp's ledger test and its GPU tests share (tests/test_despeckle.py), and the protocol its defaults
were chosen on and its quality test measures (tools/despeckle_quality.py), on the CPU alone.

A planted frame: surfaces of every type with a smooth radiance, outliers of 10..100 times it, sky bands five rows thick with lone
surface pixels inside (too few neighbours at either radius), a user-sphere patch (ordinal -2: no surface pixel while the flags say
emissive or specular), a patch of one type and one colour (ties at every rank), a black patch with outliers in it (ref = 0: the cap is
the floor) and surface pixels whose radiance is NaN.

The protocol is that of tests/antilag_tracks.py: 160 x 120, the Sun on, the camera at x = 0.10, a frame is one pass of 1, 4, 16 or 64
paths from O.randseeds(1, seed=1234), the reference one pass of 1024 paths from O.randseeds(1, seed=2). Errors are RMSE over the surface
pixels after tests/denoise_ref.py `denoise` with its defaults."""
import functools

import numpy as np

from tests import antilag_tracks as K
from tests import denoise_ref as D
from tests import despeckle_ref as DS

F = np.float32


def plant(seed, w, h, flags=0):
    """-> (rgba (h, w, 4), words (h, w, 8), prims (h, w)) of a planted frame; what does not fit a small frame is left out."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, (h, w)).astype(np.int32)
    prims = rng.integers(0, 1000, (h, w)).astype(np.int32)
    t[rng.random((h, w)) < 0.04] = -1                      # scattered sky
    rgba = (rng.uniform(0.05, 1.0, (h, w, 1)) * rng.uniform(0.5, 1.0, (h, w, 4))).astype(np.float32)
    out = rng.random((h, w)) < 0.04                        # the outliers
    rgba[out, :3] *= rng.uniform(10, 100, (int(out.sum()), 1)).astype(np.float32)
    if h >= 12:
        for y0 in range(3, h - 5, 14):                     # sky bands with lone surface pixels in their middle row
            t[y0:y0 + 5] = -1
            t[y0 + 2, 2::5] = 2
    if h >= 16 and w >= 30:
        t[h - 7:h - 2, 3:9] = 0                            # the user sphere
        prims[h - 7:h - 2, 3:9] = -2
        t[h - 8:h - 2, 11:18] = 2                          # one type, one colour
        rgba[h - 8:h - 2, 11:18, :3] = F(0.3)
        rgba[h - 6, 13, :3] = F(9.0)
        t[h - 8:h - 2, 20:28] = 1                          # black, with outliers
        rgba[h - 8:h - 2, 20:28, :3] = 0
        rgba[h - 6, 22:27:2, :3] = F(0.5)
    nan = (rng.random((h, w)) < 0.02) & (t >= 0)
    rgba[nan, :3] = np.nan
    prims[t < 0] = -1
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    words = np.zeros((h, w, 8), np.float32)
    words[..., 0] = np.where(t >= 0, rng.uniform(0.5, 4.0, (h, w)), -1.0)
    words[..., 4:7] = np.where((t >= 0)[..., None], n, 0.0)
    words[..., 7] = t.view(np.float32)
    return rgba, words, prims


SETTINGS = [dict(radius=r, rank=k) for r in (1, 2) for k in (1, 2, 3, 4)]   # both radii and every rank; the rest are the defaults


@functools.lru_cache(maxsize=None)
def cases():
    """The ledger's case set: (what, rgba, words, prims, flags, params). 37 x 19 and 64 x 48 with the user sphere diffuse, emissive and
    specular, the defaults; 37 x 19 at every radius and rank; and two settings of k, floor and min_count."""
    out = []
    for w, h in ((37, 19), (64, 48)):
        for flags in (0, D.EM_NONZERO, D.SPECULAR):
            out.append(("%dx%d flags %d" % (w, h, flags),) + plant(100 + w + flags, w, h, flags) + (flags, dict(DS.DEFAULTS)))
    for s in SETTINGS:
        out.append(("37x19 radius %(radius)d rank %(rank)d" % s,) + plant(7, 37, 19) + (0, dict(DS.DEFAULTS, **s)))
    out.append(("64x48 floor 0",) + plant(8, 64, 48, D.EM_NONZERO) + (D.EM_NONZERO, dict(DS.DEFAULTS, floor=0.0, k=1.0, min_count=1)))
    out.append(("64x48 radius 2 min_count 24",) + plant(9, 64, 48) + (0, dict(DS.DEFAULTS, radius=2, k=4.0, min_count=24)))
    return out


@functools.lru_cache(maxsize=None)
def expected(i):
    """(out, scale, summary, ledger) of case i: computed once, shared, never written to."""
    _, rgba, words, prims, flags, params = cases()[i]
    return DS.clamp(rgba, words, prims, flags, want_ledger=True, **params)


# ---- the protocol --------------------------------------------------------------------------------------------------------------------
W, H = K.W, K.H
CAMERA_X = 0.10
PATHS = (1, 4, 16, 64)
REF_PATHS = 1024
# name -> (scene, user sphere or None, emittance, userSphereFlags)
SCENES = {"scene_p_firefly": ("scene_p", (0.0, 0.0, 0.5, 0.1), 30.0, D.EM_NONZERO),
          "scene_p": ("scene_p", None, 0.0, 0),
          "box": ("box", None, 0.0, 0),
          "box_sphere": ("box", K.sphere_at(5), K.EMITTANCE, D.EM_NONZERO)}


def camera():
    return K.cpu_camera(CAMERA_X)


@functools.lru_cache(maxsize=None)
def reference(name):
    scene, us, em, flags = SCENES[name]
    return K.render(scene, camera(), us, em, flags, K.oracle().randseeds(1, seed=2)[0], REF_PATHS)


@functools.lru_cache(maxsize=None)
def frame(name, paths):
    scene, us, em, flags = SCENES[name]
    return K.render(scene, camera(), us, em, flags, K.oracle().randseeds(1, seed=1234)[0], paths)


@functools.lru_cache(maxsize=None)
def gbuffer(name):
    scene, us, _, _ = SCENES[name]
    return K.gbuffer(scene, camera(), us)


@functools.lru_cache(maxsize=None)
def surface_mask(name):
    words, prims = gbuffer(name)
    return D.surface(words, prims, SCENES[name][3])[0]


@functools.lru_cache(maxsize=None)
def denoised_error(name, paths):
    """The surface RMSE of the denoised frame, no clamp."""
    words, prims = gbuffer(name)
    flags = SCENES[name][3]
    return K.rmse(D.denoise(frame(name, paths), words, prims, flags, **D.DEFAULTS), reference(name), surface_mask(name))


def clamped_error(name, paths, **params):
    """(the surface RMSE of the clamped, then denoised frame, the clamp's summary)."""
    words, prims = gbuffer(name)
    flags = SCENES[name][3]
    c, _, summary = DS.clamp(frame(name, paths), words, prims, flags, **dict(DS.DEFAULTS, **params))
    return K.rmse(D.denoise(c, words, prims, flags, **D.DEFAULTS), reference(name), surface_mask(name)), summary


def ratio(name, paths, **params):
    """R: clamped-then-denoised over denoised."""
    return clamped_error(name, paths, **params)[0] / denoised_error(name, paths)
