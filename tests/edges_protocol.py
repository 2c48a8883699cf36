"""The protocol the edge resolve's defaults were chosen on and its tests measure (tools/edges_quality.py, tests/test_edges.py), on the
CPU alone: the oracle renders and answers the sub-pixel rays, the NumPy restatements filter (tests/denoise_ref.py) and resolve
(tests/edges_ref.py).

The box and scene P at 160 x 120, the Sun on, no user sphere, the camera at x = 0.35 of track A of tests/antilag_tracks.py. The
reference is one pass of 1024 paths from O.randseeds(1, seed=2); a frame is one pass of 1, 4, 16 or 64 paths from
O.randseeds(1, seed=1234). Errors are RMSE over the surface pixels against the reference. "Edge pixels" (the measurement's, not
gpuart_edges_mark's) are the surface pixels with an 8-neighbour that is not a surface pixel, has another type, a normal dot below 0.9
or a hit distance off by more than 5 %."""
import functools

import numpy as np

from tests import antilag_tracks as K
from tests import denoise_ref as D
from tests import edges_ref as E

W, H = K.W, K.H
SCENES = K.SCENES
CAMERA_X = 0.35
PATHS = (1, 4, 16, 64)
REF_PATHS = 1024


def camera():
    return K.cpu_camera(CAMERA_X)


@functools.lru_cache(maxsize=None)
def reference(name):
    return K.render(name, camera(), None, 0.0, 0, K.oracle().randseeds(1, seed=2)[0], REF_PATHS)


@functools.lru_cache(maxsize=None)
def frame(name, paths):
    return K.render(name, camera(), None, 0.0, 0, K.oracle().randseeds(1, seed=1234)[0], paths)


@functools.lru_cache(maxsize=None)
def gbuffer(name):
    return K.gbuffer(name, camera(), None)


@functools.lru_cache(maxsize=None)
def denoised(name, paths):
    words, prims = gbuffer(name)
    return D.denoise(frame(name, paths), words, prims, 0, **D.DEFAULTS)


def subpixel_rays(c, uv):
    """(rstart, rdir), each (n_sub, H, W, 4): the first segment of every pixel for the draws rand1 = uv[k, 0], rand2 = uv[k, 1], as
    path_tracing.glsl:144-170 forms it (rdirOrtho1/2, PixelSize, rdir = rstart - CameraPos), in float32."""
    O = K.oracle()
    rs0, rd0 = O.cam_rays(c, W, H)
    f = np.float32
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    norm = lambda v: v * (f(1) / np.sqrt(dot(v, v)))[..., None]
    d = rd0[..., :3]
    zero = np.zeros_like(d[..., 0])
    flat = (np.abs(d[..., 0]) > f(1e-5)) | (np.abs(d[..., 1]) > f(1e-5))
    with np.errstate(all="ignore"):
        o1 = np.where(flat[..., None], norm(np.stack([d[..., 1], -d[..., 0], zero], -1)), norm(np.stack([zero, -d[..., 2], d[..., 1]], -1)))
    dn = norm(d)
    o2 = np.stack([dn[..., 1] * o1[..., 2] - dn[..., 2] * o1[..., 1], dn[..., 2] * o1[..., 0] - dn[..., 0] * o1[..., 2],
                   dn[..., 0] * o1[..., 1] - dn[..., 1] * o1[..., 0]], -1)
    ps, pos = f(c[12]), np.asarray(c[0:3], np.float32)
    rs, rd = [], []
    for u, v in np.asarray(uv, np.float32):
        s = (rs0[..., :3] + ((u - f(0.5)) * o1) * ps) + ((v - f(0.5)) * o2) * ps
        rs.append(np.concatenate([s, np.zeros((H, W, 1), np.float32)], -1))
        rd.append(np.concatenate([s - pos, np.zeros((H, W, 1), np.float32)], -1))
    return np.stack(rs).astype(np.float32), np.stack(rd).astype(np.float32)


def subpixel_records(name, lst, uv):
    """(words (n_sub, n, 8), ordinals (n_sub, n)) of the sub-pixel rays of the listed pixels, as gpuart_hip_trace_subpixel lays them
    out: the oracle walks the rays."""
    O = K.oracle()
    rs, rd = subpixel_rays(camera(), uv)
    lst = np.asarray(lst, np.int64)
    k, n = len(uv), lst.size
    rs, rd = rs.reshape(k, -1, 4)[:, lst].reshape(-1, 4), rd.reshape(k, -1, 4)[:, lst].reshape(-1, 4)
    o0, o1 = O.traverse(K.tree(name), rs, rd, None)
    words = np.concatenate([o0, o1], 1).astype(np.float32)
    words[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
    return words.reshape(k, n, 8), np.zeros((k, n), np.int32)


def resolved(name, filtered, uv, normal_min=E.DEFAULTS["normal_min"], plane_tol=E.DEFAULTS["plane_tol"], want_ledger=False):
    """mark -> sub-pixel records -> resolve of a filtered frame of the protocol's view."""
    words, prims = gbuffer(name)
    lst = E.mark(words, prims, 0, normal_min, plane_tol)
    sw, sp = subpixel_records(name, lst, uv)
    return E.resolve(filtered, words, prims, lst, sw, sp, 0, len(uv), normal_min, plane_tol, want_ledger)


def surface_mask(name):
    words, prims = gbuffer(name)
    return D.surface(words, prims, 0)[0]


def edge_mask(name):
    """The measurement's edge pixels (the module's docstring)."""
    words, prims = gbuffer(name)
    surf, t = D.surface(words, prims, 0)
    n, pos = words[..., 4:7], words[..., 0]
    edge = np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                sq, inside = D.shift(surf, dy, dx)
                tq, _ = D.shift(t, dy, dx)
                nq, _ = D.shift(n, dy, dx)
                pq, _ = D.shift(pos, dy, dx)
                other = ~sq | (tq != t) | ((n * nq).sum(-1) < 0.9) | (np.abs(pq - pos) > 0.05 * pos)
                edge |= inside & other
    return surf & edge


rmse = K.rmse
