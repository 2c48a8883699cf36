"""Synthetic inputs for tests/test_filter_edges.py: G-buffers, radiance and chains of views that take the history blend
(include/gpuart_temporal.h) and the denoiser (include/gpuart_denoise.h) through the branches and edge values that a rendered G-buffer
does not reach. Everything is deterministic (seeded default_rng) and is built on the CPU; the ledgers of tests/temporal_ref.py and
tests/denoise_ref.py say which branches a case takes."""
import numpy as np

from tests import denoise_ref as R
from tests import temporal_ref as T

F = np.float32
P_A = dict(max_history=2.0, plane_tol=0.05, normal_min=0.5)
P_B = dict(max_history=32.0, plane_tol=0.005, normal_min=0.95)
DN_A = dict(iterations=3, lum_k=1.5, normal_pow2=2, depth_sigma=0.2)
DN_B = dict(iterations=8, lum_k=0.0, normal_pow2=0, depth_sigma=1.0)
US_1, US_2 = (0.1, 0.2, 0.3, 0.4), (0.1, 0.2, 0.3, 0.5)
# one below, at and one above the kernels' block sizes (64 wide; 4 and 16 high), and the largest legal shapes
SMALL_SHAPES = [(w, h) for w in (63, 64, 65) for h in (3, 4, 5, 15, 16, 17)]
LONG_SHAPES = [(65536, 1), (1, 65536)]


# ---- views and G-buffers ----------------------------------------------------------------------------------------------------------
def pinhole(pos, W, H, aspect=None):
    """12 camera floats (pos, bottomLeft, deltaHorz, deltaVert) of a camera at pos that looks along +y, its screen of height 1 at
    distance 1; aspect = the screen's width (default W / H: square pixels)."""
    pos = np.array(pos, np.float64)
    a = W / H if aspect is None else aspect
    return np.concatenate([pos, pos + np.array([-0.5 * a, 1.0, -0.5]), [a, 0.0, 0.0], [0.0, 0.0, 1.0]]).astype(np.float32)


def frame_xy(geom):
    """Frame column and row of every pixel of a share, (th, tw) each."""
    W, H, x0, y0, tw, th, br, bs = geom
    ly, lx = np.mgrid[0:th, 0:tw]
    return x0 + lx, y0 + (ly // br) * bs + ly % br


def plane_gbuffer(rng, cam, geom, y_plane=3.0, mix=True):
    """The G-buffer of the plane y = y_plane (normal (0, -1, 0)) seen through a share: hit points from a float64 ray-plane intersection
    rounded to fp32, types laid out in blocks; with mix, per pixel at random about 8 % each of sky, user sphere (ordinal -2, type 0), a
    tilted normal (cosine 0.6 to the plane's) and a hit point pushed off the plane by up to +-0.2."""
    W, H, _, _, tw, th, _, _ = geom
    fx, fy = frame_xy(geom)
    u, v = (fx + 0.5) / W, (fy + 0.5) / H
    c = cam.astype(np.float64)
    d = (c[3:6] + u[..., None] * c[6:9] + v[..., None] * c[9:12]) - c[0:3]
    t = (y_plane - c[1]) / d[..., 1]
    words = np.zeros((th, tw, 8), np.float32)
    words[..., 0] = t
    words[..., 1:4] = c[0:3] + t[..., None] * d
    words[..., 4:7] = (0, -1, 0)
    typ = (((fx // 7) + (fy // 5)) % 3).astype(np.int32)
    prims = rng.integers(0, 1000, (th, tw)).astype(np.int32)
    if mix:
        r = rng.random((th, tw))
        typ[r < 0.08] = -1
        prims[r < 0.08] = -1
        us = (r >= 0.08) & (r < 0.16)
        typ[us] = 0
        prims[us] = -2
        words[(r >= 0.16) & (r < 0.24), 4:7] = (0.8, -0.6, 0)
        off = (r >= 0.24) & (r < 0.32)
        words[off, 2] += rng.uniform(-0.2, 0.2, int(off.sum())).astype(np.float32)
    words[..., 7] = typ.view(np.float32)
    return words, prims


def radiance(rng, geom, scale=2.0):
    return (rng.uniform(0, 1, (geom[5], geom[4], 4)) * scale).astype(np.float32)


def step(rng, pos, geom, spp, us=US_1, flags=0, aspect=None, mix=True, scale=2.0):
    """One view of a chain: (rgba, spp, words, prims, the view as tests/temporal_ref.py wants it)."""
    cam = pinhole(pos, geom[0], geom[1], aspect)
    words, prims = plane_gbuffer(rng, cam, geom, mix=mix)
    return [radiance(rng, geom, scale), spp, words, prims, T.view(cam, geom, us, flags)]


def plant_behind_and_at(st, old_pos, rows=4, cols=40):
    """Moves the hit points of the first `rows` rows' first `cols` pixels behind a camera at old_pos that looks along +y, and sets those
    of the next row to old_pos exactly (d = 0, so dn = 0)."""
    words = st[2]
    cols = min(cols, words.shape[1])
    words[0:rows, 0:cols, 2] = F(old_pos[1] - 2.0)
    words[rows, 0:cols, 1:4] = np.array(old_pos, np.float32)


def plant_mirrored(old, cur, row, count=30, back=0.7):
    """Pixels whose value hangs on "k > 0" alone. `count` pixels of row `row` of the view `cur` get hit points BEHIND the camera of the
    view `old`, on the backward extension of the old camera's rays through (X + 0.8, Y + 0.8) of every other pixel pair of the old
    share's first two rows, so that step 3 maps them to fx = X + 0.3, fy = Y + 0.3 with k < 0; and the four old pixels around each of
    those get that very hit point, the same normal and the same type. Every tap then passes the class, normal and plane tests: a blend
    that forgets k > 0 takes the history there, the right one must not."""
    v = old[4]
    W, H, gx0, gy0, tw, th, br, bs = v["geom"]
    assert br >= 2 and th >= 2 and 2 * count <= tw and count <= cur[2].shape[1]
    pos, bl, dh, dv = (v[k].astype(np.float64) for k in ("pos", "bl", "dh", "dv"))
    for j in range(count):
        lx = 2 * j
        u, vv = (gx0 + lx + 0.8) / W, (gy0 + 0.8) / H      # local rows 0 and 1 are frame rows gy0 and gy0 + 1
        p = (pos - back * ((bl + u * dh + vv * dv) - pos)).astype(np.float32)
        for st, where in ((old, (slice(0, 2), slice(lx, lx + 2))), (cur, (row, j))):
            st[2][where + (slice(1, 4),)] = p
            st[2][where + (slice(4, 7),)] = (0, -1, 0)
            st[2][where + (0,)] = 1.0
            st[2][where + (7,)] = np.int32(0).view(np.float32)
            st[3][where] = 5


# the geometries: (W, H, x0, y0, tw, th, band_rows, band_stride)
G_SHARE = (96, 64, 8, 4, 80, 38, 4, 6)       # a banded share with a column window; th = 38 is not a multiple of band_rows: last band cut short
G_FULL = T.full_frame(128, 72)
G_TILE_A = (160, 120, 21, 13, 37, 23, 23, 23)
G_TILE_B = (160, 120, 30, 20, 50, 40, 40, 40)
G_BIG = T.full_frame(128, 72)
G_SMALL = (128, 72, 40, 20, 48, 30, 30, 30)
POS_0, POS_1, POS_2 = (0.0, 0.0, 0.0), (0.35, -0.3, 0.1), (-0.2, 0.15, -0.05)


def temporal_cases():
    """-> list of dict(name, steps, params, preview_at, alias_at, narrower): chains of views for run_chain. `narrower` marks the chains
    in which no view is wider than the history it reads."""
    cases = []

    def add(name, steps, params=None, preview_at=None, alias_at=None):
        preview_at = len(steps) - 1 if preview_at is None else preview_at
        narrower = all(b[4]["geom"][4] <= a[4]["geom"][4] for a, b in zip(steps, steps[1:]))
        cases.append(dict(name=name, steps=[tuple(s) for s in steps], params=params, preview_at=preview_at, alias_at=alias_at, narrower=narrower))

    # a banded share -> a full frame of another size; the history is committed twice so that its lengths differ
    for k, us1 in enumerate((US_1, US_2)):
        rng = np.random.default_rng(700 + k)
        s0 = step(rng, POS_0, G_SHARE, 3)
        s0b = [radiance(rng, G_SHARE), 2] + s0[2:]
        s1 = step(rng, POS_1, G_FULL, 1, us=us1)
        plant_behind_and_at(s1, POS_0)
        plant_mirrored(s0, s1, 6)
        add("share->full" + (", moved sphere" if k else ""), [s0, s0b, s1], alias_at=2 if k == 0 else None)
    # a full frame -> a banded share
    rng = np.random.default_rng(710)
    s0 = step(rng, POS_1, G_FULL, 2)
    s1 = step(rng, POS_0, G_SHARE, 1)
    plant_behind_and_at(s1, POS_1)
    plant_mirrored(s0, s1, 6)
    add("full->share", [s0, s1], params=P_A)
    # a rectangular tile -> another tile of the same frame, and on
    rng = np.random.default_rng(720)
    steps = [step(rng, POS_0, G_TILE_A, 2), step(rng, POS_2, G_TILE_B, 1), step(rng, POS_0, G_TILE_A, 3)]
    plant_behind_and_at(steps[1], POS_0, rows=2, cols=30)
    add("tile->tile", steps, preview_at=1)
    # smaller, smaller, larger, larger, smaller, larger: both history buffers are re-allocated and the ping-pong changes size
    rng = np.random.default_rng(730)
    order = [(G_SMALL, POS_0), (G_SMALL, POS_2), (G_BIG, POS_1), (G_BIG, POS_0), (G_SMALL, POS_2), (G_BIG, POS_1)]
    add("small, small, big, big, small, big", [step(rng, pos, g, 1 + i % 3) for i, (g, pos) in enumerate(order)], params=P_B, preview_at=4)
    # max_history 32 and histories whose lengths differ from pixel to pixel: found, not capped
    rng = np.random.default_rng(740)
    track = [(0.0, 0.0, 0.0), (0.15, 0.0, 0.0), (0.3, -0.1, 0.05), (0.45, -0.1, 0.05), (0.3, 0.0, 0.0)]
    add("long window", [step(rng, pos, G_FULL, (1, 5, 2, 9, 1)[i]) for i, pos in enumerate(track)], params=P_B, preview_at=3)
    # denormal radiance over a history of denormal colours: w * hist is denormal
    rng = np.random.default_rng(750)
    add("denormals", [step(rng, POS_0, G_FULL, 2, scale=1e-39), step(rng, (0.1, 0.0, 0.0), G_FULL, 1, scale=1e-39),
                      step(rng, (0.2, 0.0, 0.0), G_FULL, 3, scale=3e-39)], params=P_A, preview_at=1)
    # counts that (float)spp rounds
    rng = np.random.default_rng(760)
    add("spp", [step(rng, POS_0, G_TILE_A, 2 ** 24 + 1), step(rng, POS_2, G_TILE_A, 2 ** 32 - 1), step(rng, POS_0, G_TILE_A, 1),
                step(rng, POS_2, G_TILE_A, 2 ** 24 + 1)], preview_at=2)
    # the shapes
    for i, (w, h) in enumerate(SMALL_SHAPES + LONG_SHAPES):
        rng = np.random.default_rng(800 + i)
        g = T.full_frame(w, h)
        asp = 1.5 if max(w, h) > 1000 else None     # (the longest shapes keep a screen of ordinary proportions: their pixels are not square)
        add("%d x %d" % (w, h), [step(rng, POS_0, g, 2, aspect=asp), step(rng, (0.02, 0.0, 0.01), g, 1, aspect=asp)])
    return cases


def nonfinite_case():
    """Out of contract: NaN, +-inf and 3e38 scattered over the radiance and the hit points of two views, so that the history the first
    commit leaves holds them too. -> steps as temporal_cases()."""
    rng = np.random.default_rng(900)
    bad = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    steps = [step(rng, POS_0, G_SHARE, 2), step(rng, POS_1, G_FULL, 1), step(rng, POS_0, G_SHARE, 1)]
    for st in steps:
        for arr, share in ((st[0], 0.03), (st[2][..., 1:4], 0.03)):
            hit = rng.random(arr.shape) < share
            arr[hit] = bad[rng.integers(0, len(bad), int(hit.sum()))]
    return [tuple(s) for s in steps]


# ---- the denoiser -----------------------------------------------------------------------------------------------------------------
def edge_gbuffer(rng, h=45, w=70):
    """tests/test_denoise.py's synthetic_gbuffer plus what no rendered G-buffer holds: a patch of zero normals (den = 0), patches of pos = 1e-7 and pos = 0, a patch
    whose demodulated colour is constant (the variance clamp), a patch of denormal radiance and one of large finite radiance (1e15:
    the luminance squared stays finite, which is what the header requires). -> (rgba, words, prims)."""
    from tests.test_denoise import synthetic_gbuffer
    assert h >= 45 and w >= 70
    words, prims = synthetic_gbuffer(rng, h, w)
    t = words[..., 7].view(np.int32)
    surf = t >= 0
    words[5:12, 5:12, 4:7] = 0
    words[20:24, 30:40, 0] = np.where(surf[20:24, 30:40], F(1e-7), words[20:24, 30:40, 0])
    words[24:26, 30:40, 0] = np.where(surf[24:26, 30:40], F(0), words[24:26, 30:40, 0])
    rgba = rng.uniform(0, 3, (h, w, 4)).astype(np.float32)
    rgba[30:44, 50:69, :3] = R.PRIMITIVE_COLOR[t[30:44, 50:69] & 3] * F(0.7)
    rgba[0:4, 40:70, :3] = rng.uniform(0, 1, (4, 30, 3)).astype(np.float32) * F(1e-39)
    rgba[12:16, 0:20, :3] = rng.uniform(0, 1, (4, 20, 3)).astype(np.float32) * F(1e15)
    return rgba, words, prims


def denoise_cases():
    """-> list of dict(name, rgba, words, prims, flags, params)."""
    from tests.test_denoise import synthetic_gbuffer
    cases = []
    rgba, words, prims = edge_gbuffer(np.random.default_rng(11))
    for flags in (0, R.SPECULAR):
        for it in range(9):
            cases.append(dict(name="edges, flags %d, iterations %d" % (flags, it), rgba=rgba, words=words, prims=prims, flags=flags,
                              params=dict(iterations=it)))
        for p in (DN_A, DN_B):
            cases.append(dict(name="edges, flags %d, %s" % (flags, p), rgba=rgba, words=words, prims=prims, flags=flags, params=p))
    for i, (w, h) in enumerate(SMALL_SHAPES + LONG_SHAPES):
        rng = np.random.default_rng(300 + i)
        words, prims = synthetic_gbuffer(rng, h, w)
        rgba = rng.uniform(0, 2, (h, w, 4)).astype(np.float32)
        for p in (None, DN_B) if max(w, h) > 1000 else (DN_A,):
            cases.append(dict(name="%d x %d, %s" % (w, h, p), rgba=rgba, words=words, prims=prims, flags=0, params=p))
    return cases
