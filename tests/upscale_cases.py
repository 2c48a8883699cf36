"""The synthetic cases of tests/test_upscale.py: a low tile, its G-buffer and a G-buffer of the scale times larger tile, planted so that
the restatement (tests/upscale_ref.py) takes every branch the header names. No device is needed to make them.

Every pixel, low or high, shows one entry of a small palette: the sky, the user sphere, or one of a few planes that differ from one
another in exactly one thing match() asks for — the type, the normal, the distance — with a little noise on the point and the normal,
so that the normal and plane conditions also fail and hold within one entry, near their thresholds. Low pixels are drawn in blocks; a
high pixel shows what its containing low pixel shows with probability 0.6 and anything else otherwise: most output pixels find a tap,
and enough find none that every candidate of the fallback wins somewhere."""
import numpy as np

F = np.float32
TILES = [(1, 1), (3, 2), (65, 5), (130, 9)]   # (w, h) of the low tile: one pixel, narrower than a wave, a row that ends mid-wave, two blocks in y
SCALES = (2, 3, 4)
FLAGS = (0, 1, 2)                             # the user sphere diffuse, emissive, specular
# (type, ordinal, normal, distance): the sky, the user sphere, and planes of which 3 / 4 differ in type only, 4 / 5 in the normal only
# and 4 / 6 in the distance only
PALETTE = [(-1, -1, (0, 0, 0), 0.0), (0, -2, (0, 0, 1), 4.0), (0, 11, (0, 0, 1), 4.0), (1, 12, (0, 0, 1), 5.0), (2, 13, (0, 0, 1), 5.0),
           (2, 14, (0.6, 0, 0.8), 5.0), (2, 15, (0, 0, 1), 5.6)]


def _records(ids, rng, px):
    """(words, prims) of the pixels showing palette entries `ids` (h, w); `px`: the pixel's size in the plane."""
    h, w = ids.shape
    words = np.zeros((h, w, 8), np.float32)
    prims = np.zeros((h, w), np.int32)
    types = np.zeros((h, w), np.int32)
    y, x = np.mgrid[0:h, 0:w]
    for k, (t, o, n, z) in enumerate(PALETTE):
        m = ids == k
        types[m], prims[m] = t, o
        if t < 0:
            continue
        words[m, 0] = z
        words[m, 1] = (x[m] + 0.5) * px
        words[m, 2] = (y[m] + 0.5) * px
        words[m, 3] = z
        words[m, 4:7] = n
    hit = types >= 0
    noise = rng.uniform(-1, 1, (h, w, 4)).astype(np.float32)
    words[..., 3] += np.where(hit, noise[..., 0] * F(0.07), 0)           # the tolerance is 0.02 * 5 = 0.1: two noisy points may differ by 0.14
    words[..., 4:6] += np.where(hit[..., None], noise[..., 1:3] * F(0.2), 0)   # dn of two noisy normals reaches down to 0.92
    words[..., 7] = types.view(np.float32)
    return words, prims


def case(seed, w, h, scale, flags):
    """dict(filtered, words, prims, hi_words, hi_prims, scale, flags, w, h) of synthetic case `seed`."""
    rng = np.random.default_rng(seed)
    by, bx = -(-h // 2), -(-w // 3)
    low = np.kron(rng.integers(0, len(PALETTE), (by, bx)), np.ones((2, 3), np.int64))[:h, :w]
    high = np.kron(low, np.ones((scale, scale), np.int64))
    other = rng.integers(0, len(PALETTE), high.shape)
    high = np.where(rng.random(high.shape) < 0.6, high, other)
    words, prims = _records(low, rng, 0.1)
    hi_words, hi_prims = _records(high, rng, 0.1 / scale)
    filtered = rng.uniform(0.01, 4.0, (h, w, 4)).astype(np.float32)
    return dict(filtered=filtered, words=words, prims=prims, hi_words=hi_words, hi_prims=hi_prims, scale=scale, flags=flags, w=w, h=h)


def cases():
    """Every tile at every scale, the user sphere's flags going round."""
    out = []
    for i, (w, h) in enumerate(TILES):
        for j, s in enumerate(SCALES):
            out.append(case(100 + 10 * i + j, w, h, s, FLAGS[(i + j) % 3]))
    return out


def step_edge(w=8, h=4, scale=2, left=2.0, right=8.0):
    """Two planes of one type and normal at different distances meeting in a vertical step edge a quarter of an output pixel to the
    right of the centre of low column w // 2 - 1: that low pixel lies on the near plane, the right part of its output pixels on the
    far one. The low frame is `left` on the near plane and `right` on the far one, powers of two."""
    e = (w // 2 - 0.5) * scale + 0.25    # in output pixels

    def plane(n_y, n_x, px):
        x = (np.arange(n_x) + 0.5) * px
        far = np.broadcast_to(x[None, :] > e, (n_y, n_x))
        words = np.zeros((n_y, n_x, 8), np.float32)
        words[..., 0] = np.where(far, 9.0, 5.0)
        words[..., 1] = x[None, :] * 0.1
        words[..., 2] = (np.arange(n_y)[:, None] + 0.5) * px * 0.1
        words[..., 3] = words[..., 0]
        words[..., 6] = 1.0
        words[..., 7] = np.full((n_y, n_x), 2, np.int32).view(np.float32)
        return words, np.full((n_y, n_x), 13, np.int32), far

    words, prims, far = plane(h, w, float(scale))
    hi_words, hi_prims, hi_far = plane(h * scale, w * scale, 1.0)
    filtered = np.empty((h, w, 4), np.float32)
    filtered[..., :3] = np.where(far, right, left)[..., None]
    filtered[..., 3] = 1.0
    return dict(filtered=filtered, words=words, prims=prims, hi_words=hi_words, hi_prims=hi_prims, scale=scale, flags=0, w=w, h=h,
                hi_far=hi_far, far=far)
