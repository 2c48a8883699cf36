"""NumPy restatement of include/gpuart_display.h, operation by operation in the order the header states: fp32 for the histogram's
luminance and the encode, integers and float64 for the exposure. Every byte, count and gain is the one the kernels of
gpuart_amd/csrc/display/display.hip compute, bit for bit. Images are (h, w, 4) float32, row 0 at the bottom; the result is
(h, w, 4) uint8 in the same layout."""
import math

import numpy as np

F = np.float32
D = np.float64
DEFAULTS = dict(gain=1.0, auto_exposure=0, key=0.18, lo_share=0.5, hi_share=0.02, adapt=1.0, min_gain=2.0 ** -16, max_gain=2.0 ** 16,
                curve=0, white=4.0, transfer=0, dither=0)
CLAMP, REINHARD, ACES = 0, 1, 2
LINEAR, SRGB = 0, 1

# the 8x8 Bayer index matrix, B8[y][x]
B8 = np.array([[0, 32, 8, 40, 2, 34, 10, 42],
               [48, 16, 56, 24, 50, 18, 58, 26],
               [12, 44, 4, 36, 14, 46, 6, 38],
               [60, 28, 52, 20, 62, 30, 54, 22],
               [3, 35, 11, 43, 1, 33, 9, 41],
               [51, 19, 59, 27, 49, 17, 57, 25],
               [15, 47, 7, 39, 13, 45, 5, 37],
               [63, 31, 55, 23, 61, 29, 53, 21]], np.int32)


def lum(x):
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def srgb_to_linear(v):
    """The inverse sRGB function in float64 (the C library's pow, one value at a time)."""
    v = float(v)
    return v / 12.92 if v <= 0.04045 else math.pow((v + 0.055) / 1.055, 2.4)


def srgb_table():
    """E[0..255]: the fp32 nearest to the float64 value of the inverse sRGB function at j/255."""
    return np.array([srgb_to_linear(j / 255.0) for j in range(256)], np.float64).astype(np.float32)


def positive(c):
    """c > 0 ? c : 0 (a NaN and a negative become 0)."""
    with np.errstate(all="ignore"):
        return np.where(c > 0, c, F(0)).astype(np.float32)


def bins(L):
    """The bin of every luminance that is counted (finite and > 0)."""
    L = np.ascontiguousarray(L, np.float32)
    return np.clip((L.view(np.uint32) >> 21).astype(np.int64) - 380, 0, 255)


def histogram(rgba):
    """-> (h[256] as Python ints, skipped)."""
    c = np.asarray(rgba, np.float32).reshape(-1, 4)
    with np.errstate(all="ignore"):
        L = lum(positive(c[:, :3]))
        ok = np.isfinite(L) & (L > 0)
    h = np.bincount(bins(L[ok]), minlength=256)
    return [int(v) for v in h], int((~ok).sum())


def window(h, lo_share, hi_share):
    """-> (t[256], S, Nw): the part of every bin inside the pixel ranks [lo, N - hi), in ascending bin order."""
    N = sum(h)
    lo = int(np.floor(D(F(lo_share)) * D(N)))
    hi = int(np.floor(D(F(hi_share)) * D(N)))
    end = N - hi if hi < N else 0
    at, t = 0, []
    for b in range(256):
        first = max(at, lo)
        at += h[b]
        t.append(max(min(at, end) - first, 0))
    return t, sum(tb * (2 * b + 1) for b, tb in enumerate(t)), sum(t)


def target_gain(h, key=0.18, lo_share=0.5, hi_share=0.02, min_gain=2.0 ** -16, max_gain=2.0 ** 16):
    """Steps 1 to 7, float64; None where the word stays as it is (nothing counted)."""
    _, S, Nw = window(h, lo_share, hi_share)
    if sum(h) == 0 or Nw == 0:
        return None
    m = D(S) / D(Nw) / D(8) - D(32)
    i = np.floor(m)
    f = m - i
    Lavg = np.ldexp(D(1) + f, int(i))
    target = D(F(key)) / Lavg
    target = D(F(min_gain)) if target < D(F(min_gain)) else target
    target = D(F(max_gain)) if target > D(F(max_gain)) else target
    return target


def parts(y, transfer=0):
    """Step 4 for y in [0, 1] (float32): -> (k, frac)."""
    y = np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        if transfer == SRGB:
            E = srgb_table()
            k = np.clip(np.searchsorted(E, y, side="right") - 1, 0, 254)   # the largest k in 0..254 with E[k] <= y
            frac = (y - E[k]) / (E[k + 1] - E[k])
        else:
            q = y * F(255)
            k = q.astype(np.int32)
            frac = q - k.astype(np.float32)
    assert frac.dtype == np.float32
    return k, frac


def threshold(hgt, wid, dither=0, origin=(0, 0)):
    """Step 5's t: 0.5 without dither, else (hgt, wid) float32."""
    if not dither:
        return F(0.5)
    ly, lx = np.mgrid[0:hgt, 0:wid]
    return (B8[(origin[1] + ly) & 7, (origin[0] + lx) & 7].astype(np.float32) + F(0.5)) / F(64)


def encode(rgba, G=1.0, curve=0, white=4.0, transfer=0, dither=0, origin=(0, 0)):
    """The encode for a gain in force G -> (h, w, 4) uint8."""
    c = np.asarray(rgba, np.float32)
    hgt, wid = c.shape[:2]
    with np.errstate(all="ignore"):
        x = positive(c[..., :3])
        x = x * F(G)
        x = np.where(x < F(65504), x, F(65504)).astype(np.float32)
        if curve == REINHARD:
            L = lum(x)
            Lo = (L * (F(1) + L / (F(white) * F(white)))) / (F(1) + L)
            s = np.where(L > 0, Lo / L, F(0)).astype(np.float32)
            y = x * s[..., None]
        elif curve == ACES:
            y = (x * (F(2.51) * x + F(0.03))) / (x * (F(2.43) * x + F(0.59)) + F(0.14))
        else:
            y = x
        y = np.where(y < F(1), y, F(1)).astype(np.float32)
        k, frac = parts(y, transfer)
        t = threshold(hgt, wid, dither, origin)
        t = t[..., None] if dither else t
        code = k + (frac >= t)
    out = np.full((hgt, wid, 4), 255, np.uint8)
    out[..., :3] = code.astype(np.uint8)
    return out


def cli_bytes(v):
    """What gpuart_cli --ppm writes for float v: std::lround(clamp(v, 0, 1)*255.0f), a NaN as 0."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        v = np.where(v != v, F(0), np.where(v < 0, F(0), np.where(v > 1, F(1), v))).astype(np.float32)
        q = (v * F(255)).astype(np.float64)
    return np.floor(q + 0.5).astype(np.uint8)   # (q >= 0: half away from zero is half up; q + 0.5 is exact in float64)


class Display:
    """A handle's state: the histogram of the last run with auto_exposure and the exposure word."""

    def __init__(self):
        self.h, self.skipped = [0] * 256, 0
        self.reset()

    def reset(self):
        self.g, self.valid = F(1), 0

    def run(self, rgba, origin=(0, 0), **params):
        unknown = set(params) - set(DEFAULTS)
        assert not unknown, unknown
        p = dict(DEFAULTS, **params)
        G = F(p["gain"])
        if p["auto_exposure"]:
            self.h, self.skipped = histogram(rgba)
            target = target_gain(self.h, p["key"], p["lo_share"], p["hi_share"], p["min_gain"], p["max_gain"])
            if target is not None:
                g = D(self.g) + (target - D(self.g)) * D(F(p["adapt"])) if self.valid else target
                self.g, self.valid = F(g), 1
            G = F(p["gain"]) * self.g
        return encode(rgba, G, p["curve"], p["white"], p["transfer"], p["dither"], origin)

    def state(self):
        return dict(histogram=list(self.h), counted=sum(self.h), skipped=self.skipped, gain=F(self.g), valid=self.valid)
