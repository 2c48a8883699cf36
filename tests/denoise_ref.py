"""NumPy float32 restatement of the denoiser of include/gpuart_denoise.h, operation by operation in the order the header states.

Taps are accumulated one at a time in the stated order (dy outer, dx inner), never by a reduction over the tap axes, so every value is
the one the kernels of gpuart_amd/csrc/denoise/denoise.hip compute, bit for bit. Images are (h, w, 4) float32, row 0 at the bottom;
the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit (pos, p.xyz, n.xyz, type as int32 bits) and (h, w) int32 ordinals."""
import numpy as np

F = np.float32
# the reference's PRIMITIVE_COLOR (shaders/path_tracing.glsl:123-126), by primitive type; the user sphere has type 0
PRIMITIVE_COLOR = np.array([[0.65, 0.4, 0.35], [0.1, 0.2, 0.1], [0.3, 0.3, 0.3], [0.3, 0.3, 0.3]], np.float32)
H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], np.float32)
DEFAULTS = dict(iterations=5, lum_k=4.0, normal_pow2=5, depth_sigma=0.05)
EM_NONZERO, SPECULAR = 1, 2


def gt_or(a, b):
    """max(a, b) as the header states it: a > b ? a : b."""
    return np.where(a > b, a, F(b)).astype(np.float32)


def lum(x):
    return (F(0.2126) * x[..., 0] + F(0.7152) * x[..., 1]) + F(0.0722) * x[..., 2]


def surface(words, prims, us_flags):
    """(surface-pixel mask, type & 3) of a G-buffer."""
    t = np.ascontiguousarray(words[..., 7]).view(np.int32)
    s = t >= 0
    if us_flags & (EM_NONZERO | SPECULAR):
        s &= prims != -2
    return s, t & 3


def shift(a, oy, ox):
    """b[y, x] = a[y + oy, x + ox] where that lies inside the image (zero elsewhere), and the mask of where it does."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    inside = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -oy), min(h, h - oy), max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        inside[y0:y1, x0:x1] = True
    return out, inside


LEDGER_KEYS = ("not_surface", "den_zero", "pos_small", "var_clamped", "tap_outside", "tap_not_surface", "denormal_out", "denormal_state")
TINY = np.finfo(np.float32).tiny


def denormals(a):
    """How many values of a are fp32 denormals."""
    return int(((a != 0) & (np.abs(a) < TINY)).sum())


def level(mask, x, var, n, pos, zpos, s, sd_var, lum_k, normal_pow2, depth_sigma, led):
    """One à-trous level with a dilation of s over the pixels of `mask` (the denoiser's surface pixels, the variance-guided filter's
    valid ones): the 25 taps and the update -> (x, var). sd_var is the variance the luminance edge is sized by: var itself in the
    denoiser, the prefiltered one in tests/refine_ref.py. led counts tap_outside, tap_not_surface (a tap inside the tile that is not
    in the mask), den_zero and denormal_state. This is the one restatement of gpuart_amd/csrc/image/atrous.h `atrous_level`."""
    Lp = lum(x)
    sd = np.sqrt(sd_var) * F(lum_k) + F(1e-4)
    zs = (F(depth_sigma) * zpos) * F(s)
    num = np.zeros_like(x)
    den = np.zeros(x.shape[:2], np.float32)
    nv = np.zeros(x.shape[:2], np.float32)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            xq, inside = shift(x, s * dy, s * dx)
            vq, _ = shift(var, s * dy, s * dx)
            nq, _ = shift(n, s * dy, s * dx)
            pq, _ = shift(pos, s * dy, s * dx)
            sq, _ = shift(mask, s * dy, s * dx)
            v = mask & inside
            led["tap_outside"] += int((mask & ~inside).sum())
            led["tap_not_surface"] += int((v & ~sq).sum())
            v = v & sq
            hk = H[dy + 2] * H[dx + 2]
            e = (lum(xq) - Lp) / sd
            wl = F(1) / (F(1) + e * e)
            wn = gt_or((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2], 0.0)
            for _ in range(normal_pow2):
                wn = wn * wn
            dz = np.abs(pq - pos) / zs
            wz = F(1) / (F(1) + dz * dz)
            wt = ((hk * wl) * wn) * wz
            num = np.where(v[..., None], num + wt[..., None] * xq, num)
            den = np.where(v, den + wt, den)
            nv = np.where(v, nv + (wt * wt) * vq, nv)
    upd = mask & (den > 0)
    led["den_zero"] += int((mask & ~(den > 0)).sum())
    x = np.where(upd[..., None], num / den[..., None], x)
    var = np.where(upd, nv / (den * den), var)
    led["denormal_state"] += denormals(x[mask]) + denormals(var[mask])
    return x, var


def denoise(rgba, words, prims, us_flags=0, iterations=5, lum_k=4.0, normal_pow2=5, depth_sigma=0.05, want_ledger=False):
    """-> out (h, w, 4)[, ledger]. The ledger (LEDGER_KEYS -> count) says how many pixels (den_zero: per level) and taps (per level)
    took each branch, counted from the very masks that select the values below, and how many values of the outputs and of the state
    (x and var, before the first level and after each) are fp32 denormals."""
    c = np.array(rgba, np.float32)
    words = np.asarray(words).view(np.float32).reshape(c.shape[:2] + (8,))
    prims = np.asarray(prims, np.int32).reshape(c.shape[:2])
    out = c.copy()
    led = dict.fromkeys(LEDGER_KEYS, 0)
    if iterations == 0:
        return (out, led) if want_ledger else out
    with np.errstate(all="ignore"):
        surf, t = surface(words, prims, us_flags)
        led["not_surface"] = int((~surf).sum())
        a = PRIMITIVE_COLOR[t]
        # 1. demodulation and luminance
        x = np.where(surf[..., None], c[..., :3] / a, F(0)).astype(np.float32)
        L = lum(x)
        # 2. the 7x7 variance over the surface pixels inside the tile
        cnt, m1, m2 = (np.zeros(c.shape[:2], np.float32) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                Lq, inside = shift(L, dy, dx)
                sq, _ = shift(surf, dy, dx)
                v = inside & sq
                cnt = np.where(v, cnt + F(1), cnt)
                m1 = np.where(v, m1 + Lq, m1)
                m2 = np.where(v, m2 + Lq * Lq, m2)
        mean = m1 / cnt
        raw = m2 / cnt - mean * mean
        keep = raw > F(0)    # gt_or(raw, 0)
        var = np.where(keep, raw, F(0)).astype(np.float32)
        led["var_clamped"] = int((surf & ~keep & (raw < 0)).sum())
        n = np.ascontiguousarray(words[..., 4:7])
        pos = np.ascontiguousarray(words[..., 0])
        far = pos > F(1e-6)    # gt_or(pos, 1e-6)
        zpos = np.where(far, pos, F(1e-6)).astype(np.float32)
        led["pos_small"] = int((surf & ~far).sum())
        led["denormal_state"] = denormals(x[surf]) + denormals(var[surf])
        # 3. the à-trous levels
        for i in range(iterations):
            x, var = level(surf, x, var, n, pos, zpos, 1 << i, var, lum_k, normal_pow2, depth_sigma, led)
        # 4. remodulation; every other pixel is copied, alpha everywhere
        out[..., :3] = np.where(surf[..., None], x * a, c[..., :3])
        led["denormal_out"] = denormals(out[..., :3][surf])
    return (out, led) if want_ledger else out
