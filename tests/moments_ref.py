"""NumPy float32 restatement of include/gpuart_moments.h, operation by operation in the order the header states.

The 49 neighbours of the spatial estimate are accumulated one at a time in the stated order (dy outer, dx inner), never by a reduction
over the window's axes, so every value is the one the kernels of gpuart_amd/csrc/moments/moments.hip compute, bit for bit. Images are
(h, w, 4) float32, row 0 at the bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit and (h, w) int32 ordinals, as in
tests/denoise_ref.py; len and e are (h, w) float32."""
import numpy as np

from tests.denoise_ref import lum, shift, surface

F = np.float32
DEFAULTS = dict(min_batches=8.0, spatial_k=4.0)
LEDGER_KEYS = ("not_surface", "temporal", "spatial", "at_threshold", "var_clamped", "lum_below_floor", "win_outside", "win_not_surface")


def pack(rgba, spp):
    """-> {L, L*L, 1/(float)spp, a} per pixel."""
    c = np.array(rgba, np.float32)
    out = np.empty_like(c)
    with np.errstate(all="ignore"):
        l = lum(c)
        out[..., 0] = l
        out[..., 1] = l * l
        out[..., 2] = F(1) / F(spp)
        out[..., 3] = c[..., 3]
    return out


def error(rgba, length, moments, words, prims, lum_floor, us_flags=0, min_batches=8.0, spatial_k=4.0, want_ledger=False):
    """-> e (h, w)[, ledger]. rgba, length: the blended radiance and its len; moments: the blended packed image. The ledger
    (LEDGER_KEYS -> count) says how many pixels, and how many window neighbours of the pixels that take the spatial estimate, took each
    branch, counted from the very masks that select the values below: at_threshold is B == min_batches (the measured branch),
    lum_below_floor counts both branches' denominators."""
    x = np.array(rgba, np.float32)
    h, w = x.shape[:2]
    ln = np.asarray(length, np.float32).reshape(h, w)
    m = np.asarray(moments, np.float32).reshape(h, w, 4)
    words = np.asarray(words).view(np.float32).reshape(h, w, 8)
    prims = np.asarray(prims, np.int32).reshape(h, w)
    lum_floor, min_batches, spatial_k = F(lum_floor), F(min_batches), F(spatial_k)
    led = dict.fromkeys(LEDGER_KEYS, 0)
    with np.errstate(all="ignore"):
        surf, _ = surface(words, prims, us_flags)
        led["not_surface"] = int((~surf).sum())
        # 2. the measured variance
        B = ln * m[..., 2]
        tm = surf & (B >= min_batches)
        sp = surf & ~(B >= min_batches)
        led["temporal"], led["spatial"] = int(tm.sum()), int(sp.sum())
        led["at_threshold"] = int((tm & (B == min_batches)).sum())
        v = m[..., 1] - m[..., 0] * m[..., 0]
        neg = v < 0
        led["var_clamped"] = int((tm & neg).sum())
        v = np.where(neg, F(0), v).astype(np.float32)
        m_above = m[..., 0] > lum_floor     # gt_or(m.r, lum_floor)
        e_t = np.sqrt(v / (B - F(1))) / np.where(m_above, m[..., 0], lum_floor).astype(np.float32)
        # 3. the spatial estimate over the 7x7 window of surface pixels inside the tile
        L = lum(x)
        cnt, s1, s2 = (np.zeros((h, w), np.float32) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                Lq, inside = shift(L, dy, dx)
                sq, _ = shift(surf, dy, dx)
                led["win_outside"] += int((sp & ~inside).sum())
                led["win_not_surface"] += int((sp & inside & ~sq).sum())
                ok = inside & sq
                cnt = np.where(ok, cnt + F(1), cnt)
                s1 = np.where(ok, s1 + Lq, s1)
                s2 = np.where(ok, s2 + Lq * Lq, s2)
        mean = s1 / cnt
        raw = s2 / cnt - mean * mean
        var = np.where(raw > F(0), raw, F(0)).astype(np.float32)     # gt_or(raw, 0)
        L_above = L > lum_floor
        e_s = (spatial_k * np.sqrt(var)) / np.where(L_above, L, lum_floor).astype(np.float32)
        led["lum_below_floor"] = int((tm & ~m_above).sum()) + int((sp & ~L_above).sum())
        e = np.where(tm, e_t, np.where(sp, e_s, F(0))).astype(np.float32)
    return (e, led) if want_ledger else e
