"""NumPy float32 restatement of the firefly clamp of include/gpuart_despeckle.h, operation by operation in the order the header states.

ref is an order statistic: only comparisons make it, so the order in which the neighbours are visited cannot change a bit, and the
restatement may sort where the kernel of gpuart_amd/csrc/despeckle/despeckle.hip inserts. Images are (h, w, 4) float32, row 0 at the
bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit and (h, w) int32 ordinals, as in tests/denoise_ref.py."""
import numpy as np

from tests.denoise_ref import PRIMITIVE_COLOR, lum, shift, surface

F = np.float32
DEFAULTS = dict(radius=1, rank=3, k=2.0, floor=1e-3, min_count=4)
LEDGER_KEYS = ("not_surface", "own_L_invalid", "neighbour_outside", "neighbour_invalid", "too_few", "not_above_cap", "clamped", "ref_tied",
               "cap_is_floor")


def offsets(radius):
    """The neighbours' (dy, dx), dy outer and dx inner, the pixel itself left out."""
    return [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1) if (dy, dx) != (0, 0)]


def clamp(rgba, words, prims, us_flags=0, radius=1, rank=3, k=2.0, floor=1e-3, min_count=4, want_ledger=False):
    """-> (out (h, w, 4), scale (h, w), summary)[, ledger]. summary: surface, clamped, too_few as gpuart_despeckle_read_summary counts
    them. The ledger (LEDGER_KEYS -> count) says how many pixels, and for neighbour_* how many (surface pixel, offset) pairs, took each
    branch, counted from the very masks that select the values below; ref_tied: decided pixels whose ref equals the next-larger
    entry; cap_is_floor: decided pixels with k*ref + floor == floor. (Decided: a surface pixel with enough neighbours.)"""
    c = np.array(rgba, np.float32)
    words = np.asarray(words).view(np.float32).reshape(c.shape[:2] + (8,))
    prims = np.asarray(prims, np.int32).reshape(c.shape[:2])
    led = dict.fromkeys(LEDGER_KEYS, 0)
    need = max(int(min_count), int(rank))
    with np.errstate(all="ignore"):
        surf, t = surface(words, prims, us_flags)
        a = PRIMITIVE_COLOR[t]
        x = (c[..., :3] / a).astype(np.float32)
        L = lum(x)
        Lv = np.where(surf, L, F(np.nan)).astype(np.float32)
        valid = Lv == Lv
        led["not_surface"] = int((~surf).sum())
        led["own_L_invalid"] = int((surf & ~valid).sum())
        cnt = np.zeros(c.shape[:2], np.int32)
        planes = []
        for dy, dx in offsets(radius):
            vq, inside = shift(valid, dy, dx)
            Lq, _ = shift(Lv, dy, dx)
            led["neighbour_outside"] += int((surf & ~inside).sum())
            led["neighbour_invalid"] += int((surf & inside & ~vq).sum())
            nb = inside & vq
            cnt += nb
            planes.append(np.where(nb, Lq, F(-np.inf)).astype(np.float32))
        top = -np.sort(-np.stack(planes, -1), -1)    # descending; what is no neighbour sorts last
        ref = top[..., rank - 1]
        cap = (F(k) * ref + F(floor)).astype(np.float32)
        decided = surf & (cnt >= need)
        clamped = decided & (L > cap)
        led["too_few"] = int((surf & ~(cnt >= need)).sum())
        led["not_above_cap"] = int((decided & ~(L > cap)).sum())
        led["clamped"] = int(clamped.sum())
        if rank >= 2:
            led["ref_tied"] = int((decided & (top[..., rank - 2] == ref)).sum())
        led["cap_is_floor"] = int((decided & (cap == F(floor))).sum())
        s = (cap / L).astype(np.float32)
        out = c.copy()
        out[..., :3] = np.where(clamped[..., None], (x * s[..., None]) * a, c[..., :3])
        scale = np.where(clamped, s, F(1)).astype(np.float32)
    summary = dict(surface=int(surf.sum()), clamped=led["clamped"], too_few=led["too_few"])
    return (out, scale, summary, led) if want_ledger else (out, scale, summary)
