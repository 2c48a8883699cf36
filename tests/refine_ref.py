"""NumPy float32 restatement of the variance-guided filter of include/gpuart_refine.h, operation by operation in the order the header
states.

Taps and prefilter neighbours are accumulated one at a time in the stated order (dy outer, dx inner), never by a reduction over the
tap axes, so every value is the one the kernels of gpuart_amd/csrc/refine/refine.hip compute, bit for bit. Images are (h, w, 4)
float32, row 0 at the bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit and (h, w) int32 ordinals, as in
tests/denoise_ref.py; the error map is (h, w) float32, the e of tests/converge_ref.py's measure."""
import numpy as np

from tests.denoise_ref import PRIMITIVE_COLOR, denormals, gt_or, level, lum, shift, surface

F = np.float32
G = np.array([1 / 4, 1 / 2, 1 / 4], np.float32)
DEFAULTS = dict(iterations=5, lum_k=1.0, normal_pow2=5, depth_sigma=0.05)
LEDGER_KEYS = ("not_surface", "e_non_finite", "lum_below_floor", "pf_outside", "pf_invalid", "tap_outside", "tap_not_surface", "den_zero",
               "denormal_state", "denormal_out")


def refine(rgba, words, prims, error, lum_floor, us_flags=0, iterations=5, lum_k=1.0, normal_pow2=5, depth_sigma=0.05, want_ledger=False,
           prefilter=True):
    """-> out (h, w, 4)[, ledger]. The ledger (LEDGER_KEYS -> count) says how many pixels (den_zero: per level), prefilter neighbours
    and taps (per level) took each branch, counted from the very masks that select the values below, and how many values of the outputs
    and of the state (x and var, before the first level and after each) are fp32 denormals. tap_not_surface counts the taps that lie
    inside the tile and are not valid (not a surface pixel, or without a finite e). prefilter=False is the variant without step 2a
    (gv = var_p), for tools/refine_quality.py: the library has no such switch."""
    c = np.array(rgba, np.float32)
    words = np.asarray(words).view(np.float32).reshape(c.shape[:2] + (8,))
    prims = np.asarray(prims, np.int32).reshape(c.shape[:2])
    e = np.asarray(error, np.float32).reshape(c.shape[:2])
    lum_floor = F(lum_floor)
    out = c.copy()
    led = dict.fromkeys(LEDGER_KEYS, 0)
    if iterations == 0:
        return (out, led) if want_ledger else out
    with np.errstate(all="ignore"):
        # 0. validity
        surf, t = surface(words, prims, us_flags)
        fin = (e.view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
        valid = surf & fin
        led["not_surface"] = int((~surf).sum())
        led["e_non_finite"] = int((surf & ~fin).sum())
        a = PRIMITIVE_COLOR[t]
        # 1. demodulation, and the variance from the error map
        x = np.where(valid[..., None], c[..., :3] / a, F(0)).astype(np.float32)
        L = lum(x)
        above = L > lum_floor    # gt_or(L, lum_floor)
        led["lum_below_floor"] = int((valid & ~above).sum())
        sg = np.where(valid, e, F(0)) * np.where(above, L, lum_floor).astype(np.float32)
        var = (sg * sg).astype(np.float32)
        n = np.ascontiguousarray(words[..., 4:7])
        pos = np.ascontiguousarray(words[..., 0])
        zpos = gt_or(pos, 1e-6)
        led["denormal_state"] = denormals(x[valid]) + denormals(var[valid])
        # 2. the levels
        for i in range(iterations):
            # a. the 3x3 variance prefilter, never dilated
            if prefilter:
                gn = np.zeros(c.shape[:2], np.float32)
                gd = np.zeros(c.shape[:2], np.float32)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        vq, inside = shift(var, dy, dx)
                        sq, _ = shift(valid, dy, dx)
                        led["pf_outside"] += int((valid & ~inside).sum())
                        led["pf_invalid"] += int((valid & inside & ~sq).sum())
                        v = valid & inside & sq
                        g = G[dy + 1] * G[dx + 1]
                        gn = np.where(v, gn + g * vq, gn)
                        gd = np.where(v, gd + g, gd)
                gv = gn / gd
            else:
                gv = var
            # b. the taps, c. the update
            x, var = level(valid, x, var, n, pos, zpos, 1 << i, gv, lum_k, normal_pow2, depth_sigma, led)
        # 3. remodulation; every other pixel is copied, alpha everywhere
        out[..., :3] = np.where(valid[..., None], x * a, c[..., :3])
        led["denormal_out"] = denormals(out[..., :3][valid])
    return (out, led) if want_ledger else out
