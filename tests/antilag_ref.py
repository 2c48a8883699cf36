"""NumPy float32 restatement of include/gpuart_antilag.h, operation by operation in the order the header states.

The 49 neighbours of the window are accumulated one at a time in the stated order (dy outer, dx inner), never by a reduction over the
window's axes, so every value is the one the kernel of gpuart_amd/csrc/antilag/antilag.hip computes, bit for bit. Images are (h, w, 4)
float32, row 0 at the bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit and (h, w) int32 ordinals, as in
tests/denoise_ref.py; the len and alpha are (h, w) float32."""
import numpy as np

from tests.denoise_ref import lum, shift, surface

F = np.float32
DEFAULTS = dict(fast_history=4.0, min_batches=8.0, min_votes=8.0, clip=3.0, z_lo=2.0, z_hi=4.0)
LEDGER_KEYS = ("not_surface", "no_vote_short", "no_vote_same_len", "clipped", "var_zero", "few_votes", "s2_zero_change", "alpha_zero", "alpha_mid",
               "alpha_one", "win_outside")


def statistic(slow, slow_len, fast, fast_len, moments, surf, min_batches, clip, led=None):
    """Step 1 -> (votes, r, var): who votes, and every pixel's clipped r and var (meaningful where it votes)."""
    with np.errstate(all="ignore"):
        m = moments
        B = slow_len * m[..., 2]
        long_enough = B >= F(min_batches)
        shorter = fast_len < slow_len
        votes = surf & long_enough & shorter
        v = m[..., 1] - m[..., 0] * m[..., 0]
        v = np.where(v < 0, F(0), v).astype(np.float32)
        sv = (v * B) / (B - F(1))
        Bf = fast_len * m[..., 2]
        var = (sv * (F(1) / Bf - F(1) / B)).astype(np.float32)
        r = (lum(fast) - lum(slow)).astype(np.float32)
        pos = var > 0
        lim = F(clip) * np.sqrt(np.where(pos, var, F(0)).astype(np.float32))
        over, under = r > lim, r < -lim
        if led is not None:
            led["no_vote_short"] = int((surf & ~long_enough).sum())
            led["no_vote_same_len"] = int((surf & long_enough & ~shorter).sum())
            led["clipped"] = int((votes & pos & (over | under)).sum())
            led["var_zero"] = int((votes & ~pos).sum())
        r = np.where(pos, np.where(over, lim, np.where(under, -lim, r)), r).astype(np.float32)
    return votes, r, var


def mix(slow, slow_len, fast, fast_len, moments, words, prims, us_flags=0, fast_history=4.0, min_batches=8.0, min_votes=8.0, clip=3.0, z_lo=2.0,
        z_hi=4.0, want_ledger=False):
    """-> out (h, w, 4), out_len (h, w), alpha (h, w)[, ledger]. fast_history is not read (it is the window of the handle that made
    `fast`). The ledger (LEDGER_KEYS -> count) counts the pixels that took each branch from the very masks that select the values below;
    few_votes, s2_zero_change and the three alpha_* are over the surface pixels, win_outside counts their window positions outside
    the tile."""
    s = np.array(slow, np.float32)
    h, w = s.shape[:2]
    f = np.asarray(fast, np.float32).reshape(h, w, 4)
    sl = np.asarray(slow_len, np.float32).reshape(h, w)
    fl = np.asarray(fast_len, np.float32).reshape(h, w)
    m = np.asarray(moments, np.float32).reshape(h, w, 4)
    words = np.ascontiguousarray(words).view(np.float32).reshape(h, w, 8)
    prims = np.asarray(prims, np.int32).reshape(h, w)
    led = dict.fromkeys(LEDGER_KEYS, 0)
    with np.errstate(all="ignore"):
        surf, _ = surface(words, prims, us_flags)
        led["not_surface"] = int((~surf).sum())
        votes, r, var = statistic(s, sl, f, fl, m, surf, min_batches, clip, led)
        cnt, S1, S2 = (np.zeros((h, w), np.float32) for _ in range(3))
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                vq, inside = shift(votes, dy, dx)
                rq, _ = shift(r, dy, dx)
                varq, _ = shift(var, dy, dx)
                led["win_outside"] += int((surf & ~inside).sum())
                ok = inside & vq
                cnt = np.where(ok, cnt + F(1), cnt)
                S1 = np.where(ok, S1 + rq, S1)
                S2 = np.where(ok, S2 + varq, S2)
        few = cnt < F(min_votes)
        s2_pos = S2 > 0
        Z = np.where(few, F(0), np.where(s2_pos, np.abs(S1) / np.sqrt(np.where(s2_pos, S2, F(1)).astype(np.float32)),
                                         np.where(S1 == 0, F(0), F(np.inf)))).astype(np.float32)
        t = (Z - F(z_lo)) / (F(z_hi) - F(z_lo))
        alpha = np.where(t > 0, t, F(0)).astype(np.float32)
        alpha = np.where(alpha > 1, F(1), alpha).astype(np.float32)
        alpha = np.where(surf, alpha, F(0)).astype(np.float32)
        led["few_votes"] = int((surf & few).sum())
        led["s2_zero_change"] = int((surf & ~few & ~s2_pos & ~(S1 == 0)).sum())
        led["alpha_zero"] = int((surf & (alpha == 0)).sum())
        led["alpha_mid"] = int((surf & (alpha > 0) & (alpha < 1)).sum())
        led["alpha_one"] = int((surf & (alpha == 1)).sum())
        go = alpha > 0
        out = s.copy()
        for ch in range(3):
            out[..., ch] = np.where(go, s[..., ch] + alpha * (f[..., ch] - s[..., ch]), s[..., ch])
        out_len = np.where(go, sl + alpha * (fl - sl), sl).astype(np.float32)
    return (out, out_len, alpha) + ((led,) if want_ledger else ())
