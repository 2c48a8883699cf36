"""NumPy float32 restatement of include/gpuart_upscale.h, operation by operation in the order the header states.

Taps and candidates are taken one at a time in the stated order, never by a reduction, so every value is the one the kernel of
gpuart_amd/csrc/upscale/upscale.hip computes, bit for bit. Images are (h, w, 4) float32, row 0 at the bottom; a G-buffer is (h, w, 8)
float32 words of gpuart_ray_hit and (h, w) int32 ordinals; the larger frame's is (scale*h, scale*w, 8) and (scale*h, scale*w)."""
import numpy as np

F = np.float32
DEFAULTS = dict(normal_min=0.95, plane_tol=0.02)
SCALES = (2, 3, 4)
EM_NONZERO, SPECULAR = 1, 2
# the candidates of the fallback as (dy, dx), in the order they are tried
CANDIDATES = ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
SKY, SPHERE, SURFACE = 0, 1, 2
# why match() said no, in the order the header states its conditions
MATCH, BY_CLASS, BY_TYPE, BY_US, BY_NORMAL, BY_PLANE = range(6)
REASONS = ("class", "type", "us", "normal", "plane")
LEDGER_KEYS = ("tap_outside", "tap_zero_weight", "tap_counted") + tuple("tap_fails_" + r for r in REASONS) + \
    tuple("fallback_%d" % c for c in range(9)) + ("fallback_none", "weighted")


def records(words, prims, us_flags):
    """The fields match() reads of records (..., 8) / (...): dict of pos, p, n, type, us, cls."""
    words = np.asarray(words).view(np.float32)
    prims = np.asarray(prims, np.int32)
    t = np.ascontiguousarray(words[..., 7]).view(np.int32)
    hit = t >= 0
    us = hit & (prims == -2)
    cls = np.where(~hit, SKY, np.where(us & bool(us_flags & (EM_NONZERO | SPECULAR)), SPHERE, SURFACE))
    return dict(pos=words[..., 0], p=words[..., 1:4], n=words[..., 4:7], type=t, us=us, cls=cls)


def verdict(a, b, normal_min, plane_tol):
    """match(a, b) of the header, elementwise over two record dicts of one shape: MATCH, or the first condition that fails."""
    with np.errstate(all="ignore"):
        dn = (a["n"][..., 0] * b["n"][..., 0] + a["n"][..., 1] * b["n"][..., 1]) + a["n"][..., 2] * b["n"][..., 2]
        d = a["p"] - b["p"]
        dist = np.abs((b["n"][..., 0] * d[..., 0] + b["n"][..., 1] * d[..., 1]) + b["n"][..., 2] * d[..., 2])
        lim = F(plane_tol) * np.where(b["pos"] > F(1e-6), b["pos"], F(1e-6)).astype(np.float32)
        v = np.where(dist <= lim, MATCH, BY_PLANE)
        v = np.where(dn > F(normal_min), v, BY_NORMAL)
        v = np.where(a["us"] == b["us"], v, BY_US)
        v = np.where(a["type"] == b["type"], v, BY_TYPE)
        v = np.where(a["cls"] != SURFACE, MATCH, v)
        return np.where(a["cls"] == b["cls"], v, BY_CLASS)


def match(a, b, normal_min, plane_tol):
    return verdict(a, b, normal_min, plane_tol) == MATCH


def tap_positions(n_out, scale):
    """Step 1 along one axis for output coordinates 0 .. n_out-1: (x0 as int64, ax as float32)."""
    X = np.arange(n_out)
    fx = (X.astype(np.float32) + F(0.5)) / F(scale) - F(0.5)
    fl = np.floor(fx)
    return fl.astype(np.int64), (fx - fl).astype(np.float32)


def upscale(filtered, words, prims, hi_words, hi_prims, scale, us_flags=0, normal_min=0.95, plane_tol=0.02, want_ledger=False):
    """-> out (scale*h, scale*w, 4)[, ledger]. The ledger counts, per (output pixel, tap), why the tap did not count or that it did,
    and per output pixel whether the weighted mean was taken (`weighted`), which candidate of the fallback won, or that none did."""
    f = np.ascontiguousarray(filtered, np.float32)
    h, w = f.shape[:2]
    H, W = h * scale, w * scale
    centre = records(np.asarray(words).view(np.float32).reshape(h, w, 8), np.asarray(prims, np.int32).reshape(h, w), us_flags)
    r = records(np.asarray(hi_words).view(np.float32).reshape(H, W, 8), np.asarray(hi_prims, np.int32).reshape(H, W), us_flags)
    led = dict.fromkeys(LEDGER_KEYS, 0)
    x0, ax = tap_positions(W, scale)
    y0, ay = tap_positions(H, scale)
    x0, ax, y0, ay = x0[None, :], ax[None, :], y0[:, None], ay[:, None]
    cy, cx = np.broadcast_arrays((np.arange(H) // scale)[:, None], (np.arange(W) // scale)[None, :])
    wsum = np.zeros((H, W), np.float32)
    acc = np.zeros((H, W, 3), np.float32)
    with np.errstate(all="ignore"):
        for oy in (0, 1):
            wy = ay if oy else F(1.0) - ay
            for ox in (0, 1):
                wx = ax if ox else F(1.0) - ax
                wt = (wy * wx).astype(np.float32)
                ty, tx = np.broadcast_arrays(y0 + oy, x0 + ox)
                inside = (ty >= 0) & (ty < h) & (tx >= 0) & (tx < w)
                qy, qx = np.where(inside, ty, 0), np.where(inside, tx, 0)
                positive = np.broadcast_to(wt > 0, (H, W))
                v = verdict(r, {k: a[qy, qx] for k, a in centre.items()}, normal_min, plane_tol)
                counts = inside & positive & (v == MATCH)
                led["tap_outside"] += int((~inside).sum())
                led["tap_zero_weight"] += int((inside & ~positive).sum())
                for code, name in enumerate(REASONS, 1):
                    led["tap_fails_" + name] += int((inside & positive & (v == code)).sum())
                led["tap_counted"] += int(counts.sum())
                wsum = np.where(counts, wsum + wt, wsum).astype(np.float32)
                acc = np.where(counts[..., None], acc + wt[..., None] * f[qy, qx][..., :3], acc).astype(np.float32)
        weighted = wsum > 0
        led["weighted"] = int(weighted.sum())
        own = f[cy, cx]
        rgb = own[..., :3].copy()
        done = weighted.copy()
        for ci, (dy, dx) in enumerate(CANDIDATES):
            qy, qx = cy + dy, cx + dx
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)
            win = inside & ~done & match(r, {k: a[qy, qx] for k, a in centre.items()}, normal_min, plane_tol)
            rgb = np.where(win[..., None], f[qy, qx][..., :3], rgb)
            done |= win
            led["fallback_%d" % ci] += int(win.sum())
        led["fallback_none"] = int((~done).sum())
        mean = (acc / np.where(weighted, wsum, F(1.0))[..., None]).astype(np.float32)
        out = np.empty((H, W, 4), np.float32)
        out[..., :3] = np.where(weighted[..., None], mean, rgb)
        out[..., 3] = own[..., 3]
    return (out, led) if want_ledger else out


def bilinear(filtered, scale):
    """Plain bilinear upsampling with the taps and weights of step 1 and 2 and no guidance: every tap inside the tile with w > 0 counts."""
    f = np.ascontiguousarray(filtered, np.float32)
    h, w = f.shape[:2]
    sky = np.zeros((h, w, 8), np.float32)
    sky[..., 7] = np.array(-1, np.int32).view(np.float32)
    hi = np.zeros((h * scale, w * scale, 8), np.float32)
    hi[..., 7] = sky[0, 0, 7]
    return upscale(f, sky, np.full((h, w), -1, np.int32), hi, np.full((h * scale, w * scale), -1, np.int32), scale)
