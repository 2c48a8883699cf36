"""NumPy float32 restatement of the temporal accumulation of include/gpuart_temporal.h, operation by operation in the order the header
states.

The four taps are accumulated one at a time in the stated order (oy outer, ox inner), never by a reduction over the tap axes, so every
value is the one the kernel of gpuart_amd/csrc/temporal/temporal.hip computes, bit for bit. Images are (h, w, 4) float32, row 0 at the
bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit (pos, p.xyz, n.xyz, type as int32 bits) and (h, w) int32 ordinals.
A view is the dict `view()` makes; a history is None or the dict `accumulate` returns as its third value."""
import numpy as np

from tests.denoise_ref import EM_NONZERO, SPECULAR, surface   # the pixel classes' one rule and its flag bits

F = np.float32
DEFAULTS = dict(max_history=4.0, plane_tol=0.01, normal_min=0.8)


def view(cam, geom, user_sphere=(0.0, 0.0, 0.0, 0.0), us_flags=0):
    """cam: pos(3) bottomLeft(3) deltaHorz(3) deltaVert(3) [...] as given to set_camera; geom: (W, H, x0, y0, tw, th, band_rows,
    band_stride) or an object with those fields (binding.TileGeom)."""
    cam = np.asarray(cam, np.float32)
    if not isinstance(geom, (tuple, list)):
        geom = tuple(int(getattr(geom, k)) for k in ("W", "H", "x0", "y0", "tw", "th", "band_rows", "band_stride"))
    return dict(pos=cam[0:3].copy(), bl=cam[3:6].copy(), dh=cam[6:9].copy(), dv=cam[9:12].copy(), geom=tuple(int(g) for g in geom),
                user_sphere=np.array(user_sphere, np.float32), us_flags=int(us_flags))


def full_frame(W, H):
    """The geom of a tile that is the whole frame."""
    return (W, H, 0, 0, W, H, H, H)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(np.float32)


def classes(words, prims, us_flags):
    """Per pixel -1 (not a surface pixel) or (type & 3) | 4 * (the user sphere)."""
    surf, t3 = surface(words, prims, us_flags)
    return np.where(surf, t3 | np.where(prims == -2, 4, 0), -1).astype(np.int32)


def backproject(p, v):
    """Step 3 for hit points p (..., 3) and the history's view v: fx, fy, k, dn, d."""
    b = v["bl"] - v["pos"]
    N = cross(v["dh"], v["dv"])
    A = cross(v["dv"], b)
    B = cross(b, v["dh"])
    bN = dot(b, N)
    d = (p - v["pos"]).astype(np.float32)
    dn = dot(d, N)
    k = bN / dn
    u = dot(d, A) / dn
    vv = dot(d, B) / dn
    fx = u * F(v["geom"][0]) - F(0.5)
    fy = vv * F(v["geom"][1]) - F(0.5)
    return fx, fy, k, dn, d


LEDGER_PIXEL = ("not_surface", "no_history", "dn_zero", "behind", "off_left", "off_right", "off_below", "off_above", "x0_minus_1", "y0_minus_1",
                "wsum_zero", "found_uncapped", "found_capped")
LEDGER_TAP = ("tap_off_frame", "tap_off_columns", "tap_below_share", "tap_band_gap", "tap_past_share", "tap_class", "tap_sphere_moved",
              "tap_normal", "tap_plane", "tap_valid")
LEDGER_KEYS = LEDGER_PIXEL + LEDGER_TAP


def accumulate(hist, rgba, spp, words, prims, cur_view, max_history=4.0, plane_tol=0.01, normal_min=0.8, want_coords=False, want_ledger=False,
               ignore_k=False):
    """-> (out (h, w, 4), len (h, w), the history a commit leaves[, (fx, fy)][, ledger]).

    ignore_k is for the tests of the tests alone: it drops "k > 0" from the has-taps condition, as a wrong kernel might, so that a CPU
    test can show that the cases hold pixels whose value depends on that condition.

    The ledger (LEDGER_KEYS -> count) says how many pixels, and how many taps in the kernel's order of tests, took each branch. Every
    count is the population of the very mask that selects the values below — a tap leaves `ok` where it is counted — so a branch
    counted is a branch taken."""
    c = np.array(rgba, np.float32)
    h, w = c.shape[:2]
    words = np.ascontiguousarray(words).view(np.float32).reshape(h, w, 8)
    prims = np.asarray(prims, np.int32).reshape(h, w)
    assert cur_view["geom"][4:6] == (w, h) and spp >= 1
    s = F(spp)
    cls = classes(words, prims, cur_view["us_flags"])
    surf = cls >= 0
    p = np.ascontiguousarray(words[..., 1:4])
    n = np.ascontiguousarray(words[..., 4:7])
    out = c.copy()
    ln = np.where(surf, s, F(0)).astype(np.float32)
    coords = None
    led = dict.fromkeys(LEDGER_KEYS, 0)
    led["not_surface"] = int((~surf).sum())

    def cut(ok, key, gone):
        """The taps of `ok` that `gone` takes out are counted under `key` and leave."""
        led[key] += int((ok & gone).sum())
        return ok & ~gone

    with np.errstate(all="ignore"):
        if hist is None:
            led["no_history"] = int(surf.sum())
        else:
            hv = hist["view"]
            Wo, Ho, gx0, gy0, tw, th, br, bs = hv["geom"]
            sphere_same = hv["user_sphere"].tobytes() == cur_view["user_sphere"].tobytes()
            fx, fy, k, dn, d = backproject(p, hv)
            coords = (fx, fy)
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0, fy - y0
            tol = F(plane_tol) * np.sqrt(dot(d, d))
            front = surf & (dn != 0) & ((k > 0) | bool(ignore_k))
            x_lo, x_hi, y_lo, y_hi = x0 >= -1, x0 < F(Wo), y0 >= -1, y0 < F(Ho)
            has = front & x_lo & x_hi & y_lo & y_hi
            led["dn_zero"] = int((surf & ~(dn != 0)).sum())
            led["behind"] = int((surf & (dn != 0) & ~(k > 0)).sum())
            for key, side in (("off_left", x_lo), ("off_right", x_hi), ("off_below", y_lo), ("off_above", y_hi)):
                led[key] = int((front & ~side).sum())
            led["x0_minus_1"] = int((has & (x0 == -1)).sum())
            led["y0_minus_1"] = int((has & (y0 == -1)).sum())
            ix = np.where(has, x0, 0).astype(np.int64)
            iy = np.where(has, y0, 0).astype(np.int64)
            Wsum, hr, hg, hb, hl = (np.zeros((h, w), np.float32) for _ in range(5))
            for oy in (0, 1):
                wy = ay if oy else F(1) - ay
                for ox in (0, 1):
                    wt = wy * (ax if ox else F(1) - ax)
                    tx, ty = ix + ox, iy + oy
                    ok = cut(has, "tap_off_frame", ~((tx >= 0) & (tx < Wo) & (ty >= 0) & (ty < Ho)))
                    lx, ry = tx - gx0, ty - gy0
                    ok = cut(ok, "tap_off_columns", ~((lx >= 0) & (lx < tw)))
                    ok = cut(ok, "tap_below_share", ~(ry >= 0))
                    r = ry % bs
                    ly = (ry // bs) * br + r
                    ok = cut(ok, "tap_band_gap", ~(r < br))
                    ok = cut(ok, "tap_past_share", ~(ly < th))
                    lxc, lyc = np.where(ok, lx, 0), np.where(ok, ly, 0)
                    ok = cut(ok, "tap_class", ~(hist["cls"][lyc, lxc] == cls))
                    if not sphere_same:
                        ok = cut(ok, "tap_sphere_moved", ~((cls & 4) == 0))
                    nt, pt, hc = hist["n"][lyc, lxc], hist["p"][lyc, lxc], hist["col"][lyc, lxc]
                    ok = cut(ok, "tap_normal", ~(dot(nt, n) >= F(normal_min)))
                    ok = cut(ok, "tap_plane", ~(np.abs(dot((pt - p).astype(np.float32), n)) <= tol))
                    led["tap_valid"] += int(ok.sum())
                    Wsum = np.where(ok, Wsum + wt, Wsum)
                    hr = np.where(ok, hr + wt * hc[..., 0], hr)
                    hg = np.where(ok, hg + wt * hc[..., 1], hg)
                    hb = np.where(ok, hb + wt * hc[..., 2], hb)
                    hl = np.where(ok, hl + wt * hc[..., 3], hl)
            found = Wsum > 0
            nh = hl / Wsum
            under = nh < F(max_history)
            led["wsum_zero"] = int((has & ~found).sum())
            led["found_uncapped"] = int((found & under).sum())
            led["found_capped"] = int((found & ~under).sum())
            nh = np.where(under, nh, F(max_history)).astype(np.float32)
            den = nh + s
            for ch, acc in enumerate((hr, hg, hb)):
                out[..., ch] = np.where(found, (nh * (acc / Wsum) + s * c[..., ch]) / den, c[..., ch])
            ln = np.where(found, den, ln).astype(np.float32)
    col = out.copy()
    col[..., 3] = ln
    new = dict(col=col, cls=cls, n=n.copy(), p=p.copy(), view=cur_view)
    return (out, ln, new) + ((coords,) if want_coords else ()) + ((led,) if want_ledger else ())
