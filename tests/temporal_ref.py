"""NumPy float32 restatement of the temporal accumulation of include/gpuart_temporal.h, operation by operation in the order the header
states.

The four taps are accumulated one at a time in the stated order (oy outer, ox inner), never by a reduction over the tap axes, so every
value is the one the kernel of gpuart_amd/csrc/temporal/temporal.hip computes, bit for bit. Images are (h, w, 4) float32, row 0 at the
bottom; the G-buffer is (h, w, 8) float32 words of gpuart_ray_hit (pos, p.xyz, n.xyz, type as int32 bits) and (h, w) int32 ordinals.
A view is the dict `view()` makes; a history is None or the dict `accumulate` returns as its third value."""
import numpy as np

F = np.float32
DEFAULTS = dict(max_history=4.0, plane_tol=0.01, normal_min=0.8)
EM_NONZERO, SPECULAR = 1, 2


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
    t = np.ascontiguousarray(words[..., 7]).view(np.int32)
    surf = t >= 0
    if us_flags & (EM_NONZERO | SPECULAR):
        surf &= prims != -2
    return np.where(surf, (t & 3) | np.where(prims == -2, 4, 0), -1).astype(np.int32)


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


def accumulate(hist, rgba, spp, words, prims, cur_view, max_history=4.0, plane_tol=0.01, normal_min=0.8, want_coords=False):
    """-> (out (h, w, 4), len (h, w), the history a commit leaves[, (fx, fy)])."""
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
    with np.errstate(all="ignore"):
        if hist is not None:
            hv = hist["view"]
            Wo, Ho, gx0, gy0, tw, th, br, bs = hv["geom"]
            sphere_same = hv["user_sphere"].tobytes() == cur_view["user_sphere"].tobytes()
            fx, fy, k, dn, d = backproject(p, hv)
            coords = (fx, fy)
            x0, y0 = np.floor(fx), np.floor(fy)
            ax, ay = fx - x0, fy - y0
            tol = F(plane_tol) * np.sqrt(dot(d, d))
            has = surf & (dn != 0) & (k > 0) & (x0 >= -1) & (x0 < F(Wo)) & (y0 >= -1) & (y0 < F(Ho))
            ix = np.where(has, x0, 0).astype(np.int64)
            iy = np.where(has, y0, 0).astype(np.int64)
            Wsum, hr, hg, hb, hl = (np.zeros((h, w), np.float32) for _ in range(5))
            for oy in (0, 1):
                wy = ay if oy else F(1) - ay
                for ox in (0, 1):
                    wt = wy * (ax if ox else F(1) - ax)
                    tx, ty = ix + ox, iy + oy
                    ok = has & (tx >= 0) & (tx < Wo) & (ty >= 0) & (ty < Ho)
                    lx, ry = tx - gx0, ty - gy0
                    ok &= (lx >= 0) & (lx < tw) & (ry >= 0)
                    r = ry % bs
                    ly = (ry // bs) * br + r
                    ok &= (r < br) & (ly < th)
                    lxc, lyc = np.where(ok, lx, 0), np.where(ok, ly, 0)
                    ok &= hist["cls"][lyc, lxc] == cls
                    if not sphere_same:
                        ok &= (cls & 4) == 0
                    nt, pt, hc = hist["n"][lyc, lxc], hist["p"][lyc, lxc], hist["col"][lyc, lxc]
                    ok &= dot(nt, n) >= F(normal_min)
                    ok &= np.abs(dot((pt - p).astype(np.float32), n)) <= tol
                    Wsum = np.where(ok, Wsum + wt, Wsum)
                    hr = np.where(ok, hr + wt * hc[..., 0], hr)
                    hg = np.where(ok, hg + wt * hc[..., 1], hg)
                    hb = np.where(ok, hb + wt * hc[..., 2], hb)
                    hl = np.where(ok, hl + wt * hc[..., 3], hl)
            found = Wsum > 0
            nh = hl / Wsum
            nh = np.where(nh < F(max_history), nh, F(max_history)).astype(np.float32)
            den = nh + s
            for ch, acc in enumerate((hr, hg, hb)):
                out[..., ch] = np.where(found, (nh * (acc / Wsum) + s * c[..., ch]) / den, c[..., ch])
            ln = np.where(found, den, ln).astype(np.float32)
    col = out.copy()
    col[..., 3] = ln
    new = dict(col=col, cls=cls, n=n.copy(), p=p.copy(), view=cur_view)
    return (out, ln, new, coords) if want_coords else (out, ln, new)
