"""NumPy float32 restatement of include/gpuart_edges.h, operation by operation in the order the header states.

Sub-samples and candidates are taken one at a time in the stated order, never by a reduction, so every value is the one the kernels of
gpuart_amd/csrc/edges/edges.hip compute, bit for bit. Images are (h, w, 4) float32, row 0 at the bottom; a G-buffer is (h, w, 8)
float32 words of gpuart_ray_hit and (h, w) int32 ordinals; the sub-pixel records are (n_sub, n, 8) words and (n_sub, n) ordinals,
sub-sample k of list[i] at [k, i], as gpuart_hip_trace_subpixel lays them out."""
import numpy as np

from tests import denoise_ref as D

F = np.float32
DEFAULTS = dict(n_sub=8, normal_min=0.95, plane_tol=0.02)
MAX_SUB = 16
# GPUART_EDGES_ROTATION and GPUART_EDGES_RGSS: perm(k) = (k * ROTATION[n_sub]) mod n_sub, for n_sub = 4 RGSS
ROTATION = (0, 1, 1, 2, 0, 2, 5, 3, 3, 4, 3, 4, 5, 5, 5, 4, 7)
RGSS = (2, 0, 3, 1)
# the candidates of resolve as (dy, dx), in the order they are tried
CANDIDATES = ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))
SKY, SPHERE, SURFACE = 0, 1, 2
LEDGER_KEYS = tuple("cand_%d" % c for c in range(9)) + ("unmatched", "sky", "sphere", "surface", "listed", "unlisted")


def records(words, prims, us_flags):
    """The fields match() reads of records (..., 8) / (...): dict of pos, p, n, type, us, cls."""
    words = np.asarray(words).view(np.float32)
    prims = np.asarray(prims, np.int32)
    t = np.ascontiguousarray(words[..., 7]).view(np.int32)
    hit = t >= 0
    us = hit & (prims == -2)
    cls = np.where(~hit, SKY, np.where(us & bool(us_flags & (D.EM_NONZERO | D.SPECULAR)), SPHERE, SURFACE))
    return dict(pos=words[..., 0], p=words[..., 1:4], n=words[..., 4:7], type=t, us=us, cls=cls)


def match(a, b, normal_min, plane_tol):
    """match(a, b) of the header, elementwise over two record dicts of one shape."""
    with np.errstate(all="ignore"):
        same = a["cls"] == b["cls"]
        dn = (a["n"][..., 0] * b["n"][..., 0] + a["n"][..., 1] * b["n"][..., 1]) + a["n"][..., 2] * b["n"][..., 2]
        d = a["p"] - b["p"]
        dist = np.abs((b["n"][..., 0] * d[..., 0] + b["n"][..., 1] * d[..., 1]) + b["n"][..., 2] * d[..., 2])
        lim = F(plane_tol) * D.gt_or(b["pos"], 1e-6)
        surf = (a["type"] == b["type"]) & (a["us"] == b["us"]) & (dn > F(normal_min)) & (dist <= lim)
    return same & ((a["cls"] != SURFACE) | surf)


def _shift_rec(r, oy, ox):
    out = {}
    inside = None
    for k, v in r.items():
        out[k], inside = D.shift(v, oy, ox)
    return out, inside


def mark(words, prims, us_flags=0, normal_min=0.95, plane_tol=0.02, **_):
    """-> the ascending list of edge pixels (uint32); its length is the count."""
    h, w = np.asarray(prims).shape
    words = np.asarray(words).view(np.float32).reshape(h, w, 8)
    own = records(words, prims, us_flags)
    edge = np.zeros((h, w), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy == 0 and dx == 0:
                continue
            q, inside = _shift_rec(own, dy, dx)
            edge |= inside & ~match(q, own, normal_min, plane_tol)
    return np.flatnonzero(edge.reshape(-1)).astype(np.uint32)


def resolve(filtered, words, prims, lst, sub_words, sub_prims, us_flags=0, n_sub=8, normal_min=0.95, plane_tol=0.02, want_ledger=False):
    """-> out (h, w, 4)[, ledger]. The ledger counts, per (listed pixel, sub-sample), the candidate that won (cand_0 is the pixel
    itself) or `unmatched` and the sub-sample's class, and the listed (with repeats) and unlisted pixels."""
    f = np.array(filtered, np.float32)
    h, w = f.shape[:2]
    words = np.asarray(words).view(np.float32).reshape(h, w, 8)
    prims = np.asarray(prims, np.int32).reshape(h, w)
    lst = np.asarray(lst, np.int64).reshape(-1)
    n = lst.size
    out = f.copy()
    led = dict.fromkeys(LEDGER_KEYS, 0)
    led["listed"] = n
    led["unlisted"] = h * w - np.unique(lst).size
    if n == 0:
        return (out, led) if want_ledger else out
    sub_words = np.asarray(sub_words).view(np.float32).reshape(n_sub, n, 8)
    sub_prims = np.asarray(sub_prims, np.int32).reshape(n_sub, n)
    centre = records(words, prims, us_flags)
    y, x = lst // w, lst % w
    own = f[y, x]
    total = np.zeros((n, 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(n_sub):
            s = records(sub_words[k], sub_prims[k], us_flags)
            c = own[:, :3].copy()
            done = np.zeros(n, bool)
            for ci, (dy, dx) in enumerate(CANDIDATES):
                qy, qx = y + dy, x + dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)
                m = {key: v[qy, qx] for key, v in centre.items()}
                win = inside & ~done & match(s, m, normal_min, plane_tol)
                fm = f[qy, qx][:, :3]
                surf = (fm / D.PRIMITIVE_COLOR[m["type"] & 3]) * D.PRIMITIVE_COLOR[s["type"] & 3]
                c = np.where(win[:, None], np.where((s["cls"] == SURFACE)[:, None], surf, fm), c).astype(np.float32)
                done |= win
                led["cand_%d" % ci] += int(win.sum())
            led["unmatched"] += int((~done).sum())
            for name, cls in (("sky", SKY), ("sphere", SPHERE), ("surface", SURFACE)):
                led[name] += int((s["cls"] == cls).sum())
            total = total + c
        out[y, x, :3] = total / F(n_sub)
    return (out, led) if want_ledger else out


def offsets(n_sub):
    """The (n_sub, 2) sub-pixel offsets (rand1, rand2) gpuart_hip_trace_subpixel is given: gpuart_edges_offsets."""
    k = np.arange(n_sub)
    perm = np.array(RGSS) if n_sub == 4 else (k * ROTATION[n_sub]) % n_sub
    return np.stack([(k.astype(np.float32) + F(0.5)) / F(n_sub), (perm.astype(np.float32) + F(0.5)) / F(n_sub)], 1).astype(np.float32)
