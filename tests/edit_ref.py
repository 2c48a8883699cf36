"""A plain restatement of the edit contract (include/gpuart_edit.h), in Python and NumPy float32:

    edit(prims, remove, added) -> (edited_prims, source)

`prims` are the primitives of an uploaded scene as tests/test_ray_queries.tree_prims lists them, (type, 16 floats of data quads) per device
ordinal; `remove` lists device ordinals, `added` is a list of (type, 16 floats). The edited list holds the survivors in their old order,
then the additions in the order given; source[q] is the old ordinal of the survivor at q, or len(prims) + k for the k-th addition. The
tree of an edit is then tests/build_ref.build(edited_prims) or tests/ploc_ref.build(edited_prims).

An edit is refused as a whole (Refused, with first_bad: the index of the first offender, the removals counted first, then the additions;
None where no single entry is at fault) unless

    the removals are strictly ascending and below len(prims);
    every added type is 0..3 and every added payload meets the primitive rule, restated here from the text of csrc/hip/prim_rule.h: every
      word the device reads — 4 of a sphere, 7 of a disc, 12 of a triangle but every fourth, 15 of a cone — is finite and at most 2^20 in
      magnitude; a sphere's and a disc's radius (word 3) is >= 0; a cone's radii (words 3, 7) and length (11) are >= 0, and with
      tol = 1e-4 (length + r1 + r2) + 1e-30: |c1 + length axis - c2| <= tol per axis, |r1 + wc length - r2| <= tol (wc word 12),
      | |axis|^2 - 1 | <= 1e-4 where length > 0, |word 14 - axis . c1| <= 1e-4 (|c1.x| + |c1.y| + |c1.z| + 1), and |word 13 - cosB| <= 1e-3
      with cosB = 0 where |r1 - r2| < 1e-7 or length = 0, else +-rr / sqrt(h^2 + rr^2), rr = max(r1, r2), h = rr length / |r1 - r2|, the
      sign that of r1 - r2; all in fp32;
    at least one primitive is left.

device_list(edited_prims) is what the library's staging arrays hold: per primitive the 48-byte record by the uploader's arithmetic (a
triangle's edges subtracted in fp32), word 3 of the first quad the bare type — in a list of one primitive with the count 1 above it — and
the box its constructor gives it (tests/refit_ref.prim_box restates that). Shares no code with the library.
"""
import numpy as np

from tests import refit_ref as RR

F = np.float32
LIMIT = F(1048576.0)
MAX_PRIMS = 0x05555540


class Refused(ValueError):
    def __init__(self, why, first_bad=None):
        super().__init__(why)
        self.first_bad = first_bad


def prim_ok(t, d):
    """The primitive rule for a payload d (16 floats) of type t."""
    if not 0 <= t <= 3:
        return False
    d = np.asarray(d, F)
    read = {0: range(4), 1: range(7), 2: [k for k in range(12) if k % 4 != 3], 3: range(15)}[t]
    with np.errstate(all="ignore"):
        if not all(np.abs(d[k]) <= LIMIT for k in read):   # (a NaN fails the comparison)
            return False
        if t in (0, 1):
            return bool(d[3] >= 0)
        if t == 2:
            return True
        c1, r1, c2, r2, axis, length, wc, cosb_given, dot_given = d[0:3], d[3], d[4:7], d[7], d[8:11], d[11], d[12], d[13], d[14]
        if not (r1 >= 0 and r2 >= 0 and length >= 0):
            return False
        tol = F(F(F(1.0e-4) * F(F(length + r1) + r2)) + F(1.0e-30))
        for k in range(3):
            if not np.abs(F(F(c1[k] + F(length * axis[k])) - c2[k])) <= tol:
                return False
        if not np.abs(F(F(r1 + F(wc * length)) - r2)) <= tol:
            return False
        ax2 = F(F(F(axis[0] * axis[0]) + F(axis[1] * axis[1])) + F(axis[2] * axis[2]))
        if length > 0 and not np.abs(F(ax2 - F(1.0))) <= F(1.0e-4):
            return False
        dot = F(F(F(axis[0] * c1[0]) + F(axis[1] * c1[1])) + F(axis[2] * c1[2]))
        if not np.abs(F(dot_given - dot)) <= F(F(1.0e-4) * F(F(F(np.abs(c1[0]) + np.abs(c1[1])) + np.abs(c1[2])) + F(1.0))):
            return False
        cosb = F(0.0)
        if np.abs(F(r1 - r2)) >= F(1.0e-7) and length > 0:
            rr = r1 if r1 > r2 else r2
            h = F(F(rr * length) / np.abs(F(r1 - r2)))
            cosb = F((rr if r1 > r2 else -rr) / np.sqrt(F(F(h * h) + F(rr * rr))))
        return bool(np.abs(F(cosb_given - cosb)) <= F(1.0e-3))


def edit(prims, remove, added):
    n_old = len(prims)
    remove = [int(r) for r in remove]
    for i, r in enumerate(remove):
        if i and not remove[i - 1] < r:
            raise Refused("removal %d does not exceed the one before it" % i, i)
        if not 0 <= r < n_old:
            raise Refused("removal %d is not below the number of primitives" % i, i)
    for k, (t, d) in enumerate(added):
        if not prim_ok(int(t), d):
            raise Refused("addition %d is outside the primitive rule" % k, len(remove) + k)
    gone = set(remove)
    source = [i for i in range(n_old) if i not in gone] + [n_old + k for k in range(len(added))]
    if not source:
        raise Refused("the edit leaves no primitive")
    if len(source) >= MAX_PRIMS:
        raise Refused("too many primitives")
    pad = lambda d: np.concatenate([np.asarray(d, F).reshape(-1), np.zeros(16, F)])[:16]
    edited = [(int(prims[s][0]), pad(prims[s][1])) if s < n_old else (int(added[s - n_old][0]), pad(added[s - n_old][1])) for s in source]
    return edited, np.array(source, np.int32)


def type_mask(prims):
    mask = 0
    for t, _ in prims:
        mask |= 1 << t
    return mask


def device_list(prims):
    """(records (n, 3, 4) float32, boxes (n, 6) float32) of the staging arrays."""
    n = len(prims)
    recs, boxes = np.zeros((n, 3, 4), F), np.zeros((n, 6), F)
    count = 1 if n == 1 else 0
    for q, (t, d) in enumerate(prims):
        d = np.asarray(d, F)
        r = recs[q]
        r[0, :3] = d[0:3]
        r.view(np.uint32)[0, 3] = t | count << 2
        if t == 0:
            r[1, 0] = d[3]
        elif t == 1:
            r[1, :3], r[1, 3] = d[4:7], d[3]
        elif t == 2:
            r[1, :3], r[2, :3] = d[4:7] - d[0:3], d[8:11] - d[0:3]
        else:
            r[1], r[2, 0], r[2, 1:] = d[8:12], d[3], d[12:15]
        lo, hi = RR.prim_box(t, np.concatenate([d, np.zeros(16, F)])[:16])
        boxes[q, :3], boxes[q, 3:] = lo, hi
    return recs, boxes
