"""The rules of the three tree contracts (include/gpuart_refit.h, gpuart_build.h, gpuart_ploc.h) broken one at a time — what a kernel, a
shared header or a build flag could get quietly wrong —, each as a context manager that patches one function of one restatement
(tests/refit_ref.py, tests/build_ref.py, tests/ploc_ref.py) and puts it back:

    with MUTANTS["key: reciprocal division"].apply():
        quads, new_to_old = build_ref.build(prims)      # the tree a library with that fault would make

tests/test_tree_mutants.py requires of every mutant, and of every operation it touches (Mutant.ops: the Morton build, the clustered
build, the refit), a small case of tests/build_cases.py / tests/ploc_cases.py whose tree differs from the true restatement's: the device
tests compare bytes on those cases, so a fault no case notices is a fault the suite cannot see.

A fused multiply-add is emulated through float64: the product of two float32 values is exact there, and the sum is rounded to float32
once. (The sum itself is first rounded to float64; a double rounding needs a tie that 53 bits produce from 24-bit operands only by
design, and a mutant is a fault model, not a contract.) Flushing is to a zero of the same sign, of operands and results alike.

EQUIVALENT lists what no regular, orderly scene can tell from the true rule: not a gap of the cases.

    mutant                                  why no scene notices
    --------------------------------------  ----------------------------------------------------------------------------------------
    key: t >= 0 in place of t > 0           the two differ for t = +-0 and for nothing else (a NaN fails both, and the flat axis' NaN t
                                            is behind `e > 0` either way); t = +-0 gives s = t * 2^21 = +-0 and q = uint32(s) = 0, the
                                            value the branch not taken leaves.
"""
import contextlib

import numpy as np

from tests import build_ref as BR
from tests import ploc_ref as PR
from tests import refit_ref as RR

F = np.float32
TINY = np.finfo(np.float32).tiny   # the smallest normal number
MORTON, PLOC, REFIT = "morton", "ploc", "refit"


class Mutant:
    def __init__(self, ops, *patches):
        self.ops, self.patches = ops, patches

    @contextlib.contextmanager
    def apply(self):
        old = [(m, n, getattr(m, n)) for m, n, _ in self.patches]
        for m, n, f in self.patches:
            setattr(m, n, f)
        try:
            yield
        finally:
            for m, n, f in old:
                setattr(m, n, f)


def ftz(x):
    """x with every subnormal element replaced by a zero of its sign."""
    x = np.asarray(x, F)
    return np.where(np.abs(x) < TINY, np.copysign(F(0), x), x).astype(F)


def fma(a, b, c):
    """float32(a * b + c) with one rounding to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


# ---- the key ------------------------------------------------------------------------------------------------------------------------
def keys_variant(reciprocal=False, nearest=False, clamp=True, flush=False, centre_of_sum=False, shifts=(2, 1, 0), or_equal=False):
    """build_ref.keys_of with one step of the rule replaced."""
    z = (lambda v: F(ftz(v))) if flush else (lambda v: v)

    def keys_of(lo, hi, rlo, rhi):
        keys = []
        with np.errstate(all="ignore"):
            for a, b in zip(lo, hi):
                key = 0
                for k in range(3):
                    ak, bk, rl, rh = z(a[k]), z(b[k]), z(rlo[k]), z(rhi[k])
                    if centre_of_sum:
                        c = z(F(z(F(ak + bk)) * F(0.5)))
                    else:
                        c = z(F(z(F(ak * F(0.5))) + z(F(bk * F(0.5)))))
                    e = z(F(rh - rl))
                    num = z(F(c - rl))
                    t = z(F(num * z(F(F(1.0) / e)))) if reciprocal else z(F(num / e))
                    q = 0
                    if e > 0 and (t >= 0 if or_equal else t > 0):
                        s = z(F(t * BR.SCALE))
                        s = min(s, F(4294967296.0))   # (a conversion that saturates, as the device's does)
                        v = int(np.rint(s)) if nearest else int(s)
                        q = min(BR.QMAX, v) if clamp else v & BR.QMAX
                    for bit in range(21):
                        key |= ((q >> bit) & 1) << (3 * bit + shifts[k])
                keys.append(key)
        return keys
    return keys_of


def _key(**kw):
    return Mutant((MORTON, PLOC), (BR, "keys_of", keys_variant(**kw)))


# ---- the Morton topology ------------------------------------------------------------------------------------------------------------
def _delta_constant_ties(K, i, j):
    x = K[i] ^ K[j]
    if x:
        return 64 - x.bit_length()
    return 1 << 30 if i == j else 64


def _leaf_keys_second(keys, order):
    return [keys[order[min(2 * j + 1, len(order) - 1)]] for j in range((len(order) + 1) // 2)]


def _split_smallest(K, a, b):
    d_ab = BR.delta(K, a, b)
    return min(g for g in range(a, b) if BR.delta(K, a, g) > d_ab)


# ---- boxes --------------------------------------------------------------------------------------------------------------------------
def _fold_fminf(lo, hi, clo, chi):
    """fminf / fmaxf as the device's instructions order zeros: -0 below +0."""
    take_lo = (clo < lo) | ((clo == lo) & np.signbit(clo) & ~np.signbit(lo))
    take_hi = (chi > hi) | ((chi == hi) & ~np.signbit(chi) & np.signbit(hi))
    return np.where(take_lo, clo, lo), np.where(take_hi, chi, hi)


def _fold_or_equal(lo, hi, clo, chi):
    return np.where(clo <= lo, clo, lo), np.where(chi >= hi, chi, hi)


def _leaf_box_reversed(boxes):
    lo, hi = np.full(3, RR.START_LO, F), np.full(3, RR.START_HI, F)
    for a, b in reversed(list(boxes)):
        lo, hi = RR.fold(lo, hi, a, b)
    return lo, hi


_prim_box = RR.prim_box


def _prim_box_cone_swapped(t, d):
    """std::min(b, a) and std::max(B, A): of equal values the other one."""
    if t != 3:
        return _prim_box(t, d)
    d = np.asarray(d, F)
    a, b = d[0:3] - d[3], d[4:7] - d[7]
    A, B = d[0:3] + d[3], d[4:7] + d[7]
    return np.where(a < b, a, b), np.where(B < A, A, B)


def _prim_box_flushed(t, d):
    lo, hi = _prim_box(t, ftz(d))
    return ftz(lo), ftz(hi)


# ---- the clustered build ------------------------------------------------------------------------------------------------------------
def _dist_true(e):
    return ((e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2]) + e[:, 2] * e[:, 0]).astype(F)


def _dist_contracted(e):
    """What -ffp-contract=fast makes of (x*y + y*z) + z*x: fma(z, x, fma(x, y, y*z))."""
    return fma(e[:, 2], e[:, 0], fma(e[:, 0], e[:, 1], (e[:, 1] * e[:, 2]).astype(F)))


def _dist_other_association(e):
    return (e[:, 0] * e[:, 1] + (e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0])).astype(F)


def _dist_flushed(e):
    e = ftz(e)
    return ftz(ftz(ftz(e[:, 0] * e[:, 1]) + ftz(e[:, 1] * e[:, 2])) + ftz(e[:, 2] * e[:, 0]))


def nearest_variant(dist=_dist_true, tie="xor", kernel_order=False, blocks=None, short_below=0):
    """ploc_ref._nearest with one step replaced. tie: what decides between equal distances — "xor" (i xor j, the rule), "low" (the
    lower j), "near" (the nearer position, then the lower j), None (the first met); kernel_order: candidates offered as k_pl_nearest
    meets them, j = i - R .. i + R; blocks: no pairs across multiples of it; short_below: the radius towards lower positions is that
    much shorter."""
    def _nearest(lo, hi, radius):
        c = len(lo)
        best_d = np.full(c, np.inf, F)
        best_x = np.full(c, 1 << 62, np.int64)
        nn = np.full(c, -1, np.int64)
        pos = np.arange(c, dtype=np.int64)

        def offer(i, j, d):
            ok = np.ones(len(i), bool)
            if blocks:
                ok &= i // blocks == j // blocks
            if short_below:
                ok &= (j > i) | (i - j <= radius - short_below)
            x = {"xor": i ^ j, "low": j, "near": np.abs(i - j) * (1 << 32) + j, None: np.full(len(i), 1 << 62, np.int64)}[tie]
            better = ok & ((d < best_d[i]) | ((d == best_d[i]) & (x < best_x[i])))
            i, j, d, x = i[better], j[better], d[better], x[better]
            best_d[i], best_x[i], nn[i] = d, x, j

        offs = range(1, min(radius, c - 1) + 1)
        with np.errstate(all="ignore"):
            for sign, off in ([(-1, o) for o in reversed(offs)] + [(1, o) for o in offs]) if kernel_order else [(0, o) for o in offs]:
                a, b = pos[:c - off], pos[off:]
                flo, fhi = RR.fold(lo[a], hi[a], lo[b], hi[b])
                d = dist((fhi - flo).astype(F))
                if sign >= 0:
                    offer(a, b, d)
                if sign <= 0:
                    offer(b, a, d)
        lone = nn < 0          # (a block of one cluster has nobody to ask: it waits)
        nn[lone] = pos[lone]
        return nn
    return _nearest


def _near(**kw):
    return Mutant((PLOC,), (PR, "_nearest", nearest_variant(**kw)))


def _slot_upper(lower, upper):
    return upper


def _pair_swapped_leaf(a, b):
    return ("pair", b, a) if a[0] == "prim" and b[0] == "prim" else ("pair", a, b)


ALL = (MORTON, PLOC, REFIT)
MUTANTS = {
    "key: reciprocal division": _key(reciprocal=True),
    "key: round to nearest": _key(nearest=True),
    "key: no clamp": _key(clamp=False),
    "key: denormals flushed": _key(flush=True),
    "key: centre (lo + hi) * 0.5": _key(centre_of_sum=True),
    "key: x and y swapped": _key(shifts=(1, 2, 0)),
    "morton: ties get a constant delta": Mutant((MORTON,), (BR, "delta", _delta_constant_ties)),
    "morton: a leaf's key from its second primitive": Mutant((MORTON,), (BR, "leaf_keys", _leaf_keys_second)),
    "morton: the smallest qualifying g": Mutant((MORTON,), (BR, "split", _split_smallest)),
    "box: fold by fminf / fmaxf": Mutant(ALL, (RR, "fold", _fold_fminf)),
    "box: fold by <= / >=": Mutant(ALL, (RR, "fold", _fold_or_equal)),
    "box: a leaf folded in reverse": Mutant(ALL, (RR, "leaf_box", _leaf_box_reversed)),
    "box: the cone's min / max swapped": Mutant(ALL, (RR, "prim_box", _prim_box_cone_swapped)),
    "box: primitive boxes flushed": Mutant(ALL, (RR, "prim_box", _prim_box_flushed)),
    "ploc: distance contracted": _near(dist=_dist_contracted),
    "ploc: distance associated the other way": _near(dist=_dist_other_association),
    "ploc: distance flushed": _near(dist=_dist_flushed),
    "ploc: ties to the lowest j": _near(tie="low"),
    "ploc: ties to the nearest position": _near(tie="near"),
    "ploc: ties to the first met": _near(tie=None, kernel_order=True),
    "ploc: no pairs across 256-boundaries": _near(blocks=256),
    "ploc: radius 7 towards lower positions": _near(short_below=1),
    "ploc: merged into the upper partner's slot": Mutant((PLOC,), (PR, "_slot", _slot_upper)),
    "ploc: a leaf of two swapped": Mutant((PLOC,), (PR, "_pair", _pair_swapped_leaf)),
}
EQUIVALENT = {
    "key: t >= 0 in place of t > 0": _key(or_equal=True),
}
