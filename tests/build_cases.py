"""The scenes of tests/test_build_ref.py (CPU) and tests/test_build.py (GPU), the smallest at which each step of a rebuild can go wrong,
and per scene — computed once per process and left unchanged — the reference-built tree, its primitives and the restatement's tree
(tests/build_ref.py)."""
import functools

import numpy as np

from gpuart_amd import synth_scenes as S
from tests import build_ref as BR
from tests.test_ray_queries import tree_prims

SPHERE, DISC, TRIANGLE, CONE = 0, 1, 2, 3


def _some(n):
    """n primitives of mixed types at scattered places."""
    rng = np.random.default_rng(100 + n)
    out = []
    for k in range(n):
        c = rng.uniform(-2, 2, 3)
        if k % 3 == 0:
            out.append((SPHERE, [float(v) for v in c] + [float(rng.uniform(0.1, 0.4))]))
        elif k % 3 == 1:
            out.append((TRIANGLE, [float(v) for v in np.concatenate([c, c + rng.uniform(-0.5, 0.5, 3), c + rng.uniform(-0.5, 0.5, 3)])]))
        else:
            out.append((DISC, [float(v) for v in c] + [0.0, 0.0, 1.0, float(rng.uniform(0.1, 0.4))]))
    return out


def _triangles(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        c = rng.uniform(-3, 3, 3)
        out.append((TRIANGLE, [float(v) for v in np.concatenate([c, c + rng.uniform(-0.3, 0.3, 3), c + rng.uniform(-0.3, 0.3, 3)])]))
    return out


def _grid(nx, ny, z=lambda x, y: 0.0, size=4.0):
    """A mesh of 2 nx ny triangles over [-size/2, size/2]^2 at height z(x, y)."""
    xs, ys = np.linspace(-size / 2, size / 2, nx + 1), np.linspace(-size / 2, size / 2, ny + 1)
    v = lambda i, j: [float(xs[i]), float(ys[j]), float(z(xs[i], ys[j]))]
    out = []
    for j in range(ny):
        for i in range(nx):
            out.append((TRIANGLE, v(i, j) + v(i + 1, j) + v(i + 1, j + 1)))
            out.append((TRIANGLE, v(i, j) + v(i + 1, j + 1) + v(i, j + 1)))
    return out


def _mesh_20k():
    """100 x 100 x 2 triangles of a wavy sheet and 300 of them once more: equal keys beyond one block of the sort."""
    mesh = _grid(100, 100, lambda x, y: 0.3 * np.sin(2.0 * x) * np.cos(1.5 * y))
    rng = np.random.default_rng(9)
    return mesh + [mesh[int(k)] for k in rng.choice(len(mesh), 300, replace=False)]


# ---- the scenes that tell a wrong rule from the right one (tests/tree_mutants.py says which rules; tests/test_tree_mutants.py holds them to it)
def _dot(x, y, z, r=0.0):
    return (SPHERE, [float(x), float(y), float(z), float(r)])


def _rows(first=1500000, nx=10, ny=4):
    """Two anchors that make the root box [0, 2.7]^3 and nx x ny points at x = 2.7 m / 2^21, y = 2.7 (n + 0.5) / 2^21 for consecutive m
    and n, shuffled: t = x / 2.7 lands on or just below m / 2^21 by the last bit of the division, so (c - Rmin) * (1 / e) puts eight of
    the forty in the neighbouring x cell; the y cells are hit in the middle under either rule. A point that changes its x cell changes
    its place among the points of the other rows, so the order changes and not only the ties. (One row does not do: the reference
    builder lists a row's points in x order, and an order that is sorted already hides every tie.) The anchor at the maximum has t = 1
    exactly: s = 2^21, which only the clamp keeps inside 21 bits.
    Kills: key: reciprocal division, key: no clamp, key: round to nearest."""
    w, scale = np.float32(2.7), np.float32(2097152.0)
    pts = [(m, n) for m in range(first, first + nx) for n in range(first, first + ny)]
    pts = [pts[i] for i in np.random.default_rng(1).permutation(len(pts))]
    return [_dot(0, 0, 0), _dot(w, w, w)] + [_dot(w * np.float32(m) / scale, w * np.float32(n + 0.5) / scale, 1.5) for m, n in pts]


def _crowd(seed=0, n=48):
    """Two anchors and n points inside a 4 x 4 x 4 block of key cells in the middle of the root box, at fractional positions inside the
    cells (the first seed tried): the low bits of q on all three axes decide order, ties and topology.
    Kills: key: round to nearest (and whatever else moves a key by one cell)."""
    rng = np.random.default_rng(seed)
    cell = 1.0 / 2097152.0
    p = 0.5 + rng.uniform(0.0, 4.0, (n, 3)) * cell
    return [_dot(0, 0, 0), _dot(1, 1, 1)] + [_dot(*np.float32(v)) for v in p]


def _tiny():
    """Five spheres of radius 1e-20 a few 1e-20 apart and three ordinary ones: the extents of the small pairs are about 1e-20 and their
    products about 1e-40, below the smallest normal number — a distance computed with flushed denormals is 0 for all of them, and the
    xor rule pairs them instead of the distance. Every plane of the small boxes is below 2^-60: the tree is `subnormal`.
    Kills: ploc: distance flushed."""
    s = 1e-20
    small = [_dot(0.0, 0.0, 0.0, s), _dot(7 * s, s, 0.0, s), _dot(9 * s, 4 * s, 2 * s, s), _dot(20 * s, 2 * s, 5 * s, s), _dot(22 * s, 9 * s, s, s)]
    return small + [_dot(1.0, 0.5, 0.25, 0.125), _dot(0.5, 1.0, 0.75, 0.25), _dot(0.25, 0.25, 1.0, 0.125)]


def _denormals(seed=0):
    """Eight points at whole multiples, below 16, of 2^-149 on every axis (the first seed tried): every coordinate, centre and extent is
    a denormal. lo * 0.5 + hi * 0.5 rounds each half to even (1 gives 0, 3 gives 4), which (lo + hi) * 0.5 does not; flushed, every key
    and every box is zero.
    Kills: key: denormals flushed, key: centre (lo + hi) * 0.5, box: primitive boxes flushed."""
    rng = np.random.default_rng(seed)
    d = float(np.float32(2.0) ** -149)
    return [_dot(*(rng.integers(0, 16, 3) * d)) for _ in range(8)]


def _zeros():
    """Three points at zeros of mixed signs and two spheres above them: the minimum planes of the root and of the leaves below it are
    +0 or -0 by which of equal values the fold keeps.
    Kills: box: fold by fminf / fmaxf, box: fold by <= / >=, box: a leaf folded in reverse."""
    return [_dot(0.0, -0.0, 0.0), _dot(-0.0, 0.0, -0.0), _dot(0.0, 0.0, -0.0), _dot(1.0, 2.0, 3.0, 0.5), _dot(3.0, 1.0, 2.0, 0.25)]


def _zeros_update(prims):
    """The first point with +0 at x moves onto -0 and back."""
    k = next(i for i, (t, d) in enumerate(prims) if t == SPHERE and d[3] == 0 and not np.signbit(d[0]))
    there, back = prims[k][1].copy(), prims[k][1].copy()
    there[0] = -0.0
    return [(np.array([k], np.uint32), there[None]), (np.array([k], np.uint32), back[None])]


def _cone_zero():
    """A cone whose two ends reach x = 0 and z = 0 from different sides of zero: c1 - r1 = +0 and c2 - r2 = -0 (an apex, r2 = 0, at
    -0), equal values of which std::min(a, b) keeps a. Everything else lies above.
    Kills: box: the cone's min / max swapped."""
    return [(CONE, [1.0, 2.0, 1.0, -0.0, 4.0, -0.0, 1.0, 0.0]), _dot(2.0, 3.0, 2.0, 0.5), _dot(3.0, 1.0, 3.0, 0.25), _dot(1.5, 4.0, 1.5, 0.5)]


def _lattice():
    """27 equal spheres on a 3 x 3 x 3 lattice of pitch 0.37, jittered by 2e-7: the distances of neighbouring pairs agree to the last
    bits, and which is smallest depends on the rounding of every product and sum.
    Kills: ploc: distance contracted, ploc: distance associated the other way."""
    rng = np.random.default_rng(0)
    return [_dot(*(0.37 * np.array([i, j, k]) + rng.uniform(-2e-7, 2e-7, 3)), 0.1) for i in range(3) for j in range(3) for k in range(3)]


SHARP = {
    "rows42": _rows,
    "crowd50": _crowd,
    "tiny8": _tiny,
    "denormal8": _denormals,
    "zeros5": _zeros,
    "cone_zero": _cone_zero,
    "lattice27": _lattice,
}
SUBNORMAL = ("tiny8", "denormal8")   # the cases whose trees have planes below 2^-60: the quick boxes are withdrawn (box_slack = inf)
# per case, what makes its update from its primitives: a list of (ordinals, payloads), one refit on top of the other
UPDATES = {"zeros5": _zeros_update}

SCENES = {
    "n1": lambda: _some(1),                                     # the root is a leaf
    "n2": lambda: _some(2),                                      # one leaf, no record
    "n3": lambda: _some(3),
    "n4": lambda: _some(4),
    "n5": lambda: _some(5),                                      # odd: the last leaf holds one primitive
    "same64": lambda: [(SPHERE, [0.5, -0.25, 1.0, 0.75])] * 64,  # every key ties: the index tie-break carries the whole topology
    "tris257": lambda: _triangles(257, 4),                       # odd, past one 256-thread block
    "flat": lambda: _grid(9, 7),                                 # zero extent on one axis
    "box": S.box_scene,                                          # every type
    "scene_p": S.scene_p,
    "scene_d": lambda: S.scene_d(24, 24),
    "mesh20k": _mesh_20k,
}
SCENES.update(SHARP)
SMALL = [n for n in SCENES if n != "mesh20k"]


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(descs, tree: the reference-built tree, prims: tree_prims(tree), built: the restatement's tree of them, new_to_old)."""
    from oracle import oracle
    descs = SCENES[name]()
    tree = np.ascontiguousarray(oracle.build_bvh(descs)[0], np.float32)
    prims = tree_prims(tree)
    built, new_to_old = BR.build(prims)
    for a in (tree, built, new_to_old):
        a.setflags(write=False)
    return dict(descs=descs, tree=tree, prims=prims, built=built, new_to_old=new_to_old)


@functools.lru_cache(maxsize=None)
def updates(name):
    """The case's update of its reference-built tree, a list of (ordinals, payloads) applied one after the other: its own where
    UPDATES has one, else three tenths of its primitives moved by up to 0.3."""
    from tests import refit_ref as RR
    c = case(name)
    if name in UPDATES:
        return UPDATES[name](c["prims"])
    return [RR.random_update(c["tree"], np.random.default_rng(5), 0.3, 0.3)]


# ---- the cost measure and the drift track -------------------------------------------------------------------------------------------
def half_area(lo, hi):
    d = np.asarray(hi, np.float64) - np.asarray(lo, np.float64)
    return d[..., 0] * d[..., 1] + d[..., 1] * d[..., 2] + d[..., 2] * d[..., 0]


def cost_of(tree):
    """gpuart_build_cost restated: math.fsum over the records of both children's half-areas, over the root's (fp64 from the fp32 planes)."""
    import math

    from tests import converter_ref as CR
    cv = CR.convert(tree)
    r = cv["recs"]
    terms = half_area(r[:, 0, :3], r[:, 1, :3]) + half_area(r[:, 2, :3], r[:, 3, :3])
    return math.fsum(terms.tolist()) / float(half_area(cv["root_min"], cv["root_max"])), len(r)


@functools.lru_cache(maxsize=None)
def drift():
    """Scene D with every primitive translated to another primitive's place (a fixed seeded shuffle): dict(tree: as built by the reference,
    ordinals, payloads: the update, refitted: the restatement's refit of it, rebuilt: the restatement's rebuild of the refitted primitives,
    new_to_old, rays: every third camera ray of the golden frame of scene D, tests/golden/frames_scene_d_seg5.npz).
    The rays are a renderer's, aimed at the mesh whose tree the drift degrades. Random rays through the root box do not measure it: the
    ground disc makes the root a 10-unit cube, the mesh is 1.5 units, and nineteen in twenty such rays never reach it — on them the
    oracle visits 10 106 nodes in the refitted tree and 16 972 in the rebuilt one, whose top levels the disc's box loosens (the Morton
    order puts a large primitive wherever its centre falls); on the camera rays it visits 883 300 and 107 946."""
    from oracle import oracle
    from tests import refit_ref as RR
    from tests.util import golden
    c = case("scene_d")
    prims = c["prims"]
    n = len(prims)
    centre = np.zeros((n, 3))
    for i, (t, d) in enumerate(prims):
        lo, hi = RR.prim_box(t, d)
        centre[i] = (lo.astype(np.float64) + hi.astype(np.float64)) / 2
    to = np.random.default_rng(77).permutation(n)
    ordinals = np.arange(n, dtype=np.uint32)
    payloads = np.stack([RR.moved(prims[i][0], prims[i][1], centre[to[i]] - centre[i]) for i in range(n)])
    refitted = RR.refit(c["tree"], ordinals, payloads)
    rebuilt, new_to_old = BR.build(tree_prims(refitted))
    g = golden("frames_scene_d_seg5")
    rs, rd = oracle.cam_rays(g["cam"], int(g["W"]), int(g["H"]))
    rs, rd = np.ascontiguousarray(rs.reshape(-1, 4)[::3]), np.ascontiguousarray(rd.reshape(-1, 4)[::3])
    for a in (payloads, refitted, rebuilt, new_to_old, rs, rd):
        a.setflags(write=False)
    return dict(tree=c["tree"], ordinals=ordinals, payloads=payloads, refitted=refitted, rebuilt=rebuilt, new_to_old=new_to_old, rays=(rs, rd))
