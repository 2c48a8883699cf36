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


SCENES = {
    "n1": lambda: _some(1),                                      # the root is a leaf
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
