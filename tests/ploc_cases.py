"""The scenes of tests/test_ploc_ref.py (CPU) and tests/test_ploc.py (GPU): tests/build_cases.py's, and the shapes at which the clustered
rebuild (include/gpuart_ploc.h) can go wrong; per scene — computed once per process and left unchanged — the reference-built tree, its
primitives and the restatement's clustered tree (tests/ploc_ref.py)."""
import functools

import numpy as np

from tests import build_cases as BC
from tests import ploc_ref as PR
from tests.test_ray_queries import tree_prims

SCENES = {n: f for n, f in BC.SCENES.items() if n not in BC.SHARP}
SCENES.update({
    # every key ties and d(i, j) is the larger sphere's area: one merge per iteration, 39 iterations, a chain of 39 levels in which every
    # interior node has a leaf of one
    "nested40": lambda: [(BC.SPHERE, [0.0, 0.0, 0.0, float(np.float32(1.1) ** k)]) for k in range(40)],
    "n17": lambda: BC._some(17),              # 2 r + 1: the window is clipped at both ends at once
    "tris513": lambda: BC._triangles(513, 6),  # mutual pairs across two workgroup boundaries of the nearest kernel
})
SCENES.update(BC.SHARP)                        # behind the others: the device tests number their cases
# 1 099 iterations: beyond the cap, refused (no tree)
REFUSED = {"chain1100": lambda: [(BC.SPHERE, [0.0, 0.0, 0.0, 1.0 + k / 1024.0]) for k in range(1100)]}
SMALL = [n for n in SCENES if n != "mesh20k"]


CONCENTRIC = ("nested40", "chain1100")


def reference_tree(name, descs):
    """The tree the case starts from: the reference-built one — but of the concentric spheres, whose order is the case, a tree that keeps
    them in the order given: every key ties, so the Morton restatement's stable sort leaves them where they are."""
    if name in CONCENTRIC:
        from tests import build_ref as BR
        from tests import refit_ref as RR
        tree, order = BR.build([(t, RR.payload_of((t, f))) for t, f in descs])
        assert (order == np.arange(len(descs))).all()
        return tree
    from oracle import oracle
    return np.ascontiguousarray(oracle.build_bvh(descs)[0], np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(descs, tree: the reference-built tree, prims: tree_prims(tree), built: the restatement's clustered tree of them, new_to_old,
    info: what ploc_ref.build reports)."""
    if name in BC.SCENES:
        c = BC.case(name)
        descs, tree, prims = c["descs"], c["tree"], c["prims"]
    else:
        descs = SCENES[name]()
        tree = reference_tree(name, descs)
        prims = tree_prims(tree)
    info = {}
    built, new_to_old = PR.build(prims, info=info)
    for a in (tree, built, new_to_old, info["refs"]):
        a.setflags(write=False)
    return dict(descs=descs, tree=tree, prims=prims, built=built, new_to_old=new_to_old, info=info)


@functools.lru_cache(maxsize=None)
def refused(name):
    """dict(descs, tree, prims) of a scene the build refuses."""
    descs = REFUSED[name]()
    tree = reference_tree(name, descs)
    tree.setflags(write=False)
    return dict(descs=descs, tree=tree, prims=tree_prims(tree))


@functools.lru_cache(maxsize=None)
def drift_clustered():
    """The clustered tree of build_cases.drift()'s drifted primitives."""
    built, new_to_old = PR.build(tree_prims(BC.drift()["refitted"]))
    built.setflags(write=False)
    return built, new_to_old
