"""The cases of tests/test_knn.py: the values of k, the query sets of the tree tests, and the named inputs that tell each wrong rule of
tests/knn_ref.py from the right one. Everything is computed once per process and left unchanged."""
import functools

import numpy as np

from tests import nearest_cases as NC
from tests import nearest_ref as NR
from tests import within_cases as WC

F = np.float32
INF = float("inf")
KS = (1, 2, 3, 8, 9, 32)       # one, a heap of two levels, a capacity's edge from both sides (8 | 9), the most
KNN_MAX = 32


@functools.lru_cache(maxsize=None)
def tree_queries(name, kind):
    """(recs, prims, boxes, root, points) of a tree of within_cases.TREE_SCENES and its 64 interleaved queries."""
    recs, prims, boxes, root = WC.tree_arrays(name, kind)
    points = NC.points_for(boxes, 64, seed=len(prims))
    points.setflags(write=False)
    return recs, prims, boxes, root, points


@functools.lru_cache(maxsize=None)
def duplicates():
    """The Morton tree of nearest_cases.duplicates() with its own queries: six coincident spheres in at least three leaves of different
    subtrees, at the same d2 from each query — and for the first three queries that d2 is also box_d2 of every box above a copy. With
    k < 6 the answer is the k lowest ordinals: a walk that skips a box AT the worst kept d2 never sees the copies it has not met yet,
    and one that lets a tie stand keeps whichever copies it met first. With k >= 6 all six fit and neither rule can go wrong."""
    from tests import build_ref as BR
    prims, points = NC.duplicates()
    recs, dprims, boxes, root = NR.from_tree(BR.build(prims)[0])
    return recs, dprims, boxes, root, points


def unsorted_case():
    """mixed7's Morton tree and points with no radius: every query keeps k = 3 of seven primitives at three different distances. A
    max-heap's first entry is its worst, so written in the heap's order the farthest comes first: the order clause bites on every row."""
    recs, prims, boxes, root = WC.tree_arrays("mixed7", "morton")
    points = np.array(NC.points_for(boxes, 16, seed=2))
    points[:, 3] = INF
    return recs, prims, boxes, root, points, 3


def unclamped():
    """nearest_cases.unclamped(): one sphere and a point whose unclamped nearest point leaves the sphere's box by an ulp. The first record
    of the row holds q, which the clamp puts on the box's face: without it the record is another (and the miss behind it is the same)."""
    prims, points = NC.unclamped()
    recs, boxes = NC.device_list(prims)
    return recs, boxes, points, 2
