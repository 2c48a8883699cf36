"""The cases of tests/test_within.py: the rule cases of tests/nearest_cases.py under eight radii per query, the trees of the walk tests,
the named queries that tell the wrong rules from the right one, and the query sets of the device tests with the spread of list lengths
they must show. Everything is computed once per process and left unchanged."""
import functools

import numpy as np

from tests import nearest_cases as NC
from tests import nearest_ref as NR

F = np.float32
INF, NAN = float("inf"), float("nan")
RADII_PER_QUERY = 8
RADIUS_CYCLE = (0.02, 0.1, 0.25, 0.5)    # x the root extent


def root_leaf(recs):
    """The primitives as one unflagged leaf that is the root: (tree records: none, primitive records with the leaf's count in the first
    one's word 3, root ref). The rule cases have no tree of their own; their order is the ordinals'."""
    prims = np.array(recs, F)
    w = prims.view(np.uint32)
    w[0, 0, 3] = (w[0, 0, 3] & 3) | len(prims) << 2
    prims.setflags(write=False)
    return np.zeros((0, 4, 4), F), prims, NR.REF_LEAF


@functools.lru_cache(maxsize=None)
def rule_case(name):
    """dict(recs (0, 4, 4), prims, boxes, root, points (8 n, 4)) of the rule case `name`: every query under the radii 0, 1e-30, its own
    nearest distance (so that the nearest primitive is at exactly r, when the product r r rounds to its d2), that distance's nextafter
    downwards, the median of its distances to the case's primitives (a radius reaching about half of them), +inf, NaN and -1."""
    c = NC.rule_case(name)
    recs, prims, root_ref = root_leaf(c["recs"])
    boxes = c["boxes"]
    base = c["points"]
    free = np.array(base)
    free[:, 3] = INF
    nearest = NR.brute(prims, boxes, free)["dist"]
    with np.errstate(all="ignore"):
        d = np.sqrt(np.stack([NR.closest_on_prim(prims[k], boxes[k], base[:, :3])[1] for k in range(len(prims))]))
    half = np.sort(d, 0)[(len(prims) - 1) // 2]
    rows = []
    for i, p in enumerate(base[:, :3]):
        for r in (0.0, 1e-30, nearest[i], np.nextafter(nearest[i], F(-INF)), half[i], INF, NAN, -1.0):
            rows.append([*p, r])
    points = np.array(rows, F)
    points.setflags(write=False)
    lo, hi = boxes[:, :3].min(0), boxes[:, 3:].max(0)
    return dict(recs=recs, prims=prims, boxes=boxes, root=(lo, hi, root_ref), points=points)


# ---- the trees of the walk tests ---------------------------------------------------------------------------------------------------------
TREE_SCENES = {"mixed7": lambda: NC.mixed(7, 3), "mixed300": lambda: NC.mixed(300), "chain": lambda: NC.chain(24)}


def payloads(descs):
    from tests import refit_ref as RR
    return [(t, RR.payload_of((t, f))) for t, f in descs]


@functools.lru_cache(maxsize=None)
def tree(name, kind):
    """The compiled tree of a scene by the Morton ("morton") or the clustered ("clustered") restatement."""
    from tests import build_ref as BR
    from tests import ploc_ref as PR
    t = (BR if kind == "morton" else PR).build(payloads(TREE_SCENES[name]()))[0]
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def tree_arrays(name, kind):
    """(recs, prims, boxes, root) of tree(name, kind)."""
    return NR.from_tree(tree(name, kind))


# ---- the query sets ------------------------------------------------------------------------------------------------------------------------
def extent(boxes):
    boxes = np.asarray(boxes, np.float64)
    return float((boxes[:, 3:].max(0) - boxes[:, :3].min(0)).max())


def query_set(boxes, n, seed=0):
    """nearest_cases.points_for(boxes, n, seed) with the radii replaced by a cycle over RADIUS_CYCLE x the root extent; every 16th query
    keeps its special radius (0, 1e-30, NaN, negative)."""
    points = np.array(NC.points_for(boxes, n, seed))
    cycle = np.array(RADIUS_CYCLE, F) * F(extent(boxes))
    i = np.arange(n)
    points[:, 3] = np.where(i % 16 == 5, points[:, 3], cycle[i % 4])
    return points


def assert_spread(offsets, n_prims):
    """The lists of a device test's query set, by the restatement: at least 4 empty, at least 4 of exactly one item, at least 4 of 9 or
    more, and one of 33 or more where the scene has 33 primitives at all (the box scene has 9, and 11 after its edit: no list there can
    be longer, and the lists of 9 or more are its long ones)."""
    ln = np.diff(np.asarray(offsets).astype(np.int64))
    assert (ln == 0).sum() >= 4 and (ln == 1).sum() >= 4 and (ln >= 9).sum() >= 4 and (ln.max() >= 33 or n_prims < 33), \
        ((ln == 0).sum(), (ln == 1).sum(), (ln >= 9).sum(), ln.max())
