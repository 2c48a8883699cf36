"""The cases of tests/test_overlap.py: the query boxes of the rule cases and the trees, the margins, the named cases that tell the wrong
rules from the right one, and the query sets of the device tests with the spread of list lengths they must show. Everything is chosen on
the CPU, by the restatement (tests/overlap_ref.py), and left unchanged."""
import functools

import numpy as np

from tests import nearest_cases as NC
from tests import nearest_ref as NR
from tests import overlap_ref as OR
from tests import within_cases as WC

F = np.float32
INF, NAN = float("inf"), float("nan")
SIZE_CYCLE = (0.0, 0.05, 0.15, 0.4, 1.2)     # a query box's edge, x the root extent: a point ... more than the root
MARGIN_FACTORS = (0.0, None, 0.02, 0.25)     # x the root extent; None: 1e-30, below every difference of two coordinates


def margins(boxes):
    """The four margins of a scene: 0, 1e-30, 0.02 and 0.25 times the root extent."""
    e = WC.extent(boxes)
    return [float(F(1e-30)) if f is None else float(F(f * e)) for f in MARGIN_FACTORS]


def root_of(boxes):
    boxes = np.asarray(boxes, np.float64)
    return boxes[:, :3].min(0), boxes[:, 3:].max(0)


INVALID = ([NAN, 0, 0, 1, 1, 1], [0, 0, 0, 1, NAN, 1], [0, 0, 0, INF, 1, 1], [-INF, 0, 0, 1, 1, 1], [1, 0, 0, 0.5, 1, 1], [0, 0, 2, 1, 1, 1])


def special_boxes(boxes, points=None, stride=1):
    """The queries every CPU case includes: degenerate points (the case's own query points, or the primitives' box centres), every primitive's
    own box, the root box, a box outside the root, and the invalid ones — NaN, inf, lo > hi —, whose lists must be empty. stride: every
    stride-th point and primitive only."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    lo, hi = root_of(boxes)
    e = float((hi - lo).max()) or 1.0
    if points is None:
        points = (boxes[:, :3].astype(np.float64) + boxes[:, 3:]) / 2
    points = np.asarray(points, F)[:, :3]
    points = points[np.isfinite(points).all(1)]
    out = [np.concatenate([points, points], 1)[::stride], boxes[::stride], [[*lo, *hi]], [[*(hi + e), *(hi + 2 * e)]], [[*(lo - 2 * e), *(lo - e)]], INVALID]
    return np.concatenate([np.asarray(o, F).reshape(-1, 6) for o in out])


def random_boxes(boxes, n, seed=0):
    """n sub-boxes of the root at a cycle of sizes (SIZE_CYCLE), their centres uniform in the root box; every 16th query special: outside
    the root or invalid."""
    rng = np.random.default_rng(seed)
    lo, hi = root_of(boxes)
    e = float((hi - lo).max()) or 1.0
    c = rng.uniform(lo, hi, (n, 3))
    half = np.array(SIZE_CYCLE)[np.arange(n) % len(SIZE_CYCLE)][:, None] * e / 2 * rng.uniform(0.5, 1.0, (n, 3))
    half[np.arange(n) % len(SIZE_CYCLE) == 0] = 0.0
    q = np.concatenate([c - half, c + half], 1).astype(F)
    special = [[*(hi + e), *(hi + 2 * e)], *INVALID]
    for i in range(5, n, 16):
        q[i] = special[(i // 16) % len(special)]
    return q


def lengths(boxes, queries, margin):
    """The list lengths of box queries by the restatement's test, without the order: (n,) int64."""
    boxes, queries = np.asarray(boxes, F).reshape(-1, 6), np.asarray(queries, F).reshape(-1, 6)
    qlo, qhi = OR.inflate(queries, margin)
    with np.errstate(invalid="ignore"):
        hit = ((qlo[:, None] <= boxes[None, :, 3:]) & (boxes[None, :, :3] <= qhi[:, None])).all(-1)
    return (hit & OR.box_ok(queries)[:, None]).sum(1)


def query_set(boxes, n, seed=0, margin=0.0):
    """random_boxes with the spread condition seen to on the CPU: where fewer than six of them list exactly one primitive, the queries at
    i % 16 == 9 are replaced by small boxes that do — searched, by the restatement's test, among the corners and centres of the primitives'
    boxes and random points of the root, in a fixed order."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    q = random_boxes(boxes, n, seed)
    ln = lengths(boxes, q, margin)
    want = 6 - int((ln == 1).sum())
    if want > 0:
        rng = np.random.default_rng(seed + 1000)
        lo, hi = root_of(boxes)
        corners = np.concatenate([boxes[:, [0, 1, 2]], boxes[:, [3, 4, 5]], boxes[:, [0, 4, 2]], boxes[:, [3, 1, 5]], (boxes[:, :3] + boxes[:, 3:]) / 2])
        pool = np.concatenate([corners, rng.uniform(lo, hi, (4096, 3))]).astype(F)
        pool = np.concatenate([pool, pool], 1)
        ones = pool[lengths(boxes, pool, margin) == 1]
        slots = [i for i in range(9, n, 16)]
        for i, b in zip(slots, ones[:: max(1, len(ones) // max(1, len(slots)))]):
            q[i] = b
    q.setflags(write=False)
    return q


def assert_spread(offsets, n_prims):
    """WC.assert_spread: at least 4 empty lists, 4 of exactly one item, 4 of 9 or more, and one of 33 or more where the scene has 33."""
    WC.assert_spread(offsets, n_prims)


# ---- the scenes of the CPU tests ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rule_case(name):
    """dict(recs (0, 4, 4), prims, boxes, root, queries (n, 6)) of the rule case `name` of nearest_cases as one root leaf."""
    c = WC.rule_case(name)
    base = NC.rule_case(name)["points"]
    queries = np.concatenate([special_boxes(c["boxes"], base), random_boxes(c["boxes"], 32, seed=len(name))])
    queries.setflags(write=False)
    return dict(recs=c["recs"], prims=c["prims"], boxes=c["boxes"], root=c["root"], queries=queries)


@functools.lru_cache(maxsize=None)
def tree_case(name, kind):
    """(recs, prims, boxes, root, queries) of WC.tree_arrays(name, kind)."""
    recs, prims, boxes, root = WC.tree_arrays(name, kind)
    n = 96 if len(prims) > 100 else 48
    queries = np.concatenate([special_boxes(boxes, stride=max(1, len(prims) // 24)), random_boxes(boxes, n, seed=len(prims))])
    queries.setflags(write=False)
    return recs, prims, boxes, root, queries


# ---- the named cases of the wrong rules ------------------------------------------------------------------------------------------------------
def hand_leaf(boxes):
    """Primitives with hand-made boxes as one root leaf: unit spheres' records (an overlap query reads of them only the leaf's count)."""
    boxes = np.asarray(boxes, F).reshape(-1, 6)
    recs, _ = NC.device_list([NC.sphere((0, 0, 0), 1.0)] * len(boxes))
    recs0, prims, root_ref = WC.root_leaf(recs)
    lo, hi = root_of(boxes)
    return recs0, prims, boxes, (lo.astype(F), hi.astype(F), root_ref)


def touching():
    """A unit box and a query that touches it at exactly one face, x = 1, at margin 0: `<` in place of `<=` loses it."""
    return hand_leaf([[-1, -1, -1, 1, 1, 1]]), np.array([[1, -0.5, -0.5, 2, 0.5, 0.5]], F), 0.0


def margin_reaches():
    """The Morton tree of nearest_cases.duplicates() and the point (1.5, 0, 0) at margin 0.5: the inflated box touches the six coincident unit
    spheres' boxes at x = 1, the point itself lies outside the box of every leaf that holds copies only."""
    from tests import build_ref as BR
    return NR.from_tree(BR.build(NC.duplicates()[0])[0]), np.array([[1.5, 0, 0, 1.5, 0, 0]], F), 0.5


def asymmetry():
    """lo_0 = 1, hi_1 = 1 - 2^-24, m = 2^-25 as two primitives, and the same two in the other order. fl(1 - 2^-25) = 1 > hi_1: with the lower
    ordinal inflated {0, 1} is no pair; fl(hi_1 + 2^-25) = 1 >= lo_0: with the higher ordinal inflated it is one. Swapped, it is the
    other way round."""
    a, b = [1, 0, 0, 2, 1, 1], [0, 0, 0, float(F(1) - F(2.0 ** -24)), 1, 1]
    return hand_leaf([a, b]), hand_leaf([b, a]), float(F(2.0 ** -25))


def second_misses():
    """nearest_cases.second_of_two(): the root is a leaf of two (REF_TWO); a small box at the sphere overlaps the sphere's box alone."""
    from tests import build_ref as BR
    arrays = NR.from_tree(BR.build(NC.second_of_two()[0])[0])
    return arrays, np.array([[-2.1, -0.1, -0.1, -1.9, 0.1, 0.1]], F), 0.0


def coincident():
    """The Morton tree of nearest_cases.duplicates(): six coincident primitives, fifteen pairs at margin 0; listing j >= i adds every i."""
    from tests import build_ref as BR
    return NR.from_tree(BR.build(NC.duplicates()[0])[0]), 0.0
