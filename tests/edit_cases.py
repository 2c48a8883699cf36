"""The edits of tests/test_edit_ref.py (CPU) and tests/test_edit.py (GPU) on the scenes of tests/build_cases.py and tests/ploc_cases.py:
the smallest at which each step of an edit (include/gpuart_edit.h) can go wrong — the first and the last ordinal, a run of removals across
a workgroup boundary, results of 1, 2, 3, 256 and 257 primitives, one workgroup that becomes three, every type added to triangles, every
type but triangles removed. Per case — computed once per process and left unchanged — the restatement's edited list
(tests/edit_ref.py) and the restatements' trees of it (tests/build_ref.py, tests/ploc_ref.py)."""
import functools

import numpy as np

from tests import build_cases as BC
from tests import edit_ref as ER
from tests import ploc_cases as PC
from tests import refit_ref as RR

SPHERE, DISC, TRIANGLE, CONE = 0, 1, 2, 3
MODES = ("morton", "clustered")


def payloads(descs):
    return [(t, RR.payload_of((t, f))) for t, f in descs]


def one_of_each(seed=3):
    """A sphere, a disc, a triangle and a cone inside [-2, 2]^3."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-1.5, 1.5, (4, 3))
    tri = np.concatenate([c[2], c[2] + rng.uniform(-0.5, 0.5, 3), c[2] + rng.uniform(-0.5, 0.5, 3)])
    return payloads([(SPHERE, [*c[0], 0.3]), (DISC, [*c[1], 0.0, 0.6, 0.8, 0.25]), (TRIANGLE, tri.tolist()),
                     (CONE, [*c[3], *(c[3] + np.array([0.3, 0.2, 0.6])), 0.25, 0.1])])


def _not_triangles(prims):
    return [i for i, (t, _) in enumerate(prims) if t != TRIANGLE]


# name: (scene, prims -> removals, prims -> additions)
CASES = {
    "neither": ("scene_p", lambda p: [], lambda p: []),
    "remove_only": ("box", lambda p: [1, 4, 5], lambda p: []),
    "add_only": ("box", lambda p: [], lambda p: one_of_each()),
    "both": ("scene_p", lambda p: [0, 3, len(p) - 1], lambda p: one_of_each(5)[:3]),
    "boundary": ("tris513", lambda p: [0, 254, 255, 256, 257, 258, 512], lambda p: []),   # first, last, across threads 255 | 256
    "every_second": ("tris257", lambda p: list(range(0, 257, 2)), lambda p: []),
    "to_one": ("n3", lambda p: [0, 2], lambda p: []),                                      # the root is a leaf of one
    "to_one_added": ("n1", lambda p: [0], lambda p: one_of_each()[3:]),                   # ... and that one an addition
    "to_two": ("n3", lambda p: [1], lambda p: []),
    "to_three": ("n2", lambda p: [], lambda p: one_of_each()[:1]),
    "to_256": ("tris257", lambda p: [100], lambda p: []),
    "to_257": ("tris257", lambda p: [5], lambda p: one_of_each()[:1]),
    "grow": ("flat", lambda p: [7], lambda p: payloads(BC._triangles(400, 21))),          # 126 -> 525: one workgroup becomes three
    "shrink": ("tris513", lambda p: list(range(100, 400)), lambda p: []),                 # 513 -> 213
    "types_into_triangles": ("flat", lambda p: [], lambda p: one_of_each(8)),
    "triangles_left": ("box", _not_triangles, lambda p: []),
    "mesh20k": ("mesh20k", lambda p: list(range(3, len(p), 101)), lambda p: payloads(BC._triangles(150, 33)) + one_of_each(9)[:1]),
}
SMALL = [n for n in CASES if n != "mesh20k"]


def scene(name):
    return BC.case(name) if name in BC.SCENES else PC.case(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(scene, tree: the tree to upload, prims: its primitives, remove (uint32), added, types (uint32), payload (n x 16), edited: the
    restatement's list, source)."""
    sc, rem, add = CASES[name]
    s = scene(sc)
    prims = s["prims"]
    remove, added = rem(prims), add(prims)
    edited, source = ER.edit(prims, remove, added)
    payload = np.array([d for _, d in added], np.float32).reshape(-1, 16)
    return dict(scene=sc, tree=s["tree"], prims=prims, remove=np.array(remove, np.uint32), added=added,
                types=np.array([t for t, _ in added], np.uint32), payload=payload, edited=edited, source=source)


@functools.lru_cache(maxsize=None)
def built(name, mode):
    """dict(tree: the restatement's tree of the case's edited list in `mode`, new_to_old, composed: source[new_to_old], info: ploc_ref's)."""
    from tests import build_ref as BR
    from tests import ploc_ref as PR
    c = case(name)
    info = {}
    tree, new_to_old = BR.build(c["edited"]) if mode == "morton" else PR.build(c["edited"], info=info)
    composed = c["source"][new_to_old]
    for a in (tree, new_to_old, composed):
        a.setflags(write=False)
    return dict(tree=tree, new_to_old=new_to_old, composed=composed, info=info)


# ---- refusals: name -> (removals, additions, first_bad) on the scene "box" ---------------------------------------------------------
def refusals(n_old):
    good = one_of_each()

    def spoilt(k, word, value):
        t, d = good[k]
        d = d.copy()
        d[word] = value
        return [good[0], (t, d)]
    return {
        "descending": ([2, 1], [], 1),
        "repeated": ([0, 3, 3], [], 2),
        "out of range": ([1, n_old], good[:1], 1),
        "a type above 3": ([], [good[0], (4, good[0][1])], 1),
        "a NaN": ([2], spoilt(2, 5, np.nan), 2),
        "beyond 2^20": ([], spoilt(0, 1, 2.0 ** 20 * 1.5), 1),
        "a negative radius": ([], spoilt(1, 3, -0.5), 1),
        "a negative length": ([], spoilt(3, 11, -1.0), 1),
        "a cone's width coefficient": ([], spoilt(3, 12, 7.0), 1),
        "a cone's cosB": ([], spoilt(3, 13, 0.9), 1),
        "nothing left": (list(range(n_old)), [], None),
    }
