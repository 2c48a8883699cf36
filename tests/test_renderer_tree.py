"""Renderer.rebuild_tree and Renderer.edit_primitives at the sizes where the tree has no record or one: a root that is a leaf of one or
of two primitives, and three primitives under one record. There the read-back of the clustered build's ref words is skipped or is one
record long, and the host tree follows from an order alone. Both modes, scenes of tests/build_cases.py and edits of tests/edit_cases.py;
afterwards the host tree is what the host library makes of the uploaded quads without a device (binding.rebuild_tree, adopt_tree,
edit_tree, given the restatements' order and refs) byte for byte, and the refit handle binds to the new arrays."""
import pytest

from tests import build_cases as BC
from tests import edit_cases as EC
from tests import ploc_ref as PR
from tests import refit_ref as RR
from tests.test_ray_queries import tree_prims
from tests.util import same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def renderer(B, descs):
    from tests.test_temporal import TRACK, cam_dict
    r = B.Renderer(48, 32, cam_dict(TRACK[0]))
    r.set_primitives(descs)
    return r


def refits(r, descs):
    """update_primitives of the caller's first description (as it is) succeeds: the refit handle binds to the arrays as they are now."""
    return r.update_primitives([0], [descs[0]]) and r.is_ok()


@pytest.mark.parametrize("mode", EC.MODES)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_rebuild_tree_of_one_two_and_three_primitives(B, n, mode):
    descs = BC.case("n%d" % n)["descs"]
    r = renderer(B, descs)
    try:
        assert refits(r, descs)                      # (bound to the uploaded arrays: the rebuild makes that binding stale)
        uploaded = r.compile_bvh()
        perm = r.rebuild_tree(mode)
        assert perm is not None and len(perm) == n and r.is_ok()
        if mode == "morton":
            exp, order = B.rebuild_tree(uploaded)
        else:
            info = {}
            _, order = PR.build(tree_prims(uploaded), info=info)
            exp = B.adopt_tree(uploaded, order, info["refs"])
        assert (perm == order).all() and same_bits(r.compile_bvh(), exp)
        assert r.backend.scene_device().n_recs == (1 if n == 3 else 0)
        assert refits(r, descs)
    finally:
        r.close()


@pytest.mark.parametrize("mode", EC.MODES)
@pytest.mark.parametrize("name,n", [("to_one", 1), ("to_one_added", 1), ("to_two", 2), ("to_three", 3)])
def test_edit_primitives_down_to_one_two_and_three_primitives(B, name, n, mode):
    from tests.test_build import _ordinal_to_desc
    c = EC.case(name)
    descs = BC.case(c["scene"])["descs"]
    r = renderer(B, descs)
    try:
        uploaded = r.compile_bvh()
        desc_of = _ordinal_to_desc(uploaded, descs)
        gone = [desc_of[o] for o in c["remove"]]      # the caller's numbering of the case's device ordinals
        added = [RR.desc_of(t, d) for t, d in c["added"]]
        source = r.edit_primitives(gone, added, mode)
        assert source is not None and len(source) == n and r.is_ok()
        bt = EC.built(name, mode)
        exp, _ = B.edit_tree(uploaded, c["remove"], c["types"], c["payload"], order=bt["new_to_old"],
                             refs=bt["info"]["refs"] if mode == "clustered" else None)
        assert (source == bt["composed"]).all() and same_bits(r.compile_bvh(), exp)
        assert r.backend.scene_device().n_recs == (1 if n == 3 else 0)
        assert refits(r, [d for k, d in enumerate(descs) if k not in gone] + added)
    finally:
        r.close()
