"""The clustered rebuild's contract without a device (include/gpuart_ploc.h): the restatement's trees (tests/ploc_ref.py) have the shape
the contract states, are regular and orderly and fixed points of the refit rule; the host library's
BoundingVolumesHierarchy::AdoptTopology (through gpuart_adopt_tree) writes them from their order and refs in every word the device
reads, and refuses what is no tree; the clustered trees cost less than the Morton ones, by the cost measure and by the nodes the oracle
visits on the drift track; the iteration cap refuses; and the new entry points are declared and exported.

The quality conditions are those the float64 prototype of the contract met with room (costs 1.32 / 1.72 / 20.9 / 12.6 against the Morton
restatement's 11.4 / 7.8 / 41.7 / 17.0 on scene_d, scene_p, mesh20k and tris257); they are not thresholds fitted to this code."""
import ctypes as C
import os

import numpy as np
import pytest

from gpuart_amd import binding as B
from oracle import oracle as O
from tests import build_cases as BC
from tests import converter_ref as CR
from tests import ploc_cases as PC
from tests import ploc_ref as PR
from tests import refit_ref as RR
from tests.test_build_ref import _declared, same_bytes, same_device_words
from tests.test_ray_queries import tree_prims
from tests.util import exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
QUALITY = ("scene_d", "scene_p", "mesh20k", "tris257")


@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_a_clustered_tree_has_the_contracts_shape(name):
    """The tree parses, is regular and orderly, holds every primitive once in the order new_to_old says, has leaves of one or two and one
    record fewer than leaves, and its refs, depth and record count are what the restatement reports."""
    c = PC.case(name)
    n, info = len(c["prims"]), c["info"]
    assert sorted(c["new_to_old"].tolist()) == list(range(n))
    lay = CR.layout(c["built"])
    bits = c["built"].view(np.uint32)
    counts = [int(bits[a + 2, 0]) & CR.COUNT_MASK for a in lay["addr"][lay["leaf"]]]
    assert set(counts) <= {1, 2} and sum(counts) == n and len(lay["addr"]) == 2 * len(counts) - 1
    assert info["n_recs"] == len(counts) - 1 <= max(0, n - 1)
    now = tree_prims(c["built"])
    assert all(now[p][0] == c["prims"][o][0] and same_bytes(now[p][1], c["prims"][o][1]) for p, o in enumerate(c["new_to_old"]))
    cv = CR.convert(c["built"])
    assert not cv["irregular"] and not cv["disorderly"] and cv["subnormal"] == (name in BC.SUBNORMAL) == B.tree_slack(c["built"])[1]
    assert cv["max_depth"] == info["depth"] and len(cv["recs"]) == info["n_recs"] and cv["root_ref"] == info["root_ref"]
    assert (cv["recs"].view(np.uint32)[:, :2, 3].reshape(-1) == info["refs"]).all()
    tc = B.tree_class(c["built"])   # ... and the uploader's own verdict
    assert not tc["irregular"] and not tc["disorderly"]
    assert same_bytes(RR.refit(c["built"]), c["built"])   # the boxes the clustering carried are the refit rule's
    assert info["iterations"] <= PR.MAX_ITERATIONS and info["depth"] <= info["iterations"]


def test_the_small_cases_end_as_the_contract_says():
    one, two, three = PC.case("n1"), PC.case("n2"), PC.case("n3")
    assert one["info"]["iterations"] == 0 and one["info"]["n_recs"] == 0 and one["info"]["root_ref"] & PR.REF_LEAF and not one["info"]["root_ref"] & PR.REF_TWO
    assert two["info"]["iterations"] == 1 and two["info"]["n_recs"] == 0 and two["info"]["root_ref"] & PR.REF_TWO
    assert three["info"]["iterations"] == 2 and three["info"]["n_recs"] == 1


def test_total_ties_pair_up_in_one_iteration():
    """64 identical spheres: every distance ties, and the xor rule alone pairs 0-1, 2-3, ... at once — the balanced tree in six
    iterations, not one pair per iteration."""
    c = PC.case("same64")
    assert c["info"]["iterations"] == 6 and (c["new_to_old"] == np.arange(64)).all()
    lay = CR.layout(c["built"])
    assert sorted(lay["depth"][lay["leaf"]].tolist()) == [5] * 32


def test_nested_spheres_make_a_chain():
    """40 concentric spheres: one merge per iteration, 39 iterations, a chain of 39 levels (the deepest node at level 38, the root at 0)
    in which every interior node has a leaf of one."""
    c = PC.case("nested40")
    assert c["info"]["iterations"] == 39 and c["info"]["depth"] + 1 == 39 and c["info"]["n_recs"] == 38
    refs = c["info"]["refs"].reshape(-1, 2)
    leaf_of_one = ((refs & PR.REF_LEAF) != 0) & ((refs & PR.REF_TWO) == 0)
    assert leaf_of_one.any(axis=1).all()


def test_the_iteration_cap_refuses_a_chain_of_1100():
    with pytest.raises(ValueError, match="1024 iterations"):
        PR.build(PC.refused("chain1100")["prims"])


# ---- the host tree ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PC.SCENES))
def test_the_host_tree_adopts_the_restatements_topology(name):
    c = PC.case(name)
    quads = B.adopt_tree(c["tree"], c["new_to_old"], c["info"]["refs"])
    assert same_device_words(quads, c["built"]), name
    again = B.adopt_tree(quads, np.arange(len(c["prims"]), dtype=np.uint32), c["info"]["refs"])   # its own topology over its own order
    assert same_bytes(again, quads), name


def test_the_host_tree_refuses_what_is_no_tree():
    c = PC.case("scene_p")
    order, n = c["new_to_old"], len(c["prims"])
    refs = c["info"]["refs"].astype(np.int64)   # (Python-int arithmetic on the words; adopt_tree takes them back to uint32)
    n_recs = len(refs) // 2

    def spoilt(a, at, value):
        b = a.copy()
        b[at] = value
        return b
    inner = next(k for k in range(2, len(refs)) if not refs[k] & PR.REF_LEAF)
    two = next(k for k in range(len(refs)) if refs[k] & PR.REF_TWO)
    one = next(k for k in range(len(refs)) if refs[k] & PR.REF_LEAF and not refs[k] & PR.REF_TWO)
    bad = [("a repeated ordinal", spoilt(order, 1, order[0]), refs),
           ("an ordinal out of range", spoilt(order, 0, n), refs),
           ("a record index out of range", order, spoilt(refs, inner, n_recs)),
           ("a record referenced twice", order, spoilt(refs, inner, refs[inner] - 1 if refs[inner] > 1 else 0)),
           ("a record never reached", order, spoilt(refs, inner, refs[one])),
           ("a leaf of three: a ref without a count flag", order, spoilt(refs, two, refs[two] & ~(PR.REF_TWO | PR.REF_TRIS | PR.REF_SMALL))),
           ("a leaf that claims a third primitive's place", order, spoilt(refs, one, refs[one] | PR.REF_TWO)),
           ("leaves out of order", order, spoilt(refs, two, refs[two] + 2)),
           ("a first primitive out of range", order, spoilt(refs, two, refs[two] | 0x0fffffff)),
           ("too few records", order, refs[:-2]),
           ("an odd root", order, spoilt(refs, 0, refs[1]))]
    for what, o, r in bad:
        with pytest.raises(ValueError, match="-2"):
            B.adopt_tree(c["tree"], o, r)
            pytest.fail(what)
    tris = PC.case("tris257")
    trefs = tris["info"]["refs"].astype(np.int64)
    k = next(k for k in range(len(trefs)) if trefs[k] & PR.REF_TRIS)
    with pytest.raises(ValueError, match="-2"):   # the flag must say what the primitives are
        B.adopt_tree(tris["tree"], tris["new_to_old"], spoilt(trefs, k, trefs[k] ^ (PR.REF_TRIS | PR.REF_SMALL)))
    with pytest.raises(ValueError, match="-2"):   # no records over more than two primitives
        B.adopt_tree(c["tree"], order, refs[:0])
    with pytest.raises(ValueError, match="-1"):
        B.adopt_tree(c["tree"][:-1], order, refs)
    assert same_device_words(B.adopt_tree(c["tree"], order, refs), c["built"])


# ---- quality ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUALITY)
def test_a_clustered_tree_costs_less_than_the_morton_one(name):
    clustered, morton = BC.cost_of(PC.case(name)["built"])[0], BC.cost_of(BC.case(name)["built"])[0]
    print("%s: clustered %.3f, Morton %.3f, reference-built %.3f" % (name, clustered, morton, BC.cost_of(BC.case(name)["tree"])[0]))
    assert clustered < morton


def test_the_clustered_scene_d_costs_less_than_the_reference_built_one():
    """The ground disc, the large primitive, stays unmerged until the top of the tree."""
    c = PC.case("scene_d")
    assert BC.cost_of(c["built"])[0] < BC.cost_of(c["tree"])[0]


def test_the_clustered_tree_of_the_drift_track_is_walked_in_fewer_steps():
    """build_cases.drift()'s camera rays: the oracle visits fewer nodes in the clustered tree of the drifted primitives than in the Morton
    rebuild of them, and finds the same hits."""
    d = BC.drift()
    built, _ = PC.drift_clustered()
    rs, rd = d["rays"]
    a0, a1, sa = O.traverse(d["rebuilt"], rs, rd, None, want_stats=True)
    b0, b1, sb = O.traverse(built, rs, rd, None, want_stats=True)
    print("box steps: Morton %d, clustered %d" % (sa.nodes, sb.nodes))
    assert sb.nodes < sa.nodes and BC.cost_of(built)[0] < BC.cost_of(d["rebuilt"])[0]
    assert same_bytes(a0[:, 0], b0[:, 0])


# ---- the entry points -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_the_entry_points_are_declared_and_exported(lib):
    d = os.path.join(ROOT, "gpuart_amd", lib)
    names = _declared(os.path.join(ROOT, "include", "gpuart_ploc.h"), "gpuart_ploc_")
    assert exported(os.path.join(d, "libgpuart_ploc.so")) == names and "gpuart_ploc_run" in names and "gpuart_ploc_run_host" in names and len(names) == 7
    host = exported(os.path.join(d, "libgpuart.so"))
    capi = _declared(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h"), "gpuart_")
    for n in ("gpuart_adopt_tree", "gpuart_renderer_rebuild_tree_mode", "gpuart_renderer_rebuild_tree"):
        assert n in host and n in capi


def test_bad_calls_are_refused_without_a_device():
    P = B.ploc_lib()
    scene, res = B.HipScene(), B.PlocResult()
    assert P.gpuart_ploc_finish(None) == ERR_ARG and P.gpuart_ploc_last_error() == b"ploc: handle is NULL"
    assert P.gpuart_ploc_run(None, C.byref(scene), C.byref(scene), None, C.byref(res)) == ERR_ARG
    assert P.gpuart_ploc_run_host(None, C.byref(scene), C.byref(scene), None, C.byref(res)) == ERR_ARG
    assert P.gpuart_ploc_step_ms(None, None) == ERR_ARG
    assert P.gpuart_ploc_create(C.c_int(0), None) == ERR_ARG and P.gpuart_ploc_last_error() == b"ploc: out is NULL"
    assert P.gpuart_ploc_destroy(None) == 0


def test_the_result_struct_and_the_constants_match_the_header(tmp_path):
    import subprocess
    fields = [f for f, _ in B.PlocResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_ploc.h"\nint main(void) { printf("%zu", sizeof(gpuart_ploc_result));\n'
                   + "".join('printf(" %%zu", offsetof(gpuart_ploc_result, %s));\n' % f for f in fields)
                   + 'printf(" %u %u", GPUART_PLOC_RADIUS, GPUART_PLOC_MAX_ITERATIONS);\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(B.PlocResult)] + [getattr(B.PlocResult, f).offset for f in fields] + [PR.RADIUS, PR.MAX_ITERATIONS]
