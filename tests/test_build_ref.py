"""The rebuild contract without a device (include/gpuart_build.h): the host library's BoundingVolumesHierarchy::RebuildMorton (through
gpuart_rebuild_tree) writes the restatement's tree (tests/build_ref.py) in every word the device reads, with and without a given order;
the built trees have the shape the contract states, are fixed points of the refit rule, are regular and orderly, and answer rays as the
reference-built tree of the same primitives does; and the new entry points are declared, exported and refuse bad calls before any HIP call.

Rays: the camera rays of the golden frames of the same scenes (tests/golden/frames_box_seg4.npz, frames_scene_p_seg4.npz,
frames_scene_d_seg5.npz: their `cam`, W and H), every 19th ray. The test first checks on the reference-built tree alone that none of
them is a grazing or phantom case: the tree's answer is the closest of the primitives' own intersections, and no second primitive
comes within an ulp of it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from gpuart_amd import binding as B
from oracle import oracle as O
from tests import build_cases as BC
from tests import build_ref as BR
from tests import converter_ref as CR
from tests import refit_ref as RR
from tests.test_ray_queries import tree_prims
from tests.util import exported, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
DEVICE_WORDS = ("recs", "prims", "root_min", "root_max", "refs")


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def same_device_words(a, b):
    """Two canonical trees agree in every word the device reads (tests/converter_ref.py says which those are)."""
    ca, cb = CR.convert(a), CR.convert(b)
    return (all(ca[k].shape == cb[k].shape and (ca[k].view(np.uint32) == cb[k].view(np.uint32)).all() for k in DEVICE_WORDS)
            and all(ca[k] == cb[k] for k in ("root_ref", "max_depth", "num_nodes", "type_mask", "irregular", "disorderly", "subnormal")))


@pytest.mark.parametrize("name", sorted(BC.SCENES))
def test_the_host_rebuild_equals_the_restatement(name):
    c = BC.case(name)
    quads, new_to_old = B.rebuild_tree(c["tree"])
    assert (new_to_old == c["new_to_old"]).all() and same_device_words(quads, c["built"]), name
    given, again = B.rebuild_tree(c["tree"], order=c["new_to_old"])   # the device's permutation: checked, not sorted
    assert same_bytes(given, quads) and (again == new_to_old).all(), name


@pytest.mark.parametrize("name", sorted(BC.SCENES))
def test_a_built_tree_has_the_contracts_shape(name):
    """new_to_old is a permutation along which the keys ascend (ties by old ordinal), every leaf holds two primitives except the last when
    N is odd, the primitives are the old ones in the new order, and the uploader's restatement classifies the tree regular and orderly."""
    c = BC.case(name)
    n = len(c["prims"])
    perm = c["new_to_old"]
    assert sorted(perm.tolist()) == list(range(n))
    lo, hi = BR.boxes_of(c["prims"])
    keys = BR.keys_of(lo, hi, *BR.root_box(lo, hi))
    pairs = [(keys[o], int(o)) for o in perm]
    assert pairs == sorted(pairs) and all(0 <= k < 1 << 63 for k in keys)
    lay = CR.layout(c["built"])
    bits = c["built"].view(np.uint32)
    counts = [int(bits[a + 2, 0]) & CR.COUNT_MASK for a in lay["addr"][lay["leaf"]]]
    assert counts == [2] * (n // 2) + [1] * (n % 2) and len(lay["addr"]) == 2 * len(counts) - 1
    now = tree_prims(c["built"])
    assert all(now[p][0] == c["prims"][o][0] and same_bytes(now[p][1], c["prims"][o][1]) for p, o in enumerate(perm))
    cv = CR.convert(c["built"])
    assert not cv["irregular"] and not cv["disorderly"] and cv["subnormal"] == (name in BC.SUBNORMAL)
    tc = B.tree_class(c["built"])   # ... and the uploader's own verdict
    assert not tc["irregular"] and not tc["disorderly"] and B.tree_slack(c["built"])[1] == cv["subnormal"]
    assert same_bytes(c["built"][0:2, :3], np.stack(BR.root_box(lo, hi)))


@pytest.mark.parametrize("name", sorted(BC.SCENES))
def test_a_refit_with_nothing_moved_is_the_identity_on_a_built_tree(name):
    built = BC.case(name)["built"]
    assert same_bytes(RR.refit(built), built)


def test_every_tie_is_broken_by_the_index():
    """64 identical spheres: all keys equal, so the topology is the binary counting tree over 32 leaves, five levels of records."""
    c = BC.case("same64")
    assert (c["new_to_old"] == np.arange(64)).all()
    lay = CR.layout(c["built"])
    assert sorted(lay["depth"][lay["leaf"]].tolist()) == [5] * 32


def _golden_rays(name):
    g = golden({"box": "frames_box_seg4", "scene_p": "frames_scene_p_seg4", "scene_d": "frames_scene_d_seg5"}[name])
    rs, rd = O.cam_rays(g["cam"], int(g["W"]), int(g["H"]))
    return rs.reshape(-1, 4)[::19], rd.reshape(-1, 4)[::19]


def _own_hit(t, d, rs, rd):
    q = np.tile(np.asarray(d, np.float32).reshape(1, 4, 4), (len(rs), 1, 1))
    return (O.sphere(rs, rd, q[:, 0]) if t == 0 else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == 1 else
            O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == 2 else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))


@pytest.mark.parametrize("name", ["box", "scene_p", "scene_d"])
def test_a_built_tree_answers_rays_as_the_reference_built_one(name):
    c = BC.case(name)
    rs, rd = _golden_rays(name)
    o0, o1 = O.traverse(c["tree"], rs, rd, None)
    # the condition, on the reference alone: the answer is the closest own intersection, and it is alone within an ulp
    pos = np.stack([_own_hit(t, d, rs, rd)[0][:, 0] for t, d in c["prims"]]).astype(np.float64)
    pos[~(pos > 0)] = np.inf
    best = np.sort(pos, 0)[:2] if len(pos) > 1 else np.concatenate([pos, np.full_like(pos, np.inf)])
    hit = np.isfinite(best[0])
    assert hit.sum() > len(rs) // 4
    assert (o0[hit, 0].astype(np.float64) == best[0][hit]).all() and not (o0[~hit, 0] > 0).any(), "a phantom hit among the fixture's rays"
    assert (best[1][hit] > np.nextafter(best[0][hit].astype(np.float32), np.float32(np.inf))).all(), "a grazing tie among the fixture's rays"
    b0, b1 = O.traverse(c["built"], rs, rd, None)
    assert same_bytes(b0, o0) and same_bytes(b1, o1)
    # ... and the winner is the same primitive, through new_to_old
    old_winner = pos.argmin(0)[hit]
    pos_new = np.stack([_own_hit(t, d, rs, rd)[0][:, 0] for t, d in tree_prims(c["built"])]).astype(np.float64)
    pos_new[~(pos_new > 0)] = np.inf
    assert (c["new_to_old"][pos_new.argmin(0)[hit]] == old_winner).all()


def test_a_rebuild_repairs_a_drifted_tree():
    """The drift track of tests/test_build.py, on the CPU: the refitted old topology costs more, by the cost measure and by the nodes
    the oracle visits for a fixed ray set, than the tree rebuilt from the same primitives — and both give the same hits."""
    d = BC.drift()
    rs, rd = d["rays"]
    a0, a1, sa = O.traverse(d["refitted"], rs, rd, None, want_stats=True)
    b0, b1, sb = O.traverse(d["rebuilt"], rs, rd, None, want_stats=True)
    assert BC.cost_of(d["rebuilt"])[0] < BC.cost_of(d["refitted"])[0] and sb.nodes < sa.nodes
    assert same_bytes(a0[:, 0], b0[:, 0])
    assert not same_bytes(d["refitted"], d["tree"])


def test_the_host_rebuild_refuses_a_wrong_order():
    c = BC.case("scene_p")
    order = c["new_to_old"].copy()
    keys_differ = next(p for p in range(len(order) - 1) if order[p] > order[p + 1])   # (neighbours with different keys)
    swapped = order.copy()
    swapped[[keys_differ, keys_differ + 1]] = swapped[[keys_differ + 1, keys_differ]]
    repeated = order.copy()
    repeated[1] = repeated[0]
    beyond = order.copy()
    beyond[0] = len(order)
    for bad in (swapped, repeated, beyond):
        with pytest.raises(ValueError, match="-2"):
            B.rebuild_tree(c["tree"], order=bad)
    ties = BC.case("same64")
    with pytest.raises(ValueError, match="-2"):   # equal keys out of their old order
        B.rebuild_tree(ties["tree"], order=ties["new_to_old"][::-1].copy())
    with pytest.raises(ValueError, match="-1"):
        B.rebuild_tree(c["tree"][:-1])
    empty = np.ascontiguousarray(O.build_bvh([])[0], np.float32)
    with pytest.raises(ValueError, match="-2"):
        B.rebuild_tree(empty)


def _declared(header, prefix):
    return sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, open(header).read())))


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_the_entry_points_are_declared_and_exported(lib):
    d = os.path.join(ROOT, "gpuart_amd", lib)
    names = _declared(os.path.join(ROOT, "include", "gpuart_build.h"), "gpuart_build_")
    assert exported(os.path.join(d, "libgpuart_build.so")) == names and "gpuart_build_run" in names and "gpuart_build_cost" in names and len(names) == 8
    hip = exported(os.path.join(d, "libgpuart_hip.so"))
    hdr = _declared(os.path.join(ROOT, "include", "gpuart_hip.h"), "gpuart_hip_")
    for n in ("gpuart_hip_scene_reserve", "gpuart_hip_scene_rebuilt"):
        assert n in hip and n in hdr
    host = exported(os.path.join(d, "libgpuart.so"))
    capi = _declared(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h"), "gpuart_")
    for n in ("gpuart_renderer_rebuild_tree", "gpuart_renderer_tree_cost", "gpuart_rebuild_tree", "gpuart_renderer_compile_bvh"):
        assert n in host and n in capi


def test_bad_calls_are_refused_without_a_device():
    L, Bd = B.hip_lib(), B.build_lib()
    scene, res = B.HipScene(), B.BuildResult()
    cost = C.c_double()
    assert L.gpuart_hip_scene_reserve(None, C.c_uint64(1), C.byref(scene)) == ERR_ARG and b"scene_reserve" in L.gpuart_hip_last_error()
    assert L.gpuart_hip_scene_rebuilt(None, C.byref(scene)) == ERR_ARG and b"scene_rebuilt" in L.gpuart_hip_last_error()
    assert Bd.gpuart_build_finish(None) == ERR_ARG and Bd.gpuart_build_last_error() == b"build: handle is NULL"
    assert Bd.gpuart_build_run(None, C.byref(scene), C.byref(scene), None, C.byref(res)) == ERR_ARG
    assert Bd.gpuart_build_run_host(None, C.byref(scene), C.byref(scene), None, C.byref(res)) == ERR_ARG
    assert Bd.gpuart_build_cost(None, C.byref(scene), C.byref(cost)) == ERR_ARG
    assert Bd.gpuart_build_create(C.c_int(0), None) == ERR_ARG and Bd.gpuart_build_last_error() == b"build: out is NULL"
    assert Bd.gpuart_build_destroy(None) == 0


def test_the_result_struct_matches_the_header(tmp_path):
    import subprocess
    fields = [f for f, _ in B.BuildResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_build.h"\nint main(void) { printf("%zu", sizeof(gpuart_build_result));\n'
                   + "".join('printf(" %%zu", offsetof(gpuart_build_result, %s));\n' % f for f in fields) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(B.BuildResult)] + [getattr(B.BuildResult, f).offset for f in fields]
