"""The edit's contract without a device (include/gpuart_edit.h): the host library's BoundingVolumesHierarchy::EditPrimitives (through
gpuart_edit_tree) followed by its Morton rebuild, or by the restatement's clustered topology fed through AdoptTopology, writes the tree
the restatements make of the restatement's edited list (tests/edit_ref.py, tests/build_ref.py, tests/ploc_ref.py) in every word the
device reads; it refuses what the restatement refuses, with the same first offender; and the new entry points are declared and exported,
with the result struct laid out as its ctypes mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpuart_amd import binding as B
from tests import edit_cases as EC
from tests import edit_ref as ER
from tests.test_build_ref import _declared, same_device_words
from tests.test_ray_queries import tree_prims
from tests.util import exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.mark.parametrize("name", list(EC.CASES))
def test_the_host_edit_and_the_morton_rebuild_are_the_restatements(name):
    c, bt = EC.case(name), EC.built(name, "morton")
    quads, perm = B.edit_tree(c["tree"], c["remove"], c["types"], c["payload"])
    assert (perm == bt["new_to_old"]).all() and same_device_words(quads, bt["tree"]), name
    checked, again = B.edit_tree(c["tree"], c["remove"], c["types"], c["payload"], order=bt["new_to_old"])   # the device's order, only checked
    assert same_device_words(checked, bt["tree"]) and (again == perm).all()
    now = tree_prims(quads)
    assert len(now) == len(c["edited"])
    for p, o in enumerate(bt["new_to_old"]):
        assert now[p][0] == c["edited"][o][0] and (now[p][1].view(np.uint32) == c["edited"][o][1].view(np.uint32)).all()


@pytest.mark.parametrize("name", EC.SMALL)
def test_the_host_edit_adopts_the_clustered_topology(name):
    c, bt = EC.case(name), EC.built(name, "clustered")
    quads, perm = B.edit_tree(c["tree"], c["remove"], c["types"], c["payload"], order=bt["new_to_old"], refs=bt["info"]["refs"])
    assert (perm == bt["new_to_old"]).all() and same_device_words(quads, bt["tree"]), name


def test_the_restatement_edits_as_the_contract_says():
    c = EC.case("both")
    n_old, removed = len(c["prims"]), set(c["remove"].tolist())
    assert c["source"].tolist() == [i for i in range(n_old) if i not in removed] + [n_old + k for k in range(len(c["added"]))]
    for q, s in enumerate(c["source"]):
        t, d = c["prims"][s] if s < n_old else c["added"][s - n_old]
        assert c["edited"][q][0] == t and (np.asarray(c["edited"][q][1]).view(np.uint32) == np.asarray(d, np.float32).view(np.uint32)).all()
    recs, boxes = ER.device_list(EC.case("to_one")["edited"])
    assert recs.view(np.uint32)[0, 0, 3] >> 2 == 1          # a list of one is a leaf of one
    recs, boxes = ER.device_list(c["edited"])
    assert (recs.view(np.uint32)[:, 0, 3] == [t for t, _ in c["edited"]]).all() and (boxes[:, :3] <= boxes[:, 3:]).all()


def test_the_host_refuses_what_the_restatement_refuses():
    c = EC.case("remove_only")
    for what, (remove, added, first_bad) in EC.refusals(len(c["prims"])).items():
        with pytest.raises(ER.Refused) as r:
            ER.edit(c["prims"], remove, added)
        assert r.value.first_bad == first_bad, what
        with pytest.raises(ValueError, match="-2") as e:
            B.edit_tree(c["tree"], remove, [t for t, _ in added], [d for _, d in added])
        assert e.value.first_bad == first_bad, what
    with pytest.raises(ValueError, match="-3"):   # an order that is no permutation of the edited list
        B.edit_tree(c["tree"], c["remove"], [], [], order=np.zeros(len(c["edited"]), np.uint32))
    quads, _ = B.edit_tree(c["tree"], c["remove"], [], [])   # ... and the tree is untouched by all of them
    assert same_device_words(quads, EC.built("remove_only", "morton")["tree"])


# ---- declarations, exports, layout ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_the_entry_points_are_declared_and_exported(lib):
    d = os.path.join(ROOT, "gpuart_amd", lib)
    names = _declared(os.path.join(ROOT, "include", "gpuart_edit.h"), "gpuart_edit_")
    assert exported(os.path.join(d, "libgpuart_edit.so")) == names and len(names) == 8
    for n in ("create", "destroy", "run", "run_host", "compose", "step_ms", "finish", "last_error"):
        assert "gpuart_edit_" + n in names
    hip = exported(os.path.join(d, "libgpuart_hip.so"))
    hdr = _declared(os.path.join(ROOT, "include", "gpuart_hip.h"), "gpuart_hip_")
    for n in ("gpuart_hip_scene_reserve_prims", "gpuart_hip_scene_replaced"):
        assert n in hip and n in hdr
    host = exported(os.path.join(d, "libgpuart.so"))
    capi = _declared(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h"), "gpuart_")
    for n in ("gpuart_renderer_edit_primitives", "gpuart_edit_tree"):
        assert n in host and n in capi


def test_the_result_struct_is_its_ctypes_mirror(tmp_path):
    fields = [f for f, _ in B.EditResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_edit.h"\nint main(void) { printf("%%zu %s\\n", sizeof(gpuart_edit_result), %s); return 0; }\n'
                   % (" ".join(["%zu"] * len(fields)), ", ".join("offsetof(gpuart_edit_result, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(B.EditResult)] + [getattr(B.EditResult, f).offset for f in fields] == [48, 0, 4, 8, 16, 20, 32]


def test_bad_calls_are_refused_without_a_device():
    L, E = B.hip_lib(), B.edit_lib()
    scene, res = B.HipScene(), B.EditResult()
    ms = (C.c_double * 4)()
    assert L.gpuart_hip_scene_reserve_prims(None, C.c_uint64(1), C.c_uint64(1), C.byref(scene)) == ERR_ARG and b"scene_reserve_prims" in L.gpuart_hip_last_error()
    assert L.gpuart_hip_scene_replaced(None, C.byref(scene), C.c_uint32(4)) == ERR_ARG and b"scene_replaced" in L.gpuart_hip_last_error()
    for rc in (E.gpuart_edit_finish(None), E.gpuart_edit_step_ms(None, ms), E.gpuart_edit_compose(None, None, None, C.c_size_t(1), None),
               E.gpuart_edit_run(None, C.byref(scene), None, C.c_size_t(0), None, None, C.c_size_t(0), None, C.byref(scene), C.byref(res)),
               E.gpuart_edit_run_host(None, C.byref(scene), None, C.c_size_t(0), None, None, C.c_size_t(0), None, C.byref(scene), C.byref(res))):
        assert rc == ERR_ARG and E.gpuart_edit_last_error() == b"edit: handle is NULL"
    assert E.gpuart_edit_destroy(None) == 0
