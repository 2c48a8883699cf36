"""The refit contract without a device (include/gpuart_refit.h): the restatement tests/refit_ref.py is the identity on built trees, the
host library's BoundingVolumesHierarchy::Refit (through gpuart_refit_tree) equals it byte for byte and refuses what the rule refuses,
refitted trees stay regular and orderly and answer rays as a tree rebuilt from the moved primitives does, and the new entry points are
declared, exported and refuse bad calls before any HIP call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from gpuart_amd import binding as B
from gpuart_amd import synth_scenes as S
from oracle import oracle as O
from tests import converter_ref as CR
from tests import refit_ref as RR
from tests.test_ray_queries import random_rays, tree_prims
from tests.util import exported, pad4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1

SCENES = {
    "box": S.box_scene,
    "scene_p": S.scene_p,
    "scene_d": lambda: S.scene_d(48, 48),
    "tree": lambda: S.tree_scene(depth=5),
    "lattice": S.lattice_scene,
    "cluster": lambda: S.cluster_scene(n=2000),
    "cones": lambda: S.scene_p(seed=3, nspheres=0, ndiscs=0, ncones=64)[1:],   # the 64-cone scene of tests/test_kernel_variants.py
}


@functools.lru_cache(maxsize=None)
def tree_of(name):
    t = np.ascontiguousarray(O.build_bvh(SCENES[name]())[0], np.float32)
    t.setflags(write=False)
    return t


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def host_refit(tree, ordinals, payloads, touched_only=False):
    """gpuart_refit_tree: (status, quads', index of the first offending update)."""
    L = B.host_lib()
    q = np.ascontiguousarray(tree, np.float32)
    o = np.ascontiguousarray(ordinals, np.uint32).reshape(-1)
    p = np.ascontiguousarray(payloads, np.float32).reshape(-1)
    out = np.full_like(q, 7.0)
    bad = C.c_size_t(1 << 40)
    rc = L.gpuart_refit_tree(q.ctypes.data_as(C.c_void_p), C.c_size_t(q.size // 4), o.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p),
                             C.c_size_t(o.size), out.ctypes.data_as(C.c_void_p), C.byref(bad), C.c_int(1 if touched_only else 0))
    return rc, out, bad.value


@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_refit_with_nothing_moved_is_the_identity(name):
    """The rule — leaves fold their primitives' boxes, interior nodes their children's — reproduces the builder's boxes byte for byte:
    in the restatement and in the host library."""
    tree = tree_of(name)
    assert same_bytes(RR.refit(tree), tree)
    rc, out, _ = host_refit(tree, [], [])
    assert rc == 0 and same_bytes(out, tree)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_host_refit_equals_the_restatement(name):
    """Random updates (a tenth of the primitives moved by up to 0.3; one primitive; all of them): gpuart_refit_tree's quads are the
    restatement's byte for byte, differ from the input, and keep the uploader's verdict regular and orderly (tests/converter_ref.py)."""
    tree = tree_of(name)
    rng = np.random.default_rng(17)
    for share in (0.1, 0.0, 1.0):
        ordinals, payloads = RR.random_update(tree, rng, share, 0.3)
        exp = RR.refit(tree, ordinals, payloads)
        for touched_only in (False, True):   # (the form that recomputes only the moved leaves' paths gives the same tree)
            rc, out, _ = host_refit(tree, ordinals, payloads, touched_only)
            assert rc == 0 and same_bytes(out, exp), (name, share, touched_only)
        assert not same_bytes(exp, tree)
        cv = CR.convert(exp)
        assert not cv["irregular"] and not cv["disorderly"], (name, share)
        tc = B.tree_class(exp)   # ... and the uploader's own (its cone checks included)
        assert not tc["irregular"] and not tc["disorderly"], (name, share)


def rebuilt(tree, ordinals, payloads):
    """The tree the builder makes of the primitives after the move."""
    prims = tree_prims(tree)
    data = {int(o): p for o, p in zip(ordinals, payloads)}
    return O.build_bvh([RR.desc_of(t, data.get(k, d)) for k, (t, d) in enumerate(prims)])[0]


@pytest.mark.parametrize("name", ["scene_p", "discs", "triangles"])
def test_a_refitted_tree_answers_rays_as_a_rebuilt_one(name):
    """30 % of the primitives moved by up to 0.3: on 20 000 random rays the oracle finds the same hit parameter in the refitted tree
    (old topology, refitted boxes) and in the tree built from the moved primitives."""
    descs = {"scene_p": S.scene_p, "discs": lambda: S.scene_p(nspheres=0), "triangles": lambda: [d for d in S.scene_d(24, 24) if d[0] == S.TRIANGLE]}[name]()
    tree = np.ascontiguousarray(O.build_bvh(descs)[0], np.float32)
    rng = np.random.default_rng(2)
    ordinals, payloads = RR.random_update(tree, rng, 0.3, 0.3)
    refitted = RR.refit(tree, ordinals, payloads)
    other = rebuilt(tree, ordinals, payloads)
    lo, hi = refitted[0, :3].astype(np.float64), refitted[1, :3].astype(np.float64)
    assert same_bytes(refitted[0:2, :3], other[0:2, :3])   # the same root box: the same primitives
    rs, rd = random_rays(np.random.default_rng(3), 20000, lo, hi)
    a = O.traverse(refitted, pad4(rs), pad4(rd), None)[0][:, 0]
    b = O.traverse(other, pad4(rs), pad4(rd), None)[0][:, 0]
    assert (a > 0).sum() > 1000
    assert (a.view(np.uint32) == b.view(np.uint32)).all(), int((a.view(np.uint32) != b.view(np.uint32)).sum())


def test_the_host_refit_refuses_what_the_rule_refuses():
    """Each refusal names the first offending update and writes nothing."""
    tree = tree_of("box")
    prims = tree_prims(tree)
    sphere = next(k for k, (t, _) in enumerate(prims) if t == 0)
    cone = next(k for k, (t, _) in enumerate(prims) if t == 3)
    keep = lambda k: prims[k][1].copy()

    def refused(ordinals, payloads, first):
        rc, out, bad = host_refit(tree, ordinals, payloads)
        assert rc == -2 and bad == first and (out == 7.0).all(), (rc, bad, first)

    a, b = sorted((sphere, cone))
    refused([b, a], [keep(b), keep(a)], 1)                       # descending
    refused([a, a], [keep(a), keep(a)], 1)                       # repeated
    refused([a, len(prims)], [keep(a), keep(a)], 1)              # out of range
    for word, value in ((0, np.nan), (1, np.inf), (2, 2.0 ** 21), (3, -0.5)):
        d = keep(sphere)
        d[word] = value
        refused([sphere], [d], 0)
    d = keep(cone)
    d[8:11] = -d[8:11]                                           # an axis that contradicts its centres
    refused([cone], [d], 0)
    d = keep(sphere)
    d[2] = 2.0 ** 20                                             # the limit itself is inside the rule
    assert host_refit(tree, [sphere], [d])[0] == 0
    assert host_refit(tree[:-1], [], [])[0] == -1                # a truncated tree is malformed


def _declared(header, prefix):
    return sorted(set(re.findall(r"\b(%s[a-z_0-9]+)\s*\(" % prefix, open(header).read())))


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_the_entry_points_are_declared_and_exported(lib):
    d = os.path.join(ROOT, "gpuart_amd", lib)
    names = _declared(os.path.join(ROOT, "include", "gpuart_refit.h"), "gpuart_refit_")
    assert exported(os.path.join(d, "libgpuart_refit.so")) == names and "gpuart_refit_run_host" in names and len(names) == 8
    hip = exported(os.path.join(d, "libgpuart_hip.so"))
    hdr = _declared(os.path.join(ROOT, "include", "gpuart_hip.h"), "gpuart_hip_")
    for n in ("gpuart_hip_scene_device", "gpuart_hip_scene_refitted"):
        assert n in hip and n in hdr
    host = exported(os.path.join(d, "libgpuart.so"))
    capi = _declared(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h"), "gpuart_")
    for n in ("gpuart_renderer_update_primitives", "gpuart_refit_tree"):
        assert n in host and n in capi


def test_bad_calls_are_refused_without_a_device():
    """NULL contexts, handles and scenes fail with ERR_ARG and a message before any HIP call."""
    L, R = B.hip_lib(), B.refit_lib()
    scene, res = B.HipScene(), B.RefitResult()
    zero = (C.c_float * 3)(0, 0, 0)
    assert L.gpuart_hip_scene_device(None, C.byref(scene)) == ERR_ARG and b"scene_device" in L.gpuart_hip_last_error()
    assert L.gpuart_hip_scene_refitted(None, zero, zero, C.c_int(0)) == ERR_ARG and b"scene_refitted" in L.gpuart_hip_last_error()
    assert R.gpuart_refit_finish(None) == ERR_ARG and R.gpuart_refit_last_error() == b"refit: handle is NULL"
    assert R.gpuart_refit_bind(None, C.byref(scene)) == ERR_ARG
    assert R.gpuart_refit_run(None, C.byref(scene), None, None, C.c_size_t(0), C.byref(res)) == ERR_ARG
    assert R.gpuart_refit_run_host(None, C.byref(scene), None, None, C.c_size_t(0), C.byref(res)) == ERR_ARG
    assert R.gpuart_refit_create(C.c_int(0), None) == ERR_ARG and R.gpuart_refit_last_error() == b"refit: out is NULL"
    assert R.gpuart_refit_destroy(None) == 0


def test_the_scene_struct_matches_the_header(tmp_path):
    """sizeof / offsetof of gpuart_hip_scene and gpuart_refit_result as a C compiler sees the headers == the binding's ctypes structures."""
    import subprocess
    fields_s = [f for f, _ in B.HipScene._fields_]
    fields_r = [f for f, _ in B.RefitResult._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_refit.h"\nint main(void) { printf("%zu %zu", sizeof(gpuart_hip_scene), sizeof(gpuart_refit_result));\n'
                   + "".join('printf(" %%zu", offsetof(gpuart_hip_scene, %s));\n' % f for f in fields_s)
                   + "".join('printf(" %%zu", offsetof(gpuart_refit_result, %s));\n' % f for f in fields_r) + "return 0; }\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    exp = [C.sizeof(B.HipScene), C.sizeof(B.RefitResult)] + [getattr(B.HipScene, f).offset for f in fields_s] + [getattr(B.RefitResult, f).offset for f in fields_r]
    assert got == exp
