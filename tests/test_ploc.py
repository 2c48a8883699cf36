"""The tree of an uploaded scene rebuilt on the device by locally-ordered clustering (include/gpuart_ploc.h, libgpuart_ploc.so;
Backend.rebuild(mode="clustered"), Renderer.rebuild_tree("clustered")): the device arrays afterwards are what the uploader makes of the
restatement's tree (tests/ploc_ref.py, tests/converter_ref.py) byte for byte, frames and queries of the rebuilt context are the
oracle's on that tree bit for bit, the renderer's host tree follows through AdoptTopology and keeps the temporal history, a refusal
changes nothing, and the Morton path is what it was."""
import ctypes as C

import numpy as np
import pytest

from tests import build_cases as BC
from tests import build_ref as BR
from tests import converter_ref as CR
from tests import ploc_cases as PC
from tests import ploc_ref as PR
from tests import refit_ref as RR
from tests.test_build import (B, O, be, H, W, _moved_descs, _refit_by_desc, assert_arrays, check_frames, device_arrays, own_hit,  # noqa: F401 (fixtures)
                              same_arrays)
from tests.test_kernel_variants import scene_setup, to_params, tree_of as variant_tree
from tests.test_ray_queries import assert_same_bits, hook_record, tree_prims, words
from tests.util import assert_bits, same_bits, to_device

pytestmark = pytest.mark.gpu
ERR_ARG = -1


def rebuild(b, device):
    """(new_to_old as NumPy, the result's dict) of a clustered rebuild, through the device-tensor or the host entry."""
    perm = b.rebuild(out=bool(device), mode="clustered")
    if device:
        assert perm.is_cuda
        perm = perm.cpu().numpy().view(np.uint32)
    return perm, b.last_rebuild


def direct_frame(B, O, b, tree):
    cam, P, _, _, _ = scene_setup(O, tree, W, H)
    b.set_camera(cam)
    b.render_direct(to_params(B, P))
    return b.read(0).copy()


# ---- bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, name", list(enumerate(PC.SCENES)))
def test_device_arrays_equal_the_restatement(be, B, k, name):
    c = PC.case(name)
    n, info = len(c["prims"]), c["info"]
    be.upload_bvh(c["tree"])
    before = be.scene_device()
    perm, out = rebuild(be, device=k % 2 == 0)
    assert (perm == c["new_to_old"]).all(), name
    cv = assert_arrays(be, c["built"], name)
    print("%s: %d primitives, %d records, depth %d, %d iterations" % (name, n, out["n_recs"], out["max_depth"], out["iterations"]))
    assert out["n_recs"] == len(cv["recs"]) == info["n_recs"] and out["root_ref"] == cv["root_ref"] and out["max_depth"] == cv["max_depth"] == info["depth"]
    assert out["iterations"] == info["iterations"] and len(out["step_ms"]) == 6
    assert same_bits(out["root_min"], cv["root_min"]) and same_bits(out["root_max"], cv["root_max"]) and out["subnormal"] == cv["subnormal"] == (name in BC.SUBNORMAL)
    now = be.scene_device()
    assert now.generation == before.generation + 1 and now.n_prims == before.n_prims and now.exact_boxes == 0
    assert now.box_slack == B.tree_slack(c["built"])[0] and be.scene_order() == 1 and (now.box_slack == np.inf) == cv["subnormal"]
    # the bound of an fp64 sum of n_recs positive terms in any order
    assert be.tree_cost() == pytest.approx(BC.cost_of(c["built"])[0] if info["n_recs"] else 0.0, rel=max(1, info["n_recs"]) * 2.0 ** -52, abs=0)


def test_the_mark_of_the_top_levels_is_written(be, monkeypatch):
    monkeypatch.setenv("GPUART_HIP_TOP_DEPTH", "3")
    c = PC.case("scene_p")
    be.upload_bvh(c["tree"])
    be.rebuild(mode="clustered")
    exp = CR.convert(c["built"], top_depth=3)["recs"]
    assert same_bits(device_arrays(be)[0], exp) and exp.view(np.uint32)[:, 2, 3].sum() > 0


# ---- frames -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "scene_p", "scene_d", "nested40"])   # every type, round, flat with the large disc, leaves of one and deep
def test_frames_and_queries_after_a_rebuild_are_the_oracles(be, B, O, name):
    c = PC.case(name)
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.rebuild(mode="clustered")
    check_frames(B, O, be, c["built"], name)


# ---- rebuild, refit and the other build -------------------------------------------------------------------------------------------
def test_a_refit_handle_is_stale_after_a_rebuild_and_binds_again(be, B):
    R = B.refit_lib()
    c = PC.case("scene_p")
    be.upload_bvh(c["tree"])
    be.refit([], [])                       # binds the handle to the uploaded arrays
    be.rebuild(mode="clustered")
    scene, built = be.scene_device(), device_arrays(be)
    res = B.RefitResult()
    assert R.gpuart_refit_run_host(be._refit, C.byref(scene), None, None, C.c_size_t(0), C.byref(res)) == ERR_ARG
    assert b"bound to another upload" in R.gpuart_refit_last_error()
    assert same_arrays(device_arrays(be), built)
    ordinals, payloads = RR.random_update(c["built"], np.random.default_rng(5), 0.3, 0.3)
    out = be.refit(to_device(ordinals.astype(np.int32)), to_device(np.ascontiguousarray(payloads, np.float32)))   # binds again
    lay = CR.layout(c["built"])
    assert out["levels"] == int(lay["depth"][~lay["leaf"]].max()) + 1
    assert_arrays(be, RR.refit(c["built"], ordinals, payloads), "clustered rebuild, refit")


def test_the_two_builds_follow_each_other(be):
    """Morton after clustered and clustered after Morton: each lands on its restatement of the primitives it found; and the Morton path
    with no argument is what it was."""
    c = BC.case("scene_d")
    be.upload_bvh(c["tree"])
    perm = be.rebuild(out=False)
    assert (perm == c["new_to_old"]).all() and "levels" in be.last_rebuild
    assert_arrays(be, c["built"], "Morton")
    tree2, order2 = PR.build(tree_prims(c["built"]))
    perm = be.rebuild(out=False, mode="clustered")
    assert (perm == order2).all()
    assert_arrays(be, tree2, "Morton, clustered")
    tree3, order3 = BR.build(tree_prims(tree2))
    perm = be.rebuild(out=False, mode="morton")
    assert (perm == order3).all()
    assert_arrays(be, tree3, "Morton, clustered, Morton")
    with pytest.raises(ValueError, match="mode"):
        be.rebuild(mode="sah")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_the_iteration_cap_refuses_and_changes_nothing(be, B, O):
    c = PC.refused("chain1100")
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    uploaded, before, frame = device_arrays(be), be.scene_device(), direct_frame(B, O, be, c["tree"])
    with pytest.raises(B.HipError, match="ploc: the scene needs more than 1024 iterations") as e:
        be.rebuild(mode="clustered")
    assert e.value.code == ERR_ARG
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == before.generation
    assert same_bits(direct_frame(B, O, be, c["tree"]), frame)


@pytest.mark.parametrize("name", ["wild", "empty"])
def test_trees_with_exact_boxes_and_empty_scenes_are_not_rebuilt(be, B, O, name):
    tree = variant_tree(name)
    be.resize(W, H)
    be.upload_bvh(tree)
    uploaded, before, frame = device_arrays(be), be.scene_device(), direct_frame(B, O, be, tree)
    assert before.exact_boxes == 1
    with pytest.raises(B.HipError, match="ploc: src: a tree with irregular boxes") as e:
        be.rebuild(mode="clustered")
    assert e.value.code == ERR_ARG
    if name == "empty":   # ... and the dummy leaf of count 0 is refused for itself, whatever the struct says of the boxes
        P, res = B.ploc_lib(), B.PlocResult()
        spare = be.scene_reserve(before.n_recs)
        claimed = B.HipScene.from_buffer_copy(before)
        claimed.exact_boxes = 0
        claimed.root_min, claimed.root_max = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
        perm = to_device(np.zeros(1, np.int32))
        assert P.gpuart_ploc_run(be._ploc, C.byref(claimed), C.byref(spare), C.c_void_p(perm.data_ptr()), C.byref(res)) == ERR_ARG
        assert b"empty scene" in P.gpuart_ploc_last_error()
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == before.generation
    assert same_bits(direct_frame(B, O, be, tree), frame)


def test_refused_rebuilds_change_nothing(be, B, O):
    P = B.ploc_lib()
    c = PC.case("scene_p")
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.rebuild(mode="clustered")           # (makes the handle; the scene is the clustered tree from here)
    uploaded, scene, frame = device_arrays(be), be.scene_device(), direct_frame(B, O, be, c["built"])
    n = scene.n_prims
    res = B.PlocResult()
    perm = to_device(np.zeros(n, np.int32))
    h = be._ploc

    def run(src, dst):
        return P.gpuart_ploc_run(h, C.byref(src), C.byref(dst), C.c_void_p(perm.data_ptr()), C.byref(res))

    def edited(s, **kw):
        t = B.HipScene.from_buffer_copy(s)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    spare = be.scene_reserve(n - 1)
    assert spare.n_recs >= n - 1
    for what, src, dst, word in [("dst is src", scene, scene, b"too small"),   # (the scene's own arrays hold fewer than n - 1 records)
                                 ("dst's records are src's", scene, edited(spare, recs=scene.recs), b"alias"),
                                 ("dst's primitives are src's", scene, edited(spare, prims=scene.prims), b"alias"),
                                 ("dst's boxes are its primitives", scene, edited(spare, prim_boxes=spare.prims), b"overlap"),
                                 ("dst too small", scene, edited(spare, n_prims=n - 1), b"too small"),
                                 ("room for the Morton build's records only", scene, edited(spare, n_recs=(n + 1) // 2 - 1), b"too small"),
                                 ("one record short", scene, edited(spare, n_recs=n - 2), b"too small"),
                                 ("unknown layout", edited(scene, layout=2), spare, b"unknown layout"),
                                 ("unknown dst layout", scene, edited(spare, layout=0), b"unknown layout"),
                                 ("no primitives", edited(scene, n_prims=0), spare, b"empty"),
                                 ("a root box out of order", edited(scene, root_min=(C.c_float * 3)(1, 0, 0), root_max=(C.c_float * 3)(0, 1, 1)), spare, b"root box"),
                                 ("an infinite root box", edited(scene, root_max=(C.c_float * 3)(np.inf, 1, 1)), spare, b"root box")]:
        assert run(src, dst) == ERR_ARG and word in P.gpuart_ploc_last_error(), (what, P.gpuart_ploc_last_error())
    assert P.gpuart_ploc_run(h, C.byref(scene), C.byref(spare), None, C.byref(res)) == ERR_ARG
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == scene.generation
    assert same_bits(direct_frame(B, O, be, c["built"]), frame)
    be.rebuild(mode="clustered")           # ... and the handle still builds: the restatement's tree of the primitives as they lie now
    tree2, _ = PR.build(tree_prims(c["built"]))
    assert_arrays(be, tree2, "rebuilt after the refusals")


# ---- Renderer ---------------------------------------------------------------------------------------------------------------------
def test_rebuild_tree_clustered_keeps_the_history_between_two_updates(B, O):
    """update_primitives, rebuild_tree("clustered"), update_primitives with the temporal history on, as tests/test_build.py does for the
    Morton build: after each step the accumulator and the pick of every pixel are the oracle's on the restatement's tree, read_preview
    is the restatement chain's and differs from read_denoised — the history is there —, GetBVH().Compile() is the restatement's tree
    (the host tree adopted the device's topology), and the ordinals still index the caller's descriptions. The second update goes
    through the refit handle bound before the rebuild, which binds again. Then a Morton rebuild and a clustered one more, each on its
    restatement."""
    from gpuart_amd import synth_scenes as S
    from tests.test_build_ref import same_device_words
    from tests.test_temporal import SPHERE, TRACK, Shadow, cam_dict, tile_xy
    RW, RH = 48, 32
    cam = cam_dict(TRACK[0])
    descs = S.box_scene()
    tree0 = np.ascontiguousarray(O.build_bvh(descs)[0], np.float32)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], RW, RH)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    seeds = O.randseeds(9)
    crs, crd = O.cam_rays(c, RW, RH)
    crs, crd = crs.reshape(-1, 4), crd.reshape(-1, 4)
    r = B.Renderer(RW, RH, cam)
    try:
        r.set_primitives(descs)
        r.set_user_sphere(SPHERE[:3], SPHERE[3])
        r.set_temporal_history(True)
        sh = Shadow(B, r, SPHERE, 0)
        r.restart_path_tracing(1, 3)
        for _ in range(3):
            r.path_tracing_pass()
        used = [3]

        def step(tree, descs_now, what):
            """Two passes on `tree`: accumulator, pick, preview, the host tree and the ordinals."""
            exp = np.zeros((RH, RW, 4), np.float32)
            for _ in range(2):
                r.path_tracing_pass()
                O.pt_pass(tree, c, RW, RH, P, seeds[used[0]], 1, exp)
                used[0] += 1
            assert_bits(r.read_radiance(False)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), what + ": passes")
            o0, o1 = O.traverse(tree, crs, crd, SPHERE)
            hits, prims = r.pick(tile_xy(r), want_prims=True)
            assert_same_bits(words(hits), hook_record(o0, o1)[0], what + ": pick")
            got = r.read_preview()
            assert_same_bits(got, sh.preview(cam, 2), what + ": preview")
            assert not same_bits(got, r.read_denoised()), what
            assert same_device_words(r.compile_bvh(), tree), what + ": the host tree"
            flat, w = prims.reshape(-1), words(hits)
            assert (flat >= 0).sum() > 100
            for k in np.unique(flat[flat >= 0]):
                sel = np.nonzero(flat == k)[0]
                p0, p1 = own_hit(O, descs_now[k][0], RR.payload_of(descs_now[k]), crs[sel], crd[sel])
                assert_same_bits(w[sel, :7], np.concatenate([p0, p1[:, :3]], 1), "%s: description %d" % (what, k))

        idx = [k for k, d in enumerate(descs) if d[0] in (S.SPHERE, S.TRIANGLE, S.CONE)][:6][::-1]
        descs1 = _moved_descs(S, descs, idx, [0.05, -0.03, 0.04])
        sh.commit(cam, 3)
        assert r.update_primitives(idx, [descs1[k] for k in idx])      # (binds the refit handle to the uploaded arrays)
        tree1 = _refit_by_desc(tree0, descs, descs1, idx)
        step(tree1, descs1, "refitted")

        sh.commit(cam, 2)
        perm = r.rebuild_tree("clustered")
        tree2, new_to_old = PR.build(tree_prims(tree1))
        assert perm is not None and (perm == new_to_old).all() and r.is_ok()
        exp_cost, n_recs = BC.cost_of(tree2)
        assert r.tree_cost() == pytest.approx(exp_cost, rel=n_recs * 2.0 ** -52, abs=0)
        step(tree2, descs1, "clustered")

        idx2 = idx[:3] + [k for k, d in enumerate(descs) if d[0] == S.DISC][:1]
        descs2 = _moved_descs(S, descs1, idx2, [-0.04, 0.02, 0.03])
        sh.commit(cam, 2)
        assert r.update_primitives(idx2, [descs2[k] for k in idx2])   # (the refit handle, stale, binds to the rebuilt arrays)
        tree3 = _refit_by_desc(tree2, descs1, descs2, idx2)
        step(tree3, descs2, "clustered, refitted")

        perm = r.rebuild_tree()                                        # the Morton build, as before
        tree4, order4 = BR.build(tree_prims(tree3))
        assert perm is not None and (perm == order4).all() and same_device_words(r.compile_bvh(), tree4)
        perm = r.rebuild_tree("clustered")
        tree5, order5 = PR.build(tree_prims(tree4))
        assert perm is not None and (perm == order5).all() and same_device_words(r.compile_bvh(), tree5)
        assert_arrays(r.backend, tree5, "Morton, clustered")
        with pytest.raises(ValueError, match="mode"):
            r.rebuild_tree("sah")
    finally:
        r.close()


def test_rebuild_tree_clustered_refuses_a_tree_with_exact_boxes(B):
    from gpuart_amd import synth_scenes as S
    from tests.test_temporal import TRACK, cam_dict
    r = B.Renderer(48, 32, cam_dict(TRACK[0]))
    try:
        r.set_primitives(S.box_scene() + [(S.SPHERE, [float(2 ** 21), 0.0, 0.0, 1.0])])
        assert r.backend.scene_device().exact_boxes == 1
        before = r.compile_bvh()
        assert r.rebuild_tree("clustered") is None and r.is_ok()
        assert same_bits(r.compile_bvh(), before)
    finally:
        r.close()
