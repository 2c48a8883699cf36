"""The tree of an uploaded scene rebuilt on the device in Morton order (include/gpuart_build.h, libgpuart_build.so; Backend.rebuild,
Backend.tree_cost, Renderer.rebuild_tree): the device arrays afterwards are what the uploader makes of the restatement's tree
(tests/build_ref.py, tests/converter_ref.py) byte for byte, frames and queries of the rebuilt context are the oracle's on that tree bit
for bit, rebuild, refit and upload compose, a refusal changes nothing, and the cost measure is its restatement's."""
import ctypes as C

import numpy as np
import pytest

from tests import build_cases as BC
from tests import build_ref as BR
from tests import converter_ref as CR
from tests import refit_ref as RR
from tests.test_kernel_variants import scene_setup, to_params, tree_of as variant_tree
from tests.test_ray_queries import assert_same_bits, hook_record, random_rays, rays8, tree_prims, words
from tests.util import assert_bits, pad4, same_bits, to_device

pytestmark = pytest.mark.gpu
W, H = 40, 24
ERR_ARG = -1


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


def device_arrays(b):
    """(recs (R, 4, 4), prims (P, 3, 4), prim_boxes (P, 6)) read back from the context's device arrays through the HIP runtime."""
    hip = C.CDLL("libamdhip64.so.7")
    s = b.scene_device()
    recs, prims, boxes = np.zeros((s.n_recs, 4, 4), np.float32), np.zeros((s.n_prims, 3, 4), np.float32), np.zeros((s.n_prims, 6), np.float32)
    for a, ptr in ((recs, s.recs), (prims, s.prims), (boxes, s.prim_boxes)):
        if a.size:
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(a.nbytes), C.c_int(2)) == 0   # hipMemcpyDeviceToHost
    return recs, prims, boxes


def same_arrays(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def assert_arrays(b, tree, what):
    """The device arrays, and what the context knows of the tree, are the restatement's of `tree`."""
    cv = CR.convert(tree)
    recs, prims, boxes = device_arrays(b)
    assert recs.shape == cv["recs"].shape and prims.shape == cv["prims"].shape, what
    assert (recs.view(np.uint32) == cv["recs"].view(np.uint32)).all(), "%s: records differ" % what
    assert (prims.view(np.uint32) == cv["prims"].view(np.uint32)).all(), "%s: primitives differ" % what
    lo, hi = BR.boxes_of(tree_prims(tree))
    assert same_bits(boxes, np.concatenate([lo, hi], 1)), "%s: primitive boxes differ" % what
    s = b.scene_device()
    assert same_bits(np.array(s.root_min[:], np.float32), cv["root_min"]) and same_bits(np.array(s.root_max[:], np.float32), cv["root_max"]), what
    assert s.root_ref == cv["root_ref"] and s.max_depth == cv["max_depth"] and s.n_recs == len(cv["recs"]), what
    return cv


def rebuild(b, device):
    """(new_to_old as NumPy, the result's dict), through the device-tensor or the host entry."""
    perm = b.rebuild(out=bool(device))
    out = b.last_rebuild
    if device:
        assert perm.is_cuda
        perm = perm.cpu().numpy().view(np.uint32)
    return perm, out


# ---- bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, name", list(enumerate(BC.SCENES)))
def test_device_arrays_equal_the_restatement(be, B, k, name):
    c = BC.case(name)
    be.upload_bvh(c["tree"])
    before = be.scene_device()
    perm, out = rebuild(be, device=k % 2 == 0)
    assert (perm == c["new_to_old"]).all(), name
    cv = assert_arrays(be, c["built"], name)
    assert out["n_recs"] == len(cv["recs"]) == (len(c["prims"]) + 1) // 2 - 1 and out["root_ref"] == cv["root_ref"] and out["max_depth"] == cv["max_depth"]
    assert same_bits(out["root_min"], cv["root_min"]) and same_bits(out["root_max"], cv["root_max"]) and out["subnormal"] == cv["subnormal"] == (name in BC.SUBNORMAL)
    lay = CR.layout(c["built"])
    inner = ~lay["leaf"]
    assert out["levels"] == (int(lay["depth"][inner].max()) + 1 if inner.any() else 0)
    now = be.scene_device()
    assert now.generation == before.generation + 1 and now.n_prims == before.n_prims and now.exact_boxes == 0
    assert now.box_slack == B.tree_slack(c["built"])[0] and be.scene_order() == 1 and (now.box_slack == np.inf) == cv["subnormal"]
    assert be.tree_cost() == pytest.approx(BC.cost_of(c["built"])[0], rel=max(1, len(cv["recs"])) * 2.0 ** -52, abs=0)


def test_the_mark_of_the_top_levels_is_written(be, B, monkeypatch):
    """GPUART_HIP_TOP_DEPTH marks the records above that level, as the uploader's fill does."""
    monkeypatch.setenv("GPUART_HIP_TOP_DEPTH", "3")
    c = BC.case("scene_p")
    be.upload_bvh(c["tree"])
    be.rebuild()
    recs = device_arrays(be)[0]
    exp = CR.convert(c["built"], top_depth=3)["recs"]
    assert same_bits(recs, exp) and exp.view(np.uint32)[:, 2, 3].sum() == 7


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def own_hit(O, t, d, rs, rd):
    q = np.tile(np.asarray(d, np.float32).reshape(1, 4, 4), (len(rs), 1, 1))
    return (O.sphere(rs, rd, q[:, 0]) if t == 0 else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == 1 else
            O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == 2 else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))


def check_frames(B, O, b, tree, what, modes=(0, 3, 5)):
    """The direct frame, three path-tracing passes per mode, 3 000 random rays and the G-buffer of context b against the oracle on `tree`;
    every ordinal trace_rays returns names, in the tree's own numbering, the primitive whose own intersection is the hit."""
    c, P, lo, hi, us = scene_setup(O, tree, W, H)
    b.set_camera(c)
    b.render_direct(to_params(B, P))
    exp, _ = O.render_direct(tree, c, W, H, P)
    assert_bits(b.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), what + ": direct frame")
    seeds = O.randseeds(3)
    acc = np.zeros((H, W, 4), np.float32)
    for sd in seeds:
        O.pt_pass(tree, c, W, H, P, sd, 1, acc)
    for mode in modes:
        b.set_mode(mode)
        b.pt_reset()
        for sd in seeds:
            b.pt_pass(to_params(B, P), sd, 1)
        assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "%s: path tracing, mode %d" % (what, mode))
    b.set_mode(0)
    rs, rd = random_rays(np.random.default_rng(11), 3000, lo, hi)
    rs, rd = pad4(rs), pad4(rd)
    o0, o1 = O.traverse(tree, rs, rd, us)
    hits, ordinals = b.trace_rays(rays8(rs, rd), user_sphere=us, want_prims=True)
    assert_same_bits(words(hits), hook_record(o0, o1)[0], what + ": trace_rays")
    prims = tree_prims(tree)
    assert ordinals.max() < len(prims) and (ordinals >= 0).sum() > 100
    for k in np.unique(ordinals[ordinals >= 0]):
        sel = np.nonzero(ordinals == k)[0]
        p0, p1 = own_hit(O, prims[k][0], prims[k][1], rs[sel], rd[sel])
        assert_same_bits(words(hits)[sel, :7], np.concatenate([p0, p1[:, :3]], 1), "%s: ordinal %d" % (what, k))
    crs, crd = O.cam_rays(c, W, H)
    o0, o1 = O.traverse(tree, crs.reshape(-1, 4), crd.reshape(-1, 4), us)
    hits, _ = b.gbuffer(user_sphere=us)
    assert_same_bits(words(hits), hook_record(o0, o1)[0], what + ": gbuffer")


@pytest.mark.parametrize("name", ["scene_p", "scene_d", "box"])   # round, flat, every type
def test_frames_and_queries_after_a_rebuild_are_the_oracles(be, B, O, name):
    c = BC.case(name)
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.rebuild()
    check_frames(B, O, be, c["built"], name)


def test_frames_under_the_nearest_first_walk(be, B, O):
    c = BC.case("scene_d")
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.set_nearest_first(0)
    be.rebuild()
    assert be.scene_order() == 0
    check_frames(B, O, be, c["built"], "nearest first", modes=(0, 3))


def test_a_pass_requested_before_a_rebuild_renders_the_old_tree(be, B, O):
    """pass, rebuild, pass, read: the accumulator is the oracle's pass on the uploaded tree plus its pass on the built one (the box scene:
    tests/test_build_ref.py shows its camera rays free of phantom hits, and each pass is compared with the oracle on the tree it saw)."""
    c = BC.case("box")
    cam, P, _, _, _ = scene_setup(O, c["tree"], W, H)
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.set_camera(cam)
    seeds = O.randseeds(2)
    be.pt_reset()
    be.pt_pass(to_params(B, P), seeds[0], 1)     # only collected: the rebuild must flush it first
    be.rebuild()
    be.pt_pass(to_params(B, P), seeds[1], 1)
    acc = np.zeros((H, W, 4), np.float32)
    O.pt_pass(c["tree"], cam, W, H, P, seeds[0], 1, acc)
    old_only = acc.copy()
    O.pt_pass(c["built"], cam, W, H, P, seeds[1], 1, acc)
    assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "pass, rebuild, pass")
    assert not same_bits(acc, old_only)


# ---- rebuild, refit and upload ----------------------------------------------------------------------------------------------------
def test_a_refit_handle_is_stale_after_a_rebuild_and_binds_again(be, B):
    R = B.refit_lib()
    c = BC.case("scene_p")
    be.upload_bvh(c["tree"])
    be.refit([], [])                       # binds the handle to the uploaded arrays
    be.rebuild()
    scene = be.scene_device()
    built = device_arrays(be)
    res = B.RefitResult()
    assert R.gpuart_refit_run_host(be._refit, C.byref(scene), None, None, C.c_size_t(0), C.byref(res)) == ERR_ARG
    assert b"bound to another upload" in R.gpuart_refit_last_error()
    assert same_arrays(device_arrays(be), built)
    ordinals, payloads = RR.random_update(c["built"], np.random.default_rng(5), 0.3, 0.3)
    out = be.refit(to_device(ordinals.astype(np.int32)), to_device(np.ascontiguousarray(payloads, np.float32)))   # binds again
    lay = CR.layout(c["built"])
    assert out["levels"] == int(lay["depth"][~lay["leaf"]].max()) + 1
    assert_arrays(be, RR.refit(c["built"], ordinals, payloads), "rebuild, refit")


@pytest.mark.parametrize("name", ["n1", "n5", "same64", "scene_d"])
def test_a_rebuild_of_a_built_tree_is_the_identity(be, name):
    c = BC.case(name)
    be.upload_bvh(c["tree"])
    be.rebuild()
    first = device_arrays(be)
    perm, out = rebuild(be, device=True)
    assert (perm == np.arange(len(c["prims"]))).all()
    assert same_arrays(device_arrays(be), first)
    assert_arrays(be, c["built"], name)


def test_the_default_result_is_a_device_tensor_once_torch_is_in_use(be):
    """Backend.rebuild() alone returns new_to_old — on the device when the process has imported torch —, and keeps the build's report."""
    import torch
    c = BC.case("scene_p")
    be.upload_bvh(c["tree"])
    perm = be.rebuild()
    assert isinstance(perm, torch.Tensor) and perm.is_cuda and perm.dtype == torch.int32
    assert (perm.cpu().numpy().view(np.uint32) == c["new_to_old"]).all()
    assert be.last_rebuild["n_recs"] == (len(c["prims"]) + 1) // 2 - 1 and len(be.last_rebuild["step_ms"]) == 7
    again = be.rebuild(out=False)
    assert isinstance(again, np.ndarray) and again.dtype == np.uint32 and (again == np.arange(len(c["prims"]))).all()


def test_a_rebuild_into_the_former_arrays_ends_in_zeros(be):
    """The second rebuild writes into the arrays the upload made, which held more records than the built tree has: beyond the new last
    record they are zero again, as behind an upload's."""
    c = BC.case("scene_d")
    be.upload_bvh(c["tree"])
    room = be.scene_device().n_recs
    be.rebuild()
    be.rebuild()
    s = be.scene_device()
    assert s.n_recs < room
    hip = C.CDLL("libamdhip64.so.7")
    tail = np.ones((room - s.n_recs + 1, 4, 4), np.float32)   # (+ 1: the slack record past the end)
    assert hip.hipMemcpy(tail.ctypes.data_as(C.c_void_p), C.c_void_p(s.recs + 64 * s.n_recs), C.c_size_t(tail.nbytes), C.c_int(2)) == 0
    assert not tail.view(np.uint32).any()
    assert_arrays(be, c["built"], "rebuilt twice")


def test_an_upload_after_a_rebuild_restores_the_uploaded_bytes(be):
    c = BC.case("box")
    be.upload_bvh(c["tree"])
    uploaded = device_arrays(be)
    be.rebuild()
    assert not same_bits(device_arrays(be)[1], uploaded[1])
    be.upload_bvh(c["tree"])
    assert same_arrays(device_arrays(be), uploaded)
    be.rebuild()                           # (the spare set of the first scene is gone with it: reserved anew)
    assert_arrays(be, c["built"], "upload, rebuild, upload, rebuild")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wild", "disorderly", "empty"])
def test_trees_with_exact_boxes_are_not_rebuilt(be, B, name):
    be.upload_bvh(variant_tree(name))
    uploaded, before = device_arrays(be), be.scene_device()
    assert before.exact_boxes == 1
    with pytest.raises(B.HipError, match="build: src: a tree with irregular boxes") as e:
        be.rebuild()
    assert e.value.code == ERR_ARG
    spare = be.scene_reserve(before.n_recs)
    spare.n_recs = before.n_recs
    with pytest.raises(B.HipError, match="irregular") as e:
        be.scene_rebuilt(spare)
    assert e.value.code == ERR_ARG
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == before.generation
    if name == "empty":   # ... and the dummy leaf of count 0 is refused for itself, whatever the struct says of the boxes
        Bd, res = B.build_lib(), B.BuildResult()
        claimed = B.HipScene.from_buffer_copy(before)
        claimed.exact_boxes = 0
        claimed.root_min, claimed.root_max = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
        perm = to_device(np.zeros(1, np.int32))
        assert Bd.gpuart_build_run(be._build_handle(), C.byref(claimed), C.byref(spare), C.c_void_p(perm.data_ptr()), C.byref(res)) == ERR_ARG
        assert b"empty scene" in Bd.gpuart_build_last_error()
        assert same_arrays(device_arrays(be), uploaded)


def test_refused_rebuilds_change_nothing(be, B):
    Bd = B.build_lib()
    c = BC.case("scene_p")
    be.upload_bvh(c["tree"])
    uploaded, scene = device_arrays(be), be.scene_device()
    n = scene.n_prims
    res = B.BuildResult()
    perm = to_device(np.zeros(n, np.int32))
    h = be._build_handle()

    def run(src, dst):
        return Bd.gpuart_build_run(h, C.byref(src), C.byref(dst), C.c_void_p(perm.data_ptr()), C.byref(res))

    def edited(s, **kw):
        t = B.HipScene.from_buffer_copy(s)
        for k, v in kw.items():
            setattr(t, k, v)
        return t
    spare = be.scene_reserve((n + 1) // 2 - 1)
    for what, src, dst, word in [("dst is src", scene, scene, b"alias"),
                                 ("dst's records are src's", scene, edited(spare, recs=scene.recs, n_recs=scene.n_recs), b"alias"),
                                 ("dst too small", scene, edited(spare, n_prims=n - 1), b"too small"),
                                 ("too few records", scene, edited(spare, n_recs=(n + 1) // 2 - 2), b"too small"),
                                 ("unknown layout", edited(scene, layout=2), spare, b"unknown layout"),
                                 ("unknown dst layout", scene, edited(spare, layout=0), b"unknown layout"),
                                 ("no primitives", edited(scene, n_prims=0), spare, b"empty"),
                                 ("a root box out of order", edited(scene, root_min=(C.c_float * 3)(1, 0, 0), root_max=(C.c_float * 3)(0, 1, 1)), spare, b"root box"),
                                 ("an infinite root box", edited(scene, root_max=(C.c_float * 3)(np.inf, 1, 1)), spare, b"root box")]:
        assert run(src, dst) == ERR_ARG and word in Bd.gpuart_build_last_error(), (what, Bd.gpuart_build_last_error())
    assert Bd.gpuart_build_run(h, C.byref(scene), C.byref(spare), None, C.byref(res)) == ERR_ARG
    # the context: arrays that were not reserved, a changed count, a depth beyond the stacks, a bad root box
    ok = edited(spare, n_recs=(n + 1) // 2 - 1, root_min=scene.root_min, root_max=scene.root_max, max_depth=10)
    for what, built, word in [("the scene's own arrays", edited(ok, recs=scene.recs, prims=scene.prims, prim_boxes=scene.prim_boxes), "not the ones"),
                              ("another count", edited(ok, n_prims=n - 1), "primitive count"),
                              ("too deep", edited(ok, max_depth=1025), "1024"),
                              ("more records than reserved", edited(ok, n_recs=spare.n_recs + 1), "more records"),
                              ("a root ref that is no record 0", edited(ok, root_ref=5), "root ref"),
                              ("a leaf root over records", edited(ok, root_ref=0xe0000000), "root ref"),
                              ("a leaf root beyond the primitives", edited(ok, n_recs=0, root_ref=0x80000000 | n), "root ref"),
                              ("a root box out of order", edited(ok, root_min=(C.c_float * 3)(1, 0, 0), root_max=(C.c_float * 3)(0, 1, 1)), "root box")]:
        with pytest.raises(B.HipError, match=word) as e:
            be.scene_rebuilt(built)
        assert e.value.code == ERR_ARG, what
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == scene.generation
    # a stale `built`: reserved before a rebuild that has since been adopted
    be.rebuild()
    built, now = device_arrays(be), be.scene_device()
    assert now.generation == scene.generation + 1
    with pytest.raises(B.HipError, match="not the ones"):
        be.scene_rebuilt(ok)
    assert same_arrays(device_arrays(be), built) and be.scene_device().generation == now.generation
    bare = B.Backend(0)
    try:
        with pytest.raises(B.HipError, match="no scene"):
            bare.scene_reserve(1)
    finally:
        bare.close()


# ---- cost -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n2", "n3", "box", "scene_d", "mesh20k"])
def test_the_cost_is_its_restatements(be, name):
    """On the uploaded (reference-built) tree: tree_cost() is the math.fsum restatement within n_recs 2^-52 relative, the bound of an fp64
    sum of positive terms in any order; and the same value when asked again."""
    tree = BC.case(name)["tree"]
    be.upload_bvh(tree)
    exp, n_recs = BC.cost_of(tree) if name != "n2" else (0.0, 0)
    got = be.tree_cost()
    assert got == pytest.approx(exp, rel=max(1, n_recs) * 2.0 ** -52, abs=0) and be.tree_cost() == got
    assert (got > 0) == (n_recs > 0)


def test_a_rebuild_repairs_a_drifted_tree(be, O):
    """Scene D with every primitive moved to another's place and refitted: the cost and the nodes the oracle visits for the fixed ray
    set (tests/build_cases.drift says which and why) are both strictly lower after rebuild() than before. The device arrays are the
    restatement's before and after, so the oracle's count on the restatement's trees is the count of the trees on the device."""
    d = BC.drift()
    be.upload_bvh(d["tree"])
    be.refit(d["ordinals"], d["payloads"])
    assert_arrays(be, d["refitted"], "drifted")
    before = be.tree_cost()
    perm = be.rebuild(out=False)
    assert (perm == d["new_to_old"]).all()
    assert_arrays(be, d["rebuilt"], "drifted, rebuilt")
    after = be.tree_cost()
    rs, rd = d["rays"]
    steps_before = O.traverse(d["refitted"], rs, rd, None, want_stats=True)[2].nodes
    steps_after = O.traverse(d["rebuilt"], rs, rd, None, want_stats=True)[2].nodes
    print("cost %.4f -> %.4f, box steps %d -> %d" % (before, after, steps_before, steps_after))
    assert after < before and steps_after < steps_before


# ---- Renderer ---------------------------------------------------------------------------------------------------------------------
def _ordinal_to_desc(tree, descs):
    """Per device ordinal of `tree` the index of its description (the box scene's primitives are all different)."""
    keys = {(d[0], RR.payload_of(d).tobytes()): k for k, d in enumerate(descs)}
    return [keys[(t, d.tobytes())] for t, d in tree_prims(tree)]


def _moved_descs(S, descs, idx, delta):
    out = list(descs)
    for k in idx:
        t, f = descs[k]
        f = np.asarray(f, np.float32).copy()
        for a in {S.SPHERE: (0,), S.DISC: (0,), S.TRIANGLE: (0, 3, 6), S.CONE: (0, 3)}[t]:
            f[a:a + 3] += np.float32(delta)
        out[k] = (t, [float(v) for v in f])
    return out


def _refit_by_desc(tree, descs_now, descs_new, idx):
    """RR.refit of `tree`, whose primitives are descs_now, with the descriptions idx replaced by descs_new's."""
    order = {id_: o for o, id_ in enumerate(_ordinal_to_desc(tree, descs_now))}
    pairs = sorted((order[k], k) for k in idx)
    return RR.refit(tree, [o for o, _ in pairs], np.stack([RR.payload_of(descs_new[k]) for _, k in pairs]))


def test_rebuild_tree_keeps_the_history_between_two_updates(B, O):
    """update_primitives, rebuild_tree, update_primitives with the temporal history on: after each step the accumulator and the pick of
    every pixel are the oracle's on the restatement's tree (refit of the uploaded one; its rebuild; the refit of that), read_preview is
    the restatement chain's (tests/temporal_ref.py, tests/denoise_ref.py) and differs from read_denoised — the history is there —,
    GetBVH().Compile() is the restatement's tree, and trace_rays' ordinals still index the caller's descriptions."""
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
        assert r.update_primitives(idx, [descs1[k] for k in idx])
        tree1 = _refit_by_desc(tree0, descs, descs1, idx)
        step(tree1, descs1, "refitted")

        cost_before = r.tree_cost()
        exp_cost, n_recs = BC.cost_of(tree1)
        assert cost_before == pytest.approx(exp_cost, rel=n_recs * 2.0 ** -52, abs=0)
        sh.commit(cam, 2)
        perm = r.rebuild_tree()
        tree2, new_to_old = BR.build(tree_prims(tree1))
        assert perm is not None and (perm == new_to_old).all() and r.is_ok()
        exp_cost, n_recs = BC.cost_of(tree2)
        assert r.tree_cost() == pytest.approx(exp_cost, rel=n_recs * 2.0 ** -52, abs=0)
        step(tree2, descs1, "rebuilt")

        idx2 = idx[:3] + [k for k, d in enumerate(descs) if d[0] == S.DISC][:1]
        descs2 = _moved_descs(S, descs1, idx2, [-0.04, 0.02, 0.03])
        sh.commit(cam, 2)
        assert r.update_primitives(idx2, [descs2[k] for k in idx2])   # (the refit handle binds to the rebuilt arrays)
        step(_refit_by_desc(tree2, descs1, descs2, idx2), descs2, "rebuilt, refitted")
    finally:
        r.close()


def test_rebuild_tree_refuses_a_tree_with_exact_boxes(B):
    """A scene the uploader classifies disorderly (a sphere beyond 2^20): rebuild_tree is refused, the renderer stays usable."""
    from gpuart_amd import synth_scenes as S
    from tests.test_temporal import TRACK, cam_dict
    r = B.Renderer(48, 32, cam_dict(TRACK[0]))
    try:
        r.set_primitives(S.box_scene() + [(S.SPHERE, [float(2 ** 21), 0.0, 0.0, 1.0])])
        assert r.backend.scene_device().exact_boxes == 1
        before = r.compile_bvh()
        assert r.rebuild_tree() is None and r.is_ok()
        assert same_bits(r.compile_bvh(), before)
    finally:
        r.close()
