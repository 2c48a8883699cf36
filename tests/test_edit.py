"""Primitives of an uploaded scene removed and appended on the device (include/gpuart_edit.h, libgpuart_edit.so; Backend.edit,
gpuart_hip_scene_reserve_prims, gpuart_hip_scene_replaced): the staging list and `source` are the restatement's (tests/edit_ref.py), the
device arrays after the build are what the uploader makes of the restatement's tree of the edited list (tests/build_ref.py,
tests/ploc_ref.py, tests/converter_ref.py) byte for byte, frames and queries of the edited context are the oracle's on that tree bit for
bit, the kernel specialisation follows the new type mask, a refusal changes nothing, and edit, refit, rebuild and upload compose."""
import ctypes as C

import numpy as np
import pytest

from tests import build_ref as BR
from tests import converter_ref as CR
from tests import edit_cases as EC
from tests import edit_ref as ER
from tests import ploc_ref as PR
from tests import refit_ref as RR
from tests.test_kernel_variants import names_of, scene_setup, to_params, tree_of as variant_tree
from tests.test_ray_queries import assert_same_bits, hook_record, random_rays, rays8, tree_prims, words
from tests.util import assert_bits, pad4, same_bits, to_device

pytestmark = pytest.mark.gpu
W, H = 40, 24
ERR_ARG = -1
NONE = 0xffffffff


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


def from_device(ptr, shape, dtype=np.float32):
    a = np.zeros(shape, dtype)
    if a.size:
        hip = C.CDLL("libamdhip64.so.7")
        assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(a.nbytes), C.c_int(2)) == 0   # hipMemcpyDeviceToHost
    return a


def device_arrays(b):
    """(recs (R, 4, 4), prims (P, 3, 4), prim_boxes (P, 6)) read back from the context's device arrays through the HIP runtime."""
    s = b.scene_device()
    return from_device(s.recs, (s.n_recs, 4, 4)), from_device(s.prims, (s.n_prims, 3, 4)), from_device(s.prim_boxes, (s.n_prims, 6))


def same_arrays(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def assert_arrays(b, tree, what, room=None, uploaded=False):
    """The device arrays, and what the context knows of the tree, are the restatement's of `tree`; behind the records and the primitives
    the arrays end in zeros, as an upload's do (`room`: primitives the arrays are known to hold room for; `uploaded`: the boxes came with
    an upload, which leaves what lies behind them as it was allocated)."""
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
    room = max(room or 0, s.n_prims)
    assert not from_device(s.recs + 64 * s.n_recs, (16,), np.uint32).any(), "%s: the slack behind the records" % what
    assert not from_device(s.prims + 48 * s.n_prims, (12 * (room - s.n_prims) + 16,), np.uint32).any(), "%s: the slack behind the primitives" % what
    assert uploaded or not from_device(s.prim_boxes + 24 * s.n_prims, (6 * (room - s.n_prims) + 4,), np.uint32).any(), "%s: the slack behind the boxes" % what
    return cv


def edit(b, c, mode, device):
    """The composed map as NumPy int32, through the device-tensor or the NumPy path."""
    if device:
        got = b.edit(to_device(c["remove"].astype(np.int32)), to_device(c["types"].astype(np.int32)), to_device(np.ascontiguousarray(c["payload"], np.float32)), mode=mode)
        assert got.is_cuda
        return got.cpu().numpy()
    got = b.edit(c["remove"], c["types"], c["payload"], mode=mode, out=False)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32
    return got


def own_hit(O, t, d, rs, rd):
    q = np.tile(np.asarray(d, np.float32).reshape(1, 4, 4), (len(rs), 1, 1))
    return (O.sphere(rs, rd, q[:, 0]) if t == 0 else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == 1 else
            O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == 2 else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))


def check_frames(B, O, b, tree, prim_of, what):
    """The direct frame, two path-tracing passes and 1 500 random rays of context b against the oracle on `tree`; every ordinal
    trace_rays returns names, through prim_of, the primitive whose own intersection is the hit."""
    c, P, lo, hi, us = scene_setup(O, tree, W, H)
    b.resize(W, H)
    b.set_camera(c)
    b.render_direct(to_params(B, P))
    exp, _ = O.render_direct(tree, c, W, H, P)
    assert_bits(b.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), what + ": direct frame")
    acc = np.zeros((H, W, 4), np.float32)
    b.pt_reset()
    for sd in O.randseeds(2):
        O.pt_pass(tree, c, W, H, P, sd, 1, acc)
        b.pt_pass(to_params(B, P), sd, 1)
    assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), what + ": path tracing")
    rs, rd = random_rays(np.random.default_rng(11), 1500, lo, hi)
    rs, rd = pad4(rs), pad4(rd)
    o0, o1 = O.traverse(tree, rs, rd, us)
    hits, ordinals = b.trace_rays(rays8(rs, rd), user_sphere=us, want_prims=True)
    assert_same_bits(words(hits), hook_record(o0, o1)[0], what + ": trace_rays")
    assert ordinals.max() < len(tree_prims(tree)) and (ordinals >= 0).any()
    for k in np.unique(ordinals[ordinals >= 0]):
        sel = np.nonzero(ordinals == k)[0]
        t, d = prim_of(int(k))
        p0, p1 = own_hit(O, t, d, rs[sel], rd[sel])
        assert_same_bits(words(hits)[sel, :7], np.concatenate([p0, p1[:, :3]], 1), "%s: ordinal %d" % (what, k))


# ---- the library alone: the staging list --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.SMALL)
def test_the_staging_list_is_the_restatements(be, B, name):
    c = EC.case(name)
    E, h = B.edit_lib(), be._edit_handle()
    be.upload_bvh(c["tree"])
    scene, uploaded = be.scene_device(), device_arrays(be)
    n_new = len(c["edited"])
    lists = []
    for device in (False, True):
        edited, res = B.HipScene(), B.EditResult()
        if device:
            rem, typ, pay = to_device(c["remove"].astype(np.int32)), to_device(c["types"].astype(np.int32)), to_device(np.ascontiguousarray(c["payload"], np.float32))
            src = to_device(np.full(n_new, -7, np.int32))
            ptr = lambda t: C.c_void_p(t.data_ptr() if t.numel() else None)
            rc = E.gpuart_edit_run(h, C.byref(scene), ptr(rem), C.c_size_t(rem.numel()), ptr(typ), ptr(pay), C.c_size_t(typ.numel()), ptr(src), C.byref(edited), C.byref(res))
            source = src.cpu().numpy()
        else:
            source = np.full(n_new, -7, np.int32)
            rc = E.gpuart_edit_run_host(h, C.byref(scene), B._p(c["remove"]), C.c_size_t(len(c["remove"])), B._p(c["types"]), B._p(c["payload"]),
                                        C.c_size_t(len(c["types"])), B._p(source), C.byref(edited), C.byref(res))
        assert rc == 0, E.gpuart_edit_last_error()
        assert (source == c["source"]).all(), name
        recs, boxes = ER.device_list(c["edited"])
        got = from_device(edited.prims, (n_new, 3, 4)), from_device(edited.prim_boxes, (n_new, 6))
        assert (got[0].view(np.uint32) == recs.view(np.uint32)).all(), "%s: the list's records" % name
        assert same_bits(got[1], boxes), "%s: the list's boxes" % name
        lists.append(got)
        rlo, rhi = BR.root_box(boxes[:, :3], boxes[:, 3:])
        for r in (res, edited):   # == on floats: the sign of a zero plane is the reduction's own (include/gpuart_edit.h)
            assert (np.array(r.root_min[:], np.float32) == rlo).all() and (np.array(r.root_max[:], np.float32) == rhi).all(), name
        assert res.status == 0 and res.first_bad == NONE and res.n_prims == n_new and res.type_mask == ER.type_mask(c["edited"])
        assert (edited.layout, edited.exact_boxes, edited.n_prims, edited.n_recs, edited.recs, edited.generation) == (1, 0, n_new, 0, None, scene.generation)
    assert same_arrays(*lists)
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == scene.generation   # the scene itself is untouched


def test_the_root_box_takes_the_smaller_zero_whatever_the_grouping(be, B):
    """Points at zeros of mixed signs (build_cases zeros5): the reduction's minimum planes are -0 wherever a -0 is among the boxes and
    its maximum planes +0 wherever a +0 is — bits the sequential fold only reaches by the order of the list — and they compare equal."""
    from tests import build_cases as BC
    c = BC.case("zeros5")
    be.upload_bvh(c["tree"])
    scene, edited, res = be.scene_device(), B.HipScene(), B.EditResult()
    source = np.zeros(len(c["prims"]), np.int32)
    E = B.edit_lib()
    assert E.gpuart_edit_run_host(be._edit_handle(), C.byref(scene), None, C.c_size_t(0), None, None, C.c_size_t(0), B._p(source), C.byref(edited), C.byref(res)) == 0
    lo, hi = BR.boxes_of(c["prims"])
    rlo, rhi = BR.root_box(lo, hi)
    got_lo, got_hi = np.array(res.root_min[:], np.float32), np.array(res.root_max[:], np.float32)
    assert (got_lo == rlo).all() and (got_hi == rhi).all()
    assert np.signbit(got_lo).all() and (source == np.arange(len(source))).all()   # every axis has a -0 among the lower planes


# ---- bytes, frames ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", EC.MODES)
@pytest.mark.parametrize("name", EC.SMALL)
def test_an_edited_scene_is_the_restatements(be, B, O, name, mode):
    c, bt = EC.case(name), EC.built(name, mode)
    n_old, n_new = len(c["prims"]), len(c["edited"])
    arrays = []
    for device in (False, True):
        be.upload_bvh(c["tree"])
        before = be.scene_device()
        composed = edit(be, c, mode, device)
        assert (composed == bt["composed"]).all(), name
        cv = assert_arrays(be, bt["tree"], "%s, %s" % (name, mode))
        arrays.append(device_arrays(be))
        now = be.scene_device()
        assert now.n_prims == n_new and now.generation == before.generation + 1 and now.exact_boxes == 0 and be.scene_order() == 1
        assert now.box_slack == B.tree_slack(bt["tree"])[0]
        assert be.scene_info() == dict(nodes=2 * len(cv["recs"]) + 1, prims=n_new, max_depth=cv["max_depth"], device_bytes=64 * len(cv["recs"]) + 48 * n_new)
        le = be.last_edit
        assert le["n_prims"] == n_new and le["type_mask"] == ER.type_mask(c["edited"]) == cv["type_mask"] and len(le["step_ms"]) == 4
        assert le["rebuild"]["n_recs"] == len(cv["recs"]) and le["rebuild"] is be.last_rebuild
    assert same_arrays(*arrays), "the tensor path and the NumPy path differ"

    def prim_of(k):
        s = int(bt["composed"][k])
        return c["prims"][s] if s < n_old else c["added"][s - n_old]
    check_frames(B, O, be, bt["tree"], prim_of, "%s, %s" % (name, mode))


@pytest.mark.parametrize("mode", EC.MODES)
def test_an_edit_of_nothing_is_a_rebuild(be, mode):
    c = EC.case("neither")
    be.upload_bvh(c["tree"])
    perm = be.rebuild(out=False, mode=mode)
    rebuilt = device_arrays(be)
    be.upload_bvh(c["tree"])
    composed = edit(be, c, mode, device=False)
    assert (composed == perm.astype(np.int32)).all() and same_arrays(device_arrays(be), rebuilt)


def test_a_mesh_of_20k_is_edited(be, B):
    """The one large case, in Morton order through the tensor path: 200 removals spread over 80 workgroups, 151 additions."""
    c, bt = EC.case("mesh20k"), EC.built("mesh20k", "morton")
    be.upload_bvh(c["tree"])
    assert (edit(be, c, "morton", device=True) == bt["composed"]).all()
    assert_arrays(be, bt["tree"], "mesh20k")


# ---- the kernel specialisation follows the type mask ---------------------------------------------------------------------------------
@pytest.mark.parametrize("scene, gone, added, mask", [("box", (0, 3), [], 6), ("flat", (), [3], 12)])
def test_the_kernels_follow_the_new_type_mask(B, O, scene, gone, added, mask):
    """A mixed scene that becomes triangles and discs only, and a triangle scene that gains a cone: one direct frame and one pass launch
    the kernels a fresh context launches that uploaded the restatement's tree."""
    prims = EC.scene(scene)["prims"]
    remove = np.array([i for i, (t, _) in enumerate(prims) if t in gone], np.uint32)
    add = [p for p in EC.one_of_each() if p[0] in added]
    edited, _ = ER.edit(prims, remove, add)
    assert ER.type_mask(prims) != mask == ER.type_mask(edited)
    tree, _ = PR.build(edited)
    cam, P, _, _, _ = scene_setup(O, tree, W, H)
    ledgers = []
    for fresh in (False, True):
        b = B.Backend(0)
        try:
            b.resize(W, H)
            if fresh:
                b.upload_bvh(tree)
            else:
                b.upload_bvh(EC.scene(scene)["tree"])
                b.edit(remove, [t for t, _ in add], [d for _, d in add], out=False)
                assert b.last_edit["type_mask"] == mask
            b.set_camera(cam)
            b.launched()
            b.render_direct(to_params(B, P))
            b.pt_reset()
            b.pt_pass(to_params(B, P), O.randseeds(1)[0], 1)
            frames = b.read(0), b.read(1)
            ledgers.append((names_of(b.launched()), frames))
        finally:
            b.close()
    assert ledgers[0][0] == ledgers[1][0] and ledgers[0][0], (sorted(ledgers[0][0]), sorted(ledgers[1][0]))
    assert same_arrays(ledgers[0][1], ledgers[1][1])


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_edits_change_nothing(be, B, O):
    c = EC.case("remove_only")
    n = len(c["prims"])
    cam, P, _, _, _ = scene_setup(O, c["tree"], W, H)
    be.resize(W, H)
    be.upload_bvh(c["tree"])
    be.set_camera(cam)
    be.render_direct(to_params(B, P))
    frame, uploaded, scene = be.read(0), device_arrays(be), be.scene_device()
    for what, (remove, added, first_bad) in EC.refusals(n).items():
        for device in (False, True):
            case = dict(remove=np.array(remove, np.uint32), types=np.array([t for t, _ in added], np.uint32),
                        payload=np.array([d for _, d in added], np.float32).reshape(-1, 16))
            with pytest.raises(B.HipError, match="edit:") as e:
                edit(be, case, "clustered", device)
            assert e.value.code == ERR_ARG and e.value.first_bad == first_bad, what
    E, h = B.edit_lib(), be._edit_handle()
    edited, res = B.HipScene(), B.EditResult()
    source, one = to_device(np.zeros(n + 4, np.int32)), to_device(np.zeros(16, np.float32))
    zero = to_device(np.zeros(4, np.int32))

    def changed(s, **kw):
        t = B.HipScene.from_buffer_copy(s)
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    def run(src=scene, remove=None, n_remove=0, types=None, payload=None, n_add=0, src_ptr=source.data_ptr()):
        return E.gpuart_edit_run(h, C.byref(src), C.c_void_p(remove), C.c_size_t(n_remove), C.c_void_p(types), C.c_void_p(payload), C.c_size_t(n_add),
                                 C.c_void_p(src_ptr), C.byref(edited), C.byref(res))
    for what, kw, word in [("exact boxes", dict(src=changed(scene, exact_boxes=1)), b"irregular"),
                           ("an empty src", dict(src=changed(scene, n_prims=0)), b"empty"),
                           ("an unknown layout", dict(src=changed(scene, layout=2)), b"unknown layout"),
                           ("too many primitives", dict(types=zero.data_ptr(), payload=one.data_ptr(), n_add=0x05555540), b"too many"),
                           ("a NULL list", dict(n_remove=1), b"NULL"),
                           ("a NULL payload", dict(types=zero.data_ptr(), n_add=1), b"NULL"),
                           ("a NULL source", dict(src_ptr=None), b"NULL"),
                           ("a misaligned list", dict(remove=zero.data_ptr() + 2, n_remove=1), b"misaligned"),
                           ("a misaligned payload", dict(types=zero.data_ptr(), payload=one.data_ptr() + 4, n_add=1), b"misaligned")]:
        assert run(**kw) == ERR_ARG and word in E.gpuart_edit_last_error() and E.gpuart_edit_last_error().startswith(b"edit:"), (what, E.gpuart_edit_last_error())
    # the context: a bad mask, a count of 0 or beyond the room; and what scene_rebuilt refuses
    spare = be.scene_reserve_prims(n - 1, n + 2)
    assert spare.n_prims == n + 2 and spare.n_recs == n - 1
    ok = changed(spare, n_prims=n, n_recs=(n + 1) // 2 - 1, root_min=scene.root_min, root_max=scene.root_max, max_depth=10)
    for what, built, mask, word in [("a mask of 0", ok, 0, "type mask"), ("a mask of 16", ok, 16, "type mask"), ("no primitives", changed(ok, n_prims=0), 15, "primitive count"),
                                    ("beyond the room", changed(ok, n_prims=n + 3), 15, "primitive count"),
                                    ("the scene's own arrays", changed(ok, recs=scene.recs, prims=scene.prims, prim_boxes=scene.prim_boxes), 15, "not the ones"),
                                    ("too deep", changed(ok, max_depth=1025), 15, "1024"), ("more records than reserved", changed(ok, n_recs=n), 15, "more records"),
                                    ("a root ref that is no record 0", changed(ok, root_ref=5), 15, "root ref")]:
        with pytest.raises(B.HipError, match=word) as e:
            be.scene_replaced(built, mask)
        assert e.value.code == ERR_ARG, what
    for bad in (0, 0x05555540):
        with pytest.raises(B.HipError, match="primitive count"):
            be.scene_reserve_prims(1, bad)
    now = be.scene_device()
    assert same_arrays(device_arrays(be), uploaded) and (now.generation, now.n_prims, now.n_recs) == (scene.generation, scene.n_prims, scene.n_recs)
    be.render_direct(to_params(B, P))
    assert same_bits(be.read(0), frame)


def test_a_scene_with_exact_boxes_is_not_edited(be, B):
    be.upload_bvh(variant_tree("disorderly"))
    uploaded, before = device_arrays(be), be.scene_device()
    assert before.exact_boxes == 1
    with pytest.raises(B.HipError, match="edit: src: a tree with irregular boxes") as e:
        be.edit([0], [], [], out=False)
    assert e.value.code == ERR_ARG and e.value.first_bad is None
    assert same_arrays(device_arrays(be), uploaded) and be.scene_device().generation == before.generation


# ---- edit, refit, rebuild and upload ----------------------------------------------------------------------------------------------
def test_edits_refits_and_rebuilds_follow_each_other(be, B, O):
    """edit (126 -> 525: a new spare set), refit (the handle binds at the new generation), rebuild("morton") (the spare set, the
    former arrays with room for 126, is made anew), an edit that shrinks to 100 (into a set with room for 525: the tail is zeroed),
    rebuild("clustered") (room 525 is not 100: made anew): the restatements' chain at every step; then another scene is uploaded."""
    c, bt = EC.case("grow"), EC.built("grow", "clustered")
    be.upload_bvh(c["tree"])
    edit(be, c, "clustered", device=True)
    assert_arrays(be, bt["tree"], "edit")
    ordinals, payloads = RR.random_update(bt["tree"], np.random.default_rng(5), 0.2, 0.1)
    be.refit(ordinals, payloads)
    tree = RR.refit(bt["tree"], ordinals, payloads)
    assert_arrays(be, tree, "edit, refit")
    perm = be.rebuild(out=False, mode="morton")
    tree, new_to_old = BR.build(tree_prims(tree))
    assert (perm == new_to_old).all()
    assert_arrays(be, tree, "edit, refit, rebuild")
    prims = tree_prims(tree)
    remove = np.arange(50, 475, dtype=np.uint32)
    edited, source = ER.edit(prims, remove, [])
    tree, new_to_old = BR.build(edited)
    got = be.edit(remove, [], [], mode="morton", out=False)
    assert (got == source[new_to_old]).all() and len(edited) == 100
    assert_arrays(be, tree, "... an edit that shrinks", room=525)
    perm = be.rebuild(out=False, mode="clustered")
    tree, new_to_old = PR.build(tree_prims(tree))
    assert (perm == new_to_old).all()
    assert_arrays(be, tree, "... rebuild")
    other = EC.scene("box")["tree"]
    be.upload_bvh(other)
    assert_arrays(be, other, "another upload", uploaded=True)
    check_frames(B, O, be, other, lambda k: tree_prims(other)[k], "another upload")
    small = EC.case("remove_only")
    edit(be, small, "morton", device=False)   # (the spare set of the scene before went with it)
    assert_arrays(be, EC.built("remove_only", "morton")["tree"], "upload, edit")


# ---- Renderer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", EC.MODES)
def test_edit_primitives_keeps_the_history(B, O, mode):
    """edit_primitives with the temporal history on, measured as tests/test_build.py measures a rebuild's kept history: after the edit
    the accumulator and the pick of every pixel are the oracle's on the restatement's tree of the edited list, read_preview is the
    restatement chain's and differs from read_denoised — the history is there —, compile_bvh() is the restatement's tree, trace_rays'
    ordinals index the caller's edited descriptions and agree with `source`; update_primitives and rebuild_tree work afterwards. After
    set_primitives of the same list the preview is the denoised frame: that history is gone."""
    from gpuart_amd import synth_scenes as S
    from tests.test_build import _moved_descs, _ordinal_to_desc, _refit_by_desc
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
    build = BR.build if mode == "morton" else PR.build
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

        gone = [1, 6]                                   # the caller's numbering
        added = [(S.SPHERE, [0.3, 0.2, 0.4, 0.15]), (S.TRIANGLE, [-0.4, 0.1, 0.2, -0.1, 0.3, 0.3, -0.3, -0.2, 0.6])]
        desc_of = _ordinal_to_desc(tree0, descs)
        remove = sorted(o for o, d in enumerate(desc_of) if d in gone)
        edited, src = ER.edit(tree_prims(tree0), remove, EC.payloads(added))
        tree1, new_to_old = build(edited)
        sh.commit(cam, 3)
        source = r.edit_primitives(gone, added, mode)
        assert source is not None and (source == src[new_to_old]).all() and r.is_ok()
        descs1 = [d for k, d in enumerate(descs) if k not in gone] + added
        assert r.backend.scene_device().n_prims == len(descs1) == len(edited)
        step(tree1, descs1, "edited")

        idx = [0, len(descs1) - 2]                      # a survivor and the added sphere
        descs2 = _moved_descs(S, descs1, idx, [0.03, -0.02, 0.02])
        sh.commit(cam, 2)
        assert r.update_primitives(idx, [descs2[k] for k in idx])
        tree2 = _refit_by_desc(tree1, descs1, descs2, idx)
        step(tree2, descs2, "edited, refitted")
        sh.commit(cam, 2)
        perm = r.rebuild_tree("morton")
        tree3, new_to_old = BR.build(tree_prims(tree2))
        assert perm is not None and (perm == new_to_old).all()
        step(tree3, descs2, "edited, refitted, rebuilt")
        assert r.edit_primitives([0, 0], [], mode) is None and r.edit_primitives([len(descs2)], [], mode) is None and r.is_ok()
        assert same_device_words(r.compile_bvh(), tree3)

        r.set_primitives(descs2)                        # the same list through the host build: the history does not survive it
        r.restart_path_tracing(1, 2)
        for _ in range(2):
            r.path_tracing_pass()
        assert same_bits(r.read_preview(), r.read_denoised())
    finally:
        r.close()
