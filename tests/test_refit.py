"""Primitives of an uploaded scene moved and its tree refitted on the device (include/gpuart_refit.h, libgpuart_refit.so; Backend.refit,
Renderer.update_primitives): the device arrays afterwards are what the uploader makes of the restatement's tree (tests/refit_ref.py,
tests/converter_ref.py) byte for byte, frames and queries of the refitted context are the oracle's on that tree bit for bit, and a refused
update changes nothing."""
import ctypes as C
import functools

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import build_cases as BC
from tests import converter_ref as CR
from tests import refit_ref as RR
from tests.test_kernel_variants import _one_each, scene_setup, to_params, tree_of as variant_tree
from tests.test_ray_queries import hook_record, random_rays, rays8, tree_prims, words
from tests.util import assert_bits, assert_same_bits, pad4, same_bits, to_device

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


def _deep_chain():
    from tests.test_gpu_parity import deep_chain_scene
    return deep_chain_scene(40, -20)   # (within 2^20: a chain beyond it is disorderly and not refitted)


SCENES = {
    "one_each": (_one_each, {}),
    "box": (S.box_scene, {}),
    "scene_p": (S.scene_p, {}),
    "cones": (lambda: S.scene_p(seed=3, nspheres=0, ndiscs=0, ncones=64)[1:], {}),
    "tree": (lambda: S.tree_scene(depth=5), {}),
    "scene_d": (lambda: S.scene_d(24, 24), {}),
    "single": (lambda: _one_each()[2:3], {}),                 # the root is a leaf: no record
    "pair": (lambda: _one_each()[0:2], {}),
    "scene_p_min5": (S.scene_p, dict(min_prims=5)),           # leaves of more than two primitives
    "deep_chain": (_deep_chain, {}),                          # a level per node, beyond the LDS ring
}
SCENES.update({name: (f, {}) for name, f in BC.SHARP.items()})   # signed zeros, denormals, ties of the last bit: tests/build_cases.py says why


@functools.lru_cache(maxsize=None)
def tree_of(name):
    from oracle import oracle
    f, kw = SCENES[name]
    t = np.ascontiguousarray(oracle.build_bvh(f(), **kw)[0], np.float32)
    t.setflags(write=False)
    return t


def device_arrays(b):
    """(recs (R, 4, 4), prims (P, 3, 4)) read back from the context's device arrays through the HIP runtime."""
    hip = C.CDLL("libamdhip64.so.7")
    s = b.scene_device()
    recs, prims = np.zeros((s.n_recs, 4, 4), np.float32), np.zeros((s.n_prims, 3, 4), np.float32)
    for a, ptr in ((recs, s.recs), (prims, s.prims)):
        if a.size:
            assert hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(a.nbytes), C.c_int(2)) == 0   # hipMemcpyDeviceToHost
    return recs, prims


def assert_arrays(b, tree, what):
    """The device arrays are the restatement's of `tree`, byte for byte."""
    cv = CR.convert(tree)
    recs, prims = device_arrays(b)
    assert recs.shape == cv["recs"].shape and prims.shape == cv["prims"].shape, what
    assert (recs.view(np.uint32) == cv["recs"].view(np.uint32)).all(), "%s: records differ" % what
    assert (prims.view(np.uint32) == cv["prims"].view(np.uint32)).all(), "%s: primitives differ" % what
    s = b.scene_device()
    assert same_bits(np.array(s.root_min[:], np.float32), cv["root_min"]) and same_bits(np.array(s.root_max[:], np.float32), cv["root_max"]), what


def update_of(tree, rng, n, amount=0.2):
    prims = tree_prims(tree)
    n = min(n, len(prims))
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros((0, 16), np.float32)
    ordinals = np.sort(rng.choice(len(prims), n, replace=False)).astype(np.uint32)
    return ordinals, np.stack([RR.moved(prims[o][0], prims[o][1], rng.uniform(-amount, amount, 3)) for o in ordinals])


def refit(b, ordinals, payloads, device):
    if device:
        return b.refit(to_device(ordinals.astype(np.int32)), to_device(np.ascontiguousarray(payloads, np.float32)))
    return b.refit(ordinals, payloads)


# ---- bytes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_arrays_equal_the_restatement(be, B, name):
    """n = 0, 1, 63, 64, 65 and every primitive, one refit on top of the other, through the device-pointer and the host entry in turn:
    after each the records and primitives on the device are tests/converter_ref.convert of tests/refit_ref.refit's tree. The level
    launches are as many as the tree's records have levels."""
    tree = tree_of(name)
    be.upload_bvh(tree)
    assert_arrays(be, tree, name + " as uploaded")
    uploaded = device_arrays(be)
    n_prims = len(tree_prims(tree))
    rng = np.random.default_rng(5)
    cur = tree
    for k, n in enumerate((0, 1, 63, 64, 65, n_prims)):
        ordinals, payloads = update_of(cur, rng, n)
        out = refit(be, ordinals, payloads, device=k % 2 == 0)
        cur = RR.refit(cur, ordinals, payloads)
        assert_arrays(be, cur, "%s, n = %d" % (name, n))
        if n == 0:   # nothing moved: every byte as uploaded
            now = device_arrays(be)
            assert same_bits(now[0], uploaded[0]) and same_bits(now[1], uploaded[1]), name
        lay = CR.layout(cur)
        inner = ~lay["leaf"]
        assert out["levels"] == (int(lay["depth"][inner].max()) + 1 if inner.any() else 0)
        assert same_bits(out["root_min"], cur[0, :3]) and same_bits(out["root_max"], cur[1, :3]) and out["subnormal"] == CR.convert(cur)["subnormal"]
    assert not same_bits(device_arrays(be)[1], uploaded[1])
    if name in BC.SHARP:   # ... and the case's own update (tests/build_cases.updates), on the tree as uploaded
        be.upload_bvh(tree)
        cur = tree
        for k, (ordinals, payloads) in enumerate(BC.updates(name)):
            out = refit(be, ordinals, payloads, device=k % 2 == 0)
            cur = RR.refit(cur, ordinals, payloads)
            assert_arrays(be, cur, "%s, its own update, step %d" % (name, k))
            sub = CR.convert(cur)["subnormal"]
            assert out["subnormal"] == sub and (be.scene_device().box_slack == np.inf) == sub


@pytest.mark.parametrize("device", [False, True])
def test_moving_back_restores_the_uploaded_bytes(be, device):
    tree = tree_of("box")
    be.upload_bvh(tree)
    uploaded = device_arrays(be)
    prims = tree_prims(tree)
    ordinals, payloads = update_of(tree, np.random.default_rng(8), 7)
    refit(be, ordinals, payloads, device)
    moved = device_arrays(be)
    assert not same_bits(moved[0], uploaded[0]) and not same_bits(moved[1], uploaded[1])
    refit(be, ordinals, np.stack([prims[o][1] for o in ordinals]), device)
    back = device_arrays(be)
    assert same_bits(back[0], uploaded[0]) and same_bits(back[1], uploaded[1])


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def check_frames(B, O, b, tree, what, modes=(0, 3, 5)):
    """The direct frame, three path-tracing passes per mode, 3 000 random rays and the G-buffer of context b against the oracle on `tree`."""
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
    o0, o1 = O.traverse(tree, pad4(rs), pad4(rd), us)
    assert_same_bits(words(b.trace_rays(rays8(rs, rd), user_sphere=us)), hook_record(o0, o1)[0], what + ": trace_rays")
    crs, crd = O.cam_rays(c, W, H)
    o0, o1 = O.traverse(tree, crs.reshape(-1, 4), crd.reshape(-1, 4), us)
    hits, _ = b.gbuffer(user_sphere=us)
    assert_same_bits(words(hits), hook_record(o0, o1)[0], what + ": gbuffer")


@pytest.mark.parametrize("name", ["scene_p", "scene_d", "box"])   # round, flat, every type
def test_frames_and_queries_after_a_refit_are_the_oracles(be, B, O, name):
    tree = tree_of(name)
    be.resize(W, H)
    be.upload_bvh(tree)
    n_prims = len(tree_prims(tree))
    ordinals, payloads = update_of(tree, np.random.default_rng(21), max(2, n_prims // 3), 0.3)
    refit(be, ordinals, payloads, device=True)
    check_frames(B, O, be, RR.refit(tree, ordinals, payloads), name)


def sphere_update(tree, payload_of):
    """One update: the first sphere of the tree becomes payload_of(its data)."""
    prims = tree_prims(tree)
    k = next(i for i, (t, _) in enumerate(prims) if t == S.SPHERE)
    return np.array([k], np.uint32), np.stack([payload_of(prims[k][1].copy())])


def test_a_root_that_grows_changes_the_slack(be, B, O):
    """A sphere moved to coordinate 1000: the root box grows and the context's box_slack is the uploader's for the new tree."""
    tree = tree_of("scene_p")
    be.resize(W, H)
    be.upload_bvh(tree)
    before = be.scene_device().box_slack
    assert before == B.tree_slack(tree)[0]

    def far(d):
        d[0] = 1000.0
        return d
    ordinals, payloads = sphere_update(tree, far)
    be.refit(ordinals, payloads)
    new = RR.refit(tree, ordinals, payloads)
    slack, sub = B.tree_slack(new)
    assert not sub and np.isfinite(slack) and slack > before and be.scene_device().box_slack == slack
    check_frames(B, O, be, new, "root grown", modes=(0,))


def test_a_subnormal_plane_withdraws_the_quick_boxes(be, B, O):
    """A sphere of radius 0 at x = 1e-40: a box plane is subnormal, the slack is +inf and the frames are still the oracle's."""
    tree = tree_of("scene_p")
    be.resize(W, H)
    be.upload_bvh(tree)

    def tiny(d):
        d[0], d[3] = np.float32(1e-40), 0.0
        return d
    ordinals, payloads = sphere_update(tree, tiny)
    out = be.refit(ordinals, payloads)
    new = RR.refit(tree, ordinals, payloads)
    assert B.tree_slack(new) == (np.inf, True) and out["subnormal"] and be.scene_device().box_slack == np.inf
    assert_arrays(be, new, "subnormal plane")
    check_frames(B, O, be, new, "subnormal plane", modes=(0,))


def test_frames_under_the_nearest_first_walk(be, B, O):
    tree = tree_of("scene_d")
    be.resize(W, H)
    be.upload_bvh(tree)
    be.set_nearest_first(0)
    ordinals, payloads = update_of(tree, np.random.default_rng(31), 300, 0.3)
    be.refit(ordinals, payloads)
    assert be.scene_order() == 0
    check_frames(B, O, be, RR.refit(tree, ordinals, payloads), "nearest first", modes=(0, 3))


def test_a_pass_requested_before_a_refit_renders_the_old_scene(be, B, O):
    """pass, refit, pass, read: the accumulator is the oracle's pass on the old tree plus its pass on the new one."""
    tree = tree_of("box")
    c, P, _, _, _ = scene_setup(O, tree, W, H)
    be.resize(W, H)
    be.upload_bvh(tree)
    be.set_camera(c)
    ordinals, payloads = update_of(tree, np.random.default_rng(41), 9, 0.3)
    new = RR.refit(tree, ordinals, payloads)
    seeds = O.randseeds(2)
    be.pt_reset()
    be.pt_pass(to_params(B, P), seeds[0], 1)     # only collected: the refit must flush it first
    be.refit(ordinals, payloads)
    be.pt_pass(to_params(B, P), seeds[1], 1)
    acc = np.zeros((H, W, 4), np.float32)
    O.pt_pass(tree, c, W, H, P, seeds[0], 1, acc)
    O.pt_pass(new, c, W, H, P, seeds[1], 1, acc)
    assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "pass, refit, pass")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_updates_change_nothing(be, B, O):
    """Each refusal is ERR_ARG with a message that names the update, and leaves the arrays and the frames as they were."""
    tree = tree_of("box")
    be.resize(W, H)
    be.upload_bvh(tree)
    uploaded = device_arrays(be)
    prims = tree_prims(tree)
    sphere = next(k for k, (t, _) in enumerate(prims) if t == S.SPHERE)
    cone = next(k for k, (t, _) in enumerate(prims) if t == S.CONE)
    lo_, hi_ = sorted((sphere, cone))
    keep = lambda k: prims[k][1].copy()

    def edited(k, word, value):
        d = keep(k)
        d[word] = value
        return d
    flipped = keep(cone)
    flipped[8:11] = -flipped[8:11]
    cases = [("descending", [hi_, lo_], [keep(hi_), keep(lo_)], 1, "ascending"),
             ("repeated", [lo_, lo_], [keep(lo_), keep(lo_)], 1, "ascending"),
             ("out of range", [lo_, len(prims)], [keep(lo_), keep(lo_)], 1, "not below the number of primitives"),
             ("NaN", [sphere], [edited(sphere, 0, np.nan)], 0, "rule"),
             ("inf", [sphere], [edited(sphere, 1, np.inf)], 0, "rule"),
             ("2^21", [sphere], [edited(sphere, 2, 2.0 ** 21)], 0, "rule"),
             ("negative radius", [sphere], [edited(sphere, 3, -0.25)], 0, "rule"),
             ("cone axis against its centres", [cone], [flipped], 0, "rule")]
    for device in (False, True):
        for what, ordinals, payloads, first, word in cases:
            # a good update in front of the bad one: it must not be written either
            good = [k for k in range(len(prims)) if k < min(ordinals)][:1]
            o = np.array(good + list(ordinals), np.uint32)
            p = np.stack([RR.moved(prims[k][0], prims[k][1], (0.1, 0.0, 0.0)) for k in good] + list(payloads))
            with pytest.raises(B.HipError) as e:
                refit(be, o, p, device)
            assert e.value.code == ERR_ARG and e.value.first_bad == first + len(good), (what, str(e.value))
            assert "update %d" % (first + len(good)) in str(e.value) and word in str(e.value), (what, str(e.value))
            now = device_arrays(be)
            assert same_bits(now[0], uploaded[0]) and same_bits(now[1], uploaded[1]), what
    with pytest.raises(B.HipError, match="more updates"):
        be.refit(np.arange(len(prims) + 1), np.zeros((len(prims) + 1, 16), np.float32))
    with pytest.raises(ValueError):
        be.refit([0], np.zeros(15, np.float32))
    check_frames(B, O, be, tree, "after the refusals", modes=(0,))


@pytest.mark.parametrize("name", ["wild", "disorderly", "empty"])
def test_trees_with_exact_boxes_are_not_refitted(be, B, name):
    tree = variant_tree(name)
    be.upload_bvh(tree)
    uploaded = device_arrays(be)
    assert be.scene_device().exact_boxes == 1
    with pytest.raises(B.HipError, match="irregular") as e:
        be.refit([], [])
    assert e.value.code == ERR_ARG
    zero = (0.0, 0.0, 0.0)
    with pytest.raises(B.HipError, match="irregular") as e:
        be.scene_refitted(zero, zero, False)
    assert e.value.code == ERR_ARG
    now = device_arrays(be)
    assert same_bits(now[0], uploaded[0]) and same_bits(now[1], uploaded[1])


def test_a_handle_bound_before_another_upload_is_stale(be, B):
    """The scene's generation grows with every upload; a run on a handle bound to an earlier one is ERR_ARG."""
    R = B.refit_lib()
    tree = tree_of("box")
    be.upload_bvh(tree)
    be.refit([], [])
    first = be.scene_device().generation
    be.upload_bvh(tree)
    scene = be.scene_device()
    assert scene.generation == first + 1
    uploaded = device_arrays(be)
    res = B.RefitResult()
    assert R.gpuart_refit_run_host(be._refit, C.byref(scene), None, None, C.c_size_t(0), C.byref(res)) == ERR_ARG
    assert b"bound to another upload" in R.gpuart_refit_last_error()
    now = device_arrays(be)
    assert same_bits(now[0], uploaded[0]) and same_bits(now[1], uploaded[1])
    be.refit([], [])   # Backend.refit binds again
    with pytest.raises(B.HipError, match="the root box"):
        be.scene_refitted((1.0, 0.0, 0.0), (0.0, 1.0, 1.0), False)
    bare = B.Backend(0)
    try:
        with pytest.raises(B.HipError, match="no scene"):
            bare.scene_device()
    finally:
        bare.close()


# ---- Renderer ---------------------------------------------------------------------------------------------------------------------
def test_update_primitives_keeps_the_history(B, O):
    """With the temporal history on, update_primitives commits the view it leaves: read_preview afterwards is the restatement chain
    (tests/temporal_ref.py, tests/denoise_ref.py) fed with frames that are the oracle's on the refitted tree — the accumulator and the
    pick of every pixel are compared with the oracle first —, trace_rays' ordinals still index the caller's descriptions, and a refused
    update leaves everything as it was."""
    from tests.test_temporal import SPHERE, TRACK, Shadow, cam_dict, tile_xy
    RW, RH = 48, 32
    cam = cam_dict(TRACK[0])
    descs = S.box_scene()
    tree0, _ = O.build_bvh(descs)
    r = B.Renderer(RW, RH, cam)
    try:
        r.set_primitives(descs)
        r.set_user_sphere(SPHERE[:3], SPHERE[3])
        r.set_temporal_history(True)
        sh = Shadow(B, r, SPHERE, 0)
        r.restart_path_tracing(1, 3)
        for _ in range(3):
            r.path_tracing_pass()
        assert_same_bits(r.read_preview(), r.read_denoised(), "no history yet")
        # the descriptions to move, in the caller's numbering and NOT ascending in the tree's order
        idx = [k for k, d in enumerate(descs) if d[0] in (S.SPHERE, S.TRIANGLE, S.CONE)][:6][::-1]
        new_descs = list(descs)
        for k in idx:
            t, f = descs[k]
            f = np.asarray(f, np.float32).copy()
            for a in {S.SPHERE: (0,), S.TRIANGLE: (0, 3, 6), S.CONE: (0, 3)}[t]:
                f[a:a + 3] += np.float32([0.05, -0.03, 0.04])
            new_descs[k] = (t, [float(v) for v in f])
        # refusals first: nothing changes
        acc = r.read_radiance(False)
        assert not r.update_primitives([idx[0], idx[0]], [new_descs[idx[0]]] * 2)
        assert not r.update_primitives([len(descs)], [new_descs[idx[0]]])
        assert not r.update_primitives([idx[0]], [(S.DISC, [0, 0, 0, 0, 0, 1, 1])])
        sph = next(k for k, d in enumerate(descs) if d[0] == S.SPHERE)
        assert not r.update_primitives([sph], [(S.SPHERE, [0.0, 0.0, 0.0, -1.0])])
        assert not r.update_primitives([sph], [(S.SPHERE, [float(2 ** 21), 0.0, 0.0, 1.0])])
        assert same_bits(r.read_radiance(False), acc) and r.is_ok()
        sh.commit(cam, 3)
        assert r.update_primitives(idx, [new_descs[k] for k in idx])
        # the refitted tree in the restatement: the same updates by the tree's own ordinals
        order = {id_: o for o, id_ in enumerate(_ordinal_to_desc(tree0, descs))}
        pairs = sorted((order[k], k) for k in idx)
        new_tree = RR.refit(tree0, [o for o, _ in pairs], np.stack([RR.payload_of(new_descs[k]) for _, k in pairs]))
        c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], RW, RH)
        sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
        P = O.make_params(sun, S.SUN_ALTITUDE, True, SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
        seeds = O.randseeds(5)
        exp = np.zeros((RH, RW, 4), np.float32)
        for k in range(2):
            r.path_tracing_pass()
            O.pt_pass(new_tree, c, RW, RH, P, seeds[3 + k], 1, exp)
        assert_bits(r.read_radiance(False)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "passes after the update")
        crs, crd = O.cam_rays(c, RW, RH)
        o0, o1 = O.traverse(new_tree, crs.reshape(-1, 4), crd.reshape(-1, 4), SPHERE)
        hits, prims = r.pick(tile_xy(r), want_prims=True)
        assert_same_bits(words(hits), hook_record(o0, o1)[0], "pick after the update")
        got = r.read_preview()
        assert_same_bits(got, sh.preview(cam, 2), "preview after the update")
        assert not same_bits(got, r.read_denoised())   # the history is there
        # ordinals still index the caller's descriptions: the oracle's intersection of each pixel's ray with the description its ordinal
        # names, as it is now, is the pixel's hit
        flat, w = prims.reshape(-1), words(hits)
        crs, crd = crs.reshape(-1, 4), crd.reshape(-1, 4)
        for k in np.unique(flat[flat >= 0]):
            sel = np.nonzero(flat == k)[0]
            t, q = new_descs[k][0], np.tile(RR.payload_of(new_descs[k]).reshape(1, 4, 4), (len(sel), 1, 1))
            rs, rd = crs[sel], crd[sel]
            o0, o1 = (O.sphere(rs, rd, q[:, 0]) if t == S.SPHERE else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == S.DISC else
                      O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == S.TRIANGLE else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
            assert_same_bits(w[sel, :7], np.concatenate([o0, o1[:, :3]], 1), "description %d" % k)
    finally:
        r.close()


def _ordinal_to_desc(tree, descs):
    """Per device ordinal of `tree` the index of its description (the box scene's primitives are all different)."""
    keys = {}
    for k, d in enumerate(descs):
        keys[(d[0], RR.payload_of(d).tobytes())] = k
    return [keys[(t, d.tobytes())] for t, d in tree_prims(tree)]
