"""GPU parity tests (run with `-m gpu` on an MI355X): the HIP path, called through the C ABI of
include/gpuart_hip.h, against (a) the committed golden vectors of the reference GLSL on llvmpipe and
(b) the oracle on fresh seeded inputs.

Tolerance: north_star states per-channel RMSE < 1e-4 for frames. The tests below assert the much
stronger property that actually holds — float32 results identical bit for bit (0 differing pixels) —
and additionally check the stated RMSE bound so that a future relaxation stays visible.
"""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.util import fuzz_case_setup, row_checksums, GOLDEN, assert_bits, bit_mismatch, frame_golden_params, golden, pad4, rmse_per_channel, scene

pytestmark = pytest.mark.gpu

RMSE_TOL = 1e-4  # north_star: per-channel RMSE < 1e-4 vs the reference render


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def to_params(B, op):
    """oracle Params -> gpuart_params (same field layout)."""
    p = B.Params()
    C.memmove(C.byref(p), C.byref(op), C.sizeof(p))
    return p


def test_native_library_is_the_one_running(B):
    import subprocess
    maps = open("/proc/self/maps").read()
    B.hip_lib()
    maps = open("/proc/self/maps").read()
    assert "libgpuart_hip.so" in maps


def test_the_product_library_runs_the_smoke_frame():
    """The suite runs on gpuart_amd/lib_test (the product's sources + the test hooks, tests/conftest.py). The PRODUCT pair, gpuart_amd/lib —
    no hook compiled in — is what this child loads (GPUART_LIBDIR removed): __graft_entry__.smoke(), direct lighting + two path-tracing
    passes of the box scene through the C++ Renderer against the oracle, bit for bit; and it really is that library that ran."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "GPUART_LIBDIR"}
    code = ("import sys; sys.path.insert(0, %r)\nimport __graft_entry__ as g\ng.smoke()\n"
            "maps = open('/proc/self/maps').read()\n"
            "assert '/gpuart_amd/lib/libgpuart_hip.so' in maps and '/gpuart_amd/lib/libgpuart.so' in maps and 'lib_test' not in maps, 'wrong library'\n"
            "from gpuart_amd import binding as B\n"
            "try:\n    B.hip_lib().gpuart_hip_test_planner\n    raise SystemExit('the product library has a test hook')\n"
            "except AttributeError as e:\n    assert 'lib_test' in str(e)\nprint('product library ok')\n" % root)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "smoke OK" in p.stdout and "product library ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


# ---- per-function hooks vs golden vectors ---------------------------------------------------------
def test_hash_random(be):
    g = golden("hash")
    assert_bits(be.test_random(g["x"]), g["out"], "random")


def test_sin_cos_pow_sqrt(be):
    g = golden("llvmpipe_math")
    x = np.zeros((len(g["x"]), 4), np.float32)
    x[:, :2] = g["x"]
    assert_bits(be.test_math(x), g["out"], "sin/cos/pow16/sqrt")


def test_samplers(be):
    g = golden("hemisphere")
    assert_bits(be.test_hemisphere(pad4(g["v"]), pad4(g["ri"]))[:, :3], g["out"], "hemisphere sampler")
    g = golden("inside_cone")
    ha = np.float32(10) * np.float32(3.14159) / np.float32(180)
    assert_bits(be.test_inside_cone(pad4(g["v"]), pad4(g["normal"]), pad4(g["ri"]), float(ha))[:, :3], g["out"],
                "cone sampler")


def _payload(n, *quads):
    q = np.zeros((n, 16), np.float32)
    for k, a in enumerate(quads):
        q[:, 4 * k:4 * k + 4] = pad4(a)
    return q


def test_intersectors(be):
    g = golden("sphere")
    o = be.test_intersect(S.SPHERE, pad4(g["rs"]), pad4(g["rd"]), _payload(len(g["rs"]), g["sph"]))
    exp0 = g["o0"].copy(); exp1 = g["o1"].copy()
    m = exp0[:, 0] < 1e-4  # prim_hit applies the reference's visibility cut (bvh_intersection.glsl:170)
    exp0[m] = [-1, 0, 0, 0]; exp1[m] = 0
    got0 = o[0].copy(); got0[got0[:, 0] < 0, 0] = -1
    assert_bits(np.concatenate([got0, o[1]], 1), np.concatenate([exp0, exp1], 1), "sphere")

    g = golden("disc")
    dq = _payload(len(g["rs"]), g["cr"], g["dn"])
    o = be.test_intersect(S.DISC, pad4(g["rs"]), pad4(g["rd"]), dq)
    exp0 = g["o0"].copy(); exp1 = g["o1"].copy()
    m = exp0[:, 0] < 1e-4
    exp0[m] = [-1, 0, 0, 0]; exp1[m] = 0
    assert_bits(np.concatenate(o, 1), np.concatenate([exp0, exp1], 1), "disc")

    g = golden("triangle")
    o = be.test_intersect(S.TRIANGLE, pad4(g["rs"]), pad4(g["rd"]), _payload(len(g["rs"]), g["v0"], g["v1"], g["v2"]))
    exp0 = g["o0"].copy(); exp1 = g["o1"].copy()
    m = exp0[:, 0] < 1e-4
    exp0[m] = [-1, 0, 0, 0]; exp1[m] = 0
    assert_bits(np.concatenate(o, 1), np.concatenate([exp0, exp1], 1), "triangle")

    g = golden("cone")
    o = be.test_intersect(S.CONE, pad4(g["rs"]), pad4(g["rd"]), g["quads"])
    assert_bits(np.concatenate(o, 1), np.concatenate([g["o0"], g["o1"]], 1), "cone")


def test_intersectors_on_hostile_numbers(be):
    """The device intersectors (through the uploader's re-layout of the canonical payload) with NaN / +-inf / +-1e30 / denormals /
    negative radii / the reference's magic numbers in the primitive and in the ray, against the reference's GLSL on llvmpipe
    (tests/golden/*_wild.npz, make_golden.py intersect_wild; the probe applies CheckBVHPrimitiveIntersection's visibility cut)."""
    def check(name, ptype, g, quads):
        o = be.test_intersect(ptype, pad4(g["rs"]), pad4(g["rd"]), quads)
        got, exp = np.concatenate(o, 1), np.concatenate([g["o0"], g["o1"]], 1)
        same = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        bad = ~same.all(1)
        assert not bad.any(), "%s: %d of %d rows differ; first: row %d got %s expected %s" % (name, int(bad.sum()), len(bad),
                                                                                             int(np.nonzero(bad)[0][0]), got[bad][0], exp[bad][0])
    g = golden("sphere_wild"); check("sphere", S.SPHERE, g, _payload(len(g["rs"]), g["sph"]))
    g = golden("disc_wild"); check("disc", S.DISC, g, _payload(len(g["rs"]), g["cr"], g["dn"]))
    g = golden("triangle_wild"); check("triangle", S.TRIANGLE, g, _payload(len(g["rs"]), g["v0"], g["v1"], g["v2"]))
    g = golden("cone_wild"); check("cone", S.CONE, g, g["quads"])


def test_shading_functions_on_hostile_numbers(be):
    """random(), the two direction samplers and the sky on NaN / infinite / huge / denormal inputs (what a path carries after
    bouncing off a wild primitive), against the reference's GLSL on llvmpipe (tests/golden/*_wild.npz, make_golden.py shade_wild):
    Mesa's NaN-unsafe foldings (all(lessThan()) as !any(>=), constant-0 components folded out of products) and gallivm's pow() on
    NaN / inf / overflowing bases are part of what the reference computes."""
    def nanbits(got, exp, what):
        got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
        same = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        bad = ~same.reshape(len(got), -1).all(1)
        assert not bad.any(), "%s: %d of %d rows differ; first: row %d got %s expected %s" % (what, int(bad.sum()), len(bad),
                                                                                             int(np.nonzero(bad)[0][0]), got[bad][0], exp[bad][0])
    g = golden("hash_wild")
    nanbits(be.test_random(g["x"]), g["out"], "random")
    g = golden("hemisphere_wild")
    nanbits(be.test_hemisphere(pad4(g["v"]), pad4(g["ri"]))[:, :3], g["out"], "hemisphere sampler")
    g = golden("inside_cone_wild")
    ha = np.float32(10) * np.float32(3.14159) / np.float32(180)
    nanbits(be.test_inside_cone(pad4(g["v"]), pad4(g["normal"]), pad4(g["ri"]), float(ha))[:, :3], g["out"], "cone sampler")
    g = golden("sky_wild")
    nanbits(be.test_sky(pad4(g["dir"]), g["sun_dir_alt"])[:, :3], g["out"], "sky")


def test_aabb(be):
    g = golden("aabb")
    assert_bits(be.test_aabb(pad4(g["rs"]), pad4(g["rd"]), pad4(g["bmin"]), pad4(g["bmax"]))[:, :2], g["out"], "AABB")


def test_aabb_irregular_boxes(be):
    """The box test on irregular boxes (inverted / NaN / infinite axis; what wild primitives make of a node box) against the
    reference's IntersectsAABB on llvmpipe. The fast med3 form is wrong for these — the reference can hit a box through the
    planes of its one irregular axis —, so a tree that holds one runs the comparison form (Scene::exact_boxes); the hook
    decides per box as the uploader does per tree."""
    g = golden("aabb_irregular")
    assert_bits(be.test_aabb(pad4(g["rs"]), pad4(g["rd"]), pad4(g["bmin"]), pad4(g["bmax"]))[:, :2], g["out"], "AABB, irregular boxes")


def test_quick_box_answers_equal_the_six_face_tests(B, monkeypatch):
    """csrc/hip/box_quick.h answers a box from its six plane parameters alone where that is provably the reference's result and is
    withdrawn elsewhere. Two contexts — quick answers on (the default) and off (GPUART_HIP_QUICK_BOXES=0: every box through
    IntersectsAABB's six face tests) — must agree on every ray of a set made to hurt: rays aimed at corners, edges and faces of the
    box and a few ulps beside them, origins on box planes, flat boxes, dyadic coordinates (exact ties), tiny and zero direction
    components, NaN / inf / huge numbers. (The CPU soak of the same source: tests/test_quick_box.py.)"""
    rng = np.random.default_rng(20260404)
    n = 1 << 20
    f32 = np.float32
    scale = rng.choice(np.array([1, 1, 5, 0.01, 100, 1e4], f32), (n, 1))
    dy = rng.random((n, 1)) < 0.25
    centre = np.where(dy, rng.integers(-16, 17, (n, 3)) * 0.125, rng.uniform(-1, 1, (n, 3))).astype(f32) * scale
    ext = np.where(dy, rng.integers(0, 9, (n, 3)) * 0.125, rng.uniform(0, 1, (n, 3)) * rng.choice(np.array([0, 1e-6, 1e-3, 0.05, 1], f32), (n, 3))).astype(f32) * scale
    lo, hi = (centre - ext).astype(f32), (centre + ext).astype(f32)
    on = rng.integers(0, 4, (n, 3))  # target: on the lower plane, on the upper plane, between them, anywhere near
    u = rng.random((n, 3)).astype(f32)
    tgt = np.where(on == 0, lo, np.where(on == 1, hi, np.where(on == 2, lo + (hi - lo) * u, lo + (hi - lo) * (3 * u - 1)))).astype(f32)
    nudge = rng.integers(-3, 4, (n, 3)) * (rng.random((n, 3)) < 0.3)
    tgt = (tgt.view(np.int32) + nudge.astype(np.int32)).view(f32)
    org = np.where(dy, rng.integers(-16, 17, (n, 3)) * 0.125 * scale, tgt + scale * rng.choice(np.array([1e-3, 0.1, 3, 50], f32), (n, 1)) * rng.uniform(-1, 1, (n, 3))).astype(f32)
    plane = rng.random((n, 3)) < 0.05
    org = np.where(plane, np.where(rng.random((n, 3)) < 0.5, lo, hi), org).astype(f32)
    d = (tgt - org).astype(f32)
    with np.errstate(all="ignore"):
        d = np.where(dy, d, d / np.maximum(np.linalg.norm(d, axis=1, keepdims=True), f32(1e-30))).astype(f32)
    small = rng.random((n, 3)) < 0.05
    d = np.where(small, rng.choice(np.array([0.0, -0.0, 6.2e-8, -1e-12, 1e-30], f32), (n, 3)), d).astype(f32)
    hostile = rng.random((n, 3)) < 0.01
    special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e38, 1e-39, 2e6], f32)
    org = np.where(hostile, rng.choice(special, (n, 3)), org).astype(f32)
    d = np.where(np.roll(hostile, 1, axis=0), rng.choice(special, (n, 3)), d).astype(f32)
    out = []
    for quick in ("1", "0"):
        monkeypatch.setenv("GPUART_HIP_QUICK_BOXES", quick)
        b = B.Backend(0)
        try:
            out.append(b.test_aabb(pad4(org), pad4(d), pad4(lo), pad4(hi))[:, :2].copy())
        finally:
            b.close()
    q, f = out
    assert np.array_equal(q[:, 0], f[:, 0]), "hit / miss differs at %s" % np.flatnonzero(q[:, 0] != f[:, 0])[:8]
    assert np.array_equal(q[:, 1], f[:, 1]), "entry parameter differs at %s" % np.flatnonzero(q[:, 1] != f[:, 1])[:8]  # (+0 == -0)
    assert 0.2 < float(f[:, 0].mean()) < 0.9


def test_wild_scene_with_a_box_hit_through_its_irregular_axis():
    """Wild case 42874 of tests/fuzz_parity.py (found by the round-2 soak; 1 of 14 500 cases): a disc with radius -inf leaves
    its leaf with the box x, z in [-inf, inf], y in [9.9e30, -9.9e30]; the reference enters it through the y planes (entry
    clamped to 1e19) and hits the infinite disc. All three pipelines must agree with the oracle (== reference GLSL here:
    tests/golden/soak_oracle_vs_reference.py --wild 42874 1)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_parity.py"), "--wild", "42874", "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "1 scenes, 0 with differences" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]



@pytest.mark.parametrize("k", [0, 1, 2])
def test_sky(be, k):
    g = golden("sky_%d" % k)
    assert_bits(be.test_sky(pad4(g["dir"]), g["sun_dir_alt"])[:, :3], g["out"], "sky")


@pytest.mark.parametrize("name", ["camrays_64x36", "camrays_37x23"])
def test_camera_rays(be, name):
    g = golden(name)
    H, W = g["rstart"].shape[:2]
    be.resize(W, H)
    be.set_camera(g["cam"])
    rs, rd = be.test_cam_rays()
    assert_bits(rs[..., :3].reshape(-1, 3), g["rstart"].reshape(-1, 3), "rstart")
    assert_bits(rd[..., :3].reshape(-1, 3), g["rdir"].reshape(-1, 3), "rdir")


def test_camera_rays_large_frames_and_tiles(be, O):
    """UV interpolation at BASELINE sizes (1080p, 4K, 8K): tile of the device frame == oracle."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    for W, H, tile in [(1920, 1080, (900, 500, 128, 64)), (3840, 2160, (3700, 2100, 140, 60)), (7680, 4320, (3800, 2140, 96, 48))]:
        c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
        be.resize(W, H)
        be.set_tile(*tile)
        be.set_camera(c)
        rs, rd = be.test_cam_rays()
        x0, y0, tw, th = tile
        xy = np.stack(np.meshgrid(np.arange(x0, x0 + tw), np.arange(y0, y0 + th)), -1).reshape(-1, 2)
        uv = O.pixel_uv(xy, W, H)
        u, v = uv[:, 0:1], uv[:, 1:2]
        exp = (c[3:6][None, :] + c[6:9][None, :] * u) + c[9:12][None, :] * v
        assert_bits(rs[..., :3].reshape(-1, 3), exp.astype(np.float32), "rstart %dx%d" % (W, H))


# ---- traversal --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box", "scene_pc", "scene_d"])
def test_traversal(be, O, name):
    g = golden("traverse_" + name)
    tree, _ = O.build_bvh(scene(name))
    be.upload_bvh(tree)
    for rs, rd, e0, e1 in [(g["rs"], g["rd"], g["o0"], g["o1"]), (g["rs2"], g["rd2"], g["s0"], g["s1"])]:
        o0, o1 = be.test_traverse(pad4(rs), pad4(rd), S.USER_SPHERE)
        assert_bits(np.concatenate([o0, o1], 1), np.concatenate([e0, e1], 1), "closest hit " + name)
        # the order of the fast kernels (nearer child first, lower primitive index wins equal parameters) returns the same
        o0, o1 = be.test_traverse(pad4(rs), pad4(rd), S.USER_SPHERE, nearest_first=True)
        assert_bits(np.concatenate([o0, o1], 1), np.concatenate([e0, e1], 1), "closest hit, nearer child first, " + name)
        a0, _ = be.test_traverse(pad4(rs), pad4(rd), S.USER_SPHERE, any_hit=True)
        # first-hit traversal finds a hit exactly where the closest-hit query does (user sphere aside)
        bvh_hit = (e1[:, 3] >= 0) & (e1[:, 3] != 0.5)
        assert ((a0[:, 0] > 0) == bvh_hit).all()


@pytest.mark.parametrize("name", ["scene_pc", "wild_42874", "wild_7", "wild2_5", "pc_min5", "pc_levels4", "p_root_leaf", "soup_levels6"])
def test_traversal_with_hostile_rays_and_trees(be, name):
    """The device traversal (closest hit incl. the user sphere, radius 0.25) with hostile rays on a regular tree and with regular +
    hostile rays on the trees of wild scenes (irregular boxes -> the exact box test; a 200-level chain -> the spilled stack),
    and on trees with other leaf sizes than the default build's (the counting leaf loop), against the reference's
    CheckIntersectionInclUserSphere on llvmpipe (make_golden.py traverse_wild / traverse_leaves; the tree is in the fixture)."""
    g = golden("traverse_wild_" + name)
    be.upload_bvh(g["tree"])
    # the reference's order, and — trees of regular boxes — the fast kernels' (nearer child first)
    from gpuart_amd.binding import HipError
    for nearest in [False, True]:
        try:
            o0, o1 = be.test_traverse(pad4(g["rs"]), pad4(g["rd"]), (-0.4, 0.0, 0.2, 0.25), nearest_first=nearest)
        except HipError as e:  # a tree with irregular boxes has no nearest-first walk: the library says so
            assert nearest and "irregular boxes" in str(e) and name.startswith("wild"), str(e)
            continue
        got, exp = np.concatenate([o0, o1], 1), np.concatenate([g["o0"], g["o1"]], 1)
        same = (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))
        bad = ~same.all(1)
        assert not bad.any(), "%s%d of %d rays differ; first: ray %d o %s d %s got %s expected %s" % (
            "nearer child first: " if nearest else "", int(bad.sum()), len(bad), int(np.nonzero(bad)[0][0]), g["rs"][bad][0], g["rd"][bad][0], got[bad][0], exp[bad][0])


def deep_chain_scene(n=40, k0=0):
    """Spheres at x = 2^k: every split peels one sphere off -> tree depth n-1 > LDS stack depth."""
    return [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(k0, k0 + n)]


@pytest.mark.parametrize("k0", [0, -20])
def test_deep_tree_spills_the_ring_stack(be, O, B, k0):
    """k0 = 0: coordinates up to 5e11 — beyond what the uploader lets the fast kernels walk in their own order (converter.h), so
    the nearest-first hook is refused; k0 = -20: the same chain within 2^20, walked in both orders."""
    prims = deep_chain_scene(40, k0)
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    be.upload_bvh(tree)
    assert be.scene_info()["max_depth"] == depth
    rng = np.random.RandomState(5)
    n = 2048
    sc = 2.0 ** k0
    rs = np.zeros((n, 4), np.float32); rs[:, 0] = -3 * sc; rs[:, 1:3] = rng.uniform(-1, 1, (n, 2)) * sc
    tgt = np.zeros((n, 3)); k = rng.randint(0, 40, n) + k0; tgt[:, 0] = 2.0 ** k; tgt[:, 1:] = rng.normal(size=(n, 2)) * (2.0 ** (k - 2))[:, None]
    rd = np.zeros((n, 4), np.float32); rd[:, :3] = tgt - rs[:, :3]
    e0, e1 = O.traverse(tree, rs, rd, S.USER_SPHERE)
    o0, o1 = be.test_traverse(rs, rd, S.USER_SPHERE)
    assert (e1[:, 3] >= 0).mean() > 0.3
    assert_bits(np.concatenate([o0, o1], 1), np.concatenate([e0, e1], 1), "closest hit through the spill path")
    if k0 == 0:
        with pytest.raises(B.HipError, match="do not bound their contents"):
            be.test_traverse(rs, rd, S.USER_SPHERE, nearest_first=True)
    else:
        o0, o1 = be.test_traverse(rs, rd, S.USER_SPHERE, nearest_first=True)
        assert_bits(np.concatenate([o0, o1], 1), np.concatenate([e0, e1], 1), "closest hit through the spill path, nearer child first")


def test_every_tree_keeps_the_reference_order_by_default_and_nearest_first_is_opt_in(B, O, monkeypatch):
    """The library's own choice since round 5: every tree of regular boxes is walked in the reference's order by kernel variants without
    the certificate's bookkeeping (scene_order 1), an irregular one with exact box tests (2). The nearer-child-first walk of round 4
    (scene_order 0) is opt-in — GPUART_HIP_NEAREST_MIN_PRIMS at context creation, or gpuart_hip_set_nearest_first on a live context,
    which re-decides for the scene already uploaded — and the frames of the golden scenes are the reference's bits either way."""
    monkeypatch.delenv("GPUART_HIP_NEAREST_MIN_PRIMS", raising=False)
    b = B.Backend(0)
    try:
        for opt_in, names in ((None, ("frames_box_seg5", "frames_scene_p_seg4", "frames_scene_pc_seg5", "frames_tree_seg5", "frames_scene_d_seg5")),
                              (1024, ("frames_box_seg5", "frames_tree_seg5", "frames_scene_d_seg5")), (0, ("frames_box_seg5", "frames_scene_pc_seg5"))):
            for name in names:
                g = golden(name)
                W, H = int(g["W"]), int(g["H"])
                descs = scene(str(g["scene"]))
                tree, _ = O.build_bvh(descs)
                b.resize(W, H); b.upload_bvh(tree); b.set_camera(g["cam"])
                if opt_in is not None:
                    b.set_nearest_first(opt_in)          # after the upload: the choice is re-made for the scene in place
                assert b.scene_order() == (1 if opt_in is None or len(descs) < opt_in else 0), (name, opt_in)
                mk = frame_golden_params(O, g)
                for mode in (0, 3, 5):
                    b.set_mode(mode)
                    b.render_direct(to_params(B, mk()))
                    assert_bits(b.read(0)[..., :3].reshape(-1, 3), g["direct"].reshape(-1, 3), "%s direct, mode %d, opt-in %s" % (name, mode, opt_in))
                    b.pt_reset()
                    b.pt_pass(to_params(B, mk()), g["seeds"][0], 1)
                    assert_bits(b.read(1)[..., :3].reshape(-1, 3), g["pt_pass1"].reshape(-1, 3), "%s first pass, mode %d, opt-in %s" % (name, mode, opt_in))
            b.set_nearest_first(0xffffffff)
        b.set_mode(0)
        b.upload_bvh(O.build_bvh([(S.SPHERE, [0, 0, 1, -0.5])])[0])
        assert b.scene_order() == 2
    finally:
        b.close()
    monkeypatch.setenv("GPUART_HIP_NEAREST_MIN_PRIMS", "0")
    b = B.Backend(0)
    try:
        b.upload_bvh(O.build_bvh(scene("box"))[0])
        assert b.scene_order() == 0
    finally:
        b.close()


def test_phantom_hits_are_why_nearest_first_is_opt_in(be, B, O):
    """tests/golden/order_adversary.npz (make_golden.py order_adversary): 16 scenes of four primitives and one ray each. The ray grazes a
    triangle by ~1e-6 rad; the reference's Moeller-Trumbore (shaders/triangle.glsl:50-76) divides two cancelled sums and accepts a
    PHANTOM hit — a small dyadic parameter far in front of the triangle's own box —; a disc stands between the phantom and the box.
    Expected values: the reference's own GLSL on llvmpipe (it returns the phantom: its walk reaches the triangle's leaf first, with
    nothing closer). The product's walks — reference order: the test hook, the renderer's default kernels — must return exactly that.
    The opt-in nearest-first walk sees the disc first, prunes the triangle's leaf (entered beyond the disc by far more than its band)
    and never tests the triangle: its certificate, computed from what it did test, cannot notice. That is asserted too — if it ever
    stops being true the walk has become sound and can be the default again."""
    g = golden("order_adversary")
    n = int(g["n"])
    assert n >= 16
    differing = 0
    for i in range(n):
        tree = g["tree%d" % i]
        be.upload_bvh(tree)
        rs, rd = pad4(g["rs%d" % i][None]), pad4(g["rd%d" % i][None])
        exp = np.concatenate([g["o0_%d" % i], g["o1_%d" % i]])[None]
        assert exp[0, 7] == 2.0  # the reference's winner is the triangle ...
        o0, o1 = be.test_traverse(rs[:, :3], rd[:, :3], (0, 0, 0, 0))
        assert_bits(np.concatenate([o0, o1], 1), exp, "adversary %d, reference order" % i)
        n0, n1 = be.test_traverse(rs[:, :3], rd[:, :3], (0, 0, 0, 0), nearest_first=True)
        if n0[0, 0] != exp[0, 0]:
            differing += 1
            assert n1[0, 3] == 1.0 and n0[0, 0] == g["nf%d" % i]   # ... the nearest-first walk's is the disc in front, as the model of make_golden.py predicted
    assert differing == n, "the nearest-first walk now agrees with the reference on %d of %d phantom hits: re-examine why it is opt-in" % (n - differing, n)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_phantom_hits_in_whole_frames(B, O, k):
    """tests/golden/order_adversary_frame_k.npz: the phantom hit through the PRODUCT's render kernels. One pixel's first-segment ray grazes a
    triangle; the reference's own path-tracing program (the fixture) shows the triangle's phantom in that pixel, in front of the disc that
    stands before the triangle. The default walks — launch pipeline, k_run, megakernel: modes 0 / 3 / 5 / 2 — must render the reference's
    frames bit for bit; with the nearest-first walk opted in the pixel shows something else (and only the reference-order megakernel,
    mode 2, still shows the reference's) — which is why it is opt-in."""
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam, tree, seeds = g["cam"], g["tree"], g["seeds"]
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(cam[12]), cam[0:3], int(g["max_segments"]), 0.01)
    px, py = (int(v) for v in g["pixel"])
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(cam)
        b.set_nearest_first(0xffffffff)            # the product's default, whatever the suite's environment says
        assert b.scene_order() == 1
        for mode in (0, 3, 5, 2):
            b.set_mode(mode)
            b.pt_reset()
            b.pt_pass(to_params(B, P), seeds[0], 1)
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), g["pt_pass1"].reshape(-1, 3), "adversary frame %d, first pass, mode %d" % (k, mode))
            b.pt_pass(to_params(B, P), seeds[1], 1)
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), g["pt_acc"].reshape(-1, 3), "adversary frame %d, two passes, mode %d" % (k, mode))
        b.set_nearest_first(0)                     # opt in, on this small tree too
        assert b.scene_order() == 0
        for mode in (0, 3, 5):
            b.set_mode(mode)
            b.pt_reset()
            b.pt_pass(to_params(B, P), seeds[0], 1)
            got = b.read(1)[..., :3]
            assert (got[py, px].view(np.uint32) != g["pt_pass1"][py, px].view(np.uint32)).any(), "mode %d: the opt-in walk shows the phantom too?" % mode
            others = np.ones((H, W), bool); others[py, px] = False
            assert_bits(got[others], g["pt_pass1"][others], "adversary frame %d, opt-in walk, every OTHER pixel, mode %d" % (k, mode))
        b.set_mode(0)
    finally:
        b.close()


def test_rays_on_which_visiting_order_decides(be, O):
    """Four rays found by tools/order_rays.py among 1.7e9 (tests/golden/order_rays.npz): each meets a box whose entry parameter, as
    the reference computes it, is NOT its slab entry — the face the ray enters through fails its own test by rounding at an
    edge, and the running minimum falls on the face the ray leaves through. Such a box claims to be entered beyond hits that
    lie inside it, and what the reference finds there depends on when its walk arrives. A nearest-first walk without the
    certificate (device_scene.h: odd boxes) returned a hit 0.04 % to 3 % further away on each of them. Expected values: the
    reference's own GLSL on llvmpipe."""
    g = golden("order_rays")
    for name, descs in (("cfg3", S.scene_d()), ("tree", S.tree_scene())):
        tree, _ = O.build_bvh(descs)
        be.upload_bvh(tree)
        rs, rd = g[name + "_rs"], g[name + "_rd"]
        e0, e1 = g[name + "_o0"], g[name + "_o1"]  # the reference's GLSL on llvmpipe (make_golden.py order_rays)
        assert (e1[:, 3] >= 0).all()
        for nearest in (False, True):
            o0, o1 = be.test_traverse(rs, rd, (0, 0, 0, 0), nearest_first=nearest)
            assert_bits(np.concatenate([o0, o1], 1), np.concatenate([e0, e1], 1), "%s rays, nearest first %s" % (name, nearest))


@pytest.mark.parametrize("flavour,seed", [("--wild", 100138), ("--wild2", 101453), ("--wild2", 100145), ("--wild2", 101115)])
def test_hostile_scenes_that_keep_the_reference_order(flavour, seed):
    """Scenes of the hostile classes whose boxes are regular but do not bound what they hold in any useful sense — a triangle
    with a vertex at -1e30 or +-1e19 (the intersector's `origin - v0` swallows the origin: its hit parameter is off by whole
    units), negative radii — rendered wrongly by a nearest-first walk: the uploader finds them (converter.h prim_in_box)
    and such a tree is walked in the reference's order throughout."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_parity.py"), flavour, str(seed), "1"], capture_output=True, text=True)
    assert r.returncode == 0 and "1 scenes, 0 with differences" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# ---- frames -----------------------------------------------------------------------------------------
FRAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "frames_*.npz")))


def check_frame(got, ref, what):
    r = rmse_per_channel(got, ref)
    assert (r < RMSE_TOL).all(), "%s: RMSE %s exceeds %g" % (what, r, RMSE_TOL)
    n = bit_mismatch(got[..., :3].reshape(-1, 3), ref.reshape(-1, 3))
    assert n == 0, "%s: %d pixels differ bitwise (RMSE %s)" % (what, n, r)


@pytest.mark.parametrize("name", FRAMES)
def test_frames_vs_reference_goldens(B, be, O, name):
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    be.resize(W, H)
    be.upload_bvh(tree)
    be.set_camera(g["cam"])
    mk = frame_golden_params(O, g)
    if "direct" in g:
        be.render_direct(to_params(B, mk()))
        check_frame(be.read(0), g["direct"], "direct")
    if "direct_nosun" in g:
        be.render_direct(to_params(B, mk(False)))
        check_frame(be.read(0), g["direct_nosun"], "direct, sun off")
    seeds = g["seeds"]
    npass = int(g["npasses"]) if "npasses" in g else 2
    be.pt_reset()
    for k in range(npass):
        be.pt_pass(to_params(B, mk()), seeds[k], 1)
        if k == 0:
            check_frame(be.read(1), g["pt_pass1"], "PT pass 1")
    check_frame(be.read(1), g["pt_acc"], "PT accumulated")
    if "pt_3paths" in g:
        be.pt_reset()
        be.pt_pass(to_params(B, mk()), seeds[0], 3)
        check_frame(be.read(1), g["pt_3paths"], "PT 3 paths/pass")


def test_birth_order_of_the_paths_changes_no_pixel(B, O):
    """Which path slot holds which pixel is a table (Frame::tile_order: a permutation of the tile's 8x8 pixel blocks): a path's random
    numbers come from hit positions and the pass's seed (path_tracing.glsl:164-165, 220), so the reference's frames must come out for
    ANY permutation — row-major, reversed, random, and the library's own (single-pass runs of the persistent kernel: the first counts
    the shaded segments per block, a device sort orders the blocks by them, the following runs are born most expensive first). Full
    frames against the reference's goldens, a ragged tile against the crop, direct lighting, k_run and the launch pipeline, several
    paths per pass; every pass flushed alone so that runs of one pass happen."""
    b = B.Backend(0)
    try:
        for name in ("frames_scene_d_seg5", "frames_scene_pc_seg5"):
            g = golden(name)
            W, H = int(g["W"]), int(g["H"])
            npass = int(g["npasses"]) if "npasses" in g else 2
            b.resize(W, H); b.upload_bvh(O.build_bvh(scene(str(g["scene"])))[0]); b.set_camera(g["cam"])
            P = to_params(B, frame_golden_params(O, g)())
            rng = np.random.RandomState(11)
            for tile in (None, (5, 3, 99, 61)):
                if tile:
                    b.set_tile(*tile)
                    x0, y0, tw, th = tile
                else:
                    x0, y0, tw, th = 0, 0, W, H
                crop = lambda a: a[y0:y0 + th, x0:x0 + tw]
                tiles = ((tw + 7) // 8) * ((th + 7) // 8)
                for label, order in (("row-major", np.arange(tiles)), ("reversed", np.arange(tiles)[::-1]), ("random", rng.permutation(tiles)), ("own", None)):
                    b.test_tile_order(order)
                    for mode in (0, 3, 5):
                        what = "%s, tile %s, %s order, mode %d: " % (name, tile, label, mode)
                        b.set_mode(mode)
                        b.render_direct(P)
                        check_frame(b.read(0), crop(g["direct"]), what + "direct")
                        b.pt_reset()
                        for k in range(npass):
                            b.pt_pass(P, g["seeds"][k], 1)
                            b.flush()
                            if k == 0:
                                check_frame(b.read(1), crop(g["pt_pass1"]), what + "first pass")
                        check_frame(b.read(1), crop(g["pt_acc"]), what + "%d passes" % npass)
                        b.pt_reset()
                        b.pt_pass(P, g["seeds"][0], 3)
                        check_frame(b.read(1), crop(g["pt_3paths"]), what + "3 paths per pass")
                    cur = b.test_current_tile_order()
                    if order is not None:
                        assert np.array_equal(cur, order.astype(np.uint32))
                    else:
                        # the library's own: in use after the single-pass runs above, a permutation, and not the trivial one on a frame
                        # whose blocks differ in cost (sky / floor / mesh)
                        assert cur is not None and np.array_equal(np.sort(cur), np.arange(tiles)), what
                        assert not np.array_equal(cur, np.arange(tiles)), what
            b.set_mode(0)
        # bad tables are refused
        with pytest.raises(B.HipError):
            b.test_tile_order(np.zeros(tiles, np.uint32))
        with pytest.raises(B.HipError):
            b.test_tile_order(np.arange(tiles + 1))
        # a change of the tile drops the table
        b.test_tile_order(np.arange(tiles)[::-1])
        b.set_tile(0, 0, 64, 40)
        assert b.test_current_tile_order() is None
    finally:
        b.close()


def test_blocks_are_sorted_by_cost_class_most_expensive_first(be):
    """k_tile_order alone (gpuart_hip_test_sort_tiles): a permutation; classes of the largest count (24 of them) in descending order;
    row-major within a class (stable) — neighbouring blocks stay neighbours; all-equal counts give the row-major order."""
    rng = np.random.RandomState(5)
    for n in (1, 7, 511, 512, 513, 144, 32400, 200001):
        for kind in ("random", "few", "equal", "zero", "ramp"):
            cost = {"random": rng.randint(0, 5000, n), "few": rng.choice([64, 128, 320], n), "equal": np.full(n, 77), "zero": np.zeros(n, np.int64),
                    "ramp": np.arange(n)}[kind].astype(np.uint32)
            order = be.test_sort_tiles(cost)
            assert np.array_equal(np.sort(order), np.arange(n)), (n, kind)
            mx = int(cost.max())
            cls = 23 - (cost.astype(np.uint64) * 24 // (mx + 1)).astype(np.int64)
            want = np.argsort(cls, kind="stable")
            assert np.array_equal(order, want.astype(np.uint32)), (n, kind)


@pytest.mark.parametrize("mode", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("name", ["frames_box_seg5", "frames_scene_pc_seg5", "frames_scene_d_seg8", "frames_box_usph_fuzzy",
                                  "frames_box_usph_em", "frames_tree_near_seg5", "frames_scene_p_seg4"])
def test_other_execution_modes_give_identical_frames(B, be, O, name, mode):
    """Every execution mode against the same goldens as the default: 1 reference work (k_run, full queries, counters),
    2 megakernel, 3 launch-per-stage wavefront pipeline, 4 executed-work counters (k_run), 5 persistent run kernel always
    (mode 0 picks 3 or 5 by the size of the pass sequence)."""
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(g["cam"])
    mk = frame_golden_params(O, g)
    be.set_mode(mode)
    try:
        if "direct" in g:
            be.render_direct(to_params(B, mk()))
            check_frame(be.read(0), g["direct"], "direct")
        npass = int(g["npasses"]) if "npasses" in g else 2
        be.pt_reset()
        for k in range(npass):
            be.pt_pass(to_params(B, mk()), g["seeds"][k], 1)
        check_frame(be.read(1), g["pt_acc"], "PT accumulated")
        if "pt_3paths" in g:
            be.pt_reset()
            be.pt_pass(to_params(B, mk()), g["seeds"][0], 3)
            check_frame(be.read(1), g["pt_3paths"], "PT 3 paths/pass")
    finally:
        be.set_mode(0)


@pytest.mark.parametrize("mode", [3, 5])
@pytest.mark.parametrize("name", ["frames_box_seg5", "frames_scene_d_seg8", "frames_tree_near_seg5"])
def test_the_opt_in_nearest_first_kernels_on_the_goldens(B, O, name, mode):
    """The opt-in walk (gpuart_hip_set_nearest_first: nearer child first + certificate + second walk) is still shipped: a few goldens of the
    reference's GLSL through its pipeline and k_run variants in the DEFAULT suite, whatever GPUART_TEST_ORDER says (the whole suite runs on
    it with GPUART_TEST_ORDER=nearest; tests/fuzz_parity.py renders every random scene under both settings). None of these scenes holds a
    phantom hit, so the frames must equal the reference's."""
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(g["cam"])
        b.set_nearest_first(0)
        assert b.scene_order() == 0
        mk = frame_golden_params(O, g)
        b.set_mode(mode)
        if "direct" in g:
            b.render_direct(to_params(B, mk()))
            check_frame(b.read(0), g["direct"], "direct")
        npass = int(g["npasses"]) if "npasses" in g else 2
        b.pt_reset()
        for k in range(npass):
            b.pt_pass(to_params(B, mk()), g["seeds"][k], 1)
        check_frame(b.read(1), g["pt_acc"], "PT accumulated, nearest-first walk, mode %d" % mode)
    finally:
        b.close()


@pytest.mark.parametrize("k0", [0, -19])
def test_deep_tree_frames(B, be, O, k0):
    """A 39-level tree (deeper than the LDS ring stack): frames through the spill path == oracle. k0 = 0: spheres out to 5e11,
    which the uploader keeps in the reference's order (kernels without thin-wave modes); k0 = -19: the chain within 2^20, through
    the fast kernels (nearer child first, thin-wave modes with partly spilled stacks)."""
    prims = deep_chain_scene(40, k0) + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    cam = dict(pos=(-6.0, -9.0, 4.0), up=(0.0, 0.0, 1.0), fov_y=60.0, screen_dist=0.2)
    cam["dir"] = (8.0, 9.0, -4.0)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    for k in range(2):
        O.pt_pass(tree, c, W, H, P, seeds[k], 1, acc)
    assert (acc[..., :3].sum(-1) > 0).mean() > 0.5
    # default, launch pipeline, run kernel: a draining wave regroups its rays (thin-wave modes) with part of their stacks spilled
    for mode in (0, 3, 5):
        be.set_mode(mode)
        be.pt_reset()
        for k in range(2):
            be.pt_pass(to_params(B, P), seeds[k], 1)
        assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "deep tree PT, mode %d" % mode)
    be.set_mode(0)
    be.render_direct(to_params(B, P))
    exp, _ = O.render_direct(tree, c, W, H, P)
    assert_bits(be.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "deep tree direct")


def test_segment_and_weight_limits(B, be, O):
    """maxSegments / minWeight edge values: 0 segments, weight >= 1, weight 0 with a long segment budget."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 64, 40
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    for ms, mw in [(0, 0.01), (5, 1.0), (5, 1.5), (12, 0.0), (3, 0.2), (2, 0.01)]:
        P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], ms, mw)
        acc = np.zeros((H, W, 4), np.float32)
        O.pt_pass(tree, c, W, H, P, [0.3, 0.6, 0.9, 0.1], 2, acc)
        for mode in (0, 2):
            be.set_mode(mode)
            be.pt_reset()
            be.pt_pass(to_params(B, P), [0.3, 0.6, 0.9, 0.1], 2)
            assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "maxSegments=%d minWeight=%g mode %d" % (ms, mw, mode))
        be.set_mode(0)


def test_segment_bound_next_to_albedo_powers(B, be, O):
    """minWeight just below a power of an albedo (shaders/path_tracing.glsl:138-139,177: the loop continues while every
    channel of colorWeight is > MIN_WEIGHT): the host's bound on the number of segment launches must not cut the segment
    the reference still runs. An all-sphere pit (every bounce multiplies by the sphere albedo, so colorWeight.z is exactly
    0.35^k) and Scene P, maxSegments 8, wavefront pipeline and megakernel against the oracle."""
    a = np.float32(0.35); b = np.float32(0.4)
    p4 = a * a * a * a
    p5 = b * b * b * b * b
    weights = [float(np.nextafter(p4, np.float32(0))), float(p4 / np.float32(1.00005)), float(np.nextafter(p5, np.float32(0))),
               float(p4), float(np.nextafter(a * a, np.float32(0)))]
    rng = np.random.RandomState(4)
    pit = [(S.SPHERE, [0.0, 0.0, -100.0, 100.0])] + [
        (S.SPHERE, [float(np.float32(x)), float(np.float32(y)), 0.25, 0.3]) for x, y in rng.uniform(-1.2, 1.2, (40, 2))]
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 64, 40
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    deep = 0
    for prims in (pit, S.scene_p()):
        tree, _ = O.build_bvh(prims)
        be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
        for mw in weights:
            P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, mw)
            acc = np.zeros((H, W, 4), np.float32)
            st = O.pt_pass(tree, c, W, H, P, [0.3, 0.6, 0.9, 0.1], 2, acc)
            deep += st.segments
            for mode in (0, 2):
                be.set_mode(mode)
                be.pt_reset()
                be.pt_pass(to_params(B, P), [0.3, 0.6, 0.9, 0.1], 2)
                assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "minWeight=%.9g mode %d" % (mw, mode))
            be.set_mode(0)
    assert deep > 0


@pytest.mark.parametrize("max_levels,min_prims", [(1024, 2), (1024, 5), (4, 2), (1, 2), (7, 1)])
def test_leaves_of_any_size(B, be, O, max_levels, min_prims):
    """The uploader routes leaves of one or two primitives through fetch-at-once paths (triangle pairs, pairs of any type) and
    all others through the counting loop; trees built with other leaf sizes / depth limits than the reference's defaults
    (`BoundingVolumesHierarchy(prims, maxNumLevels, minPrimitivesPerNode)`, src/bvh.h:78) put every kernel family
    (triangle + disc, sphere + disc, all types) on every path: direct lighting and path tracing (pipeline, run kernel,
    reference-work mode, megakernel) against the oracle."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 72, 40
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    rng = np.random.RandomState(11)
    mesh = [(S.DISC, [0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 30.0])]
    for _ in range(60):
        o = rng.uniform(-1.5, 1.5, 3); o[2] = abs(o[2]) * 0.5 + 0.05
        mesh.append((S.TRIANGLE, [float(np.float32(v)) for v in np.concatenate([o, o + rng.uniform(-0.5, 0.5, 3), o + rng.uniform(-0.5, 0.5, 3)])]))
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    for name, prims in (("mesh", mesh), ("scene_p", S.scene_p()), ("scene_pc", scene("scene_pc"))):
        tree, _ = O.build_bvh(prims, max_levels=max_levels, min_prims=min_prims)
        be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
        d = O.render_direct(tree, c, W, H, P)[0]
        be.render_direct(to_params(B, P))
        assert_bits(be.read(0)[..., :3].reshape(-1, 3), d[..., :3].reshape(-1, 3), "%s direct" % name)
        acc = np.zeros((H, W, 4), np.float32)
        seeds = O.randseeds(3, seed=77)
        for k in range(3):
            O.pt_pass(tree, c, W, H, P, seeds[k], 1, acc)
        for mode in (0, 5, 3, 1, 2):
            be.set_mode(mode)
            be.pt_reset()
            for k in range(3):
                be.pt_pass(to_params(B, P), seeds[k], 1)
            assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "%s mode %d" % (name, mode))
        be.set_mode(0)


def test_segment_budget_is_capped(B, be, O):
    """maxSegments beyond GPUART_HIP_MAX_SEGMENTS (1024) is refused instead of allocating counters for 1e9 launches."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], 32, 16)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    be.resize(32, 16); be.upload_bvh(tree); be.set_camera(c)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 10 ** 9, 0.0)
    with pytest.raises(B.HipError):
        be.pt_pass(to_params(B, P), [0.3, 0.6, 0.9, 0.1], 1)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 1024, 0.0)
    be.pt_reset(); be.pt_pass(to_params(B, P), [0.3, 0.6, 0.9, 0.1], 1)
    acc = np.zeros((16, 32, 4), np.float32)
    O.pt_pass(tree, c, 32, 16, P, [0.3, 0.6, 0.9, 0.1], 1, acc)
    assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "maxSegments 1024, minWeight 0")


def test_renderer_api_box_scene(B):
    """The C++ gpuart::Renderer driven like the reference app drives it (src/main.cpp:609-623,549-599)."""
    g = golden("frames_box_seg5")
    W, H = int(g["W"]), int(g["H"])
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(W, H, cam)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.init_box()
    assert r.is_ok()
    r.render_direct()
    check_frame(r.read_direct(), g["direct"], "Renderer direct")
    r.restart_path_tracing(1, 8)
    done = [r.path_tracing_pass() for _ in range(10)]
    assert done == [1, 2, 3, 4, 5, 6, 7, 8, 8, 8]  # stops at pathsPerPixel (src/renderer.cpp:534,567-570)
    check_frame(r.read_radiance(False), g["pt_acc"], "Renderer 8 passes")
    norm = r.read_radiance(True)
    np.testing.assert_array_equal(norm[..., :3], g["pt_acc"] / np.float32(8))
    # any setter restarts the accumulation (src/renderer.h:199-283); the RNG is NOT re-seeded
    r.set_sun(S.SUN_AZIMUTH, S.SUN_ALTITUDE, True)
    assert r.path_tracing_pass() == 1
    r.close()


def test_two_renderers_on_one_device_do_not_disturb_each_other(B):
    """The ABI promises independent contexts (include/gpuart_hip.h): two Renderers on the same device, different scenes and frame
    sizes, their passes interleaved call by call and their pipelines in flight at the same time, each reproduce the reference's
    golden frames (what gpuart_cli --gpus N relies on, one context per device, and any host that keeps a preview beside a render)."""
    ga, gb = golden("frames_box_seg5"), golden("frames_scene_pc_seg5")
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    ra = B.Renderer(int(ga["W"]), int(ga["H"]), cam)
    rb = B.Renderer(int(gb["W"]), int(gb["H"]), cam)
    for r in (ra, rb):
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    ra.init_box()
    rb.set_primitives(scene("scene_pc"))
    ra.render_direct(); rb.render_direct()
    na, nb = int(ga["npasses"]) if "npasses" in ga else 8, int(gb["npasses"]) if "npasses" in gb else 2
    ra.restart_path_tracing(1, na); rb.restart_path_tracing(1, nb)
    for k in range(max(na, nb)):  # interleaved, nothing observed in between: both contexts have runs in flight
        if k < na: ra.path_tracing_pass()
        if k < nb: rb.path_tracing_pass()
    check_frame(rb.read_radiance(False), gb["pt_acc"], "second renderer, %d passes" % nb)
    check_frame(ra.read_radiance(False), ga["pt_acc"], "first renderer, %d passes" % na)
    check_frame(ra.read_direct(), ga["direct"], "first renderer, direct")
    check_frame(rb.read_direct(), gb["direct"], "second renderer, direct")
    ra.close(); rb.close()


def test_reference_work_mode_counters_match_oracle(B, be, O):
    g = golden("frames_scene_pc_seg5")
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene("scene_pc"))
    be.resize(W, H)
    be.upload_bvh(tree)
    be.set_camera(g["cam"])
    mk = frame_golden_params(O, g)
    be.set_mode(1)
    try:
        be.counters(reset=True)
        be.render_direct(to_params(B, mk()))
        check_frame(be.read(0), g["direct"], "direct (reference-work mode)")
        c = be.counters(reset=True)
        _, st = O.render_direct(tree, g["cam"], W, H, mk(), nthreads=4)
        assert (c.rays, c.nodes, list(c.prim_tests)) == (st.rays, st.nodes, list(st.prim_tests))
        be.pt_reset()
        be.pt_pass(to_params(B, mk()), g["seeds"][0], 1)
        check_frame(be.read(1), g["pt_pass1"], "PT (reference-work mode)")
        c = be.counters(reset=True)
        acc = np.zeros((H, W, 4), np.float32)
        st = O.pt_pass(tree, g["cam"], W, H, mk(), g["seeds"][0], 1, acc, nthreads=4)
        assert (c.rays, c.nodes, list(c.prim_tests), c.segments) == (st.rays, st.nodes, list(st.prim_tests), st.segments)
    finally:
        be.set_mode(0)


# ---- edge cases ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (37, 23), (65, 9)])
def test_ragged_frame_sizes(B, be, O, W, H):
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    be.render_direct(to_params(B, P))
    exp, _ = O.render_direct(tree, c, W, H, P)
    assert_bits(be.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "direct %dx%d" % (W, H))
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    be.pt_reset()
    for k in range(2):
        be.pt_pass(to_params(B, P), seeds[k], 2)
        O.pt_pass(tree, c, W, H, P, seeds[k], 2, acc)
    assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "PT %dx%d" % (W, H))


def test_empty_scene_and_single_primitive(B, be, O):
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 48, 32
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    for prims in [[], [(S.SPHERE, [0, 0, 0.5, 0.5])]]:
        tree, _ = B.compile_bvh(prims)
        be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
        be.pt_reset()
        be.pt_pass(to_params(B, P), [0.1, 0.2, 0.3, 0.4], 1)
        acc = np.zeros((H, W, 4), np.float32)
        O.pt_pass(tree, c, W, H, P, [0.1, 0.2, 0.3, 0.4], 1, acc)
        assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "PT, %d primitives" % len(prims))


def test_inverted_and_degenerate_boxes(B, be, O):
    """Negative radii give inverted boxes (min > max), which the reference's comparisons can never hit; flat
    triangles give zero-thickness boxes. Both must behave exactly like the oracle."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 80, 48
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    prims = S.box_scene() + [(S.SPHERE, [0.3, -0.5, 0.4, -0.2]), (S.SPHERE, [-0.5, -0.6, 0.3, -0.1]),
                             (S.DISC, [0.2, 0.2, 0.5, 0, 0, 1, -0.3]), (S.CONE, [-0.5, 0.5, 0, -0.5, 0.5, 0.4, -0.1, -0.2]),
                             (S.TRIANGLE, [-0.8, -0.9, 0.5, 0.8, -0.9, 0.5, 0.0, -0.2, 0.5])]
    tree, _ = B.compile_bvh(prims)
    otree, _ = O.build_bvh(prims)
    assert (tree.view(np.uint32) == otree.view(np.uint32)).all()
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    be.render_direct(to_params(B, P))
    exp, _ = O.render_direct(tree, c, W, H, P)
    assert_bits(be.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "direct")
    acc = np.zeros((H, W, 4), np.float32)
    be.pt_reset()
    for k, seed in enumerate(O.randseeds(3)):
        be.pt_pass(to_params(B, P), seed, 1)
        O.pt_pass(tree, c, W, H, P, seed, 1, acc)
    assert_bits(be.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "PT")


def test_malformed_tree_is_rejected(B, be):
    tree, _ = B.compile_bvh(S.box_scene())
    bad = tree.copy()
    bad.view(np.uint32)[2, 2] = 10 ** 6  # upper-child address far outside the array
    with pytest.raises(B.HipError):
        be.upload_bvh(bad)
    with pytest.raises(B.HipError):
        be.upload_bvh(tree[:2])
    # an upper child that points back into its sibling's subtree (a DAG): rejected, not converted in exponential time
    dag = tree.copy()
    u = dag.view(np.uint32)
    assert u[2, 0] & 0x80000000 == 0 and u[2, 2] > 6   # the root is an interior node
    u[2, 2] = 6                                        # its upper child := an address inside the lower subtree
    with pytest.raises(B.HipError):
        be.upload_bvh(dag)
    be.upload_bvh(tree)


# ---- BASELINE-size properties (1080p dragon-class scene) ------------------------------------------------
@pytest.fixture(scope="module")
def dragon_1080p(B, O):
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 1920, 1080
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = B.compile_bvh(S.scene_d())
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    return W, H, c, tree, P


def test_full_size_tile_split_equals_whole_frame(B, be, O, dragon_1080p):
    """cfg3 (1080p, dragon-class, depth 8): a frame rendered as 4 interleaved row bands + 2 column tiles is
    bit-identical to the whole frame (tiles are independent: SURVEY.md §8(e)); two runs are identical."""
    W, H, c, tree, P = dragon_1080p
    seeds = O.randseeds(2)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)

    def render(tile):
        be.set_tile(*tile)
        be.pt_reset()
        for k in range(2):
            be.pt_pass(to_params(B, P), seeds[k], 1)
        return be.read(1)

    whole = render((0, 0, W, H))
    again = render((0, 0, W, H))
    assert bit_mismatch(whole.reshape(-1, 4), again.reshape(-1, 4)) == 0
    assert np.isfinite(whole[..., :3]).all() and whole[..., :3].min() >= 0
    for tile in [(0, 0, W, 270), (0, 270, W, 270), (0, 540, 960, 540), (960, 540, 960, 540), (123, 457, 333, 101)]:
        x0, y0, tw, th = tile
        part = render(tile)
        assert bit_mismatch(part.reshape(-1, 4), whole[y0:y0 + th, x0:x0 + tw].reshape(-1, 4)) == 0, tile
    # a sample of pixels against the oracle (a 96x64 window on the mesh)
    win = (900, 500, 96, 64)
    acc = np.zeros((win[3], win[2], 4), np.float32)
    for k in range(2):
        O.pt_pass(tree, c, W, H, P, seeds[k], 1, acc, tile=win, nthreads=4)
    x0, y0, tw, th = win
    assert_bits(whole[y0:y0 + th, x0:x0 + tw, :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "1080p window vs oracle")


def test_full_size_interleaved_tiles_equal_whole_frame(B, be, O, dragon_1080p):
    """The 8-way interleaved sharding bench.py uses at N=8: every rank's rows are bit-identical to the whole frame's."""
    from gpuart_amd import sharding
    W, H, c, tree, P = dragon_1080p
    seeds = O.randseeds(2)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    be.pt_reset()
    for k in range(2):
        be.pt_pass(to_params(B, P), seeds[k], 1)
    whole = be.read(1)
    for rank in (0, 3, 7):
        y0, n, band, stride, rows = sharding.interleaved_rows(rank, 8, H)
        be.set_tile_interleaved(0, y0, W, n, band, stride)
        be.pt_reset()
        for k in range(2):
            be.pt_pass(to_params(B, P), seeds[k], 1)
        part = be.read(1)
        assert bit_mismatch(part.reshape(-1, 4), whole[rows].reshape(-1, 4)) == 0, rank
    be.set_tile(0, 0, W, H)


def test_4k_and_8k_configs(B, O):
    """cfg4 (3840x2160, whole frame on one GPU) and cfg5 (7680x4320, one of 8 interleaved shares): a few progressive
    passes through the Renderer API; windows of the result against the oracle, whole-frame sanity."""
    from gpuart_amd import sharding
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    prims = B.make_prims(S.scene_d())
    tree, _ = O.build_bvh(S.scene_d())
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    seeds = O.randseeds(3)
    for (W, H, share) in [(3840, 2160, None), (7680, 4320, (5, 8))]:
        r = B.Renderer(W, H, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(prims)
        r.set_max_path_segments(8)
        rows = np.arange(H)
        if share:
            y0, n, band, stride, rows = sharding.interleaved_rows(share[0], share[1], H)
            assert r.set_interleaved_tile(0, y0, W, n, band, stride)
        r.restart_path_tracing(1, 3)
        assert [r.path_tracing_pass() for _ in range(3)] == [1, 2, 3]
        acc = r.read_radiance(False)
        r.close()
        assert acc.shape == (len(rows), W, 4) and np.isfinite(acc[..., :3]).all() and acc[..., :3].min() >= 0
        # an oracle window in the middle of the mesh: 64 columns x the first 16 local rows at/after frame row H/2
        c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
        P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
        l0 = int(np.searchsorted(rows, H // 2))
        x0 = W // 2 - 32
        for k in range(l0, l0 + 16, 8):      # 8-row groups are contiguous frame rows in both layouts
            gy = int(rows[k])
            exp = np.zeros((8, 64, 4), np.float32)
            for sd in seeds:
                O.pt_pass(tree, c, W, H, P, sd, 1, exp, tile=(x0, gy, 64, 8), nthreads=4)
            assert_bits(acc[k:k + 8, x0:x0 + 64, :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "%dx%d window" % (W, H))


@pytest.mark.parametrize("cfg", ["cfg4", "cfg5"])
def test_cfg4_and_cfg5_at_their_stated_depth(B, O, cfg):
    """BASELINE.json's two deep configurations rendered to their full depth through the Renderer in its default mode, as
    Renderer::RenderPathTracingPass accumulates them (reference src/renderer.cpp:534-616): cfg4 = Scene D, 3840x2160, 1024
    progressive passes of 1 path per pixel (RestartPathTracing(1, 1024): 16 plan-sized runs of 64 passes); cfg5 = 7680x4320,
    256 passes, share 5 of an 8-way split (what one of 8 GPUs renders). Three 64x8 windows of the accumulator — on the mesh,
    on the floor, at the horizon — against the oracle accumulating the same 1024 / 256 RandSeeds, bit for bit."""
    from gpuart_amd import sharding
    W, H, passes, share = {"cfg4": (3840, 2160, 1024, None), "cfg5": (7680, 4320, 256, (5, 8))}[cfg]
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(W, H, cam)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_primitives(B.make_prims(S.scene_d()))
    r.set_max_path_segments(8)
    rows = np.arange(H)
    if share:
        y0, n, band, stride, rows = sharding.interleaved_rows(share[0], share[1], H)
        assert r.set_interleaved_tile(0, y0, W, n, band, stride)
    r.restart_path_tracing(1, passes)
    done = [r.path_tracing_pass() for _ in range(passes)]
    assert done == list(range(1, passes + 1)) and r.path_tracing_pass() == passes  # (one more call renders nothing)
    acc = r.read_radiance(False)
    norm = r.read_radiance(True)
    r.close()
    assert acc.shape == (len(rows), W, 4) and np.isfinite(acc[..., :3]).all() and acc[..., :3].min() >= 0
    np.testing.assert_array_equal(norm[..., :3], acc[..., :3] / np.float32(passes))  # pt_normalize.glsl:44-47
    tree, _ = O.build_bvh(S.scene_d())
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    seeds = O.randseeds(passes)
    hits = 0
    for fx, fy in ((0.5, 0.5), (0.3, 0.12), (0.7, 0.62)):  # mesh / floor / around the horizon (benchmark camera)
        k = int(np.searchsorted(rows, int(fy * H))) // 8 * 8  # an 8-row group: contiguous frame rows in both layouts
        gy, x0 = int(rows[k]), int(fx * W) // 8 * 8
        exp = np.zeros((8, 64, 4), np.float32)
        for sd in seeds:
            O.pt_pass(tree, c, W, H, P, sd, 1, exp, tile=(x0, gy, 64, 8), nthreads=8)
        assert_bits(acc[k:k + 8, x0:x0 + 64, :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "%s window at (%d, %d) after %d passes" % (cfg, x0, gy, passes))
        hits += 1
    assert hits == 3


def test_full_size_accumulation_is_additive(B, be, O, dragon_1080p):
    """accum after passes (s0, s1) == single-pass(s0) + single-pass(s1) in float32 (path_tracing.glsl:255)."""
    W, H, c, tree, P = dragon_1080p
    seeds = O.randseeds(2)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    be.set_tile(0, 300, W, 256)
    singles = []
    for k in range(2):
        be.pt_reset(); be.pt_pass(to_params(B, P), seeds[k], 1); singles.append(be.read(1))
    be.pt_reset()
    for k in range(2):
        be.pt_pass(to_params(B, P), seeds[k], 1)
    both = be.read(1)
    np.testing.assert_array_equal(both[..., :3], singles[0][..., :3] + singles[1][..., :3])
    # direct lighting is idempotent and independent of path-tracing state
    be.render_direct(to_params(B, P)); d1 = be.read(0)
    be.render_direct(to_params(B, P)); d2 = be.read(0)
    np.testing.assert_array_equal(d1, d2)


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("plan,npaths", [(0, 1), (7, 1), (70, 1), (1000, 1), (70, 3)])
def test_pass_grouping_never_changes_the_result(B, be, O, plan, npaths, mode):
    """gpuart_hip_pt_pass only queues; passes travel through the pipeline in runs whose size follows the plan hint
    (gpuart_hip_pt_plan), the tile size and explicit flushes. Whatever the grouping — one pass at a time with a read-back
    after each, runs of up to 64 passes on a small tile, flushes in odd places, several paths per pass — the accumulator
    is the float32 sum of the single passes in pass order (path_tracing.glsl:252-255), and equals the oracle's."""
    W, H = 64, 40
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    K = 70 if npaths == 1 else 20
    seeds = O.randseeds(K)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    be.set_mode(mode)  # 0: this small frame goes through the persistent run kernel; 3: the launch pipeline
    # one pass at a time, observed after each: the reference's own schedule
    be.pt_reset()
    for k in range(K):
        be.pt_pass(to_params(B, P), seeds[k], npaths)
        if k % 9 == 0:
            be.read(1)
    step_by_step = be.read(1)
    # queued with a plan, flushed in odd places
    be.pt_reset(); be.pt_plan(plan)
    for k in range(K):
        be.pt_pass(to_params(B, P), seeds[k], npaths)
        if k in (3, 4, 40):
            be.flush()
    grouped = be.read(1)
    be.set_mode(0)
    assert_bits(grouped.reshape(-1, 4), step_by_step.reshape(-1, 4), "grouped vs step by step, plan %d" % plan)
    if plan == 70:
        acc = np.zeros((H, W, 4), np.float32)
        for k in range(K):
            O.pt_pass(tree, c, W, H, P, seeds[k], npaths, acc)
        assert_bits(grouped[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "vs oracle")


@pytest.mark.parametrize("env", [
    {"GPUART_HIP_LANE_BUDGET_MB": "64", "GPUART_HIP_BATCH_MPATHS": "1", "GPUART_HIP_SMALL_KPATHS": "0"},
    {"GPUART_HIP_PASSES_IN_FLIGHT": "1", "GPUART_HIP_MAX_BATCH": "3", "GPUART_HIP_LEAN_KERNELS": "0", "GPUART_HIP_SMALL_KPATHS": "0"},
    {"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "16", "GPUART_HIP_REFILL_LANES": "1", "GPUART_HIP_LEAF_LANES": "64",
     "GPUART_HIP_PLAN_RUN_PERCENT": "10", "GPUART_HIP_SMALL_KPATHS": "0"},
    # the persistent run kernel (what mode 0 picks for this small sequence): tiny grid, eager refills, generic kernels
    {"GPUART_HIP_RUN_WAVES_PER_CU": "1", "GPUART_HIP_REFILL_LANES": "1", "GPUART_HIP_LEAN_KERNELS": "0", "GPUART_HIP_MAX_BATCH": "5"},
    {"GPUART_HIP_RUN_WAVES_PER_CU": "32", "GPUART_HIP_REFILL_LANES": "64", "GPUART_HIP_LEAF_LANES": "1", "GPUART_HIP_LANE_BUDGET_MB": "64"},
    # every box test through its six face tests (no quick answers: csrc/hip/box_quick.h), both pipelines
    {"GPUART_HIP_QUICK_BOXES": "0"},
    {"GPUART_HIP_QUICK_BOXES": "0", "GPUART_HIP_SMALL_KPATHS": "0"},
])
def test_scheduling_knobs_never_change_the_result(B, O, env, monkeypatch):
    """Memory budget, lanes in flight, run sizes, persistent-grid size, refill / leaf thresholds, kernel specialisation:
    none of the tuning knobs may change a bit of the accumulator (Scene D tile, 12 passes, vs the oracle)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    W, H = 192, 96
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("scene_d"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    K = 12
    seeds = O.randseeds(K)
    acc = np.zeros((H, W, 4), np.float32)
    for k in range(K):
        O.pt_pass(tree, c, W, H, P, seeds[k], 1, acc, nthreads=8)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(c)
        b.pt_reset(); b.pt_plan(K)
        for k in range(K):
            b.pt_pass(to_params(B, P), seeds[k], 1)
        got = b.read(1)
    finally:
        b.close()
    assert_bits(got[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "knobs %s" % env)


@pytest.mark.parametrize("sc,npaths", [("scene_d", 1), ("scene_p", 1), ("scene_pc", 3)])
def test_passes_observed_one_by_one(B, O, sc, npaths):
    """The reference's interactive loop (src/main.cpp:549-599): one pass per GUI frame, observed after each. Every pass is then its
    own run of the persistent kernel: the accumulator after every pass equals the oracle's, also across a reset, a camera change and
    a resize (1 and 3 paths per pixel and pass)."""
    W, H = 200, 104
    cam = dict(S.BENCH_CAMERA if sc == "scene_d" else S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    tree, _ = O.build_bvh(scene(sc))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    b = B.Backend(0)
    try:
        for (w, h, dx) in ((W, H, 0.0), (W, H, 0.3), (W - 56, H + 8, 0.3)):
            pos = [cam["pos"][0] + dx, cam["pos"][1], cam["pos"][2]]
            c = O.camera(pos, cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], w, h)
            P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
            b.resize(w, h); b.upload_bvh(tree); b.set_camera(c)
            b.pt_reset()
            seeds = O.randseeds(5, seed=31)
            acc = np.zeros((h, w, 4), np.float32)
            for k in range(5):
                O.pt_pass(tree, c, w, h, P, seeds[k], npaths, acc, nthreads=8)
                b.pt_pass(to_params(B, P), seeds[k], npaths)
                assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "%s %dx%d pass %d" % (sc, w, h, k))
    finally:
        b.close()


def test_random_cases_vs_reference_goldens(B, be, O):
    """The 24 random cases rendered by the reference's shaders on llvmpipe (tests/golden/fuzz_frames.npz): the HIP path
    reproduces direct lighting and the accumulated path-tracing passes bit for bit, wavefront and megakernel mode."""
    g = golden("fuzz_frames")
    for seed in g["cases"]:
        seed = int(seed)
        case, tree, cam, P, seeds = fuzz_case_setup(O, seed)
        be.resize(case["W"], case["H"]); be.upload_bvh(tree); be.set_camera(cam)
        for mode in (0, 2):
            be.set_mode(mode)
            be.render_direct(to_params(B, P))
            assert_bits(be.read(0)[..., :3].reshape(-1, 3), g["direct_%d" % seed].reshape(-1, 3), "case %d direct, mode %d" % (seed, mode))
            be.pt_reset()
            for k in range(case["passes"]):
                be.pt_pass(to_params(B, P), seeds[k], case["npaths"])
            assert_bits(be.read(1)[..., :3].reshape(-1, 3), g["pt_acc_%d" % seed].reshape(-1, 3), "case %d PT, mode %d" % (seed, mode))
        be.set_mode(0)


@pytest.mark.parametrize("mode", [3, 5])
@pytest.mark.parametrize("sc,tag", [("scene_d", "1080p"), ("scene_d", "4k"), ("scene_p", "1080p")])
def test_full_size_frame_vs_reference_checksums(B, be, O, sc, tag, mode):
    """BASELINE cfg3 at FULL size as rendered by the reference's shaders on llvmpipe (per-row checksums of the float bit
    patterns, tests/golden/fullsize_scene_d_1080p.npz): the HIP path's direct-lighting frame and its accumulator after
    one and two passes give the same checksums — full-size parity against the reference itself, not only the oracle.
    ("scene_p", "1080p") is BASELINE cfg2: Scene P (256 spheres + 16 discs), depth 4, default camera — the generic
    (all primitive types) BVH-query kernels at a BASELINE size; cfg1 (256x256 direct lighting, whole frame as bits) is
    frames_scene_p_seg4 in test_frames_vs_reference_goldens."""
    g = golden("fullsize_%s_%s" % (sc, tag))
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(sc))
    cam = g["cam"]
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(cam[12]), cam[0:3], int(g["max_segments"]), 0.01)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(cam)
    be.render_direct(to_params(B, P))
    np.testing.assert_array_equal(row_checksums(be.read(0)), g["direct"])
    be.set_mode(mode)  # both path-tracing pipelines at the BASELINE sizes: 3 launch pipeline, 5 persistent run kernel
    try:
        be.pt_reset()
        for k in range(int(g["npasses"])):
            be.pt_pass(to_params(B, P), g["seeds"][k], 1)
            np.testing.assert_array_equal(row_checksums(be.read(1)), g["pt_acc%d" % (k + 1)])
    finally:
        be.set_mode(0)


@pytest.mark.parametrize("wild", [False, True, "wild2", "lattice", "grazing"])
def test_random_scenes_soak(wild):
    """tests/fuzz_parity.py: 60 random scenes of all four primitive types incl. degenerate ones (zero radii, zero-area
    and axis-aligned triangles, exact duplicates, cylinders), random cameras, user-sphere modes, Sun on/off, depths 1-8,
    1-2 paths per pass; direct lighting + 3 path-tracing passes in the wavefront and the megakernel mode, all bit for bit
    equal to the oracle. `wild`: a quarter of the primitives additionally carry NaN, +-inf, +-1e30, +-1e-30 or -0
    coordinates (1 500 plain and 600 wild scenes of the same tool found no difference; the oracle itself was held against
    the reference's shaders on 300 plain and 120 wild cases, tests/golden/soak_oracle_vs_reference.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # "wild2": the second class of hostile numbers (negative radii, the reference's magic numbers 1e19 / 1e-4 / 1e-8 / 1e-10, the
    # ends of the float range, denormals, odd cameras / user spheres / Sun altitudes; 8 000 cases of it found no difference)
    # "lattice" (round 4): coplanar, overlapping axis-aligned triangles and discs, coincident spheres — boxes that are not
    # conservative for their primitives in fp32, where the reference's winner hinges on its visiting order and the fast kernels'
    # nearest-first walk has to notice (device_scene.h "Visiting order"): without its certificate 133 of 1 500 such scenes differed
    # "grazing" (round 5): fans of triangulated sheets seen edge-on — frames full of the reference's phantom hits (shaders/triangle.glsl:50-76
    # at grazing angles), which only a walk in the reference's order reproduces: the default walks must equal the oracle (which equals the
    # reference's GLSL on 2 000 cases of the class); the opt-in nearest-first walk is rendered too, its differing scenes counted, not failed
    cmd = [sys.executable, os.path.join(root, "tests", "fuzz_parity.py")] + (["--" + wild] if isinstance(wild, str) else ["--wild"] if wild else []) + ["0", "60"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "60 scenes, 0 with differences" in r.stdout


@pytest.mark.parametrize("flavour", ["", "--wild", "--wild2", "--lattice"])
def test_random_scenes_through_the_renderer_api(flavour):
    """The same random cases through the C++ gpuart::Renderer — its own BVH build and upload (Renderer::SetPrimitives), camera
    basis, Sun direction and RandSeed draws instead of the oracle's — in both path-tracing pipelines: the whole product against
    the oracle, bit for bit (tests/fuzz_parity.py --renderer; 300 plain + 300 wild cases found no difference)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "fuzz_parity.py"), "--renderer"] + ([flavour] if flavour else []) + ["0", "40"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "40 scenes, 0 with differences" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("flavour", ["", "--wild"])
def test_random_scenes_rendered_as_shares_of_several_ranks(flavour):
    """The multi-GPU decomposition on random cases: the frame rendered as the shares of 2, 3 or 5 ranks (row bands of 1, 3, 8 or
    16 rows dealt round-robin, gpuart_hip_share_of_rank / _set_share), every share scattered into the frame as the gather's root
    does — equal to the oracle's whole frame bit for bit, in both pipelines (tests/fuzz_parity.py --shares; 600 plain + 400 wild
    cases found no difference)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "fuzz_parity.py"), "--shares"] + ([flavour] if flavour else []) + ["0", "40"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and "40 scenes, 0 with differences" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_checkpoint_resume_is_bit_identical(B, tmp_path):
    """8 passes == 3 passes + SaveCheckpoint + (new Renderer) LoadCheckpoint + 5 passes, including the RNG state."""
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    W, H = 96, 64
    prims = S.scene_p(seed=3, nspheres=96, ndiscs=24, ncones=64)

    def fresh():
        r = B.Renderer(W, H, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(prims)
        return r

    r = fresh()
    r.restart_path_tracing(1, 8)
    for _ in range(8):
        r.path_tracing_pass()
    whole = r.read_radiance(False)
    r.close()

    r = fresh()
    r.restart_path_tracing(1, 8)
    for _ in range(3):
        r.path_tracing_pass()
    ck = str(tmp_path / "render.ck")
    assert r.save_checkpoint(ck)
    r.close()

    r = fresh()
    r.restart_path_tracing(1, 8)
    assert r.load_checkpoint(ck)
    done = [r.path_tracing_pass() for _ in range(6)]
    assert done == [4, 5, 6, 7, 8, 8]
    resumed = r.read_radiance(False)
    assert not r.load_checkpoint(str(tmp_path / "missing.ck"))
    r.update_viewport(W // 2, H)
    assert not r.load_checkpoint(ck)  # viewport mismatch is refused
    r.close()
    np.testing.assert_array_equal(whole, resumed)


def test_headless_cli(B, O, tmp_path):
    """gpuart_cli (replaces the reference's GUI main loop): Box scene, direct + progressive PT, PFM/PPM output."""
    import json, subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpuart_amd", "bin", "gpuart_cli")
    pfm, ppm = str(tmp_path / "o.pfm"), str(tmp_path / "o.ppm")
    W, H = 80, 60
    out = subprocess.run([exe, "--scene", "box", "--width", str(W), "--height", str(H), "--mode", "pt", "--spp", "4",
                          "--per-pass", "2", "--pfm", pfm, "--ppm", ppm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    info = json.loads(out.stdout.strip().splitlines()[-1])
    assert info["paths_per_pixel"] == 4 and info["passes"] == 2
    raw = open(pfm, "rb").read()
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    assert raw.startswith(head)
    img = np.frombuffer(raw[len(head):], np.float32).reshape(H, W, 3)
    # the same render through the oracle: 2 passes of 2 paths, normalised by 4
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(S.box_scene())
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    acc = np.zeros((H, W, 4), np.float32)
    for seed in O.randseeds(2):
        O.pt_pass(tree, c, W, H, P, seed, 2, acc)
    assert_bits(img.reshape(-1, 3), (acc[..., :3] / np.float32(4)).reshape(-1, 3), "CLI PFM vs oracle")
    # the 8-bit image: what the reference's default framebuffer shows of that frame (src/renderer.cpp:601-616 draws the
    # normalised radiance into an 8-bit unsigned-normalised buffer: clamp to [0, 1], x 255, round to nearest), top row first
    raw8 = open(ppm, "rb").read()
    head8 = b"P6\n%d %d\n255\n" % (W, H)
    assert raw8.startswith(head8) and len(raw8) == len(head8) + W * H * 3
    got8 = np.frombuffer(raw8[len(head8):], np.uint8).reshape(H, W, 3)
    scaled = (np.clip(img, 0.0, 1.0).astype(np.float32) * np.float32(255.0)).astype(np.float64)
    exp8 = np.floor(scaled + 0.5).astype(np.uint8)[::-1]
    np.testing.assert_array_equal(got8, exp8)
    assert exp8.min() < 255 and exp8.max() == 255 and len(np.unique(exp8)) > 50  # a real image: clamped highlights and a range of greys


def test_headless_cli_resume_continues_to_more_paths(tmp_path):
    """gpuart_cli --resume: 4 spp with --checkpoint, then --resume ... --spp 8 == a straight 8-spp run, bit for bit."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", "72", "--height", "40", "--mode", "pt"]
    ck, a, b = str(tmp_path / "r.ck"), str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    for args in (["--spp", "4", "--checkpoint", ck], ["--resume", ck, "--spp", "8", "--pfm", a], ["--spp", "8", "--pfm", b]):
        out = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
    assert '"paths_per_pixel": 8' in out.stdout
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.rccl
def test_rccl_gather_with_one_rank(B, be, O):
    """The gather of include/gpuart_hip.h on real RCCL, as far as one GPU allows: communicator of one rank (ncclGetUniqueId,
    ncclCommInitRank through dlopen; ncclCommCount / ncclCommUserRank read back), exchange of share + status (ncclAllGather), empty
    send/recv group, the root's export + row scatter into a device frame. Shares that do not cover every frame row exactly once
    are refused on every rank BEFORE anything is transferred (a share 1 of 3 alone; an empty share alone), and an empty share
    renders nothing without failing. The N > 1 transfers run on the driver's 8-GPU node; their host logic is covered by
    tests/test_sharding_gloo.py."""
    import torch
    W, H = 72, 40
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    with pytest.raises(B.HipError):
        be.comm_info()  # no communicator yet
    be.comm_init(1, 0, B.comm_unique_id())
    try:
        assert be.comm_info() == (1, 0)
        for bands in (8, 3):  # the whole frame as one share, in bands of 8 and of 3 rows
            share = B.share_of_rank(W, H, 0, 1, bands)
            be.set_share(share)
            g = be.get_share()
            assert (g.y0, g.th, g.band_rows, g.band_stride) == (0, H, bands, bands)
            be.pt_reset()
            for seed in O.randseeds(2):
                be.pt_pass(to_params(B, P), seed, 1)
            tile = be.read(1, 2.0)
            full = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            be.gather(1, 2.0, 0, full.data_ptr())
            be.wait(30000)
            assert_bits(full.cpu().numpy().reshape(-1, 4), tile.reshape(-1, 4), "gathered rows")
        full = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
        # a share that leaves rows to nobody: refused, nothing written
        be.set_share(B.share_of_rank(W, H, 1, 3))
        be.pt_reset()
        be.pt_pass(to_params(B, P), O.randseeds(1)[0], 1)
        with pytest.raises(B.HipError, match="belongs to no rank"):
            be.gather(1, 1.0, 0, full.data_ptr())
        be.finish()
        # the root without a frame buffer: its own verdict travels with its share, the call fails instead of hanging
        be.set_share(B.share_of_rank(W, H, 0, 1))
        with pytest.raises(B.HipError, match="frame buffer"):
            be.gather(1, 1.0, 0, 0)
        # an empty share (more ranks than bands): rendering is a no-op, the context stays usable
        be.resize(W, 8)
        be.set_share(B.share_of_rank(W, 8, 1, 2))
        assert be.get_share().th == 0
        be.pt_reset()
        be.pt_pass(to_params(B, P), O.randseeds(1)[0], 1)
        be.render_direct(to_params(B, P))
        be.finish()
        with pytest.raises(B.HipError, match="belongs to no rank"):
            be.gather(1, 1.0, 0, full.data_ptr())
        assert (full.cpu().numpy() == -7.0).all()
    finally:
        be.comm_destroy()
        be.resize(W, H)


@pytest.mark.rccl
def test_gather_gives_up_within_its_bound_and_the_context_survives(B, O, monkeypatch):
    """The exchange of the shares cannot complete (one GPU: the stream is held by gpuart_hip_test_stall, as a peer that never
    arrives would hold it): gpuart_hip_gather must come back with GPUART_HIP_ERR_TIMEOUT within GPUART_HIP_GATHER_TIMEOUT_MS — it
    used to copy the all-gathered table into a pageable vector on its own stack BEFORE the bounded wait, i.e. either block in that
    copy for ever or, giving up, leave a queued copy pointing at freed memory. The table now lives in pinned memory owned by the
    context: when the stall ends the queued exchange completes harmlessly, and the next gather works."""
    import time
    import torch
    monkeypatch.setenv("GPUART_HIP_GATHER_TIMEOUT_MS", "150")
    W, H = 72, 40
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene("box"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    b2 = B.Backend(0)
    try:
        b2.resize(W, H); b2.upload_bvh(tree); b2.set_camera(c)
        b2.comm_init(1, 0, B.comm_unique_id())
        b2.pt_reset()
        b2.pt_pass(to_params(B, P), O.randseeds(1)[0], 1)
        tile = b2.read(1)
        full = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        b2.test_stall(1500)
        t0 = time.perf_counter()
        with pytest.raises(B.HipError) as e:
            b2.gather(1, 1.0, 0, full.data_ptr())
        dt = time.perf_counter() - t0
        assert e.value.code == -4 and "not complete after 150 ms" in str(e.value), str(e.value)  # GPUART_HIP_ERR_TIMEOUT
        assert 0.14 < dt < 1.0, dt
        with pytest.raises(B.HipError) as e:
            b2.wait(100)  # still stalled: the bounded wait of gpuart_hip_wait says so too
        assert e.value.code == -4
        b2.wait(10000)    # the stall ends by itself; what the abandoned call had queued completes into the context's own table
        assert (full.cpu().numpy() == -7.0).all()  # nothing was transferred by the call that gave up
        b2.gather(1, 1.0, 0, full.data_ptr())
        b2.wait(10000)
        assert_bits(full.cpu().numpy().reshape(-1, 4), tile.reshape(-1, 4), "gather after a timed-out one")
    finally:
        b2.comm_destroy()
        b2.close()


def _run_cli(args, what, env=None, timeout=180):
    """gpuart_cli as a child process; a child that does not end is reported with what it had printed, not as a bare TimeoutExpired."""
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpuart_amd", "bin", "gpuart_cli")
    p = subprocess.Popen([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    try:
        out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        p.kill()
        out, err = p.communicate()
        raise AssertionError("gpuart_cli (%s) did not end within %d s; stdout: %s stderr: %s" % (what, timeout, out[-1500:], err[-3000:]))
    assert p.returncode == 0, "%s: %s" % (what, err[-3000:])
    return out


@pytest.mark.rccl
def test_headless_cli_gather_path(tmp_path):
    """gpuart_cli's multi-GPU read-out (Renderer::GatherRadiance -> gpuart_hip_gather_all over ncclCommInitAll) with the one
    rank a single-GPU box allows == the plain read-back."""
    base = ["--scene", "box", "--width", "72", "--height", "40", "--mode", "pt", "--spp", "3"]
    a, b = str(tmp_path / "a.pfm"), str(tmp_path / "b.pfm")
    _run_cli(base + ["--pfm", a], "plain read-back")
    # (NCCL_DEBUG=WARN: if RCCL's own initialisation ever stalls on a box, its messages are in the failure text)
    _run_cli(base + ["--pfm", b], "read-out through ncclCommInitAll + gpuart_hip_gather_all", env=dict(os.environ, GPUART_CLI_FORCE_GATHER="1", NCCL_DEBUG="WARN"))
    assert open(a, "rb").read() == open(b, "rb").read()


@pytest.mark.rccl
def test_frame_sharded_over_several_gpus_equals_the_single_gpu_frame(tmp_path):
    """Where the box has more than one GPU (the driver's 8-GPU node; a one-GPU box skips): gpuart_cli --gpus N renders one frame
    as N interleaved shares on N devices and gathers it through RCCL inside the library (ncclCommInitAll, share + status
    all-gather, grouped send / recv to the root, row scatter) — the PFM must equal the single-GPU one byte for byte. This is the
    only place where the N > 1 transfers of gpuart_hip_gather_all run under test."""
    import subprocess
    import torch
    n_dev = torch.cuda.device_count()
    if n_dev < 2:
        pytest.skip("one GPU: the multi-rank RCCL transfers need at least two devices")
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", "200", "--height", "136", "--mode", "pt", "--spp", "4"]
    one = str(tmp_path / "one.pfm")
    out = subprocess.run(base + ["--pfm", one], capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr
    for n in sorted({2, min(n_dev, 4), min(n_dev, 8)}):
        many = str(tmp_path / ("gpus%d.pfm" % n))
        out = subprocess.run(base + ["--gpus", str(n), "--pfm", many], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert open(one, "rb").read() == open(many, "rb").read(), "%d GPUs: the gathered frame differs from the single-GPU frame" % n


# ---- row N1 of SURVEY 8(f): the product's own loaders and scenes, on the GPU ------------------------------------------
def _loader_case(name, tmp_path):
    """(renderer.init_*(file written for it), camera selector) for a frames_<name>*.npz fixture."""
    if name == "cluster":
        path = str(tmp_path / "cluster_100k.dat"); S.write_lines(path, S.cluster_dat_lines())
        return (lambda r: r.init_cluster(path))
    if name == "tree":
        path = str(tmp_path / "tree1_21k.dat"); S.write_lines(path, S.tree_dat_lines())
        return (lambda r: r.init_tree(path))
    path = str(tmp_path / "dragon_stand_in.ply")
    model, faces = S.dragon_class_mesh()
    S.write_ply(path, model, faces)
    return (lambda r: r.init_dragon(path))


@pytest.mark.parametrize("fixture", ["frames_cluster_seg5", "frames_cluster_near_seg5", "frames_tree_seg5", "frames_tree_near_seg5", "frames_scene_d_seg5"])
def test_scenes_through_the_products_loaders_equal_the_reference_frames(B, fixture, tmp_path):
    """InitCluster / InitTree / InitDragon (csrc/host/scenes.cpp: file -> Utils::LoadPrimitives / LoadMeshFromPLY -> SetPrimitives ->
    BVH build, compile, upload) on the seeded stand-ins of the absent data files, rendered through the Renderer; direct lighting
    and the accumulated passes equal the frames the reference's GLSL produced on llvmpipe for the same scenes, bit for bit."""
    g = golden(fixture)
    name = str(g["scene"])
    W, H = int(g["W"]), int(g["H"])
    near = "_near" in fixture
    cam = dict(S.NEAR_CAMERAS[name] if near else S.BENCH_CAMERA if name == "scene_d" else S.DEFAULT_CAMERA)  # as make_golden.py chose them
    cam["dir"] = S.camera_dir(cam)
    init = _loader_case(name, tmp_path)
    r = B.Renderer(W, H, cam)
    try:
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        assert init(r) and r.is_ok()
        r.set_max_path_segments(int(g["max_segments"]))
        r.render_direct()
        check_frame(r.read_direct(), g["direct"], fixture + " direct")
        if "direct_nosun" in g:
            r.set_sun(S.SUN_AZIMUTH, S.SUN_ALTITUDE, direct=False)
            r.render_direct()
            check_frame(r.read_direct(), g["direct_nosun"], fixture + " direct, Sun off")
            r.set_sun(S.SUN_AZIMUTH, S.SUN_ALTITUDE, direct=True)
        r.set_seed(5489)
        r.restart_path_tracing(1, 2)
        assert r.path_tracing_pass() == 1
        check_frame(r.read_radiance(False), g["pt_pass1"], fixture + " pass 1")
        assert r.path_tracing_pass() == 2
        check_frame(r.read_radiance(False), g["pt_acc"], fixture + " accumulated")
        if "pt_3paths" in g:
            r.set_seed(5489)
            r.restart_path_tracing(3, 3)
            assert r.path_tracing_pass() == 3
            check_frame(r.read_radiance(False), g["pt_3paths"], fixture + " 3 paths per pass")
    finally:
        r.close()


def test_the_run_shape_that_faulted_in_round_2(B, be, O, dragon_1080p):
    """1080p, a plan of 20 passes, ten passes + flush, twice (gpurun_out/k20_plans.txt of round 2: a 10-pass run handed to lanes
    that hold 8 passes read past the path buffers). The planner (csrc/hip/run_planner.h, tests/test_run_planner.py) splits such a
    flush; the frame equals the oracle in a window, in the default mode and with k_run forced."""
    W, H, c, tree, P = dragon_1080p
    seeds = O.randseeds(20)
    x0, y0 = W // 2 - 32, H // 2
    exp = np.zeros((8, 64, 4), np.float32)
    for sd in seeds:
        O.pt_pass(tree, c, W, H, P, sd, 1, exp, tile=(x0, y0, 64, 8), nthreads=4)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    for mode in (0, 5):
        be.set_mode(mode)
        be.pt_reset()
        be.pt_plan(20)
        for half in range(2):
            for k in range(10):
                be.pt_pass(to_params(B, P), seeds[10 * half + k], 1)
            be.flush()
        acc = be.read(1)
        assert_bits(acc[y0:y0 + 8, x0:x0 + 64, :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "20 passes as 10 + 10, mode %d" % mode)
    be.set_mode(0)


def test_dragon871k_window_at_1080p(B, O):
    """The reference's largest scene at its size (src/main.cpp:321 "dragon 871k"; here the 871 200-triangle stand-in + floor disc,
    75 MB of tree — it no longer fits the L2s) through Renderer::SetPrimitives at BASELINE's frame size: two progressive passes,
    an oracle window in the middle of the mesh, whole-frame sanity. (The same tree at 128x72 against the reference's GLSL:
    frames_dragon871k_seg8 in test_frames_vs_reference_goldens.)"""
    W, H = 1920, 1080
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    descs = scene("dragon871k")
    r = B.Renderer(W, H, cam)
    try:
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(B.make_prims(descs))
        assert r.is_ok() and r.backend.scene_info()["prims"] == 871201
        r.set_max_path_segments(8)
        r.restart_path_tracing(1, 2)
        assert [r.path_tracing_pass() for _ in range(2)] == [1, 2]
        acc = r.read_radiance(False)
    finally:
        r.close()
    assert np.isfinite(acc[..., :3]).all() and acc[..., :3].min() >= 0
    tree, _ = O.build_bvh(descs)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    x0, y0 = W // 2 - 32, H // 2
    exp = np.zeros((16, 64, 4), np.float32)
    for sd in O.randseeds(2):
        O.pt_pass(tree, c, W, H, P, sd, 1, exp, tile=(x0, y0, 64, 16), nthreads=4)
    assert (exp[..., :3].sum(-1) > 0).mean() > 0.5
    assert_bits(acc[y0:y0 + 16, x0:x0 + 64, :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "871k-triangle scene, 1080p window")
