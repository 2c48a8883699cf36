"""The edge-aware denoiser (include/gpuart_denoise.h, libgpuart_denoise.so) and the device G-buffer that guides it (gpuart_hip_gbuffer):
the G-buffer against pick, the filter against its NumPy restatement (tests/denoise_ref.py) bit for bit, its quality on rendered frames,
Renderer::ReadDenoised, gpuart_cli --denoise and the argument checks."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import denoise_ref as R
from tests.util import assert_same_bits, default_camera, exported, filter_params_layout, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SPHERE = (-0.4, 0.0, 0.2, 0.25)   # a user sphere in view of the default camera
P_A = dict(iterations=3, lum_k=1.5, normal_pow2=2, depth_sigma=0.2)   # two non-default settings
P_B = dict(iterations=8, lum_k=0.0, normal_pow2=0, depth_sigma=1.0)


def _declared():
    return sorted(set(re.findall(r"\b(gpuart_denoise_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "gpuart_denoise.h")).read())))


def synthetic_gbuffer(rng, h, w):
    """(h, w, 8) record words and (h, w) ordinals of a made-up tile: surfaces of every type, sky, user-sphere pixels."""
    t = rng.integers(-1, 4, (h, w)).astype(np.int32)
    prims = rng.integers(0, 1000, (h, w)).astype(np.int32)
    us = (rng.random((h, w)) < 0.2) & (t >= 0)
    t[us] = 0
    prims[us] = -2
    prims[t < 0] = -1
    n = rng.normal(size=(h, w, 3))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    words = np.zeros((h, w, 8), np.float32)
    words[..., 0] = np.where(t >= 0, rng.uniform(0.5, 4.0, (h, w)), -1.0)
    words[..., 4:7] = np.where((t >= 0)[..., None], n, 0.0)
    words[..., 7] = t.view(np.float32)
    return words, prims


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_denoise_library_exports_exactly_its_header(lib):
    names = _declared()
    assert len(names) == 7, names
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_denoise.so")
    assert exported(path) == names
    # the filter knows nothing of the scene: it does not link the renderer's back end
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart_hip.so" not in dyn, dyn
    assert "gpuart_hip_gbuffer" in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so"))
    assert "gpuart_renderer_read_denoised" in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))


def test_params_record_matches_the_header(tmp_path):
    from gpuart_amd import binding as B
    got = filter_params_layout(tmp_path, "denoise")
    P = B.DenoiseParams
    assert got == [C.sizeof(P), P.iterations.offset, P.lum_k.offset, P.normal_pow2.offset, P.depth_sigma.offset, 8] == [16, 0, 4, 8, 12, 8]
    assert B.DENOISE_DEFAULTS == R.DEFAULTS


def test_restatement_passes_through_what_it_does_not_filter():
    """iterations = 0 is the identity; sky pixels always, and emissive or mirror user-sphere pixels, come out bit for bit as they went
    in (alpha everywhere); a diffuse or fuzzy user sphere is filtered like any surface."""
    from gpuart_amd import binding as B
    assert B.DENOISE_DEFAULTS == R.DEFAULTS   # the defaults the restatement assumes are the library's
    rng = np.random.default_rng(5)
    h, w = 23, 37
    words, prims = synthetic_gbuffer(rng, h, w)
    rgba = rng.uniform(0, 3, (h, w, 4)).astype(np.float32)
    assert same_bits(R.denoise(rgba, words, prims, 0, iterations=0), rgba)
    t = words[..., 7].view(np.int32)
    for flags in (0, R.EM_NONZERO, R.SPECULAR, R.EM_NONZERO | R.SPECULAR, 4):
        out = R.denoise(rgba, words, prims, flags, iterations=3)
        still = (t < 0) | ((prims == -2) & bool(flags & 3))
        assert same_bits(out[still], rgba[still]) and same_bits(out[..., 3], rgba[..., 3]), flags
        changed = ~(out[..., :3].view(np.uint32) == rgba[..., :3].view(np.uint32)).all(2)
        assert changed[~still].mean() > 0.9, flags
        assert changed[prims == -2].any() != bool(flags & 3), flags


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def dn(B):
    d = B.Denoiser(0)
    yield d
    d.close()


_TREES = {}


def tree(O, name):
    if name not in _TREES:
        _TREES[name] = O.build_bvh(scene(name))[0]
    return _TREES[name]


def camera(O, W, H):
    cam = default_camera()
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def frame(be, O, name, W, H):
    be.upload_bvh(tree(O, name))
    be.resize(W, H)
    be.set_camera(camera(O, W, H))


def tile_pixels(be):
    """The frame pixel of every tile pixel, in local order."""
    g = be.get_share()
    ly, lx = np.divmod(np.arange(g.tw * g.th), g.tw)
    return np.stack([g.x0 + lx, g.y0 + (ly // g.band_rows) * g.band_stride + ly % g.band_rows], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "scene_p", "scene_d", "tree"])
def test_gbuffer_equals_pick_of_every_tile_pixel(be, B, O, name):
    """Every type class, with and without the user sphere, on a full frame, a rectangular tile, share 1 of 3, 1x1 and 4K; the ledger of a
    gbuffer call is exactly the k_ray_query<T, RQ_PIXELS> that pick launches on the same scene."""
    from tests.test_kernel_variants import RQ_PIXELS, expected_kernels, names_of
    saw_sphere = False
    for W, H, geom in [(160, 120, "full"), (160, 120, "tile"), (160, 120, "share"), (1, 1, "full"), (3840, 2160, "full")]:
        frame(be, O, name, W, H)
        if geom == "tile":
            be.set_tile(21, 13, 37, 23)
        elif geom == "share":
            be.set_share(B.share_of_rank(W, H, 1, 3))
        xy = tile_pixels(be)
        _, _, tw, th = be.tile
        for us in (None, SPHERE):
            exp, ep = be.pick(xy, user_sphere=us, want_prims=True)
            hits, prims = be.gbuffer(user_sphere=us)
            assert hits.shape == (th, tw) and prims.shape == (th, tw)
            assert same_bits(hits.reshape(-1).view(np.float32), exp.view(np.float32)), (name, W, H, geom, us)
            assert (prims.reshape(-1) == ep).all(), (name, W, H, geom, us)
            saw_sphere |= bool((ep == -2).any())
    assert saw_sphere or name == "tree", "the user sphere is never in view"
    be.launched(reset=True)
    be.gbuffer(user_sphere=SPHERE)
    got = names_of(be.launched())
    assert [got] == expected_kernels("query", B.tree_class(tree(O, name)), source=RQ_PIXELS)[0], got
    be.pick(xy[:5], user_sphere=SPHERE)
    assert names_of(be.launched()) == got


@pytest.mark.gpu
def test_gbuffer_leaves_rendering_alone(B, O):
    """A G-buffer among collected passes: the accumulator, the counters and the timings' launch count are those of a run without it, and
    its records those of one made with nothing pending."""
    W, H = 96, 64
    c = camera(O, W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P0 = O.make_params(sun, S.SUN_ALTITUDE, True, SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    P = B.Params()
    C.memmove(C.byref(P), C.byref(P0), C.sizeof(P))
    seeds = O.randseeds(6)

    import torch
    us = (C.c_float * 4)(*SPHERE)

    def run(with_gbuffer):
        b = B.Backend(0)
        hits = torch.zeros((3, H, W, 8), device="cuda:0")
        prims = torch.zeros((3, H, W), dtype=torch.int32, device="cuda:0")
        try:
            b.resize(W, H); b.upload_bvh(tree(O, "scene_p")); b.set_camera(c)
            b.set_mode(4)
            b.pt_reset(); b.pt_plan(6)
            torch.cuda.synchronize()
            for k in range(6):
                b.pt_pass(P, seeds[k], 1)
                if with_gbuffer and k % 2 == 0:   # the C call alone: no finish between the passes
                    b._chk(b.L.gpuart_hip_gbuffer(b.ctx, us, C.c_void_p(hits[k // 2].data_ptr()), C.c_void_p(prims[k // 2].data_ptr())))
            acc = b.read(1)
            cnt = b.counters().as_dict()
            runs = b.kernel_time(0)[1]
            quiet = b.gbuffer(user_sphere=SPHERE)
            return acc, cnt, runs, (hits.cpu().numpy(), prims.cpu().numpy()), quiet
        finally:
            b.close()

    acc0, cnt0, n0, _, _ = run(False)
    acc1, cnt1, n1, gb, quiet = run(True)
    assert same_bits(acc0, acc1) and cnt0 == cnt1 and n0 == n1, (cnt0, cnt1, n0, n1)
    for k in range(3):
        assert same_bits(gb[0][k], quiet[0].view(np.float32).reshape(H, W, 8)) and (gb[1][k] == quiet[1]).all(), k


def rendered(be, B, O, name, W, H, passes, us_em=0.0, us_flags=0):
    """A normalised accumulator of `passes` one-path passes with SPHERE in view, and the tile's G-buffer."""
    frame(be, O, name, W, H)
    c = camera(O, W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P0 = O.make_params(sun, S.SUN_ALTITUDE, True, SPHERE, us_em, us_flags, float(c[12]), c[0:3], 5, 0.01)
    P = B.Params()
    C.memmove(C.byref(P), C.byref(P0), C.sizeof(P))
    be.pt_reset()
    for s in O.randseeds(passes, seed=77):
        be.pt_pass(P, s, 1)
    rgba = be.read(1, divide_by=float(passes))
    hits, prims = be.gbuffer(user_sphere=SPHERE)
    return rgba, hits, prims


def check_entry_points(dn, rgba, hits, prims, flags, params, what):
    """The host entry point and the device one (torch tensors) against the restatement."""
    import torch
    exp = R.denoise(rgba, hits, prims, flags, **dict(R.DEFAULTS, **(params or {})))
    got = dn.run(rgba, hits, prims, flags, params=params)
    assert_same_bits(got, exp, what + ", host")
    out = torch.full(rgba.shape, 7.0, device="cuda:0")
    res = dn.run(to_device(rgba), to_device(hits.view(np.float32).reshape(rgba.shape[:2] + (8,))), to_device(prims), flags, params=params, out=out)
    assert res is out
    assert_same_bits(out.cpu().numpy(), exp, what + ", torch")
    return exp


@pytest.mark.gpu
def test_denoiser_equals_the_restatement(be, dn, B, O):
    """Rendered and seeded random radiance over real G-buffers (the box with a diffuse, an emissive and a mirror user sphere; scene P), at
    1x1, 3x2, 37x23 and 160x120, for iterations 0 to 8 and two other settings, through the host and the device entry points."""
    rng = np.random.default_rng(1234)
    for name, em, flags in [("box", 0.0, 0), ("box", 3.0, R.EM_NONZERO), ("box", 0.0, R.SPECULAR), ("scene_p", 0.0, 0)]:
        for W, H in [(1, 1), (3, 2), (37, 23), (160, 120)]:
            rgba, hits, prims = rendered(be, B, O, name, W, H, 3, em, flags)
            noise = rng.uniform(0, 2, (H, W, 4)).astype(np.float32)
            for src, img in (("rendered", rgba), ("random", noise)):
                its = range(9) if W * H > 6 or src == "rendered" else (0, 5)
                for it in its:
                    check_entry_points(dn, img, hits, prims, flags, dict(iterations=it), "%s %dx%d %s flags %d iterations %d" % (name, W, H, src, flags, it))
                for p in (P_A, P_B):
                    check_entry_points(dn, img, hits, prims, flags, p, "%s %dx%d %s flags %d %s" % (name, W, H, src, flags, p))
            if W * H > 1000:
                assert (prims == -2).any() and (hits["type"] < 0).any()


@pytest.mark.gpu
def test_denoiser_at_1080p(be, dn, B, O):
    rgba, hits, prims = rendered(be, B, O, "scene_p", 1920, 1080, 2)
    exp = check_entry_points(dn, rgba, hits, prims, 0, None, "scene_p 1920x1080 defaults")
    assert not same_bits(exp, rgba)


def surface_rmse(img, ref, mask):
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt((d[mask] ** 2).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_denoising_cuts_the_error_of_low_sample_frames(B, name):
    """160x120, the default camera, the Sun on, no user sphere: against a 512-spp frame of another seed, the surface-pixel RMSE of the
    denoised 1-spp and 4-spp frames is at most 0.75x that of the raw ones."""
    W, H = 160, 120
    cam = default_camera()
    r = B.Renderer(W, H, cam)
    try:
        r.set_primitives(scene(name))
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0)
        r.set_seed(2)
        r.restart_path_tracing(64, 512)
        while r.path_tracing_pass() < 512:
            pass
        ref = r.read_radiance(True)
        y, x = np.divmod(np.arange(W * H), W)
        mask = (r.pick(np.stack([x, y], 1))["type"] >= 0).reshape(H, W)
        ratios = []
        for spp in (1, 4):
            r.set_seed(1234)
            r.restart_path_tracing(1, spp)
            while r.path_tracing_pass() < spp:
                pass
            raw, den = r.read_radiance(True), r.read_denoised()
            ratios.append(surface_rmse(den, ref, mask) / surface_rmse(raw, ref, mask))
        print("%s: denoised / raw surface RMSE at 1 and 4 spp: %.3f %.3f" % (name, ratios[0], ratios[1]))
        assert max(ratios) <= 0.75, ratios
    finally:
        r.close()


@pytest.mark.gpu
def test_read_denoised_filters_the_accumulator_and_leaves_it_alone(B):
    """Renderer.read_denoised = the restatement of read_radiance(normalized) with pick of every tile pixel; passes after it, the
    accumulator and the counters are those of a run without it. The G-buffer follows the user sphere, the camera and the tile."""
    W, H = 96, 64
    cam = default_camera()
    y, x = np.divmod(np.arange(W * H), W)
    xy = np.stack([x, y], 1)

    def expected(r, params=None, pixels=xy):
        _, _, tw, th = r.tile
        hits, prims = r.pick(pixels, want_prims=True)
        return R.denoise(r.read_radiance(True), hits, prims.reshape(th, tw), r.params().userSphereFlags, **dict(R.DEFAULTS, **(params or {})))

    def run(with_reads):
        r = B.Renderer(W, H, cam)
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
            r.backend.set_mode(4)
            r.restart_path_tracing(1, 12)
            for k in range(12):
                r.path_tracing_pass()
                if with_reads and k in (2, 7):
                    assert_same_bits(r.read_denoised(), expected(r), "read_denoised after %d passes" % (k + 1))
                    assert_same_bits(r.read_denoised(P_A), expected(r, P_A), "read_denoised, other parameters")
            return r.read_radiance(False), r.backend.counters().as_dict()
        finally:
            r.close()

    acc0, cnt0 = run(False)
    acc1, cnt1 = run(True)
    assert same_bits(acc0, acc1) and cnt0 == cnt1
    r = B.Renderer(W, H, cam)
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(SPHERE[:3], SPHERE[3], specular=True)
        r.restart_path_tracing(1, 4)
        for _ in range(4):
            r.path_tracing_pass()
        assert_same_bits(r.read_denoised(), expected(r), "mirror sphere")
        r.set_user_sphere((0.3, -0.2, 0.3), 0.3)   # the sphere moves: a new G-buffer
        r.path_tracing_pass()
        assert_same_bits(r.read_denoised(), expected(r), "moved sphere")
        cam2 = dict(cam, pos=(0.6, -2.5, 1.2))
        cam2["dir"] = S.camera_dir(cam2)
        r.set_camera(cam2)
        r.path_tracing_pass()
        assert_same_bits(r.read_denoised(), expected(r), "new camera")
        r.set_tile(10, 6, 40, 30)
        r.path_tracing_pass()
        ly, lx = np.divmod(np.arange(40 * 30), 40)
        assert_same_bits(r.read_denoised(), expected(r, pixels=np.stack([10 + lx, 6 + ly], 1)), "tile")
    finally:
        r.close()


@pytest.mark.gpu
def test_cli_writes_the_denoised_frame(B, tmp_path):
    """gpuart_cli --denoise --pfm: the restatement of the raw frame the same command writes without --denoise."""
    W, H = 64, 48
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    imgs = {}
    for tag, extra in (("raw", []), ("den", ["--denoise"])):
        pfm = str(tmp_path / (tag + ".pfm"))
        out = subprocess.run([exe, "--scene", "box", "--width", str(W), "--height", str(H), "--spp", "4", "--per-pass", "1",
                              "--user-sphere", "-0.4,0,0.2,0.25,2"] + extra + ["--pfm", pfm], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert json.loads(out.stdout.strip().splitlines()[-1])["paths_per_pixel"] == 4
        raw = open(pfm, "rb").read()
        head = b"PF\n%d %d\n-1.0\n" % (W, H)
        assert raw.startswith(head)
        imgs[tag] = np.frombuffer(raw[len(head):], np.float32).reshape(H, W, 3)
    # the CLI's camera looks at (0, 0, 0.95) from its default position; its user sphere is emissive
    cam = default_camera()
    r = B.Renderer(W, H, cam)
    try:
        r.init_box()
        r.set_user_sphere((-0.4, 0.0, 0.2), 0.25, emittance=2.0)
        y, x = np.divmod(np.arange(W * H), W)
        hits, prims = r.pick(np.stack([x, y], 1), want_prims=True)
    finally:
        r.close()
    rgba = np.concatenate([imgs["raw"], np.zeros((H, W, 1), np.float32)], 2)
    exp = R.denoise(rgba, hits, prims.reshape(H, W), R.EM_NONZERO)
    assert_same_bits(imgs["den"], exp[..., :3], "gpuart_cli --denoise")
    assert (prims == -2).any()


@pytest.mark.gpu
def test_argument_errors(be, dn, B, O):
    """Every ERR_ARG case of the denoiser and of the G-buffer returns the error with a message and writes nothing."""
    import torch
    L, LH = dn.L, be.L
    h, w = 4, 4
    rgba = np.ones((h * w + 1, 4), np.float32)
    hits = np.zeros((h * w + 1, 8), np.float32)
    prims = np.zeros(h * w + 2, np.int32)
    out = np.full((h * w + 1, 4), 7.0, np.float32)
    ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
    good = dict(rgba=ptr(rgba), hits=ptr(hits), prims=ptr(prims), w=w, h=h, p=None, out=ptr(out))

    def call(fn, **kw):
        a = dict(good, **kw)
        return getattr(L, fn)(dn.h, a["rgba"], a["hits"], a["prims"], C.c_uint32(0), C.c_uint32(a["w"]), C.c_uint32(a["h"]), a["p"], a["out"])

    nine = B.denoise_params(dict(iterations=9))
    cases = [("gpuart_denoise_run_host", dict(rgba=None), "NULL"), ("gpuart_denoise_run_host", dict(hits=None), "NULL"),
             ("gpuart_denoise_run_host", dict(prims=None), "NULL"), ("gpuart_denoise_run_host", dict(out=None), "NULL"),
             ("gpuart_denoise_run_host", dict(rgba=ptr(rgba, 2)), "misaligned"), ("gpuart_denoise_run_host", dict(prims=ptr(prims, 1)), "misaligned"),
             ("gpuart_denoise_run_host", dict(w=0), "bad size"), ("gpuart_denoise_run_host", dict(h=0), "bad size"),
             ("gpuart_denoise_run_host", dict(w=65537), "bad size"), ("gpuart_denoise_run_host", dict(p=C.byref(nine)), "iterations"),
             ("gpuart_denoise_run_host", dict(p=C.byref(B.denoise_params(dict(depth_sigma=0.0)))), "depth_sigma"),
             ("gpuart_denoise_run_host", dict(p=C.byref(B.denoise_params(dict(normal_pow2=17)))), "normal_pow2")]
    dev = [torch.zeros(h * w * 8 + 8, device="cuda:0") for _ in range(3)]
    dp = lambda t, k=0: C.c_void_p(t.data_ptr() + k)
    dgood = dict(rgba=dp(dev[0]), hits=dp(dev[1]), prims=dp(dev[2]), out=dp(dev[0]))
    cases += [("gpuart_denoise_run", dict(dgood, rgba=dp(dev[0], 4)), "misaligned"), ("gpuart_denoise_run", dict(dgood, hits=dp(dev[1], 8)), "misaligned"),
              ("gpuart_denoise_run", dict(dgood, out=dp(dev[0], 4)), "misaligned"), ("gpuart_denoise_run", dict(dgood, prims=dp(dev[2], 2)), "misaligned"),
              ("gpuart_denoise_run", dict(dgood, p=C.byref(nine)), "iterations"), ("gpuart_denoise_run", dict(dgood, w=0), "bad size")]
    for fn, kw, msg in cases:
        rc = call(fn, **kw)
        assert rc == ERR_ARG and msg in L.gpuart_denoise_last_error().decode(), (fn, kw, msg, rc, L.gpuart_denoise_last_error())
    assert (out == 7.0).all()
    assert call("gpuart_denoise_run_host") == 0 and not (out[:h * w] == 7.0).all() and (out[h * w] == 7.0).all()
    # the G-buffer: no scene, no frame size, no camera; NULL or misaligned pointers
    g = torch.zeros(64 * 64 * 8 + 8, device="cuda:0")
    us = (C.c_float * 4)(*SPHERE)
    fresh = B.Backend(0)
    try:
        gb = lambda b, hp, pp=None: LH.gpuart_hip_gbuffer(b.ctx, us, hp, pp)
        assert gb(fresh, dp(g)) == ERR_ARG and "no scene" in LH.gpuart_hip_last_error().decode()
        fresh.upload_bvh(tree(O, "box"))
        assert gb(fresh, dp(g)) == ERR_ARG and "frame size" in LH.gpuart_hip_last_error().decode()
        fresh.resize(8, 8)
        assert gb(fresh, dp(g)) == ERR_ARG and "camera" in LH.gpuart_hip_last_error().decode()
        fresh.set_camera(camera(O, 8, 8))
        for hp, pp in ((None, None), (dp(g, 4), None), (dp(g), dp(g, 2))):
            assert gb(fresh, hp, pp) == ERR_ARG, (hp, pp)
        assert (g == 0).all()
        assert gb(fresh, dp(g), dp(g, 8 * 8 * 32)) == 0
        fresh.finish()
        assert (g[:8 * 8 * 8] != 0).any()
    finally:
        fresh.close()
    # the Renderer: no scene
    cam = default_camera()
    r = B.Renderer(16, 8, cam)
    try:
        with pytest.raises(B.HipError):
            r.read_denoised()
        with pytest.raises(ValueError):
            r.read_denoised(dict(iterations=2, sigma=1))
    finally:
        r.close()
