"""The G-buffer-guided upscaler: libgpuart_upscale.so against its NumPy restatement (tests/upscale_ref.py) bit for bit,
gpuart_hip_gbuffer_scaled against a context resized to the larger frame, and Renderer.read_upscaled / read_upscaled_display against
the composition of those pieces."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import display_ref as DR
from tests import upscale_cases as K
from tests import upscale_ref as U
from tests.util import assert_same_bits, exported, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
ENTRY_POINTS = ["gpuart_upscale_" + n for n in ("create", "defaults", "destroy", "finish", "last_error", "run", "run_host")]
NEW_HOST = ["gpuart_renderer_read_upscaled", "gpuart_renderer_read_upscaled_display"]
OTHER_LIBS = ("denoise", "temporal", "converge", "refine", "adaptive", "moments", "display", "antilag", "edges", "despeckle")
P_X = dict(normal_min=0.5, plane_tol=0.1)   # a non-default setting


def _declared(name):
    return sorted(set(re.findall(r"\b(gpuart_%s_[a-z_0-9]+)\s*\(" % name, open(os.path.join(ROOT, "include", "gpuart_%s.h" % name)).read())))


def ref(c, **params):
    return U.upscale(c["filtered"], c["words"], c["prims"], c["hi_words"], c["hi_prims"], c["scale"], c["flags"], **dict(U.DEFAULTS, **params))


# ---- CPU: the libraries' boundaries and the record ------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_libraries_export_the_new_entry_points(lib):
    assert _declared("upscale") == ENTRY_POINTS
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_upscale.so")
    assert exported(path) == ENTRY_POINTS
    # images alone: the HIP runtime, and neither the renderer's back end nor another image library
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart" not in dyn and "libamdhip64" in dyn, dyn
    hip = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so"))
    assert "gpuart_hip_gbuffer_scaled" in hip and not [n for n in hip if "upscale" in n]
    assert re.search(r"\bgpuart_hip_gbuffer_scaled\s*\(", open(os.path.join(ROOT, "include", "gpuart_hip.h")).read())
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    capi = open(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h")).read()
    for n in NEW_HOST:
        assert n in host and re.search(r"\b%s\s*\(" % n, capi), n
    for other in OTHER_LIBS:
        names = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % other))
        assert names == _declared(other), other


def test_params_record_and_defaults_match_the_header(tmp_path):
    from gpuart_amd import binding as B
    fields = ("normal_min", "plane_tol")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_upscale.h"\n#define P gpuart_upscale_params\n'
                   'int main(void) { printf("%%zu %s %%u %%u\\n", sizeof(P), %s, GPUART_UPSCALE_MIN_SCALE, GPUART_UPSCALE_MAX_SCALE); return 0; }\n'
                   % (" ".join(["%zu"] * len(fields)), ", ".join("offsetof(P, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Pm = B.UpscaleParams
    assert got[:3] == [C.sizeof(Pm)] + [getattr(Pm, f).offset for f in fields] == [8, 0, 4]
    assert tuple(range(got[3], got[4] + 1)) == U.SCALES == B.UPSCALE_SCALES == K.SCALES
    assert B.UPSCALE_DEFAULTS == U.DEFAULTS and tuple(U.DEFAULTS) == fields
    with pytest.raises(ValueError):
        B.upscale_params(dict(normal_min=0.5, sigma=1))
    hdr = open(os.path.join(ROOT, "include", "gpuart_upscale.h")).read()
    stated = ", ".join("%s %g" % (f, U.DEFAULTS[f]) for f in fields)
    assert hdr.count(stated) == 2, stated
    L = C.CDLL(os.path.join(ROOT, "gpuart_amd", "lib_test", "libgpuart_upscale.so"))
    p = Pm()
    assert L.gpuart_upscale_defaults(C.byref(p)) == 0 and L.gpuart_upscale_defaults(None) == ERR_ARG
    assert {f: getattr(p, f) for f in fields} == pytest.approx(U.DEFAULTS) and p.normal_min == F(U.DEFAULTS["normal_min"])


def test_the_header_keeps_edge_resolves_classes_and_match_word_for_word():
    def stated(name):
        text = open(os.path.join(ROOT, "include", "gpuart_%s.h" % name)).read()
        m = re.search(r"( \*   match\(a, b\), a record a against a centre record b:\n(?: \*     .*\n){3})", text)
        cls = re.search(r"( \*   sky      type < 0;\n \*   sphere .*\n)", text)
        assert m and cls, name
        return m.group(1), cls.group(1)
    assert stated("upscale") == stated("edges")


def test_cases_take_every_branch():
    """Over the synthetic cases every counter of the restatement's ledger is above zero, but one: candidate (0, 0) of the fallback
    cannot win. The containing low pixel c = (X / scale, Y / scale) is always one of the four taps, inside the tile, with wx >= 0.5
    and wy >= 0.5 (it is the tap nearest to the output pixel's centre in each direction), so w >= 0.25 > 0; a record that matches
    centre_c therefore has Wsum > 0 and never reaches the fallback. The candidate stays in the contract (it costs the rare path one
    test); its counter is asserted to be zero."""
    total = dict.fromkeys(U.LEDGER_KEYS, 0)
    for c in K.cases():
        out, led = U.upscale(c["filtered"], c["words"], c["prims"], c["hi_words"], c["hi_prims"], c["scale"], c["flags"], want_ledger=True)
        n = c["w"] * c["h"] * c["scale"] ** 2
        assert out.shape == (c["h"] * c["scale"], c["w"] * c["scale"], 4)
        assert led["weighted"] + sum(led["fallback_%d" % k] for k in range(9)) + led["fallback_none"] == n
        assert sum(led[k] for k in U.LEDGER_KEYS if k.startswith("tap_")) == 4 * n
        if c["scale"] == 3 and c["w"] > 1:   # X = 1 (mod 3): fx is an integer, ax = 0, and the tap to the right, if inside, has no weight
            assert led["tap_zero_weight"] > 0
        for k in total:
            total[k] += led[k]
    assert total.pop("fallback_0") == 0
    assert all(v > 0 for v in total.values()), total
    assert len(K.cases()) == len(K.TILES) * len(K.SCALES) and {c["flags"] for c in K.cases()} == {0, 1, 2}


def test_weights_of_scale_three_vanish_where_the_issue_says():
    x0, ax = U.tap_positions(12, 3)
    assert (ax[1::3] == 0).all() and (ax[0::3] > 0).all() and (ax[2::3] > 0).all()
    assert (x0[1::3] == np.arange(4)).all()
    for s in U.SCALES:   # the containing pixel is a tap, with at least half the weight
        x0, ax = U.tap_positions(8 * s, s)
        c = np.arange(8 * s) // s
        w_c = np.where(x0 == c, F(1) - ax, np.where(x0 + 1 == c, ax, F(-1)))
        assert (w_c >= 0.5).all(), s


def test_a_step_edge_comes_out_exact_where_bilinear_does_not():
    """Two surfaces meeting in a step edge, the low frame constant at a power of two on each, scale 2: the weights are 1/16, 3/16 and
    9/16, every product, sum and quotient is exact, and every output pixel equals its own surface's constant. Plain bilinear
    upsampling of the same frame does not."""
    c = K.step_edge()
    assert (c["hi_far"] != np.kron(c["far"], np.ones((2, 2), bool))).any()    # the edge cuts through a low pixel
    x0, ax = U.tap_positions(16, 2)
    assert set(np.unique(np.outer([F(1) - ax, ax], [F(1) - ax, ax]))) == {F(1 / 16), F(3 / 16), F(9 / 16)}
    out, led = U.upscale(c["filtered"], c["words"], c["prims"], c["hi_words"], c["hi_prims"], 2, want_ledger=True)
    exp = np.where(c["hi_far"], F(8), F(2))
    assert (out[..., :3] == exp[..., None]).all() and (out[..., 3] == 1).all()
    assert led["tap_fails_plane"] > 0 and led["weighted"] == exp.size
    plain = U.bilinear(c["filtered"], 2)
    wrong = (plain[..., 0] != exp)
    assert wrong.any() and (plain[..., 0][~wrong] == exp[~wrong]).all()
    assert wrong[:, 7:9].all() and not wrong[:, :7].any() and not wrong[:, 9:].any()   # the output columns whose two taps straddle the edge


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    import torch   # before the first handle: this file's first GPU test makes one before any tensor (module fixtures come before `bounded`)
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def up(B):
    h = B.Upscaler(0)
    yield h
    h.close()


@pytest.fixture(autouse=True)
def bounded(request):
    """Every GPU test of this file runs as one phase of the library's watchdog (gpuart_hip_phase_begin): a test that hangs ends the
    process after two minutes instead of waiting for ever. A device that no longer answers after a test ends the session: nothing more
    is started on it."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    import torch
    from gpuart_amd import binding
    was = binding.phase_log(False)
    with binding.phase("tests/test_upscale.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device failed after %s: %s" % (request.node.name, e), 3)


def run_both(up, c, params=None, what=""):
    """The library on device memory and on host memory against the restatement."""
    exp = ref(c, **(params or {}))
    dev = [to_device(c[k]) for k in ("filtered", "words", "prims", "hi_words", "hi_prims")]
    got = up.run(c["scale"], dev[0], dev[1], dev[2], dev[3], dev[4], c["flags"], params)
    assert_same_bits(got.cpu().numpy(), exp, what + " (device memory)")
    got = up.run(c["scale"], c["filtered"], c["words"], c["prims"], c["hi_words"], c["hi_prims"], c["flags"], params)
    assert_same_bits(got, exp, what + " (host memory)")
    return exp


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(K.TILES) * len(K.SCALES)))
def test_library_equals_the_restatement_on_synthetic_tiles(up, i):
    c = K.cases()[i]
    what = "%d x %d at scale %d, flags %d" % (c["w"], c["h"], c["scale"], c["flags"])
    exp = run_both(up, c, None, what)
    other = run_both(up, c, P_X, what + ", other parameters")
    if c["w"] > 1:
        assert not same_bits(exp, other), what


CAM = dict(S.DEFAULT_CAMERA, pos=(0.35, -3.05, 1.0))
CAM["dir"] = S.camera_dir(CAM)
SPHERE = (-0.4, 0.0, 0.2, 0.25)
USER_SPHERES = {"none": (None, 0), "diffuse": (SPHERE, 0), "emissive": (SPHERE, 1)}


def make_backend(B, O, name, W, H, tile=None):
    c = O.camera(CAM["pos"], CAM["dir"], CAM["up"], CAM["fov_y"], CAM["screen_dist"], W, H)
    tree, _ = O.build_bvh(scene(name))
    be = B.Backend(0)
    be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
    if tile is not None:
        be.set_tile(*tile)
    return be, c


def words_of(hits, prims):
    return np.ascontiguousarray(hits).view(F).reshape(prims.shape + (8,))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_library_equals_the_restatement_on_real_gbuffers(B, O, up, name):
    be, _ = make_backend(B, O, name, 40, 30)
    try:
        rng = np.random.default_rng(7)
        filtered = rng.uniform(0.01, 4.0, (30, 40, 4)).astype(F)
        for us_name, (us, flags) in USER_SPHERES.items():
            hits, prims = be.gbuffer(user_sphere=us)
            for s in K.SCALES:
                hh, hp = be.gbuffer_scaled(s, user_sphere=us)
                assert hp.shape == (30 * s, 40 * s)
                c = dict(filtered=filtered, words=words_of(hits, prims), prims=prims, hi_words=words_of(hh, hp), hi_prims=hp, scale=s, flags=flags)
                exp = run_both(up, c, None, "%s, user sphere %s, scale %d" % (name, us_name, s))
                assert not same_bits(exp, U.bilinear(filtered, s))
                if us is not None:
                    assert (hp == -2).any()
    finally:
        be.close()


@pytest.mark.gpu
def test_upscale_argument_errors(B, up):
    import torch
    c = K.case(5, 9, 4, 2, 1)
    w, h, s = 9, 4, 2
    f, words, prims, hw, hp = [to_device(c[k]) for k in ("filtered", "words", "prims", "hi_words", "hi_prims")]
    out = torch.full((h * s, w * s, 4), 7.0, device="cuda:0")
    host_out = np.full((h * s, w * s, 4), 7.0, F)
    L = up.L
    dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    pr = lambda **kw: C.byref(B.UpscaleParams(**dict(U.DEFAULTS, **kw)))
    null = C.c_void_p(0)

    def run(handle=up.h, s_=s, f_=None, hits=None, prims_=None, w_=w, h_=h, hh=None, hp_=None, pr_=None, out_=None):
        return L.gpuart_upscale_run(handle, s_, f_ if f_ is not None else dp(f), hits if hits is not None else dp(words),
                                    prims_ if prims_ is not None else dp(prims), w_, h_, hh if hh is not None else dp(hw),
                                    hp_ if hp_ is not None else dp(hp), 1, pr_, out_ if out_ is not None else dp(out))

    def run_host(s_=s, w_=w, pr_=None, out_=None):
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        return L.gpuart_upscale_run_host(up.h, s_, p(c["filtered"]), p(c["words"]), p(c["prims"]), w_, h, p(c["hi_words"]), p(c["hi_prims"]), 1, pr_,
                                         out_ if out_ is not None else p(host_out))
    assert run(handle=None) == ERR_ARG and b"handle is NULL" in L.gpuart_upscale_last_error()
    for bad in (0, 1, 5, 2 ** 32 - 1):
        assert run(s_=bad) == ERR_ARG and run_host(s_=bad) == ERR_ARG, bad
    assert b"scale" in L.gpuart_upscale_last_error()
    for k in ("f_", "hits", "prims_", "hh", "hp_", "out_"):
        assert run(**{k: null}) == ERR_ARG, k
    assert run(f_=dp(f, 4)) == ERR_ARG and run(hits=dp(words, 8)) == ERR_ARG and run(hh=dp(hw, 4)) == ERR_ARG and run(out_=dp(out, 4)) == ERR_ARG
    assert run(prims_=dp(prims, 2)) == ERR_ARG and run(hp_=dp(hp, 1)) == ERR_ARG
    assert b"misaligned" in L.gpuart_upscale_last_error()
    assert run_host(out_=C.c_void_p(host_out.ctypes.data + 2)) == ERR_ARG
    assert run(w_=0) == ERR_ARG and run(h_=0) == ERR_ARG and run_host(w_=0) == ERR_ARG
    assert run(w_=32769) == ERR_ARG and run(s_=4, h_=16385) == ERR_ARG and b"65536" in L.gpuart_upscale_last_error()
    for bad in (dict(normal_min=1.5), dict(normal_min=-1.5), dict(normal_min=float("nan")), dict(plane_tol=-1.0), dict(plane_tol=float("inf")),
                dict(plane_tol=float("nan"))):
        assert run(pr_=pr(**bad)) == ERR_ARG and run_host(pr_=pr(**bad)) == ERR_ARG, bad
    # out overlapping any input: one buffer holding out and, inside it, each input in turn
    both = torch.full((h * s * w * s * 4 + 64,), 7.0, device="cuda:0")
    for k in ("f_", "hits", "prims_", "hh", "hp_"):
        assert run(out_=dp(both), **{k: dp(both, 64)}) == ERR_ARG and b"overlaps" in L.gpuart_upscale_last_error(), k
    up.finish()
    assert (out == 7.0).all() and (both == 7.0).all() and (host_out == 7.0).all()
    assert run(pr_=None) == 0                       # NULL: the defaults
    up.finish()
    assert_same_bits(out.cpu().numpy(), ref(c), "after the refusals")


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,tile", [(40, 30, None), (40, 30, (7, 5, 21, 13)), (33, 17, None), (33, 17, (3, 1, 17, 9))])
def test_gbuffer_scaled_equals_the_gbuffer_of_a_resized_context(B, O, W, H, tile):
    be, cam = make_backend(B, O, "scene_p", W, H, tile)
    big = B.Backend(0)
    try:
        big.upload_bvh(O.build_bvh(scene("scene_p"))[0])
        for s in K.SCALES:
            big.resize(s * W, s * H)
            big.set_camera(cam)
            if tile is not None:
                big.set_tile(*[s * v for v in tile])
            for us in (None, SPHERE):
                eh, ep = big.gbuffer(user_sphere=us)
                gh, gp = be.gbuffer_scaled(s, user_sphere=us)
                what = "%d x %d, tile %s, scale %d, user sphere %s" % (W, H, tile, s, us)
                assert gp.shape == ep.shape and (gp == ep).all(), what
                assert_same_bits(words_of(gh, gp), words_of(eh, ep), what)
                assert (gp >= 0).any() and ((gp == -2).any() == (us is not None)), what
    finally:
        be.close()
        big.close()


@pytest.mark.gpu
def test_gbuffer_scaled_changes_nothing_else_and_checks_its_arguments(B, O):
    import torch
    from tests.test_gen_walk import params, sun_params
    seeds = O.randseeds(2)

    def run(scaled):
        be, cam = make_backend(B, O, "box", 40, 30, (7, 5, 21, 13))
        try:
            Pm = params(B, sun_params(O, cam, 5))
            be.set_mode(4)
            be.pt_reset()
            be.pt_pass(Pm, seeds[0], 1)
            first = be.gbuffer(user_sphere=SPHERE)
            be.pt_pass(Pm, seeds[1], 1)        # collected, not flushed by the query
            be.launched()
            if scaled:
                dev = torch.device("cuda", 0)
                for s, us in ((2, SPHERE), (3, None)):
                    hits = torch.empty((13 * s, 21 * s, 8), dtype=torch.float32, device=dev)
                    prims = torch.empty((13 * s, 21 * s), dtype=torch.int32, device=dev)
                    assert be.L.gpuart_hip_gbuffer_scaled(be.ctx, C.c_uint32(s), B._user_sphere(us), C.c_void_p(hits.data_ptr()),
                                                          C.c_void_p(prims.data_ptr())) == 0
                names = be.launched(reset=False)    # the query kernel alone
                assert names and all("k_ray_query" in n for n in names), names
                g = be.get_share()
                assert be.tile == (7, 5, 21, 13) and (g.W, g.H, g.x0, g.y0, g.tw, g.th) == (40, 30, 7, 5, 21, 13)
            second = be.gbuffer(user_sphere=SPHERE)
            be.finish()
            return first, second, be.read(1), be.counters().as_dict(), be.kernel_time(0)[1], be.launched()
        finally:
            be.close()

    plain, with_call = run(False), run(True)
    for a, b in ((plain[0], with_call[0]), (plain[1], with_call[1]), (plain[0], plain[1])):
        assert (a[1] == b[1]).all() and same_bits(words_of(*a), words_of(*b))
    assert same_bits(plain[2], with_call[2]) and plain[3:5] == with_call[3:5], (plain[3:5], with_call[3:5])
    assert plain[5] == with_call[5] and plain[3]["rays"] > 0, (plain[5], with_call[5])

    be, cam = make_backend(B, O, "box", 40, 30)
    try:
        hits = torch.full((30 * 4, 40 * 4, 8), 7.0, device="cuda:0")
        prims = torch.full((30 * 4, 40 * 4), 7, dtype=torch.int32, device="cuda:0")
        L, dp = be.L, lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        call = lambda s=2, h=None, p=None, ctx=be.ctx: L.gpuart_hip_gbuffer_scaled(ctx, C.c_uint32(s), None, h if h is not None else dp(hits),
                                                                                  p if p is not None else dp(prims))
        for s in (0, 1, 5, 2 ** 32 - 1):
            assert call(s) == ERR_ARG and b"scale" in L.gpuart_hip_last_error(), s
        null = C.c_void_p(0)
        assert call(ctx=None) == ERR_ARG and call(h=null) == ERR_ARG and call(p=null) == ERR_ARG
        assert call(h=dp(hits, 4)) == ERR_ARG and call(p=dp(prims, 2)) == ERR_ARG
        be.set_tile_interleaved(0, 0, 40, 16, 8, 16)          # two bands of 8 rows, 16 apart
        assert call() == ERR_ARG and b"interleaved" in L.gpuart_hip_last_error()
        be.set_tile_interleaved(0, 8, 40, 16, 8, 8)           # two bands, back to back: one rectangle
        assert call() == 0
        be.finish()
        exp = B.Backend(0)
        try:
            exp.resize(80, 60); exp.upload_bvh(O.build_bvh(scene("box"))[0]); exp.set_camera(cam); exp.set_tile(0, 16, 80, 32)
            eh, ep = exp.gbuffer()
        finally:
            exp.close()
        n = 80 * 32
        assert (prims.reshape(-1)[:n].cpu().numpy() == ep.reshape(-1)).all() and (prims.reshape(-1)[n:] == 7).all()
        assert same_bits(hits.reshape(-1, 8)[:n].cpu().numpy(), words_of(eh, ep).reshape(-1, 8)) and (hits.reshape(-1, 8)[n:] == 7.0).all()
        fresh = B.Backend(0)
        try:
            assert call(ctx=fresh.ctx) == ERR_ARG and b"no scene" in L.gpuart_hip_last_error()
            fresh.upload_bvh(O.build_bvh(scene("box"))[0])
            assert call(ctx=fresh.ctx) == ERR_ARG and b"no frame size" in L.gpuart_hip_last_error()
            fresh.resize(40, 30)
            assert call(ctx=fresh.ctx) == ERR_ARG and b"no camera" in L.gpuart_hip_last_error()
            fresh.resize(20000, 8)
            fresh.set_camera(cam)
            assert call(4, ctx=fresh.ctx) == ERR_ARG and b"65536" in L.gpuart_hip_last_error()
        finally:
            fresh.close()
    finally:
        be.close()


# ---- GPU: the Renderer -------------------------------------------------------------------------------------------------------------
def cam_at(x):
    cam = dict(S.DEFAULT_CAMERA, pos=(x, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    return cam


def composed(B, up, r, low, scale, params=None):
    """The pieces composed: the Upscaler on the low frame with the back end's two G-buffers for the renderer's user sphere."""
    gp = r.params()
    us = tuple(gp.userSphere)
    hits, prims = r.backend.gbuffer(user_sphere=us)
    hh, hp = r.backend.gbuffer_scaled(scale, user_sphere=us)
    return up.run(scale, low, words_of(hits, prims), prims, words_of(hh, hp), hp, gp.userSphereFlags, params)


def ray_queries(r):
    return [n for n in r.backend.launched() if "k_ray_query" in n]


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, (5, 3, 33, 17)])
def test_read_upscaled_equals_the_composition_of_the_pieces(B, up, tile):
    """Every source, at scales 2 and 3, with edge resolve off and on: read_upscaled is the Upscaler on what the plain read returns
    with edge resolve off, the display read is the display restatement of that, the plain reads with edge resolve on are what they
    were before the call, and the larger frame's G-buffer is made once per view, user sphere, scene and scale."""
    from tests.test_moments import LUM_FLOOR
    descs = scene("box")
    r = B.Renderer(48, 32, cam_at(0.35))
    try:
        r.set_primitives(descs)
        r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
        if tile:
            assert r.set_tile(*tile)
        r.set_temporal_history(True)
        r.set_history_variance(True)
        r.render_direct()
        r.restart_path_tracing(1, 8)
        for _ in range(2):
            r.path_tracing_pass()
        r.set_camera(cam_at(0.40))                 # a commit: the previews have a history to blend
        r.restart_path_tracing(1, 8)
        r.render_direct()
        converged, summary = r.render_until(1e30, 0.0, 2, LUM_FLOOR)
        assert converged and summary["batches"] == 2
        reads = {"radiance": lambda: r.read_radiance(True), "direct": r.read_direct, "denoised": r.read_denoised, "preview": r.read_preview,
                 "guided_preview": lambda: r.read_guided_preview(LUM_FLOOR), "refined": lambda: r.read_refined(LUM_FLOOR)}
        assert set(reads) == set(B.DISPLAY_SOURCES)
        th, tw = r.tile[3], r.tile[2]
        low = {k: f() for k, f in reads.items()}
        exp = {}
        for k in reads:
            for s in (2, 3):
                exp[k, s] = composed(B, up, r, low[k], s)
                got = r.read_upscaled(k, s, LUM_FLOOR)
                assert got.shape == (s * th, s * tw, 4)
                assert_same_bits(got, exp[k, s], "%s at scale %d" % (k, s))
                assert (r.read_upscaled_display(k, s, None, LUM_FLOOR) == DR.encode(exp[k, s])).all(), (k, s)
        assert not same_bits(exp["denoised", 2], U.bilinear(low["denoised"], 2))
        assert_same_bits(r.read_upscaled("denoised", 2, LUM_FLOOR, P_X), composed(B, up, r, low["denoised"], 2, P_X), "other parameters")
        for k in reads:                             # the reads in between changed nothing
            assert_same_bits(reads[k](), low[k], k + " after the upscaled reads")

        # edge resolve on: skipped for the upscaled reads, as ever for the others
        r.set_edge_resolve(True)
        resolved = {k: f() for k, f in reads.items()}
        assert not same_bits(resolved["denoised"], low["denoised"])
        for k in reads:
            assert_same_bits(r.read_upscaled(k, 2, LUM_FLOOR), exp[k, 2], k + " with edge resolve on")
            assert_same_bits(reads[k](), resolved[k], k + " after it")
        assert r.get_edge_resolve()
        r.set_edge_resolve(False)

        # the cache of the larger frame's G-buffer
        r.read_upscaled("denoised", 2)
        r.backend.launched()
        assert_same_bits(r.read_upscaled("denoised", 2), exp["denoised", 2], "the same view again")
        assert_same_bits(r.read_upscaled("radiance", 2), exp["radiance", 2], "another source of the same view")
        assert not ray_queries(r)

        def once(what, scale=2, source="denoised"):
            """After the low G-buffer has been made again by a plain read, an upscaled read launches the query kernel; the next does not."""
            lo = reads[source]()
            r.backend.launched()
            got = r.read_upscaled(source, scale)
            assert ray_queries(r), what
            assert_same_bits(got, composed(B, up, r, lo, scale), what)
            r.backend.launched()
            assert_same_bits(r.read_upscaled(source, scale), got, what + ", cached")
            assert not ray_queries(r), what

        once("a change of scale", 3)
        once("the scale changed back")
        r.set_camera(cam_at(0.45))
        r.path_tracing_pass()
        once("after SetCamera")
        r.set_user_sphere_pos((-0.2, 0.1, 0.3))
        r.path_tracing_pass()
        once("after SetUserSpherePos")
        assert r.update_primitives([0], [descs[0]])
        r.path_tracing_pass()
        once("after UpdatePrimitives")
    finally:
        r.close()


@pytest.mark.gpu
def test_read_upscaled_refusals(B):
    r = B.Renderer(48, 32, cam_at(0.35))
    try:
        r.set_primitives(scene("box"))
        r.restart_path_tracing(1, 4)
        r.path_tracing_pass()
        before = r.read_denoised()
        r.backend.launched()
        for s in (0, 1, 5):
            assert r.read_upscaled("denoised", s) is None and r.read_upscaled_display("denoised", s) is None
        assert r.read_upscaled("denoised", 2, params=dict(normal_min=2.0)) is None
        assert r.read_upscaled("refined", 2) is None            # no estimate yet: read_refined gives None
        assert r.read_upscaled(17, 2) is None
        assert r.set_interleaved_tile(0, 8, 48, 16, 8, 16)
        r.path_tracing_pass()
        r.backend.launched()
        assert r.read_upscaled("denoised", 2) is None and r.read_upscaled_display("radiance", 2) is None
        assert not r.backend.launched()
        assert r.read_denoised() is not None
        assert r.set_tile(0, 0, 48, 32)
        r.restart_path_tracing(1, 4)
        r.path_tracing_pass()
        assert r.read_denoised().shape == before.shape
        assert r.read_upscaled("denoised", 4).shape == (128, 192, 4)
    finally:
        r.close()


@pytest.mark.gpu
def test_gpuart_cli_upscale(tmp_path):
    cli = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [cli, "--scene", "box", "--width", "48", "--height", "32", "--spp", "2", "--denoise"]

    def ppm(path):
        data = open(path, "rb").read()
        head = data.split(b"\n", 3)
        return tuple(int(v) for v in head[1].split()), head[3]
    small, big = str(tmp_path / "small.ppm"), str(tmp_path / "big.ppm")
    subprocess.run(base + ["--display", small], check=True, capture_output=True, timeout=120)
    subprocess.run(base + ["--display", big, "--upscale", "2"], check=True, capture_output=True, timeout=120)
    assert ppm(small)[0] == (48, 32) and ppm(big)[0] == (96, 64) and len(ppm(big)[1]) == 96 * 64 * 3
    for bad in (["--upscale", "2"], ["--display", big, "--upscale", "5"], ["--display", big, "--upscale", "2", "--gpus", "2"]):
        p = subprocess.run(base + bad, capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "--upscale" in p.stderr, (bad, p.stderr)
