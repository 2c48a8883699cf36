"""The variance-guided filter (include/gpuart_refine.h, libgpuart_refine.so): the library's boundary, the properties of its NumPy
restatement (tests/refine_ref.py), the kernels against the restatement bit for bit on synthetic tiles that take every branch and on
rendered frames, Renderer::ReadRefined, gpuart_cli --refine, the argument checks, and its quality on frames of 8 to 64 paths."""
import ctypes as C
import functools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import denoise_ref as D
from tests import filter_cases as FC
from tests import refine_ref as R
from tests import temporal_ref as T
from tests.test_denoise import synthetic_gbuffer
from tests.util import assert_same_bits, default_camera, exported, filter_params_layout, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
FLOOR = 20                  # every ledger entry over the synthetic case set (as tests/test_filter_edges.py)
LUM_FLOOR = 1.0 / 256
SPHERE = (-0.4, 0.0, 0.2, 0.25)   # a user sphere in view of the default camera
P_A = dict(iterations=3, lum_k=0.0, normal_pow2=2, depth_sigma=0.2)   # two non-default settings
P_B = dict(iterations=8, lum_k=1.5, normal_pow2=0, depth_sigma=1.0)   # (a step of 128: beyond every tile below but the 300s)
# one below, at and one above the 64 x 4 row block, several blocks, one pixel, one row, one column
SIZES = [(1, 1), (63, 3), (64, 4), (65, 5), (129, 9), (37, 23), (1, 300), (300, 1)]
BAD_E = (np.nan, np.inf, -np.inf)
# the bound of the quality test at 8 paths: (ratio tools/refine_quality.py measures on the CPU oracle for batches of 4 paths + 1) / 2
# (profiles/refine.txt section 1: box 0.522, scene P 0.762 with the default lum_k)
B_AT_8 = {"box": 0.761, "scene_p": 0.881}


def _declared():
    return sorted(set(re.findall(r"\b(gpuart_refine_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "gpuart_refine.h")).read())))


# ---- CPU: the library's boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_refine_library_exports_exactly_its_header(lib):
    names = _declared()
    assert len(names) == 7, names
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_refine.so")
    assert exported(path) == names
    # the filter knows nothing of the scene: it links the HIP runtime and not the renderer's back end
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart_hip.so" not in dyn and "libamdhip64" in dyn, dyn
    assert "gpuart_renderer_read_refined" in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    assert not [n for n in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so")) if "refine" in n]


def test_params_record_matches_the_header(tmp_path):
    from gpuart_amd import binding as B
    got = filter_params_layout(tmp_path, "refine")
    P = B.RefineParams
    assert got == [C.sizeof(P), P.iterations.offset, P.lum_k.offset, P.normal_pow2.offset, P.depth_sigma.offset, 8] == [16, 0, 4, 8, 12, 8]
    assert B.REFINE_DEFAULTS == R.DEFAULTS
    with pytest.raises(ValueError):
        B.refine_params(dict(iterations=2, sigma=1))


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_finish_of_no_handle_is_an_argument_error(lib):
    """gpuart_refine_finish(NULL) fails before any HIP call, with the library's own prefix."""
    L = C.CDLL(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_refine.so"))
    L.gpuart_refine_last_error.restype = C.c_char_p
    assert L.gpuart_refine_finish(None) == ERR_ARG
    assert L.gpuart_refine_last_error() == b"refine: handle is NULL"
    p = (C.c_uint32 * 4)()
    assert L.gpuart_refine_defaults(p) == 0 and L.gpuart_refine_defaults(None) == ERR_ARG
    got = np.frombuffer(bytes(p), np.uint32)
    assert (got[0], got[1:2].view(F)[0], got[2], got[3:4].view(F)[0]) == (R.DEFAULTS["iterations"], F(R.DEFAULTS["lum_k"]), R.DEFAULTS["normal_pow2"],
                                                                        F(R.DEFAULTS["depth_sigma"]))


# ---- CPU: the restatement's properties ---------------------------------------------------------------------------------------------
def synthetic_tile(seed=5, h=23, w=37):
    rng = np.random.default_rng(seed)
    words, prims = synthetic_gbuffer(rng, h, w)
    rgba = rng.uniform(0, 3, (h, w, 4)).astype(F)
    e = rng.uniform(0.01, 0.5, (h, w)).astype(F)
    return rgba, words, prims, e


def test_restatement_passes_through_what_it_does_not_filter():
    """iterations = 0 is the identity; pixels that are not surface pixels (for the five flag values of the denoiser's test) and pixels
    whose e is NaN, +inf or -inf come out bit for bit as they went in, alpha everywhere; and a pixel with such an e leaves every
    other pixel as a run in which it is sky does."""
    rgba, words, prims, e = synthetic_tile()
    assert same_bits(R.refine(rgba, words, prims, e, LUM_FLOOR, iterations=0), rgba)
    t = words[..., 7].view(np.int32)
    for flags in (0, D.EM_NONZERO, D.SPECULAR, D.EM_NONZERO | D.SPECULAR, 4):
        out = R.refine(rgba, words, prims, e, LUM_FLOOR, flags, iterations=3)
        still = (t < 0) | ((prims == -2) & bool(flags & 3))
        assert same_bits(out[still], rgba[still]) and same_bits(out[..., 3], rgba[..., 3]), flags
        changed = ~(out[..., :3].view(np.uint32) == rgba[..., :3].view(np.uint32)).all(2)
        assert changed[~still].mean() > 0.9, flags
        assert changed[prims == -2].any() != bool(flags & 3), flags
    surf = np.argwhere(t >= 0)
    rng = np.random.default_rng(6)
    for bad in BAD_E:
        spots = surf[rng.choice(len(surf), 40, replace=False)]
        e2 = e.copy()
        e2[spots[:, 0], spots[:, 1]] = bad
        out = R.refine(rgba, words, prims, e2, LUM_FLOOR, iterations=3)
        planted = np.zeros(t.shape, bool)
        planted[spots[:, 0], spots[:, 1]] = True
        assert same_bits(out[planted], rgba[planted]) and same_bits(out[..., 3], rgba[..., 3]), bad
        # the same tile with those pixels sky: no other pixel may tell the difference
        words2, prims2 = words.copy(), prims.copy()
        words2[planted, 7] = np.int32(-1).view(F)
        prims2[planted] = -1
        sky = R.refine(rgba, words2, prims2, e, LUM_FLOOR, iterations=3)
        assert same_bits(out[~planted], sky[~planted]), bad
        assert not same_bits(out, R.refine(rgba, words, prims, e, LUM_FLOOR, iterations=3))


def test_filter_tightens_as_the_error_falls():
    """The same tile with its error map scaled by 1, 1/4, 1/16 and 0: the mean absolute change of the valid pixels falls strictly from
    each scale to the next (with e = 0 only sd's 1e-4 is left)."""
    rng = np.random.default_rng(9)
    geom = T.full_frame(37, 23)
    words, prims = FC.plane_gbuffer(rng, FC.pinhole(FC.POS_0, 37, 23), geom)
    rgba = FC.radiance(rng, geom)
    e = rng.uniform(0.1, 0.5, (23, 37)).astype(F)
    valid = D.surface(words, prims, 0)[0]
    change = []
    for k in (1.0, 1 / 4, 1 / 16, 0.0):
        out = R.refine(rgba, words, prims, e * F(k), LUM_FLOOR)
        change.append(float(np.abs(out[..., :3].astype(np.float64) - rgba[..., :3])[valid].mean()))
    assert change[0] > change[1] > change[2] > change[3] >= 0, change


def plant(rng, rgba, words, prims, e):
    """What no rendered input holds, scattered over a tile (about 4 % of the pixels each): e of NaN, +inf, -inf, 0 and below 0; zero
    normals (den = 0); denormal colours; colours whose demodulated luminance is below every lum_floor used here."""
    h, w = e.shape
    r = rng.random((h, w))
    for k, bad in enumerate(BAD_E):
        e[(r >= 0.04 * k) & (r < 0.04 * (k + 1))] = bad
    e[(r >= 0.12) & (r < 0.16)] = 0
    e[(r >= 0.16) & (r < 0.20)] *= F(-1)
    words[(r >= 0.20) & (r < 0.24), 4:7] = 0
    m = (r >= 0.24) & (r < 0.28)
    rgba[m, :3] = rng.uniform(0, 1, (int(m.sum()), 3)).astype(F) * F(1e-39)
    m = (r >= 0.28) & (r < 0.32)
    rgba[m, :3] = rng.uniform(0, 1, (int(m.sum()), 3)).astype(F) * F(1e-4)


@functools.lru_cache(maxsize=None)
def cases():
    """-> list of dict(name, rgba, words, prims, error, lum_floor, flags, params, exp, ledger): every size with the defaults and the two
    other settings, the flags and the floor changing from case to case; and tests/filter_cases.py's edge G-buffer. The restatement
    runs once per case, here."""
    out = []

    def add(name, rgba, words, prims, e, lum_floor, flags, params):
        exp, led = R.refine(rgba, words, prims, e, lum_floor, flags, **dict(R.DEFAULTS, **(params or {})), want_ledger=True)
        for a in (rgba, words, prims, e, exp):
            a.setflags(write=False)
        out.append(dict(name=name, rgba=rgba, words=words, prims=prims, error=e, lum_floor=lum_floor, flags=flags, params=params, exp=exp, ledger=led))

    for i, (w, h) in enumerate(SIZES):
        rng = np.random.default_rng(500 + i)
        words, prims = synthetic_gbuffer(rng, h, w)
        rgba = rng.uniform(0, 3, (h, w, 4)).astype(F)
        e = rng.uniform(0.01, 0.5, (h, w)).astype(F)
        if w * h > 1:
            plant(rng, rgba, words, prims, e)
        for j, p in enumerate((None, P_A, P_B)):
            flags = (0, D.SPECULAR, D.EM_NONZERO)[(i + j) % 3]
            add("%d x %d, flags %d, %s" % (w, h, flags, p), rgba, words, prims, e, (LUM_FLOOR, 0.5)[(i + j) % 2], flags, p)
    rgba, words, prims = FC.edge_gbuffer(np.random.default_rng(11))
    rng = np.random.default_rng(12)
    e = rng.uniform(0.01, 0.5, rgba.shape[:2]).astype(F)
    e[rng.random(e.shape) < 0.05] = np.nan
    for it in (1, 2, 5):
        add("edges, iterations %d" % it, rgba, words, prims, e, LUM_FLOOR, 0, dict(iterations=it))
    return out


def total_ledger(cs):
    return {k: sum(c["ledger"][k] for c in cs) for k in R.LEDGER_KEYS}


def test_cases_take_every_branch():
    led = total_ledger(cases())
    print(led)
    assert set(led) == {"not_surface", "e_non_finite", "lum_below_floor", "pf_outside", "pf_invalid", "tap_outside", "tap_not_surface", "den_zero",
                        "denormal_state", "denormal_out"}
    assert all(v >= FLOOR for v in led.values()), led


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def rf(B):
    r = B.Refine(0)
    yield r
    r.close()


@pytest.fixture(autouse=True)
def bounded(request):
    """Every GPU test of this file runs as one phase of the library's watchdog (gpuart_hip_phase_begin): a test that hangs ends the
    process after two minutes instead of waiting for ever."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    from gpuart_amd import binding
    was = binding.phase_log(False)
    with binding.phase("tests/test_refine.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)


def check_entry_points(rf, rgba, words, prims, e, lum_floor, flags, params, exp, what):
    """The host entry point, the device one (torch tensors) into a separate output, and the device one in place, against `exp`."""
    import torch
    words = np.ascontiguousarray(words).view(F).reshape(rgba.shape[:2] + (8,))
    got = rf.run(rgba, words, prims, e, lum_floor, flags, params=params)
    assert_same_bits(got, exp, what + ", host")
    d = [to_device(a) for a in (rgba, words, prims, e)]
    out = torch.full(rgba.shape, 7.0, device="cuda:0")
    res = rf.run(d[0], d[1], d[2], d[3], lum_floor, flags, params=params, out=out)
    assert res is out
    assert_same_bits(out.cpu().numpy(), exp, what + ", device")
    assert_same_bits(d[0].cpu().numpy(), rgba, what + ", device: the input")
    rf.run(d[0], d[1], d[2], d[3], lum_floor, flags, params=params, out=d[0])
    assert_same_bits(d[0].cpu().numpy(), exp, what + ", device, in place")


@pytest.mark.gpu
def test_kernels_equal_the_restatement_on_synthetic_tiles(rf):
    cs = cases()
    led = total_ledger(cs)
    assert all(v >= FLOOR for v in led.values()), led
    for c in cs:
        check_entry_points(rf, c["rgba"], c["words"], c["prims"], c["error"], c["lum_floor"], c["flags"], c["params"], c["exp"], c["name"])
    c = cases()[-1]
    check_entry_points(rf, c["rgba"], c["words"], c["prims"], c["error"], c["lum_floor"], 0, dict(iterations=0), c["rgba"], "iterations 0")


def until(r, per_pass, cap, batch=4):
    """cap paths in batches of `batch` with a threshold nothing reaches."""
    r.restart_path_tracing(per_pass, cap)
    converged, s = r.render_until(0.0, 0.0, batch, LUM_FLOOR)
    assert not converged and s["total"] == cap and s["batches"] == cap // batch, s
    return s


def expected_refined(r, B, params=None):
    """The restatement on what the Renderer shows: the normalised accumulator, the tile's G-buffer and the error map."""
    hits, prims = r.backend.gbuffer(user_sphere=tuple(r.params().userSphere))
    e = r.read_error_map(LUM_FLOOR)
    return R.refine(r.read_radiance(True), hits, prims, e, LUM_FLOOR, r.params().userSphereFlags, **dict(R.DEFAULTS, **(params or {})))


@pytest.mark.gpu
def test_kernels_equal_the_restatement_on_rendered_frames(rf, B):
    """The box, 64 x 48, a diffuse user sphere, 4 batches of 4 paths: Refine.run on read_error_map and Backend.gbuffer through both entry
    points, and read_refined, equal the restatement; the same on a rectangular tile and on an interleaved share."""
    W, H = 64, 48
    r = B.Renderer(W, H, default_camera())
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(SPHERE[:3], SPHERE[3])
        for geom in ("full", "tile", "share"):
            if geom == "tile":
                assert r.set_tile(11, 7, 37, 23)
            elif geom == "share":
                assert r.set_interleaved_tile(0, 4, W, 16, 4, 12)
            until(r, 1, 16)
            rgba, e = r.read_radiance(True), r.read_error_map(LUM_FLOOR)
            hits, prims = r.backend.gbuffer(user_sphere=SPHERE)
            assert e.shape == prims.shape == rgba.shape[:2]
            for p in (None, P_A, P_B):
                exp = R.refine(rgba, hits, prims, e, LUM_FLOOR, 0, **dict(R.DEFAULTS, **(p or {})))
                check_entry_points(rf, rgba, hits, prims, e, LUM_FLOOR, 0, p, exp, "%s, %s" % (geom, p))
                assert_same_bits(r.read_refined(LUM_FLOOR, p), exp, "read_refined, %s, %s" % (geom, p))
            if geom == "full":
                assert (prims == -2).any() and (hits["type"] < 0).any() and not same_bits(exp, rgba)
    finally:
        r.close()


@pytest.mark.gpu
def test_refine_at_1080p(rf, B):
    """cfg3's scene and camera at 1920 x 1080, seeded random radiance and error map: 16 of the 64 x 4 blocks, two frame corners among
    them, equal the restatement on the block and the 67 pixels around it that five levels reach; the rest only has to finish."""
    import torch
    W, H, M = 1920, 1080, 67   # M = sum over the levels of 2 * 2^i + 1
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    try:
        be.upload_bvh(quads)
        be.resize(W, H)
        be.set_camera(B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H))
        hits = torch.empty((H, W, 8), dtype=torch.float32, device="cuda:0")
        prims = torch.empty((H, W), dtype=torch.int32, device="cuda:0")
        be.gbuffer(user_sphere=S.USER_SPHERE, out=hits, prims_out=prims)
    finally:
        be.close()
    rng = np.random.default_rng(3)
    rgba = rng.uniform(0, 2, (H, W, 4)).astype(F)
    e = rng.uniform(0.01, 0.3, (H, W)).astype(F)
    out = rf.run(to_device(rgba), hits, prims, to_device(e), LUM_FLOOR).cpu().numpy()
    words, prims = hits.cpu().numpy(), prims.cpu().numpy()
    surf = words[..., 7].view(np.int32) >= 0
    assert surf.any() and not same_bits(out, rgba)
    nbx, nby = W // 64, H // 4
    blocks = [(0, 0), (nbx - 1, nby - 1)] + [(int(rng.integers(0, nbx)), int(rng.integers(0, nby))) for _ in range(14)]
    for bx, by in blocks:
        x0, y0 = max(0, bx * 64 - M), max(0, by * 4 - M)
        x1, y1 = min(W, bx * 64 + 64 + M), min(H, by * 4 + 4 + M)
        exp = R.refine(rgba[y0:y1, x0:x1], words[y0:y1, x0:x1], prims[y0:y1, x0:x1], e[y0:y1, x0:x1], LUM_FLOOR)
        ys, xs = slice(by * 4 - y0, by * 4 - y0 + 4), slice(bx * 64 - x0, bx * 64 - x0 + 64)
        assert_same_bits(out[by * 4:by * 4 + 4, bx * 64:bx * 64 + 64], exp[ys, xs], "block (%d, %d)" % (bx, by))


@pytest.mark.gpu
def test_read_refined_filters_the_accumulator_and_leaves_everything_alone(B):
    """Renderer.read_refined = the restatement of read_radiance(normalized), the G-buffer and read_error_map. With and without such
    reads among the batches, the accumulator, the counters, the number of timed launches, RenderUntil's summaries, the error map, the
    denoised preview (its cached G-buffer) and the preview with the temporal history are the same. None before the second batch and
    after a restart."""
    W, H = 96, 64
    cam = default_camera()
    cam2 = dict(cam, pos=(0.6, -2.5, 1.2))
    cam2["dir"] = S.camera_dir(cam2)

    def run(with_reads):
        r = B.Renderer(W, H, cam)
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
            r.set_temporal_history(True)
            r.backend.set_mode(4)
            r.restart_path_tracing(1, 4)
            for _ in range(4):
                r.path_tracing_pass()
            if with_reads:
                assert r.read_refined(LUM_FLOOR) is None and r.read_error_map(LUM_FLOOR) is None   # no RenderUntil yet
            r.set_camera(cam2)   # commits the view to the history and restarts the accumulation
            r.restart_path_tracing(1, 12)
            for _ in range(4):
                r.path_tracing_pass()
            d0 = r.read_denoised()
            # the 4 paths so far are the first batch; a threshold everything meets stops after the second
            converged, s1 = r.render_until(1e30, 0.0, 4, LUM_FLOOR)
            assert converged and s1["total"] == 8 and s1["batches"] == 2
            if with_reads:
                assert_same_bits(r.read_refined(LUM_FLOOR), expected_refined(r, B), "read_refined after 8 paths")
                assert_same_bits(r.read_refined(LUM_FLOOR, P_B), expected_refined(r, B, P_B), "read_refined, other parameters")
            converged, s2 = r.render_until(0.0, 0.0, 4, LUM_FLOOR)
            assert not converged and s2["total"] == 12 and s2["batches"] == 3
            if with_reads:
                got = r.read_refined(LUM_FLOOR)
                assert_same_bits(got, expected_refined(r, B), "read_refined after 12 paths")
                assert not same_bits(got, r.read_radiance(True))
            res = (r.read_radiance(False), r.backend.counters().as_dict(), r.backend.kernel_time(0)[1], s1, s2, r.read_error_map(LUM_FLOOR), d0,
                   r.read_denoised(), r.read_preview())
            if with_reads:
                r.restart_path_tracing(1, 12)
                assert r.read_refined(LUM_FLOOR) is None
                r.path_tracing_pass()
                assert r.read_refined(LUM_FLOOR) is None
            return res
        finally:
            r.close()

    a, b = run(False), run(True)
    assert a[1:5] == b[1:5], (a[1:5], b[1:5])
    for k, what in ((0, "accumulator"), (5, "error map"), (6, "denoised before"), (7, "denoised after"), (8, "preview")):
        assert_same_bits(b[k], a[k], what)


def read_pfm(path, w, h):
    raw = open(path, "rb").read()
    head = b"PF\n%d %d\n-1.0\n" % (w, h)
    assert raw.startswith(head), raw[:32]
    return np.frombuffer(raw[len(head):], F).reshape(h, w, 3)


@pytest.mark.gpu
def test_cli_refine(B, tmp_path):
    """gpuart_cli --until ... --refine writes the bytes read_refined returns for the same render; --refine without --until, with
    --denoise or with --gpus 2 is refused with a message; a run that never reached two batches writes the raw frame and says so."""
    W, H = 64, 48
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", str(W), "--height", str(H), "--per-pass", "1", "--user-sphere", "-0.4,0,0.2,0.25,0"]
    unt = ["--until", "0", "--until-batch", "4", "--until-floor", "0.01"]
    pfm = str(tmp_path / "refined.pfm")
    out = subprocess.run(base + ["--spp", "12"] + unt + ["--refine", "--pfm", pfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert lines[0]["batches"] == 3 and lines[1]["paths_per_pixel"] == 12, lines
    # the CLI's camera looks at (0, 0, 0.95) from its default position
    r = B.Renderer(W, H, default_camera())
    try:
        r.init_box()
        r.set_user_sphere((-0.4, 0.0, 0.2), 0.25, emittance=0.0)
        r.restart_path_tracing(1, 12)
        assert r.render_until(0.0, 0.0, 4, 0.01)[1]["batches"] == 3
        exp = r.read_refined(0.01)
        assert not same_bits(exp, r.read_radiance(True))
        assert_same_bits(read_pfm(pfm, W, H), exp[..., :3], "gpuart_cli --refine")
        raw = r.read_radiance(True)
    finally:
        r.close()
    for extra, msg in ((["--spp", "8", "--refine"], "--until"), (["--spp", "8", "--refine", "--denoise"] + unt, "--denoise"),
                       (["--spp", "8", "--refine", "--gpus", "2"] + unt, "--until")):
        out = subprocess.run(base + extra + ["--pfm", pfm], capture_output=True, text=True, timeout=120)
        assert out.returncode != 0 and msg in out.stderr and "gpuart_cli:" in out.stderr and not out.stdout, (extra, out.returncode, out.stdout, out.stderr)
    # one batch reaches the cap: no estimate, the raw frame
    out = subprocess.run(base + ["--spp", "4"] + unt + ["--refine", "--pfm", pfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "raw frame" in out.stderr, (out.returncode, out.stderr)
    r = B.Renderer(W, H, default_camera())
    try:
        r.init_box()
        r.set_user_sphere((-0.4, 0.0, 0.2), 0.25, emittance=0.0)
        r.restart_path_tracing(1, 4)
        for _ in range(4):
            r.path_tracing_pass()
        raw = r.read_radiance(True)
    finally:
        r.close()
    assert_same_bits(read_pfm(pfm, W, H), raw[..., :3], "gpuart_cli --refine without an estimate")


@pytest.mark.gpu
def test_argument_errors(rf, B):
    """Every ERR_ARG rule of the header, once: the error, a message that names the rule, and nothing written to out."""
    import torch
    L = rf.L
    h, w = 4, 4
    rgba = np.ones((h * w + 1, 4), F)
    hits = np.zeros((h * w + 1, 8), F)
    prims = np.zeros(h * w + 2, np.int32)
    err = np.full(h * w + 2, 0.1, F)
    out = np.full((h * w + 1, 4), 7.0, F)
    ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
    good = dict(rgba=ptr(rgba), hits=ptr(hits), prims=ptr(prims), error=ptr(err), floor=LUM_FLOOR, w=w, h=h, p=None, out=ptr(out))

    def call(fn, **kw):
        a = dict(good, **kw)
        return getattr(L, fn)(rf.h, a["rgba"], a["hits"], a["prims"], C.c_uint32(0), a["error"], C.c_float(a["floor"]), C.c_uint32(a["w"]),
                              C.c_uint32(a["h"]), a["p"], a["out"])

    par = lambda **kw: C.byref(B.refine_params(kw))
    host = "gpuart_refine_run_host"
    cases = [(host, dict(rgba=None), "NULL"), (host, dict(hits=None), "NULL"), (host, dict(prims=None), "NULL"), (host, dict(error=None), "NULL"),
             (host, dict(out=None), "NULL"), (host, dict(rgba=ptr(rgba, 2)), "misaligned"), (host, dict(hits=ptr(hits, 2)), "misaligned"),
             (host, dict(out=ptr(out, 2)), "misaligned"), (host, dict(prims=ptr(prims, 1)), "misaligned"), (host, dict(error=ptr(err, 2)), "misaligned"),
             (host, dict(w=0), "bad size"), (host, dict(h=0), "bad size"), (host, dict(w=65537), "bad size"), (host, dict(h=65537), "bad size"),
             (host, dict(p=par(iterations=9)), "iterations"), (host, dict(p=par(lum_k=float("nan"))), "lum_k"), (host, dict(p=par(lum_k=float("inf"))), "lum_k"),
             (host, dict(p=par(lum_k=-0.5)), "lum_k"), (host, dict(p=par(depth_sigma=0.0)), "depth_sigma"),
             (host, dict(p=par(depth_sigma=float("inf"))), "depth_sigma"), (host, dict(p=par(normal_pow2=17)), "normal_pow2"),
             (host, dict(floor=0.0), "lum_floor"), (host, dict(floor=-1.0), "lum_floor"), (host, dict(floor=float("inf")), "lum_floor"),
             (host, dict(floor=float("nan")), "lum_floor")]
    dev = [torch.zeros(h * w * 8 + 8, device="cuda:0") for _ in range(4)]
    dout = torch.full((h * w * 4 + 8,), 7.0, device="cuda:0")
    dp = lambda t, k=0: C.c_void_p(t.data_ptr() + k)
    dgood = dict(rgba=dp(dev[0]), hits=dp(dev[1]), prims=dp(dev[2]), error=dp(dev[3]), out=dp(dout))
    run = "gpuart_refine_run"
    cases += [(run, dict(dgood, rgba=dp(dev[0], 4)), "misaligned"), (run, dict(dgood, hits=dp(dev[1], 8)), "misaligned"),
              (run, dict(dgood, out=dp(dout, 4)), "misaligned"), (run, dict(dgood, prims=dp(dev[2], 2)), "misaligned"),
              (run, dict(dgood, error=dp(dev[3], 2)), "misaligned"), (run, dict(dgood, p=par(iterations=9)), "iterations"),
              (run, dict(dgood, w=0), "bad size"), (run, dict(dgood, floor=0.0), "lum_floor")]
    for fn, kw, msg in cases:
        rc = call(fn, **kw)
        assert rc == ERR_ARG and msg in L.gpuart_refine_last_error().decode(), (fn, kw, msg, rc, L.gpuart_refine_last_error())
    assert getattr(L, host)(None, *([None] * 3), C.c_uint32(0), None, C.c_float(1), C.c_uint32(1), C.c_uint32(1), None, None) == ERR_ARG
    assert b"handle is NULL" in L.gpuart_refine_last_error()
    assert (out == 7.0).all() and bool((dout == 7.0).all())
    assert call(host) == 0 and not (out[:h * w] == 7.0).all() and (out[h * w] == 7.0).all()
    # the Renderer: unknown parameter names, parameters out of range
    r = B.Renderer(16, 8, default_camera())
    try:
        r.init_box()
        until(r, 1, 8)
        with pytest.raises(ValueError):
            r.read_refined(LUM_FLOOR, dict(iterations=2, sigma=1))
        assert r.read_refined(LUM_FLOOR, dict(iterations=9)) is None and r.read_refined(0.0) is None
        assert r.read_refined(LUM_FLOOR) is not None
    finally:
        r.close()


def surface_rmse(img, ref, mask):
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt((d[mask] ** 2).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_refining_never_hurts(B, name):
    """160 x 120, the default camera, the Sun on, no user sphere, against a 512-path frame of another seed: rendered in batches of 4
    paths, the surface-pixel RMSE of read_refined at 8, 16, 32 and 64 paths is at most that of the raw frame; at 32 and 64 paths it
    is below read_denoised's; at 8 paths it is at most B_AT_8 of the raw frame's."""
    W, H = 160, 120
    r = B.Renderer(W, H, default_camera())
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
        ratios = {}
        for paths in (8, 16, 32, 64):
            r.set_seed(1234)
            until(r, 4, paths)
            raw = surface_rmse(r.read_radiance(True), ref, mask)
            ratios[paths] = (surface_rmse(r.read_refined(LUM_FLOOR), ref, mask) / raw, surface_rmse(r.read_denoised(), ref, mask) / raw)
        print("%s: surface RMSE relative to the raw frame's, refined / denoised: %s; the bound at 8 paths: %.3f"
              % (name, ", ".join("%d paths %.3f / %.3f" % ((p,) + v) for p, v in ratios.items()), B_AT_8[name]))
        assert all(v[0] <= 1.0 for v in ratios.values()), ratios
        assert ratios[32][0] < ratios[32][1] and ratios[64][0] < ratios[64][1], ratios
        assert ratios[8][0] <= B_AT_8[name], ratios
    finally:
        r.close()
