"""Renderer::SetFireflyClamp (include/gpuart_despeckle.h through the host): with the switch on every filtered read and every temporal
commit takes the clamped frame — held to the chain of restatements over the renderer's own accumulator and G-buffer, bit for bit —
and nothing else sees a clamped value; with it off every read is what it was."""
import os
import subprocess

import numpy as np
import pytest

from tests import denoise_ref as D
from tests import despeckle_ref as DS
from tests import display_ref as DR
from tests import refine_ref as R
from tests import temporal_ref as T
from tests.test_moments import LUM_FLOOR, Shadow
from tests.test_temporal import TRACK, cam_dict
from tests.util import assert_same_bits, default_camera, same_bits, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
# name -> (user sphere, emittance): scene P with the small bright sphere of profiles/despeckle.txt, the box with tests/test_denoise.py's
SETUPS = {"scene_p": ((0.0, 0.0, 0.5, 0.1), 30.0), "box": ((-0.4, 0.0, 0.2, 0.25), 2.0)}
P_X = dict(radius=1, rank=2, k=1.5, floor=0.0, min_count=3)   # a non-default setting


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(autouse=True)
def bounded(request):
    """Every GPU test of this file runs as one phase of the library's watchdog (gpuart_hip_phase_begin): a test that hangs ends the
    process after two minutes instead of waiting for ever."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    from gpuart_amd import binding
    was = binding.phase_log(False)
    with binding.phase("tests/test_firefly_clamp.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)


def test_gpuart_cli_refuses_the_options_alone():
    """No device is needed for a usage error: --firefly-clamp without a filter, its options without it, and more than one GPU."""
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", "32", "--height", "24"]
    for args, said in ((["--firefly-clamp"], "give --denoise or --refine"), (["--denoise", "--firefly-k", "2"], "give --firefly-clamp"),
                       (["--denoise", "--firefly-rank", "2"], "give --firefly-clamp"), (["--denoise", "--firefly-clamp", "--gpus", "2"], "usage:")):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=60)
        assert bad.returncode == 2 and said in bad.stderr, (args, bad.returncode, bad.stderr)


def renderer(B, name, cam=None):
    r = B.Renderer(W, H, cam or default_camera())
    r.set_primitives(scene(name))
    us, em = SETUPS[name]
    r.set_user_sphere(us[:3], us[3], emittance=em)
    return r


def view_of(r):
    """(the normalised accumulator, hits, prims, userSphereFlags) of the renderer's view."""
    gp = r.params()
    hits, prims = r.backend.gbuffer(user_sphere=tuple(gp.userSphere))
    return r.read_radiance(True), hits, prims, gp.userSphereFlags


def clamped(r, params=None):
    """The restatement's clamp of the renderer's view -> (frame, hits, prims, flags, summary)."""
    rgba, hits, prims, flags = view_of(r)
    out, _, summary = DS.clamp(rgba, hits, prims, flags, **dict(DS.DEFAULTS, **(params or {})))
    return out, hits, prims, flags, summary


class ClampedShadow(Shadow):
    """tests/test_moments.py's restatement side of a Renderer with the history and its variance on, fed clamped frames."""

    def __init__(self, B, r, temporal=None, clamp=None):
        super().__init__(B, r, temporal)
        self.clamp = clamp

    def _inputs(self, cam):
        rgba, hits, prims, v, flags = super()._inputs(cam)
        if self.clamp is not None:
            rgba = DS.clamp(rgba, hits, prims, flags, **dict(DS.DEFAULTS, **self.clamp))[0]
        return rgba, hits, prims, v, flags

    def plain_preview(self, cam, spp):
        """read_preview: the radiance blend, then the denoiser."""
        rgba, hits, prims, v, flags = self._inputs(cam)
        x, _, _ = T.accumulate(self.hx, rgba, spp, hits, prims, v, **self.tp)
        return D.denoise(x, hits, prims, flags, **D.DEFAULTS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_p", "box"])
@pytest.mark.parametrize("paths", [2, 8])
def test_filtered_reads_take_the_clamped_frame(B, name, paths):
    """read_denoised = the denoiser's restatement of the clamp's restatement of read_radiance(normalized) with the tile's G-buffer;
    read_display of it the display restatement of that frame; firefly_summary the restatement's counts; other parameters reach the
    clamp; read_radiance and read_display("radiance") are what they are without the switch; switched off, read_denoised is today's."""
    r = renderer(B, name)
    try:
        r.restart_path_tracing(1, paths)
        for _ in range(paths):
            r.path_tracing_pass()
        raw, shown = r.read_radiance(True), r.read_display("radiance")
        assert r.firefly_summary() is None and not r.get_firefly_clamp()
        today = r.read_denoised()
        r.set_firefly_clamp(True)
        assert r.get_firefly_clamp()
        c, hits, prims, flags, summary = clamped(r)
        exp = D.denoise(c, hits, prims, flags, **D.DEFAULTS)
        assert_same_bits(r.read_denoised(), exp, "read_denoised")
        assert r.firefly_summary() == summary
        if name == "scene_p":   # (the scene with fireflies: the clamp has work)
            assert summary["clamped"] > 0 and not same_bits(exp, today), summary
        assert (r.read_display("denoised") == DR.encode(exp)).all()
        assert same_bits(r.read_radiance(True), raw) and (r.read_display("radiance") == shown).all()
        r.set_firefly_clamp(True, P_X)
        c, hits, prims, flags, summary = clamped(r, P_X)
        assert_same_bits(r.read_denoised(), D.denoise(c, hits, prims, flags, **D.DEFAULTS), "other parameters")
        assert r.firefly_summary() == summary
        with pytest.raises(ValueError):
            r.set_firefly_clamp(True, dict(rank=5))
        with pytest.raises(ValueError):
            r.set_firefly_clamp(True, dict(sigma=1))
        assert_same_bits(r.read_denoised(), D.denoise(c, hits, prims, flags, **D.DEFAULTS), "a refused setting changes nothing")
        r.set_firefly_clamp(False)
        assert_same_bits(r.read_denoised(), today, "switched off")
        assert same_bits(r.read_radiance(True), raw)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_p", "box"])
def test_read_refined_takes_the_clamped_frame(B, name):
    """Two batches of 4 paths: read_refined = the variance-guided filter's restatement of the clamped frame with read_error_map, which
    is the raw accumulator's (the estimate never sees a clamped value)."""
    r = renderer(B, name)
    try:
        r.restart_path_tracing(1, 8)
        converged, s = r.render_until(0.0, 0.0, 4, LUM_FLOOR)
        assert not converged and s["batches"] == 2
        e, today = r.read_error_map(LUM_FLOOR), r.read_refined(LUM_FLOOR)
        r.set_firefly_clamp(True)
        c, hits, prims, flags, summary = clamped(r)
        exp = R.refine(c, hits, prims, e, LUM_FLOOR, flags, **R.DEFAULTS)
        assert_same_bits(r.read_refined(LUM_FLOOR), exp, "read_refined")
        assert r.firefly_summary() == summary and same_bits(r.read_error_map(LUM_FLOOR), e)
        assert (r.read_display("refined", None, LUM_FLOOR) == DR.encode(exp)).all()
        if name == "scene_p":
            assert summary["clamped"] > 0 and not same_bits(exp, today), summary
        r.set_firefly_clamp(False)
        assert_same_bits(r.read_refined(LUM_FLOOR), today, "switched off")
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_p", "box"])
def test_the_history_takes_clamped_frames_and_the_switch_drops_it(B, name):
    """A three-view track, 2 paths per view, the history and its variance on: read_preview and read_guided_preview equal the
    restatements' chain fed clamped frames at every view. Changing the clamp's parameters, and switching it off, drops the history:
    the next preview is read_denoised, and with the switch off that is today's."""
    cams = [cam_dict(p) for p in TRACK[:3]]
    tparams = dict(max_history=8.0)
    r = renderer(B, name, cams[0])
    try:
        r.set_temporal_history(True, tparams)
        r.set_history_variance(True)
        r.set_firefly_clamp(True)
        sh = ClampedShadow(B, r, tparams, clamp={})
        r.restart_path_tracing(1, 2)
        for i, cam in enumerate(cams):
            if i:
                sh.commit(cams[i - 1], 2)
                r.set_camera(cam)
            r.path_tracing_pass(); r.path_tracing_pass()
            got = r.read_preview()
            assert_same_bits(got, sh.plain_preview(cam, 2), "read_preview, view %d" % i)
            assert_same_bits(r.read_guided_preview(LUM_FLOOR), sh.preview(cam, 2), "read_guided_preview, view %d" % i)
            if i:
                assert not same_bits(got, r.read_denoised())   # (the history is in it)
        unclamped = ClampedShadow(B, r, tparams)
        unclamped.hx, unclamped.hm = sh.hx, sh.hm
        assert not same_bits(r.read_preview(), unclamped.plain_preview(cams[2], 2))   # (and the clamp)
        r.set_firefly_clamp(True)                 # (the same setting again: the history stays)
        assert_same_bits(r.read_preview(), sh.plain_preview(cams[2], 2), "same setting")
        r.set_firefly_clamp(True, P_X)            # other parameters: the history has seen other inputs
        assert_same_bits(r.read_preview(), r.read_denoised(), "new parameters dropped the history")
        sh = ClampedShadow(B, r, tparams, clamp=P_X)
        sh.commit(cams[2], 2)
        r.set_camera(cams[1])
        r.path_tracing_pass(); r.path_tracing_pass()
        assert_same_bits(r.read_preview(), sh.plain_preview(cams[1], 2), "a new history with the new parameters")
        assert not same_bits(r.read_preview(), r.read_denoised())
        r.set_firefly_clamp(False)                # off: dropped again, and every read is today's
        rgba, hits, prims, flags = view_of(r)
        today = D.denoise(rgba, hits, prims, flags, **D.DEFAULTS)
        assert_same_bits(r.read_denoised(), today, "switched off: read_denoised")
        assert_same_bits(r.read_preview(), today, "switched off: no history")
        assert_same_bits(r.read_guided_preview(LUM_FLOOR), ClampedShadow(B, r, tparams).preview(cams[1], 2), "switched off: the guided preview")
    finally:
        r.close()


@pytest.mark.gpu
def test_the_switch_leaves_everything_else_alone(B):
    """A run with the switch never touched and one with it on and clamped reads among the passes: read_radiance, read_display of the
    radiance, the accumulator of the passes that follow, the counters, the timed launches, RenderUntil's summaries and the error map are
    the same; the G-buffer the second run cached is the first's (switched off at the end, its filtered reads are the first's)."""
    def run(on):
        r = renderer(B, "scene_p")
        try:
            if on:
                r.set_firefly_clamp(True)
            r.backend.set_mode(4)
            r.restart_path_tracing(1, 12)
            raw, filtered = [], []
            for k in range(4):
                r.path_tracing_pass()
                if k in (0, 3):
                    assert r.read_denoised() is not None
                    raw += [r.read_radiance(False), r.read_radiance(True)]
            converged, s1 = r.render_until(1e30, 0.0, 4, LUM_FLOOR)
            assert converged and s1["batches"] == 2
            assert r.read_refined(LUM_FLOOR) is not None and (not on or r.firefly_summary()["clamped"] > 0)
            raw += [r.read_radiance(False), r.read_error_map(LUM_FLOOR), r.read_display("radiance")]
            converged, s2 = r.render_until(0.0, 0.0, 4, LUM_FLOOR)
            assert not converged and s2["total"] == 12
            raw += [r.read_radiance(False), r.read_error_map(LUM_FLOOR)]
            if on:
                r.set_firefly_clamp(False)
            filtered += [r.read_denoised(), r.read_refined(LUM_FLOOR), r.read_preview(), r.read_display("denoised")]
            return raw, filtered, (r.backend.counters().as_dict(), r.backend.kernel_time(0)[1], s1, s2)
        finally:
            r.close()

    off, on = run(False), run(True)
    assert off[2] == on[2], (off[2], on[2])
    for k, (a, b) in enumerate(zip(off[0] + off[1], on[0] + on[1])):
        assert a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all(), "result %d" % k


@pytest.mark.gpu
def test_gpuart_cli_firefly_clamp(B, tmp_path):
    """gpuart_cli --denoise --firefly-clamp [--firefly-k K --firefly-rank R] writes the bytes the binding reads; the options alone are
    usage errors."""
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", str(W), "--height", str(H), "--spp", "4", "--per-pass", "1", "--seed", "7", "--user-sphere", "-0.4,0,0.2,0.25,2"]
    head = b"PF\n%d %d\n-1.0\n" % (W, H)
    imgs = []
    for k, extra in enumerate(([], ["--firefly-clamp"], ["--firefly-clamp", "--firefly-k", "1.5", "--firefly-rank", "2"])):
        pfm = str(tmp_path / ("f%d.pfm" % k))
        out = subprocess.run(base + ["--denoise"] + extra + ["--pfm", pfm], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        raw = open(pfm, "rb").read()
        assert raw.startswith(head)
        imgs.append(np.frombuffer(raw[len(head):], np.float32).reshape(H, W, 3))
    r = B.Renderer(W, H, default_camera())
    try:
        r.init_box()
        r.set_user_sphere((-0.4, 0.0, 0.2), 0.25, emittance=2.0)
        r.set_seed(7)
        r.restart_path_tracing(1, 4)
        for _ in range(4):
            r.path_tracing_pass()
        for img, params in zip(imgs, (False, None, dict(k=1.5, rank=2))):
            r.set_firefly_clamp(params is not False, params or None)
            assert_same_bits(img, r.read_denoised()[..., :3], "gpuart_cli, %s" % (params,))
    finally:
        r.close()
    assert not same_bits(imgs[0], imgs[1]) and not same_bits(imgs[1], imgs[2])
    for args in (["--firefly-clamp"], ["--denoise", "--firefly-k", "2"], ["--denoise", "--firefly-clamp", "--firefly-rank", "9"]):
        bad = subprocess.run(base + args, capture_output=True, text=True, timeout=120)
        assert bad.returncode in (1, 2) and "firefly" in bad.stderr, (args, bad.returncode, bad.stderr)
