"""The step of a path after a finished closest-hit query — path_tracing.glsl:182-233, then where the path goes and what is stored for it —
is one pair of device functions (kernels_pipeline.h segment_shade / segment_store) for k_shade and for k_gen where it shades segment 0
(GPUART_HIP_GEN_SHADE 1 and 2); k_run's PRODUCE keeps its own text of the same step; shadow_retire closes a Sun-shadow query for k_trace,
k_gen (level 2) and k_run. This holds them to each other directly: the same passes through the launch pipeline at every level of the knob
(mode 3), through the planner's choice (mode 0), through k_run (mode 5), through its counting form (mode 4) and through its reference-work
form (mode 1, which also asks the Sun-shadow queries whose answer cannot matter) give one accumulator, bit for bit — on every branch the
step can take. One case per branch is also held to the oracle: what all of them share, only a reference outside them can fault."""
import contextlib
import os

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.util import assert_bits

W, H = 67, 45   # ragged 8x8 blocks on both sides: padding slots sit inside the packets and the batches
NPATHS = 2      # the second path of a pass commits on top of what the first left in PathBuffers::color
NPASSES = 3     # one run of three interleaved passes
SPHERE = (0.1, -0.9, 0.75, 0.2)   # in front of the camera (tests/test_gen_shade.py)
# (mode, GPUART_HIP_GEN_SHADE): the launch pipeline at the three levels of the knob first — the others are compared with its level 0
CALLERS = [(3, "0"), (3, "1"), (3, "2"), (0, None), (5, None), (4, None), (1, None)]
SCENES = {"flat": lambda: S.scene_d(48, 48), "spheres": S.scene_p}


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        if value is not None:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old


@pytest.fixture(scope="module")
def stage(B, O):
    """name -> (camera, one context per caller with the scene uploaded, the tree): built once per scene, every case renders on them."""
    made = {}

    def get(name):
        if name not in made:
            tree, _ = O.build_bvh(SCENES[name]())
            cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
            c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
            ctxs = []
            made[name] = (c, ctxs, tree)
            for mode, knob in CALLERS:
                with _env("GPUART_HIP_GEN_SHADE", knob):   # read once, at create
                    b = B.Backend(0)
                ctxs.append(b)
                b.resize(W, H); b.upload_bvh(tree); b.set_camera(c)
                b.set_mode(mode)
        return made[name]

    yield get
    for _, ctxs, _ in made.values():
        for b in ctxs:
            b.close()


def _oracle_params(O, c, flags, sun_on, max_segments, min_weight=0.01):
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    return O.make_params(sun, S.SUN_ALTITUDE, sun_on, SPHERE, 3.0 if flags & 1 else 0.0, flags, float(c[12]), c[0:3], max_segments, min_weight)


def _params(B, O, c, *args, **kw):
    import ctypes as C
    op = _oracle_params(O, c, *args, **kw)
    p = B.Params()
    C.memmove(C.byref(p), C.byref(op), C.sizeof(p))
    return p


def _render(b, P, seeds):
    """(accumulator, segments counted) of the passes as one run on context b."""
    b.pt_reset()
    b.counters(reset=True)
    for s in seeds:
        b.pt_pass(P, s, NPATHS)
    b.flush()
    acc = b.read(1)[..., :3].copy()
    return acc, int(b.counters().segments)


def _callers_agree(stage, B, O, scene_name, what, *args, oracle=False, **kw):
    """Every caller's accumulator is mode 3's with the knob at 0 — and, with `oracle`, that one is the CPU restatement's: the callers
    share the step, so a mistake in it is common to them all and only a reference outside them sees it."""
    c, ctxs, tree = stage(scene_name)
    P = _params(B, O, c, *args, **kw)
    seeds = O.randseeds(NPASSES)
    outs = [_render(b, P, seeds) for b in ctxs]
    ref = outs[0][0]
    assert np.isfinite(ref).all() and ref.max() > 0, what
    if oracle:
        exp = np.zeros((H, W, 4), np.float32)
        for s in seeds:
            O.pt_pass(tree, c, W, H, _oracle_params(O, c, *args, **kw), s, NPATHS, exp, nthreads=8)
        assert_bits(ref.reshape(-1, 3), exp[..., :3].reshape(-1, 3), "%s %s: mode 3 with GPUART_HIP_GEN_SHADE=0 vs the oracle" % (scene_name, what))
    for (mode, knob), (got, _) in zip(CALLERS[1:], outs[1:]):
        assert_bits(got.reshape(-1, 3), ref.reshape(-1, 3),
                    "%s %s: mode %d%s vs mode 3 with GPUART_HIP_GEN_SHADE=0" % (scene_name, what, mode, " with GPUART_HIP_GEN_SHADE=" + knob if knob else ""))
    seg4, seg1 = outs[CALLERS.index((4, None))][1], outs[CALLERS.index((1, None))][1]
    assert seg4 == seg1 and seg4 > 0, "%s %s: mode 4 counted %d segments, mode 1 %d" % (scene_name, what, seg4, seg1)
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 1, 2, 6])   # diffuse, emissive (the path breaks at the sphere), mirror, fuzzy mirror
@pytest.mark.parametrize("scene_name", ["flat", "spheres"])
def test_every_caller_of_the_segment_step_gives_the_same_accumulator(stage, B, O, scene_name, flags):
    """Sun on and off x maxSegments 1 (no knob level applies: k_shade(0) alone), 2 (the survivors of segment 0 end at the bound) and 5."""
    frames = {}
    for sun_on in (True, False):
        for max_segments in (1, 2, 5):
            frames[sun_on, max_segments] = _callers_agree(stage, B, O, scene_name, "flags %d, sun %s, maxSegments %d" % (flags, sun_on, max_segments),
                                                          flags, sun_on, max_segments, oracle=sun_on and max_segments == 5)
    assert (frames[True, 5] != frames[False, 5]).any(), "the Sun term reaches the frame"
    assert (frames[True, 5] != frames[True, 1]).any(), "later segments reach the frame"


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", ["flat", "spheres"])
def test_every_caller_agrees_where_paths_end_by_weight_at_segment_zero(stage, B, O, scene_name):
    """minWeight 0.5: every albedo has a component of at most 0.5, so no path goes on after segment 0 although maxSegments is 5 — each ends
    with its Sun-shadow query (sun[slot].w = 1: the retire commits) or, where the Sun cannot matter, is committed by the step itself."""
    for flags in (0, 1):
        weight = _callers_agree(stage, B, O, scene_name, "flags %d, minWeight 0.5" % flags, flags, True, 5, min_weight=0.5, oracle=flags == 0)
        bound = _callers_agree(stage, B, O, scene_name, "flags %d, maxSegments 1" % flags, flags, True, 1)
        assert_bits(weight.reshape(-1, 3), bound.reshape(-1, 3), "%s: paths ended by weight vs by the segment bound" % scene_name)


@pytest.mark.gpu
def test_the_user_sphere_is_in_the_frame(stage, B, O):
    """What the flags select is seen: the emissive sphere's frame is not the diffuse one's, on either scene."""
    for scene_name in SCENES:
        c, ctxs, _ = stage(scene_name)
        seeds = O.randseeds(NPASSES)
        diffuse, _ = _render(ctxs[0], _params(B, O, c, 0, True, 5), seeds)
        emissive, _ = _render(ctxs[0], _params(B, O, c, 1, True, 5), seeds)
        assert (diffuse != emissive).any(-1).mean() > 0.01, scene_name
