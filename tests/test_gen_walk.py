"""k_gen walks the camera rays it generates (GPUART_HIP_GEN_WALK, kernels_pipeline.h k_gen, gpuart_hip.hip launch_run): where the camera
rays' k_trace launch would walk them as packets and a later k_trace launch follows in the run, the wave that computes 64 first rays walks
them from its registers and that launch is not made. The knob is a scheduling choice: 0 (the separate launch) and 1 must give the same
accumulator bit for bit — and the reference's, wherever a golden or the oracle says what that is. The frames run through the launch
pipeline (mode 3), on the goldens of tests/test_packet_walk.py at their sizes."""
import os
import re

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.util import assert_bits, frame_golden_params, golden, scene

KNOBS = ("0", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def params(B, op):
    import ctypes as C
    p = B.Params()
    C.memmove(C.byref(p), C.byref(op), C.sizeof(p))
    return p


def sun_params(O, cam, max_segments, sun_on=True):
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    return O.make_params(sun, S.SUN_ALTITUDE, sun_on, S.USER_SPHERE, 0.0, 0, float(cam[12]), cam[0:3], max_segments, 0.01)


def bench_camera(O, W, H):
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def render(B, monkeypatch, knob, tree, cam, W, H, P, runs, npaths=1, tile=None, interleaved=None, order=None, env=None):
    """The accumulator after the pass sequences `runs` (lists of seeds, each flushed as one run of interleaved passes) through the launch
    pipeline on a fresh context with GPUART_HIP_GEN_WALK = knob."""
    monkeypatch.setenv("GPUART_HIP_GEN_WALK", knob)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(cam)
        assert b.scene_order() == 1, "k_gen walks trees that are walked in the reference's order"
        if tile is not None:
            b.set_tile(*tile)
        if interleaved is not None:
            b.set_tile_interleaved(*interleaved)
        if order is not None:
            b.test_tile_order(order)
        b.set_mode(3)
        b.pt_reset()
        for seeds in runs:
            for s in seeds:
                b.pt_pass(params(B, P), s, npaths)
            b.flush()
        return b.read(1)[..., :3].copy()
    finally:
        b.close()


def both(B, monkeypatch, what, *args, expected=None, **kw):
    """Renders with the knob at 0 and at 1; the two frames are the same bits, a real picture, and `expected` if there is one."""
    outs = [render(B, monkeypatch, knob, *args, **kw) for knob in KNOBS]
    assert np.isfinite(outs[0]).all() and outs[0].max() > 0, what
    assert_bits(outs[1].reshape(-1, 3), outs[0].reshape(-1, 3), "%s, GPUART_HIP_GEN_WALK=1 vs 0" % what)
    if expected is not None:
        for knob, got in zip(KNOBS, outs):
            assert_bits(got.reshape(-1, 3), np.asarray(expected).reshape(-1, 3), "%s, GPUART_HIP_GEN_WALK=%s vs the reference" % (what, knob))
    return outs[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_tree_seg5"])   # flat, round, all types: every branch of k_gen's type switch
def test_gen_walk_equals_the_goldens(B, O, monkeypatch, name):
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    both(B, monkeypatch, name, tree, g["cam"], W, H, frame_golden_params(O, g)(True), [seeds], expected=g["pt_acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_gen_walk_keeps_the_phantom_hits(B, O, monkeypatch, k):
    """order_adversary_frame_k: a camera ray grazes a triangle, and the reference's order shows its phantom hit. k_gen's packet walks that order."""
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam, tree, seeds = g["cam"], g["tree"], g["seeds"]
    monkeypatch.delenv("GPUART_HIP_NEAREST_MIN_PRIMS", raising=False)
    both(B, monkeypatch, "adversary frame %d" % k, tree, cam, W, H, sun_params(O, cam, int(g["max_segments"])), [seeds[:1]], expected=g["pt_pass1"])


@pytest.mark.gpu
def test_gen_walk_on_a_tree_that_spills_the_ring(B, O, monkeypatch):
    """The 39-level sphere chain of tests/test_packet_walk.py (deeper than the LDS ring): k_gen's packet spills to the lane's spill area and comes back."""
    prims = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    c = O.camera((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5)
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, 1, acc)
    both(B, monkeypatch, "deep tree", tree, c, W, H, P, [seeds], expected=acc[..., :3])


@pytest.fixture(scope="module")
def scene_d(O):
    return O.build_bvh(scene("scene_d"))[0]


@pytest.mark.gpu
def test_gen_walk_on_ragged_frames(B, O, monkeypatch, scene_d):
    """101x67: neither side a multiple of 8, so padding slots sit inside k_gen's packets (against the oracle). 8x8: one block — with several
    passes a few packets, and most waves of the grid get nothing."""
    W, H = 101, 67
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(5)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(scene_d, c, W, H, P, s, 1, acc, nthreads=8)
    both(B, monkeypatch, "ragged frame", scene_d, c, W, H, P, [seeds], expected=acc[..., :3])
    W, H = 8, 8
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds[:3]:
        O.pt_pass(scene_d, c, W, H, P, s, 1, acc)
    both(B, monkeypatch, "8x8 frame", scene_d, c, W, H, P, [seeds[:3]], expected=acc[..., :3])


@pytest.mark.gpu
def test_gen_walk_on_tiles_shares_run_lengths_paths_and_birth_orders(B, O, monkeypatch, scene_d):
    """Scene D at 380x212: a rectangular tile; a share of interleaved row bands whose last band is ragged (rank 2 of 8: bands 2, 10, 18 and
    the four rows of band 26); runs of 1, 3 and 8 interleaved passes in one sequence; two paths per pixel (the j = 1 launch of k_gen); a
    permuted birth order of the 8x8 blocks (Frame::tile_order through the test hook)."""
    from gpuart_amd import sharding
    W, H = 380, 212
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(12)
    y0, n, band, stride, rows = sharding.interleaved_rows(2, 8, H)
    assert n % 8 == 4 and rows[-1] == H - 1, "the share's last band is ragged"
    full = both(B, monkeypatch, "runs of 1, 3 and 8 passes", scene_d, c, W, H, P, [seeds[:1], seeds[1:4], seeds[4:12]])
    one_by_one = render(B, monkeypatch, "1", scene_d, c, W, H, P, [[s] for s in seeds])
    assert_bits(one_by_one.reshape(-1, 3), full.reshape(-1, 3), "12 runs of one pass vs runs of 1, 3 and 8")
    both(B, monkeypatch, "tile", scene_d, c, W, H, P, [seeds[:3]], tile=(37, 21, 203, 117))
    share = both(B, monkeypatch, "share", scene_d, c, W, H, P, [seeds[:1], seeds[1:4], seeds[4:12]], interleaved=(0, y0, W, n, band, stride))
    assert_bits(share.reshape(-1, 3), full[rows].reshape(-1, 3), "the share's rows vs the full frame's")
    both(B, monkeypatch, "2 paths per pixel", scene_d, c, W, H, P, [seeds[:3]], npaths=2)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    order = np.random.RandomState(11).permutation(tiles)
    born = both(B, monkeypatch, "permuted birth order", scene_d, c, W, H, P, [seeds[:1], seeds[1:4], seeds[4:12]], order=order)
    assert_bits(born.reshape(-1, 3), full.reshape(-1, 3), "permuted birth order vs row-major")


@pytest.mark.gpu
def test_gen_walk_with_and_without_a_later_launch(B, O, monkeypatch):
    """Which sequence a run takes. Sun off, depth >= 2: k_gen walks, k_trace(1, -1) follows. Sun on, depth 1: k_gen walks, the Sun-shadow
    launch follows. Sun off, depth 1: the camera rays' launch would be the run's only BVH-query launch — today's sequence. maxSegments = 0:
    no segment at all, k_gen commits the paths. Against the oracle (Scene P, 96x64)."""
    tree, _ = O.build_bvh(scene("scene_p"))
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(3)
    for sun_on, depth in [(False, 4), (True, 1), (False, 1), (True, 0)]:
        P = sun_params(O, c, depth, sun_on)
        acc = np.zeros((H, W, 4), np.float32)
        for s in seeds:
            O.pt_pass(tree, c, W, H, P, s, 1, acc)
        both(B, monkeypatch, "sun %s, maxSegments %d" % (sun_on, depth), tree, c, W, H, P, [seeds], expected=acc[..., :3])


@pytest.mark.gpu
def test_gen_walk_takes_chunks_from_the_cursor(B, O, monkeypatch, scene_d):
    """One wave per CU and chunks of 64 slots on a 160x120 frame with 3 passes: 57 600 path slots, of which the waves' static first chunks
    cover CUs x 64 (a third of the slots at most on a device of up to 300 CUs; an MI355X has 256) — the rest comes through k_gen's cursor."""
    W, H = 160, 120
    assert W * H * 3 >= 3 * 300 * 64
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(3)
    env = {"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "64"}
    got = both(B, monkeypatch, "cursor path", scene_d, c, W, H, P, [seeds], env=env)
    monkeypatch.delenv("GPUART_HIP_WAVES_PER_CU"); monkeypatch.delenv("GPUART_HIP_CHUNK")
    assert_bits(render(B, monkeypatch, "1", scene_d, c, W, H, P, [seeds]).reshape(-1, 3), got.reshape(-1, 3), "default grid and chunk vs one wave per CU, chunks of 64")
    # chunks that are no multiple of 64: packets of 48
    assert_bits(render(B, monkeypatch, "1", scene_d, c, W, H, P, [seeds], env={"GPUART_HIP_CHUNK": "48"}).reshape(-1, 3), got.reshape(-1, 3), "chunks of 48")


@pytest.mark.gpu
def test_gen_walk_knob_is_clamped(B, O, monkeypatch):
    """Values beyond 0 / 1 are clamped like every GPUART_HIP_* knob's; none changes a bit."""
    g = golden("frames_scene_p_seg4")
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    for knob in ("7", "-3"):
        got = render(B, monkeypatch, knob, tree, g["cam"], W, H, frame_golden_params(O, g)(True), [seeds])
        assert_bits(got.reshape(-1, 3), g["pt_acc"].reshape(-1, 3), "GPUART_HIP_GEN_WALK=%s" % knob)


def test_gen_walk_knob_is_read_at_create_and_documented():
    """Without a device: the knob is parsed where the others are (gpuart_hip_create's env_u32: default 1, clamped to 0 .. 1) and listed in
    LAB_NOTES.md's knob table."""
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "hip", "gpuart_hip.hip")).read()
    create = src[src.index("int gpuart_hip_create("):src.index("int gpuart_hip_destroy(gpuart_hip_ctx *c) {")]
    assert re.search(r'c->gen_walk\s*=\s*env_u32\("GPUART_HIP_GEN_WALK",\s*1,\s*0,\s*1\)', create)
    assert src.count('"GPUART_HIP_GEN_WALK"') == 1, "read once, at create"
    notes = open(os.path.join(ROOT, "LAB_NOTES.md")).read()
    assert re.search(r"^\| `GPUART_HIP_GEN_WALK` \| 1 \|", notes, re.M)
