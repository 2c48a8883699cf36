"""Packet walks in k_trace (GPUART_HIP_PACKET, device_scene.h trav_packet): a wave walks the camera rays (1) and also the Sun-shadow rays of
segment 0 (2) as packets of 64 through one walk of the tree in the reference's order. The knob is a scheduling choice: every value must
give bit-identical accumulators, equal to the reference's. The frames run through the launch pipeline (mode 3: k_trace, whatever the
length of the pass sequence); the GD_REF_ORDER kernels are the flat (Scene D), round (Scene P, the cluster, the deep sphere chain) and
all-types (the tree) ones."""
import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.util import assert_bits, frame_golden_params, golden, scene

pytestmark = pytest.mark.gpu

KNOBS = ("0", "1", "2")


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


def render(B, monkeypatch, knob, tree, cam, W, H, P, seeds, npaths=1, tile=None, interleaved=None):
    """The accumulator after len(seeds) passes through the launch pipeline on a fresh context with GPUART_HIP_PACKET = knob."""
    monkeypatch.setenv("GPUART_HIP_PACKET", knob)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(cam)
        assert b.scene_order() == 1, "the packet walk is for trees walked in the reference's order"
        if tile is not None:
            b.set_tile(*tile)
        if interleaved is not None:
            b.set_tile_interleaved(*interleaved)
        b.set_mode(3)
        b.pt_reset()
        for s in seeds:
            b.pt_pass(params(B, P), s, npaths)
        return b.read(1)[..., :3].copy()
    finally:
        b.close()


@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_cluster_seg5", "frames_tree_seg5"])
@pytest.mark.parametrize("sun_on", [True, False])
def test_packet_walks_equal_the_goldens(B, O, monkeypatch, name, sun_on):
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    P = frame_golden_params(O, g)(sun_on)
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    if sun_on:
        exp = g["pt_acc"].reshape(-1, 3)
    else:
        acc = np.zeros((H, W, 4), np.float32)
        for s in seeds:
            O.pt_pass(tree, g["cam"], W, H, P, s, 1, acc, nthreads=8)
        exp = acc[..., :3].reshape(-1, 3)
    for knob in KNOBS:
        got = render(B, monkeypatch, knob, tree, g["cam"], W, H, P, seeds)
        assert_bits(got.reshape(-1, 3), exp, "%s, sun %s, GPUART_HIP_PACKET=%s" % (name, sun_on, knob))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_packet_walks_keep_the_phantom_hits(B, O, monkeypatch, k):
    """order_adversary_frame_k: a camera ray grazes a triangle, and the reference's order shows its phantom hit. A packet walks that order."""
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam, tree, seeds = g["cam"], g["tree"], g["seeds"]
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(cam[12]), cam[0:3], int(g["max_segments"]), 0.01)
    monkeypatch.delenv("GPUART_HIP_NEAREST_MIN_PRIMS", raising=False)
    for knob in KNOBS:
        got = render(B, monkeypatch, knob, tree, cam, W, H, P, seeds[:1])
        assert_bits(got.reshape(-1, 3), g["pt_pass1"].reshape(-1, 3), "adversary frame %d, GPUART_HIP_PACKET=%s" % (k, knob))


def test_packet_walks_on_a_tree_that_spills_the_ring(B, O, monkeypatch):
    """A 39-level sphere chain within 2^20 (deeper than the LDS ring; fast-form boxes): a packet's stack spills to global memory and comes back."""
    prims = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    c = O.camera((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, 1, acc)
    for knob in KNOBS:
        got = render(B, monkeypatch, knob, tree, c, W, H, P, seeds)
        assert_bits(got.reshape(-1, 3), acc[..., :3].reshape(-1, 3), "deep tree, GPUART_HIP_PACKET=%s" % knob)


def test_packet_walks_on_ragged_frames_tiles_and_shares(B, O, monkeypatch):
    """Scene D: a ragged frame (padding slots; query counts that are not multiples of 64), a rectangular tile and a share of interleaved
    row bands, several passes per run and three paths per pixel — every knob value gives the same bits, and the ragged frame the oracle's."""
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    tree, _ = O.build_bvh(scene("scene_d"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    W, H = 101, 67
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    seeds = O.randseeds(5)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, 1, acc, nthreads=8)
    for knob in KNOBS:
        got = render(B, monkeypatch, knob, tree, c, W, H, P, seeds)
        assert_bits(got.reshape(-1, 3), acc[..., :3].reshape(-1, 3), "ragged frame, GPUART_HIP_PACKET=%s" % knob)
    W, H = 384, 216
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 8, 0.01)
    from gpuart_amd import sharding
    y0, n, band, stride, _ = sharding.interleaved_rows(3, 8, H)
    for what, kw in [("tile", dict(tile=(37, 21, 203, 117))), ("share", dict(interleaved=(0, y0, W, n, band, stride))),
                     ("3 paths", dict(npaths=3))]:
        outs = [render(B, monkeypatch, knob, tree, c, W, H, P, seeds[:3], **kw) for knob in KNOBS]
        assert np.isfinite(outs[0]).all() and outs[0].max() > 0, what
        for knob, got in zip(KNOBS[1:], outs[1:]):
            assert_bits(got.reshape(-1, 3), outs[0].reshape(-1, 3), "%s, GPUART_HIP_PACKET=%s vs 0" % (what, knob))
