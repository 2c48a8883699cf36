"""Round 11: an upper-only step of the packet walk (device_scene.h trav_packet: no lane leaves by the lower child, some lane's walk stacks
the upper one) enters the upper child from registers instead of pushing the entry and popping it at once. Wave-level bookkeeping only:
every frame must stay what it was, bit for bit, across
    mode 3 with the packet knobs at their defaults (k_gen walks the camera packets and segment 0's Sun-shadow packets, k_trace the rest),
    GPUART_HIP_PACKET=0 (every query per lane, through k_trace's wide loop),
    mode 1 (the reference-order kernels),
and equal to the stored golden where there is one. The per-lane round is held by the GPUART_HIP_PACKET=0 column of every case.
On the CPU: tools/trav_stack_check.cpp, the traversal stack's own source — a push followed by its pop at depths 7, 8 and 9."""
import os
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.test_packet_walk import params
from tests.util import assert_bits, frame_golden_params, golden, scene

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KNOBS = ("GPUART_HIP_PACKET", "GPUART_HIP_GEN_WALK", "GPUART_HIP_GEN_SHADE", "GPUART_HIP_SHADOW_POOL", "GPUART_HIP_BLOCK_ORDER",
         "GPUART_HIP_PACKET_MAX_PRIMS", "GPUART_HIP_POOL_MIN_PASSES", "GPUART_HIP_NEAREST_MIN_PRIMS")
VARIANTS = (("mode 3, default knobs", 3, {}), ("mode 3, GPUART_HIP_PACKET=0", 3, {"GPUART_HIP_PACKET": "0"}), ("mode 1", 1, {}))


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def render(B, monkeypatch, mode, env, tree, cam, W, H, P, seeds):
    """The accumulator after len(seeds) passes, planned as one sequence, on a fresh context with only `env` of the packet knobs set."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(cam)
        assert b.scene_order() == 1, "the packet walk is for trees walked in the reference's order"
        b.set_mode(mode)
        b.pt_reset()
        if len(seeds) > 1:
            b.pt_plan(len(seeds))
        for s in seeds:
            b.pt_pass(params(B, P), s, 1)
        return b.read(1)[..., :3].copy()
    finally:
        b.close()


def hold(B, monkeypatch, what, tree, cam, W, H, P, seeds, exp=None, variants=VARIANTS):
    """Every variant's frame equals the first one's, and the golden's if there is one; the frame shows something."""
    first = None
    for name, mode, env in variants:
        got = render(B, monkeypatch, mode, env, tree, cam, W, H, P, seeds).reshape(-1, 3)
        if first is None:
            first = got
            assert np.isfinite(got).all() and got.max() > 0, what
        else:
            assert_bits(got, first, "%s: %s against %s" % (what, name, variants[0][0]))
        if exp is not None:
            assert_bits(got, np.asarray(exp, np.float32).reshape(-1, 3), "%s: %s against the golden" % (what, name))
    return first


def sun_params(O, cam, segments, sun_on=True):
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    return O.make_params(sun, S.SUN_ALTITUDE, sun_on, S.USER_SPHERE, 0.0, 0, float(cam[12]), cam[0:3], segments, 0.01)


@gpu
@pytest.mark.parametrize("look", [1.0, -1.0])
def test_first_step_upper_only(B, O, monkeypatch, look):
    """Two clusters of spheres 40 apart on the x axis and a camera between them that looks at one: the other lies behind every camera ray.
    The root splits the clusters, so in one of the two views the root's LOWER child is missed by the whole packet — whichever side the
    builder calls lower — and the packet's first step is upper-only."""
    rng = np.random.RandomState(11)
    prims = [(S.SPHERE, [float(sx * 20.0 + rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), float(rng.uniform(-3, 3)), float(rng.uniform(0.3, 0.9))])
             for sx in (-1.0, 1.0) for _ in range(40)]
    tree, _ = O.build_bvh(prims)
    W, H = 64, 40
    cam = O.camera((0.0, 0.5, 0.3), (look, 0.0, 0.0), (0.0, 0.0, 1.0), 50.0, 0.2, W, H)
    hold(B, monkeypatch, "two clusters, looking along %+.0f x" % look, tree, cam, W, H, sun_params(O, cam, 4), O.randseeds(2))


@gpu
def test_upper_only_steps_on_both_sides_of_the_ring(B, O, monkeypatch):
    """The spilling tree of tests/test_packet_walk.py (a 39-level sphere chain; the LDS ring holds 8 entries): upper-only steps happen with
    the stack inside the ring, at its edge and in the spill column."""
    prims = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    cam = O.camera((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    P = sun_params(O, cam, 5)
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, cam, W, H, P, s, 1, acc, nthreads=8)
    hold(B, monkeypatch, "deep tree", tree, cam, W, H, P, seeds, exp=acc[..., :3])


@gpu
@pytest.mark.parametrize("pool", ["1", "0"])
def test_shadow_packets_with_finished_lanes(B, O, monkeypatch, pool):
    """Scene D, a run of 8 passes (the pool's minimum): the Sun-shadow packets of k_gen hold lanes in state DONE — pixels on the sky, paths
    without a shadow query, queries settled by their first hit — while the others make upper-only steps. Pool on and off."""
    g = golden("frames_scene_d_seg8")
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene("scene_d"))
    variants = (("mode 3, GPUART_HIP_SHADOW_POOL=" + pool, 3, {"GPUART_HIP_SHADOW_POOL": pool}),) + VARIANTS[1:]
    hold(B, monkeypatch, "scene D, 8 passes, pool " + pool, tree, g["cam"], W, H, frame_golden_params(O, g)(True), O.randseeds(8), variants=variants)


@gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_order_adversary_frames(B, O, monkeypatch, k):
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam = g["cam"]
    P = sun_params(O, cam, int(g["max_segments"]))
    hold(B, monkeypatch, "adversary frame %d" % k, g["tree"], cam, W, H, P, g["seeds"][:1], exp=g["pt_pass1"])


@gpu
@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_tree_seg5"])
def test_goldens_of_the_three_type_classes(B, O, monkeypatch, name):
    """Flat (Scene D), round (Scene P) and all types (the tree): at GPUART_HIP_PACKET=0 every query goes through the wide loop."""
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    hold(B, monkeypatch, name, tree, g["cam"], W, H, frame_golden_params(O, g)(True), g["seeds"][:int(g["npasses"])], exp=g["pt_acc"])


@gpu
@pytest.mark.parametrize("size,passes", [((8, 8), 1), ((13, 9), 1), ((13, 9), 3)])
def test_ragged_and_tiny_frames(B, O, monkeypatch, size, passes):
    """8x8 with one pass: a queue of exactly 64 entries, shorter than one chunk; 13x9: padding slots, queue lengths that are no multiple of 64."""
    W, H = size
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    tree, _ = O.build_bvh(scene("scene_d"))
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(passes)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, 1, acc)
    hold(B, monkeypatch, "%dx%d, %d passes" % (W, H, passes), tree, c, W, H, P, seeds, exp=acc[..., :3])


@gpu
@pytest.mark.parametrize("passes", [1, 3, 8])
@pytest.mark.parametrize("sun_on", [True, False])
def test_run_lengths_and_the_sun(B, O, monkeypatch, passes, sun_on):
    """Runs of 1, 3 and 8 passes (k_gen's levels differ by the run: the pool from 8 passes on), Sun on and off (no shadow packets)."""
    g = golden("frames_scene_d_seg8")
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene("scene_d"))
    hold(B, monkeypatch, "scene D, %d passes, sun %s" % (passes, sun_on), tree, g["cam"], W, H, frame_golden_params(O, g)(sun_on), g["seeds"][:passes])


def test_a_push_and_its_pop_leave_the_stack_as_it_was(tmp_path):
    """CPU: csrc/hip/trav_stack.h itself. The pop returns the entry pushed, sp is what it was and every older entry still comes back in
    order — inside the ring (depth 7), with the ring full (8: the push moves the oldest ring entry to the spill column and `base` up by
    one, which no pop can tell) and beyond (9)."""
    exe = str(tmp_path / "trav_stack_check")
    subprocess.run(["g++", "-O2", "-Wall", "-I", os.path.join(ROOT, "gpuart_amd", "csrc", "hip"), "-o", exe,
                    os.path.join(ROOT, "tools", "trav_stack_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "identity holds at every depth" in r.stdout, r.stdout[-1500:] + r.stderr[-1500:]
    lines = {int(line.split(":")[0].split()[1]): line for line in r.stdout.splitlines() if line.startswith("depth")}
    assert "base  0 ->  0" in lines[7] and "base  0 ->  1" in lines[8] and "base  1 ->  2" in lines[9], (lines[7], lines[8], lines[9])
