"""k_gen's pooled Sun-shadow packets and the Z-order of the path slots inside an 8x8 block (kernels_pipeline.h k_gen `shade` == 3, block_pixel;
gpuart_hip.hip launch_run): GPUART_HIP_SHADOW_POOL = 1 on top of GPUART_HIP_GEN_SHADE = 2 lets a wave carry the shadow lanes of one packet
over to the next and walk them 64 at a time; GPUART_HIP_BLOCK_ORDER = 1 maps pixel w of a block by bit de-interleave instead of row-major.
Both are scheduling choices: the accumulator must be the same bit for bit for the pooled walk against level 2 and level 0 and for order 1
against order 0 — and the reference's, wherever a golden or the oracle says what that is. The frames run through the launch pipeline
(mode 3) with the helpers of tests/test_gen_shade.py, on its shapes, and on the pool's own edge cases."""
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.test_gen_shade import bench_camera, oracle_acc, render, sun_params, tree_of
from tests.util import assert_bits, frame_golden_params, golden, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (GPUART_HIP_GEN_SHADE, GPUART_HIP_SHADOW_POOL, GPUART_HIP_BLOCK_ORDER): the first is what the others are compared with. Every run pools where the
# pool is on (GPUART_HIP_POOL_MIN_PASSES = 1) and takes the order named; the library's own choice by the run: the test of the run lengths below.
VARIANTS = [("0", "0", "0"), ("2", "0", "0"), ("2", "1", "0"), ("2", "1", "1"), ("2", "0", "1"), ("0", "0", "1")]


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def every(B, monkeypatch, what, *args, expected=None, dark=False, env=None, **kw):
    """Renders with every variant; the frames are the same bits, a real picture, and `expected` if there is one."""
    outs = []
    for shade, pool, order in VARIANTS:
        e = dict(env or {}, GPUART_HIP_SHADOW_POOL=pool, GPUART_HIP_POOL_MIN_PASSES="1", GPUART_HIP_BLOCK_ORDER=order)
        outs.append(render(B, monkeypatch, shade, *args, env=e, **kw))
    assert np.isfinite(outs[0]).all() and (dark or outs[0].max() > 0), what
    for v, got in zip(VARIANTS[1:], outs[1:]):
        assert_bits(got.reshape(-1, 3), outs[0].reshape(-1, 3), "%s, shade / pool / order %s vs %s" % (what, v, VARIANTS[0]))
    if expected is not None:
        assert_bits(outs[0].reshape(-1, 3), np.asarray(expected).reshape(-1, 3), "%s vs the reference" % what)
    return outs[0]


def shadow_lanes(O, tree, c, W, H, P, seed):
    """(H, W) bool: the oracle's first segment of this pass hits the tree with the face-forwarded normal towards the Sun — the lanes that ask
    a Sun-shadow query at segment 0 (diffuse scenes, no user sphere in view)."""
    rs, rd = O.first_segment_rays(c, W, H, P, seed)
    o0, o1 = O.traverse(tree, rs.reshape(-1, 4), rd.reshape(-1, 4))
    n, d = o1[:, :3], rd.reshape(-1, 4)[:, :3]
    n = np.where((n * d).sum(1, keepdims=True) > 0, -n, n)
    sun = np.array(list(P.sunDirAlt)[:3], np.float32)
    return ((o0[:, 0] > 0) & ((n * sun).sum(1) > 0)).reshape(H, W)


NO_SPHERE = (0.0, 0.0, -1000.0, 0.0)


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_tree_seg5"])   # flat, round, all types
def test_pool_and_order_equal_the_goldens(B, O, monkeypatch, name):
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    every(B, monkeypatch, name, tree, g["cam"], W, H, frame_golden_params(O, g)(True), [seeds], expected=g["pt_acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_pool_and_order_keep_the_phantom_hits(B, O, monkeypatch, k):
    """order_adversary_frame_k: a camera ray grazes a triangle, and the reference's order shows its phantom hit."""
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam, tree, seeds = g["cam"], g["tree"], g["seeds"]
    monkeypatch.delenv("GPUART_HIP_NEAREST_MIN_PRIMS", raising=False)
    every(B, monkeypatch, "adversary frame %d" % k, tree, cam, W, H, sun_params(O, cam, int(g["max_segments"])), [seeds[:1]], expected=g["pt_pass1"])


@pytest.mark.gpu
def test_pool_on_a_tree_that_spills_the_ring(B, O, monkeypatch):
    """The 39-level sphere chain of tests/test_packet_walk.py: a pooled packet spills to the lane's spill area and comes back."""
    prims = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    c = O.camera((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5)
    seeds = O.randseeds(2)
    every(B, monkeypatch, "deep tree", tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


# ---- frame shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("W, H, passes", [(8, 8, 3), (70, 37, 3), (70, 37, 8)])
def test_pool_and_order_on_small_and_ragged_frames(B, O, monkeypatch, W, H, passes):
    """8x8: one block. 70x37: neither side a multiple of 8 — under Z-order the padding slots of an edge block are scattered through its
    packets, not whole rows of them. Against the oracle."""
    scene_d = tree_of("scene_d")
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(passes)
    every(B, monkeypatch, "%dx%d, %d passes" % (W, H, passes), scene_d, c, W, H, P, [seeds], expected=oracle_acc(O, scene_d, c, W, H, P, seeds))


@pytest.mark.gpu
def test_pool_and_order_on_tiles_shares_run_lengths_paths_and_block_lists(B, O, monkeypatch):
    """Scene D at 72x212: runs of 1, 3 and 8 interleaved passes in one sequence (packets of 64, 21 1/3 and 8 pixels); a rectangular tile; a
    share of interleaved row bands whose last band is ragged; two paths per pixel; a list of active blocks for the later runs."""
    from gpuart_amd import sharding
    scene_d = tree_of("scene_d")
    W, H = 72, 212
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(12)
    y0, n, band, stride, rows = sharding.interleaved_rows(2, 8, H)
    assert n % 8 == 4 and rows[-1] == H - 1, "the share's last band is ragged"
    runs = [seeds[:1], seeds[1:4], seeds[4:12]]
    full = every(B, monkeypatch, "runs of 1, 3 and 8 passes", scene_d, c, W, H, P, runs)
    # the defaults: the order and the pool chosen run by run (Z-order from 4 passes on, the pool from 8 passes on), in one sequence
    for k in ("GPUART_HIP_SHADOW_POOL", "GPUART_HIP_POOL_MIN_PASSES", "GPUART_HIP_BLOCK_ORDER", "GPUART_HIP_POOL_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    assert_bits(render(B, monkeypatch, "2", scene_d, c, W, H, P, runs).reshape(-1, 3), full.reshape(-1, 3), "the library's choice by the run")
    every(B, monkeypatch, "tile", scene_d, c, W, H, P, [seeds[:3]], tile=(13, 21, 43, 117))
    share = every(B, monkeypatch, "share", scene_d, c, W, H, P, runs, interleaved=(0, y0, W, n, band, stride))
    assert_bits(share.reshape(-1, 3), full[rows].reshape(-1, 3), "the share's rows vs the full frame's")
    every(B, monkeypatch, "2 paths per pixel", scene_d, c, W, H, P, [seeds[:3]], npaths=2)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    blocks = np.flatnonzero(np.random.RandomState(5).rand(tiles) < 0.3)
    listed = every(B, monkeypatch, "active blocks", scene_d, c, W, H, P, runs, blocks=blocks)
    assert not np.array_equal(listed, full), "the list leaves blocks out"


@pytest.mark.gpu
def test_pool_takes_chunks_from_the_cursor(B, O, monkeypatch):
    """One wave per CU and chunks of 64 slots on a 160x120 frame with 3 passes (tests/test_gen_shade.py): most chunks come through k_gen's
    cursor, and with one packet per chunk every pool walk is the partial one at the chunk's end. Chunks of 48: packets that are not full.
    Chunks of 4096: the pool is walked full many times inside a chunk. The default grid and chunk."""
    scene_d = tree_of("scene_d")
    W, H = 160, 120
    assert W * H * 3 >= 3 * 300 * 64
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(3)
    one = {"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "64", "GPUART_HIP_POOL_CHUNK": "64"}
    got = every(B, monkeypatch, "cursor path", scene_d, c, W, H, P, [seeds], env=one)
    for env in ({}, {"GPUART_HIP_POOL_CHUNK": "48"}, {"GPUART_HIP_POOL_CHUNK": "4096"}, {"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_POOL_CHUNK": "128"}):
        for order in ("0", "1"):
            e = dict(env, GPUART_HIP_SHADOW_POOL="1", GPUART_HIP_POOL_MIN_PASSES="1", GPUART_HIP_BLOCK_ORDER=order)
            assert_bits(render(B, monkeypatch, "2", scene_d, c, W, H, P, [seeds], env=e).reshape(-1, 3), got.reshape(-1, 3), "pooled, %s" % e)


# ---- the branches of segment 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sun_on", [True, False])
@pytest.mark.parametrize("depth", [2, 8])
def test_pool_with_and_without_the_sun_at_depth_two_and_eight(B, O, monkeypatch, sun_on, depth):
    """Scene P, 96x64, against the oracle. Sun off: no lane ever joins the pool."""
    tree = tree_of("scene_p")
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(3)
    P = sun_params(O, c, depth, sun_on)
    every(B, monkeypatch, "sun %s, maxSegments %d" % (sun_on, depth), tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("flags, em", [(0, 0.0), (1, 3.0), (2, 0.0)])   # diffuse (asks the Sun), emissive (breaks), mirror (asks nothing)
def test_pool_with_a_user_sphere(B, O, monkeypatch, flags, em):
    tree = tree_of("scene_p")
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(2)
    P = sun_params(O, c, 5, sphere=(0.1, -0.9, 0.75, 0.2), em=em, flags=flags)
    every(B, monkeypatch, "user sphere flags %d" % flags, tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


# ---- the pool's edge cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_pool_that_is_never_filled_and_a_sun_below_every_horizon(B, O, monkeypatch):
    """A camera that looks up sees the sky only: no lane ever joins the pool. A floor under a Sun below its horizon: dot(sun, n) <= 0 at every
    hit, no lane asks, the pool stays empty although every lane hit something."""
    W, H = 96, 64
    seeds = O.randseeds(2)
    tree = tree_of("scene_p")
    c = O.camera((0.0, 0.0, 50.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5)
    assert not shadow_lanes(O, tree, c, W, H, P, seeds[0]).any()
    every(B, monkeypatch, "sky only", tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))
    floor, _ = O.build_bvh([(S.DISC, [0, 0, 0, 0, 0, 1, 40]), (S.DISC, [0.5, 0.5, 0, 0, 0, 1, 1])])
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 5, sun=(0.6, 0.0, -0.8))
    every(B, monkeypatch, "sun below the floor", floor, c, W, H, P, [seeds], expected=oracle_acc(O, floor, c, W, H, P, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("passes", [1, 2, 8])
def test_pool_where_every_lane_asks(B, O, monkeypatch, passes):
    """A floor seen from straight above under a high Sun, 64x48: every slot of every packet asks a shadow query, so every packet fills the pool
    exactly and nothing is left behind — the partial walk at a chunk's end finds the pool empty."""
    floor, _ = O.build_bvh([(S.DISC, [0, 0, 0, 0, 0, 1, 40]), (S.DISC, [0.5, 0.5, 0, 0, 0, 1, 1])])
    W, H = 64, 48
    c = O.camera((0.0, 0.0, 5.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5, sphere=NO_SPHERE)
    seeds = O.randseeds(passes)
    for s in seeds:
        assert shadow_lanes(O, floor, c, W, H, P, s).all()
    every(B, monkeypatch, "floor only, %d passes" % passes, floor, c, W, H, P, [seeds], expected=oracle_acc(O, floor, c, W, H, P, seeds))


@pytest.mark.gpu
def test_pool_that_crosses_several_packets_before_its_first_walk(B, O, monkeypatch):
    """A column of small spheres against the sky, 64x128 with one pass per run: a packet is one 8x8 block, and no block holds more than 24
    shadow lanes, most far fewer — the pool takes the lanes of several packets before it holds 64. With chunks of 4096 slots it is walked
    full inside a chunk; with chunks of 128 the two packets of a chunk never fill it and every walk is a partial one."""
    prims = [(S.SPHERE, [0.0, 0.0, 0.12 * k, 0.09]) for k in range(-60, 61)]
    tree, _ = O.build_bvh(prims)
    W, H = 64, 128
    c = O.camera((0.0, -10.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5, sphere=NO_SPHERE, sun=(0.0, -0.8, 0.6))
    seeds = O.randseeds(2)
    lanes = shadow_lanes(O, tree, c, W, H, P, seeds[0])
    per_block = lanes.reshape(H // 8, 8, W // 8, 8).sum((1, 3))
    assert lanes.sum() >= 128 and per_block.max() <= 24, (int(lanes.sum()), int(per_block.max()))
    exp = oracle_acc(O, tree, c, W, H, P, seeds)
    for chunk in ("4096", "128"):
        every(B, monkeypatch, "thin column, chunks of %s" % chunk, tree, c, W, H, P, [[s] for s in seeds], expected=exp,
              env={"GPUART_HIP_POOL_CHUNK": chunk, "GPUART_HIP_WAVES_PER_CU": "1"})


@pytest.mark.gpu
def test_pool_whose_last_walk_is_one_query(B, O, monkeypatch):
    """An 8x8 frame, one pass: one packet. The camera stands between the Sun and a small sphere and looks at it, so what it sees of the sphere is
    lit; the radius is the first of a list at which exactly one first segment hits. That query is all the pool ever holds."""
    W, H = 8, 8
    sun = np.array([0.0, -0.8, 0.6], np.float32)
    c = O.camera(tuple(10.0 * sun), tuple(-sun), (0.0, 0.0, 1.0), 30.0, 0.2, W, H)
    seeds = O.randseeds(1)
    for radius in (0.02, 0.04, 0.07, 0.1, 0.14, 0.2, 0.27, 0.35):
        tree, _ = O.build_bvh([(S.SPHERE, [0.0, 0.0, 0.0, radius]), (S.SPHERE, [0.0, 50.0, 0.0, 0.5])])
        P = sun_params(O, c, 5, sphere=NO_SPHERE, sun=sun)
        if shadow_lanes(O, tree, c, W, H, P, seeds[0]).sum() == 1:
            break
    else:
        pytest.fail("no radius of the list puts the sphere under exactly one first segment")
    every(B, monkeypatch, "one query", tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


# ---- without a device ------------------------------------------------------------------------------------------------------------------
def block_pixel_text():
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "hip", "kernels_pipeline.h")).read()
    m = re.search(r"GD_FN void block_pixel\(uint32_t order, uint32_t w, uint32_t &x, uint32_t &y\) \{.*?\n\}\n", src, re.S)
    assert m, "block_pixel's definition"
    return src, m.group(0)


def test_block_order_one_is_a_bijection_with_compact_groups(tmp_path):
    """block_pixel's own text (kernels_pipeline.h), compiled for the host: order 0 is row-major; order 1 is a bijection of the 64 pixels in
    which every aligned group of 8 consecutive w covers a 4x2 rectangle and every aligned group of 16 a 4x4 one. slot_pixel goes through it."""
    src, text = block_pixel_text()
    prog = tmp_path / "block_pixel.cpp"
    prog.write_text("#include <cstdint>\n#include <cstdio>\n#define GD_FN static inline\n" + text +
                    "int main() { for (uint32_t o = 0; o < 2; o++) for (uint32_t w = 0; w < 64; w++) { uint32_t x, y; block_pixel(o, w, x, y); "
                    'printf("%u %u\\n", x, y); } return 0; }\n')
    exe = tmp_path / "block_pixel"
    subprocess.run(["g++", "-std=c++17", "-o", str(exe), str(prog)], check=True)
    xy = np.array(subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split(), np.int64).reshape(2, 64, 2)
    w = np.arange(64)
    assert np.array_equal(xy[0], np.stack([w & 7, w >> 3], 1)), "order 0 is row-major"
    z = xy[1]
    assert z.min() == 0 and z.max() == 7 and len({(int(x), int(y)) for x, y in z}) == 64, "a bijection of the 8x8 pixels"
    for size, (gw, gh) in ((8, (4, 2)), (16, (4, 4))):
        for g in z.reshape(64 // size, size, 2):
            x0, y0 = g.min(0)
            assert x0 % gw == 0 and y0 % gh == 0 and g[:, 0].max() == x0 + gw - 1 and g[:, 1].max() == y0 + gh - 1, (size, g.tolist())
            assert len({(int(x), int(y)) for x, y in g}) == size
    body = src[src.index("GD_FN bool slot_pixel("):]
    assert "block_pixel(f.block_order, w, x, y);" in body[:body.index("\n}\n")]


def test_pool_and_order_knobs_are_read_at_create_and_documented():
    """GPUART_HIP_SHADOW_POOL, GPUART_HIP_POOL_CHUNK, GPUART_HIP_POOL_MIN_PASSES and GPUART_HIP_BLOCK_ORDER are parsed where the others are, once,
    and listed in LAB_NOTES.md's knob table with their defaults; the block order travels in Frame, chosen by the run at 2."""
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "hip", "gpuart_hip.hip")).read()
    create = src[src.index("int gpuart_hip_create("):src.index("int gpuart_hip_destroy(gpuart_hip_ctx *c) {")]
    notes = open(os.path.join(ROOT, "LAB_NOTES.md")).read()
    for pat, name in ((r'c->shadow_pool\s*=\s*env_u32\("GPUART_HIP_SHADOW_POOL",\s*([01]),\s*0,\s*1\)', "GPUART_HIP_SHADOW_POOL"),
                      (r'c->pool_chunk\s*=\s*env_u32\("GPUART_HIP_POOL_CHUNK",\s*(\d+),\s*16,\s*4096\)', "GPUART_HIP_POOL_CHUNK"),
                      (r'c->pool_min_passes\s*=\s*env_u32\("GPUART_HIP_POOL_MIN_PASSES",\s*(\d+),\s*1,\s*MAX_BATCH\)', "GPUART_HIP_POOL_MIN_PASSES"),
                      (r'c->block_order\s*=\s*env_u32\("GPUART_HIP_BLOCK_ORDER",\s*([012]),\s*0,\s*2\)', "GPUART_HIP_BLOCK_ORDER")):
        m = re.search(pat, create)
        assert m, name
        assert src.count('"%s"' % name) == 1, "%s: read once, at create" % name
        assert re.search(r"^\| `%s` \| %s \|" % (name, m.group(1)), notes, re.M), "%s in LAB_NOTES.md's knob table" % name
    assert "c->frame.block_order = c->block_order == 1 ? 1u : 0u;" in create
    run = src[src.index("int launch_run(gpuart_hip_ctx *c, size_t first, size_t count) {"):]
    assert "if (c->block_order == 2) fr.block_order = count >= 4 ? 1u : 0u;" in run
    assert "gen_shade == 2 && c->shadow_pool && count >= c->pool_min_passes ? 3 : gen_shade;" in run
