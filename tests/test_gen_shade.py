"""k_gen shades segment 0 of the paths whose camera rays it walked (GPUART_HIP_GEN_SHADE, kernels_pipeline.h k_gen, gpuart_hip.hip launch_run):
where k_gen walks and the run has a segment 1, level 1 shades segment 0 from the wave's registers and k_shade(0) is not launched; level 2 also
walks the Sun-shadow queries of those hits as packets of the same wave. The knob is a scheduling choice: 0, 1 and 2 must give the same
accumulator bit for bit — and the reference's, wherever a golden or the oracle says what that is. The frames run through the launch pipeline
(mode 3), on the goldens and shapes of tests/test_gen_walk.py, and on every branch segment 0 can take."""
import functools
import os
import re

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.util import assert_bits, frame_golden_params, golden, scene

KNOBS = ("0", "1", "2")
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


def sun_params(O, cam, max_segments, sun_on=True, sphere=S.USER_SPHERE, em=0.0, flags=0, min_weight=0.01, sun=None):
    alt = S.SUN_ALTITUDE
    if sun is None:
        sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    return O.make_params(sun, alt, sun_on, sphere, em, flags, float(cam[12]), cam[0:3], max_segments, min_weight)


def bench_camera(O, W, H):
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def oracle_acc(O, tree, c, W, H, P, seeds, npaths=1):
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(tree, c, W, H, P, s, npaths, acc, nthreads=8)
    return acc[..., :3]


def render(B, monkeypatch, knob, tree, cam, W, H, P, runs, npaths=1, tile=None, interleaved=None, order=None, env=None, blocks=None, info=None):
    """The accumulator after the pass sequences `runs` (lists of seeds, each flushed as one run of interleaved passes) through the launch
    pipeline on a fresh context with GPUART_HIP_GEN_SHADE = knob. `blocks`: the first run covers the frame, the others this list of 8x8
    blocks. `info`: a dict that receives the launch ledger and the birth order in use at the end."""
    monkeypatch.setenv("GPUART_HIP_GEN_SHADE", knob)
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
        b.launched()
        for i, seeds in enumerate(runs):
            if blocks is not None and i == 1:
                b.set_active_blocks(blocks)
            for s in seeds:
                b.pt_pass(params(B, P), s, npaths)
            b.flush()
        out = b.read(1)[..., :3].copy()
        if info is not None:
            info["launched"] = b.launched()
            info["order"] = b.test_current_tile_order()
        return out
    finally:
        for k in (env or {}):
            monkeypatch.delenv(k)
        b.close()


def three(B, monkeypatch, what, *args, expected=None, dark=False, **kw):
    """Renders with the knob at 0, 1 and 2; the three frames are the same bits, a real picture, and `expected` if there is one."""
    outs = [render(B, monkeypatch, knob, *args, **kw) for knob in KNOBS]
    assert np.isfinite(outs[0]).all() and (dark or outs[0].max() > 0), what
    for knob, got in zip(KNOBS[1:], outs[1:]):
        assert_bits(got.reshape(-1, 3), outs[0].reshape(-1, 3), "%s, GPUART_HIP_GEN_SHADE=%s vs 0" % (what, knob))
    if expected is not None:
        for knob, got in zip(KNOBS, outs):
            assert_bits(got.reshape(-1, 3), np.asarray(expected).reshape(-1, 3), "%s, GPUART_HIP_GEN_SHADE=%s vs the reference" % (what, knob))
    return outs[0]


@functools.lru_cache(maxsize=None)
def tree_of(name):
    from oracle import oracle
    return oracle.build_bvh(scene(name))[0]


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_tree_seg5"])   # flat, round, all types: every branch of the type switch, for both packets
def test_gen_shade_equals_the_goldens(B, O, monkeypatch, name):
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    three(B, monkeypatch, name, tree, g["cam"], W, H, frame_golden_params(O, g)(True), [seeds], expected=g["pt_acc"])


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_gen_shade_keeps_the_phantom_hits(B, O, monkeypatch, k):
    """order_adversary_frame_k: a camera ray grazes a triangle, and the reference's order shows its phantom hit; segment 0 is shaded from it."""
    g = golden("order_adversary_frame_%d" % k)
    W, H = int(g["W"]), int(g["H"])
    cam, tree, seeds = g["cam"], g["tree"], g["seeds"]
    monkeypatch.delenv("GPUART_HIP_NEAREST_MIN_PRIMS", raising=False)
    three(B, monkeypatch, "adversary frame %d" % k, tree, cam, W, H, sun_params(O, cam, int(g["max_segments"])), [seeds[:1]], expected=g["pt_pass1"])


@pytest.mark.gpu
def test_gen_shade_on_a_tree_that_spills_the_ring(B, O, monkeypatch):
    """The 39-level sphere chain of tests/test_packet_walk.py (deeper than the LDS ring): both packets of a wave — camera rays, then the
    Sun-shadow queries of their hits — spill to the lane's spill area and come back."""
    prims = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]
    tree, depth = O.build_bvh(prims)
    assert depth > 16
    W, H = 96, 64
    c = O.camera((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5)
    seeds = O.randseeds(2)
    three(B, monkeypatch, "deep tree", tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


# ---- frame shapes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gen_shade_on_ragged_frames(B, O, monkeypatch):
    """101x67: neither side a multiple of 8, so padding slots sit inside the packets and shading must skip them (against the oracle). 8x8: one
    block — with three passes 192 slots, fewer than one staging flush holds: only the flush at the end of the wave's loop runs."""
    scene_d = tree_of("scene_d")
    W, H = 101, 67
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(5)
    three(B, monkeypatch, "ragged frame", scene_d, c, W, H, P, [seeds], expected=oracle_acc(O, scene_d, c, W, H, P, seeds))
    W, H = 8, 8
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    three(B, monkeypatch, "8x8 frame", scene_d, c, W, H, P, [seeds[:3]], expected=oracle_acc(O, scene_d, c, W, H, P, seeds[:3]))


@pytest.mark.gpu
def test_gen_shade_on_tiles_shares_run_lengths_paths_birth_orders_and_block_lists(B, O, monkeypatch):
    """Scene D at 380x212: a rectangular tile; a share of interleaved row bands whose last band is ragged; runs of 1, 3 and 8 interleaved passes
    in one sequence; two paths per pixel (the j = 1 launch commits into a plane that j = 0 wrote); a permuted birth order of the 8x8 blocks; a
    list of active blocks for the later runs (gpuart_hip_set_active_blocks)."""
    from gpuart_amd import sharding
    scene_d = tree_of("scene_d")
    W, H = 380, 212
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(12)
    y0, n, band, stride, rows = sharding.interleaved_rows(2, 8, H)
    assert n % 8 == 4 and rows[-1] == H - 1, "the share's last band is ragged"
    runs = [seeds[:1], seeds[1:4], seeds[4:12]]
    full = three(B, monkeypatch, "runs of 1, 3 and 8 passes", scene_d, c, W, H, P, runs)
    one_by_one = render(B, monkeypatch, "2", scene_d, c, W, H, P, [[s] for s in seeds])
    assert_bits(one_by_one.reshape(-1, 3), full.reshape(-1, 3), "12 runs of one pass vs runs of 1, 3 and 8")
    three(B, monkeypatch, "tile", scene_d, c, W, H, P, [seeds[:3]], tile=(37, 21, 203, 117))
    share = three(B, monkeypatch, "share", scene_d, c, W, H, P, runs, interleaved=(0, y0, W, n, band, stride))
    assert_bits(share.reshape(-1, 3), full[rows].reshape(-1, 3), "the share's rows vs the full frame's")
    three(B, monkeypatch, "2 paths per pixel", scene_d, c, W, H, P, [seeds[:3]], npaths=2)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    order = np.random.RandomState(11).permutation(tiles)
    born = three(B, monkeypatch, "permuted birth order", scene_d, c, W, H, P, runs, order=order)
    assert_bits(born.reshape(-1, 3), full.reshape(-1, 3), "permuted birth order vs row-major")
    blocks = np.flatnonzero(np.random.RandomState(5).rand(tiles) < 0.3)
    listed = three(B, monkeypatch, "active blocks", scene_d, c, W, H, P, runs, blocks=blocks)
    assert not np.array_equal(listed, full), "the list leaves blocks out"


@pytest.mark.gpu
def test_gen_shade_takes_chunks_from_the_cursor(B, O, monkeypatch):
    """One wave per CU and chunks of 64 slots on a 160x120 frame with 3 passes: 57 600 path slots, of which the waves' static first chunks
    cover CUs x 64 (a third at most on a device of up to 300 CUs) — the rest comes through k_gen's cursor, a wave shades several packets, and
    both the flush after SHADE_ROUNDS packets and the one at the end of the loop run. Chunks of 48: packets that are not full."""
    scene_d = tree_of("scene_d")
    W, H = 160, 120
    assert W * H * 3 >= 3 * 300 * 64
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(3)
    got = three(B, monkeypatch, "cursor path", scene_d, c, W, H, P, [seeds], env={"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "64"})
    for knob in KNOBS[1:]:
        assert_bits(render(B, monkeypatch, knob, scene_d, c, W, H, P, [seeds]).reshape(-1, 3), got.reshape(-1, 3), "default grid and chunk, knob %s" % knob)
        assert_bits(render(B, monkeypatch, knob, scene_d, c, W, H, P, [seeds], env={"GPUART_HIP_CHUNK": "48"}).reshape(-1, 3), got.reshape(-1, 3), "chunks of 48, knob %s" % knob)


# ---- the branches of segment 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sun_on", [True, False])
@pytest.mark.parametrize("depth", [2, 5, 8])
def test_gen_shade_with_and_without_the_sun_at_every_depth(B, O, monkeypatch, sun_on, depth):
    """Scene P, 96x64, against the oracle. Depth 2: the survivors of segment 0 are shaded once more and end there."""
    tree = tree_of("scene_p")
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(3)
    P = sun_params(O, c, depth, sun_on)
    three(B, monkeypatch, "sun %s, maxSegments %d" % (sun_on, depth), tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


@pytest.mark.gpu
def test_gen_shade_leaves_depth_one_and_no_segments_to_the_separate_launches(B, O, monkeypatch):
    """maxSegments = 1 with the Sun on: k_gen walks, but no k_shade(1) follows — every knob value takes the sequence of knob 0, and launches
    the same kernels. minWeight >= 1 and maxSegments = 0: no segment at all, k_gen commits the paths. Against the oracle."""
    tree = tree_of("scene_p")
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(3)
    P = sun_params(O, c, 1)
    exp = oracle_acc(O, tree, c, W, H, P, seeds)
    ledgers = []
    for knob in KNOBS:
        info = {}
        assert_bits(render(B, monkeypatch, knob, tree, c, W, H, P, [seeds], info=info).reshape(-1, 3), exp.reshape(-1, 3), "depth 1, knob %s" % knob)
        ledgers.append(info["launched"])
    assert ledgers[0] == ledgers[1] == ledgers[2] and any("k_shade" in n for n in ledgers[0]), ledgers
    for what, P in (("minWeight 1", sun_params(O, c, 5, min_weight=1.0)), ("maxSegments 0", sun_params(O, c, 0))):
        three(B, monkeypatch, what, tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))


@pytest.mark.gpu
@pytest.mark.parametrize("flags, em", [(0, 0.0), (1, 3.0), (2, 0.0), (6, 0.0)])   # diffuse (ush), emissive (breaks), mirror, fuzzy mirror
def test_gen_shade_with_a_user_sphere_in_every_mode(B, O, monkeypatch, flags, em):
    """A user sphere in front of the camera covers part of the frame (the frame differs from the one without it): `ush` and `specular` reach
    path_finish, the emissive sphere breaks the path at segment 0, a mirror asks no shadow query. Scene P, 96x64, against the oracle."""
    tree = tree_of("scene_p")
    W, H = 96, 64
    c = bench_camera(O, W, H)
    seeds = O.randseeds(2)
    sphere = (0.1, -0.9, 0.75, 0.2)
    P = sun_params(O, c, 5, sphere=sphere, em=em, flags=flags)
    got = three(B, monkeypatch, "user sphere flags %d" % flags, tree, c, W, H, P, [seeds], expected=oracle_acc(O, tree, c, W, H, P, seeds))
    P0 = sun_params(O, c, 5)
    assert (got != render(B, monkeypatch, "0", tree, c, W, H, P0, [seeds])).any(-1).mean() > 0.02, "the sphere is in the frame"


@pytest.mark.gpu
def test_gen_shade_when_no_path_survives_segment_zero_or_none_asks_for_the_sun(B, O, monkeypatch):
    """A camera that looks up from above the scene sees the sky only: every path breaks at segment 0, queue[1] and shadow_queue stay empty.
    A floor alone under a Sun below its horizon: dot(sun, n) <= 0 at every hit, no lane wants a shadow query, and level 2 skips the walk."""
    W, H = 96, 64
    seeds = O.randseeds(2)
    tree = tree_of("scene_p")
    c = O.camera((0.0, 0.0, 50.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 60.0, 0.2, W, H)
    P = sun_params(O, c, 5)
    sky = oracle_acc(O, tree, c, W, H, P, seeds)
    three(B, monkeypatch, "sky only", tree, c, W, H, P, [seeds], expected=sky)
    floor, _ = O.build_bvh([(S.DISC, [0, 0, 0, 0, 0, 1, 40]), (S.DISC, [0.5, 0.5, 0, 0, 0, 1, 1])])
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 5, sun=(0.6, 0.0, -0.8))
    three(B, monkeypatch, "sun below the floor", floor, c, W, H, P, [seeds], expected=oracle_acc(O, floor, c, W, H, P, seeds))


@pytest.mark.gpu
def test_gen_shade_keeps_the_birth_order_of_single_pass_runs(B, O, monkeypatch):
    """Single-pass runs with the library's own birth order. (The launch pipeline never gathers tile costs — only single-pass runs of modes 0
    and 5 do, and those are k_run's — so tile_cost_add in k_gen sees no table, as in k_shade(0); what can be compared is the order in use
    after the runs and the frame of the following run.)"""
    scene_d = tree_of("scene_d")
    W, H = 101, 67
    c = bench_camera(O, W, H)
    P = sun_params(O, c, 8)
    seeds = O.randseeds(4)
    frames, orders = [], []
    for knob in KNOBS:
        info = {}
        frames.append(render(B, monkeypatch, knob, scene_d, c, W, H, P, [[s] for s in seeds], info=info))
        orders.append(info["order"])
    for knob, f, o in zip(KNOBS[1:], frames[1:], orders[1:]):
        assert_bits(f.reshape(-1, 3), frames[0].reshape(-1, 3), "single-pass runs, knob %s" % knob)
        assert (o is None and orders[0] is None) or np.array_equal(o, orders[0])


@pytest.mark.gpu
def test_gen_shade_knob_is_clamped(B, O, monkeypatch):
    """Values beyond 0 .. 2 are clamped like every GPUART_HIP_* knob's; none changes a bit."""
    g = golden("frames_scene_p_seg4")
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    seeds = g["seeds"][:int(g["npasses"]) if "npasses" in g else 2]
    for knob in ("7", "-3"):
        got = render(B, monkeypatch, knob, tree, g["cam"], W, H, frame_golden_params(O, g)(True), [seeds])
        assert_bits(got.reshape(-1, 3), g["pt_acc"].reshape(-1, 3), "GPUART_HIP_GEN_SHADE=%s" % knob)


# ---- without a device ------------------------------------------------------------------------------------------------------------------
def test_gen_shade_knob_is_read_at_create_documented_and_applied_where_stated():
    """The knob is parsed where the others are (gpuart_hip_create's env_u32: clamped to 0 .. 2), read once, listed in LAB_NOTES.md's knob
    table with that default, and launch_run fuses exactly where k_gen walks and the run has a segment 1."""
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "hip", "gpuart_hip.hip")).read()
    create = src[src.index("int gpuart_hip_create("):src.index("int gpuart_hip_destroy(gpuart_hip_ctx *c) {")]
    m = re.search(r'c->gen_shade\s*=\s*env_u32\("GPUART_HIP_GEN_SHADE",\s*([012]),\s*0,\s*2\)', create)
    assert m
    assert create.index('"GPUART_HIP_GEN_WALK"') < create.index('"GPUART_HIP_GEN_SHADE"')
    assert src.count('"GPUART_HIP_GEN_SHADE"') == 1, "read once, at create"
    assert re.search(r"uint32_t gen_shade = %s;" % m.group(1), src), "the field's initialiser is the default"
    run = src[src.index("int launch_run(gpuart_hip_ctx *c, size_t first, size_t count) {"):]
    assert re.search(r"const int gen_shade = gen_walk && nseg >= 2 \? \(int\)c->gen_shade : 0;", run)
    assert "c->gen_shade" not in run.replace("(int)c->gen_shade : 0;", "", 1), "launch_run decides once"
    notes = open(os.path.join(ROOT, "LAB_NOTES.md")).read()
    assert re.search(r"^\| `GPUART_HIP_GEN_SHADE` \| %s \|" % m.group(1), notes, re.M)
