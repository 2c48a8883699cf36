"""Round 12: the cadence of k_trace's wide loop (GD_ROUND_STEPS box steps between two passes through the round tail) is wave-level
bookkeeping: a lane's walk is a state machine on its own registers and its own stack column, so every frame must stay what it was, bit for
bit, across
    mode 3 with the packet knobs at their defaults,
    GPUART_HIP_PACKET=0 (every query per lane, through k_trace's wide loop),
    mode 1 (the reference-order kernels),
each on a fresh context, and equal to the stored golden or the oracle's frame where there is one. The cases put every exit of the wide loop
— no lane busy, the refill threshold, the thin-wave thresholds — on, one before and one after a step, whatever GD_ROUND_STEPS is, and pops
of one, two and three trips on both sides of the ring's edge. The pattern and the helpers are tests/test_issue_budget.py's."""
import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.test_issue_budget import VARIANTS, hold, sun_params
from tests.util import frame_golden_params, golden, scene

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def with_knobs(knobs, variants=VARIANTS):
    """The variants with the scheduling knobs `knobs` set in every one of them."""
    return tuple((name + " " + " ".join("%s=%s" % kv for kv in sorted(knobs.items())), mode, dict(env, **knobs)) for name, mode, env in variants)


@pytest.fixture(scope="module")
def scene_d_tree(O):
    return O.build_bvh(scene("scene_d"))[0]


@pytest.fixture(scope="module")
def oracle_frames(O, scene_d_tree):
    """The oracle's accumulator of Scene D from the bench camera at depth 8, by (W, H, passes); computed once per frame shape."""
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    made = {}

    def frame(W, H, passes):
        if (W, H, passes) not in made:
            c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
            P = sun_params(O, c, 8)
            seeds = O.randseeds(passes)
            acc = np.zeros((H, W, 4), np.float32)
            for s in seeds:
                O.pt_pass(scene_d_tree, c, W, H, P, s, 1, acc, nthreads=8)
            acc.setflags(write=False)
            made[(W, H, passes)] = (c, P, seeds, acc[..., :3])
        return made[(W, H, passes)]
    return frame


# (golden, depth): depths 1 and 8 for every type class, and the golden's own depth (Scene D's is 8) where its stored frame can be compared
GOLDEN_DEPTHS = [("frames_scene_d_seg8", 1), ("frames_scene_d_seg8", 8), ("frames_scene_p_seg4", 1), ("frames_scene_p_seg4", 4), ("frames_scene_p_seg4", 8),
                 ("frames_tree_seg5", 1), ("frames_tree_seg5", 5), ("frames_tree_seg5", 8)]


@gpu
@pytest.mark.parametrize("sun_on", [True, False], ids=["sun", "nosun"])
@pytest.mark.parametrize("passes", [1, 3, 8], ids=lambda k: "%dpasses" % k)
@pytest.mark.parametrize("name,depth", GOLDEN_DEPTHS, ids=["%s-depth%d" % nd for nd in GOLDEN_DEPTHS])
def test_goldens_of_the_three_type_classes(B, O, monkeypatch, name, depth, passes, sun_on):
    """Flat (Scene D), round (Scene P) and all types (the tree), runs of 1, 3 and 8 passes, Sun on and off, at depth 1, at depth 8 and at the
    golden's own depth (4 and 5 for Scene P and the tree); the golden holds the accumulator after one pass, Sun on, at its own depth."""
    g = golden(name)
    W, H = int(g["W"]), int(g["H"])
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    cam = g["cam"]
    own_depth = depth == int(g["max_segments"])
    P = frame_golden_params(O, g)(sun_on) if own_depth else sun_params(O, cam, depth, sun_on)
    exp = g["pt_pass1"] if passes == 1 and sun_on and own_depth else None
    hold(B, monkeypatch, "%s, %d passes, sun %s, depth %d" % (name, passes, sun_on, depth), tree, cam, W, H, P, g["seeds"][:passes], exp=exp)


@gpu
@pytest.mark.parametrize("name", ["frames_scene_d_seg8", "frames_scene_p_seg4", "frames_tree_seg5"])
def test_goldens_after_their_own_passes(B, O, monkeypatch, name):
    g = golden(name)
    tree, _ = O.build_bvh(scene(str(g["scene"])))
    hold(B, monkeypatch, name, tree, g["cam"], int(g["W"]), int(g["H"]), frame_golden_params(O, g)(True), g["seeds"][:int(g["npasses"])], exp=g["pt_acc"])


@gpu
@pytest.mark.parametrize("k", [0, 1, 2])
def test_phantom_hit_frames(B, O, monkeypatch, k):
    """order_adversary_frame_k: a ray grazes a triangle and the reference's order shows its phantom hit — the order of a lane's walk is its own."""
    g = golden("order_adversary_frame_%d" % k)
    cam = g["cam"]
    hold(B, monkeypatch, "adversary frame %d" % k, g["tree"], cam, int(g["W"]), int(g["H"]), sun_params(O, cam, int(g["max_segments"])),
         g["seeds"][:1], exp=g["pt_pass1"])


@gpu
@pytest.mark.parametrize("chunk", ["16", "128"])
@pytest.mark.parametrize("leaf_share", ["1", "3", "64"])
@pytest.mark.parametrize("leaf_lanes", ["1", "16", "64"])
@pytest.mark.parametrize("refill_lanes", ["1", "16", "64"])
def test_extreme_scheduling_knobs(B, monkeypatch, scene_d_tree, oracle_frames, refill_lanes, leaf_lanes, leaf_share, chunk):
    """`stay` = 63, 48 and 0 (the wave leaves the loop after one finished lane, after 16, only when all are done); a leaf quorum that every
    lane at a leaf reaches (leaf_lanes 1, or leaf_share 64) and one that only the last lanes reach (leaf_lanes 64 with leaf_share 1): the
    loop's exits and the leaf step fall on either step of a round. 40 x 24: 960 queries in segment 0, exactly 15 waves' worth; the queues of the later segments are ragged."""
    W, H = 40, 24
    c, P, seeds, exp = oracle_frames(W, H, 2)
    knobs = {"GPUART_HIP_REFILL_LANES": refill_lanes, "GPUART_HIP_LEAF_LANES": leaf_lanes, "GPUART_HIP_LEAF_SHARE": leaf_share, "GPUART_HIP_CHUNK": chunk}
    hold(B, monkeypatch, "knobs %s" % knobs, scene_d_tree, c, W, H, P, seeds, exp=exp, variants=with_knobs(knobs))


@gpu
@pytest.mark.parametrize("size", [(11, 3), (8, 4), (31, 1), (17, 1), (4, 4), (15, 1)])
def test_thin_wave_thresholds_straddled(B, monkeypatch, scene_d_tree, oracle_frames, size):
    """One-pass frames of 33, 32, 31, 17, 16 and 15 pixels: one wave whose queue is dry from the start holds one ray more than, exactly and one
    ray fewer than the 32 (16) at which it moves to pairs (quads) of lanes — the hand-over is reached on, before and after a round's first step."""
    W, H = size
    c, P, seeds, exp = oracle_frames(W, H, 1)
    hold(B, monkeypatch, "%dx%d, one pass" % (W, H), scene_d_tree, c, W, H, P, seeds, exp=exp)


@gpu
@pytest.mark.parametrize("size", [(128, 72), (13, 9), (8, 8)])
def test_cursor_path(B, monkeypatch, scene_d_tree, oracle_frames, size):
    """One wave per CU and chunks of 16: at 128 x 72 the queue of segment 0 (9216 entries at GPUART_HIP_PACKET=0) is longer than the static
    chunks of every wave together, so later chunks come from the cursor — a refill between any two steps; the ragged and the 8 x 8 frame end
    inside their static chunks."""
    W, H = size
    c, P, seeds, exp = oracle_frames(W, H, 1)
    knobs = {"GPUART_HIP_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "16"}
    hold(B, monkeypatch, "%dx%d, chunks of 16" % (W, H), scene_d_tree, c, W, H, P, seeds, exp=exp, variants=with_knobs(knobs))


# A 39-level chain of spheres on the x axis, each twice as far and twice as large as the one before (the spilling tree of
# tests/test_issue_budget.py; the LDS ring holds 8 entries), and a floor disc.
CHAIN = [(S.SPHERE, [float(2.0 ** k), 0.0, 0.0, float(2.0 ** (k - 2))]) for k in range(-19, 21)] + [(S.DISC, [0, 0, -0.3, 0, 0, 1, 40])]


@pytest.fixture(scope="module")
def chain(O):
    tree, depth = O.build_bvh(CHAIN)
    assert depth > 16
    return tree


@gpu
@pytest.mark.parametrize("view", ["across", "outwards", "inwards"])
def test_pops_across_the_ring_and_the_spill_column(B, O, monkeypatch, chain, view):
    """`across`: the view of tests/test_issue_budget.py. `outwards` / `inwards`: the camera looks along the chain's axis from its small end and
    from beyond its large end. A ray along the axis enters the box of every level, so its stack grows past the ring into the spill column;
    the sphere it hits first lies before all the others on one of the two views, whichever child the builder calls lower: from then on the
    stacked entries of consecutive levels are beyond the closest hit, and one pop skips two, three and more of them in a row. Counted once
    (profiles/r12/chain_pop_stats.txt): 3.08 trips per lane and call on average in `outwards`, 1.34 in `across`, 1.00 in `inwards`."""
    W, H = (96, 64) if view == "across" else (24, 16)
    pos, to = {"across": ((-6.0, -9.0, 4.0), (8.0, 9.0, -4.0)), "outwards": ((-0.5, 0.0, 0.02), (1.0, 0.0, 0.0)),
               "inwards": ((3.0e6, 0.0, 0.02), (-1.0, 0.0, 0.0))}[view]
    cam = O.camera(pos, to, (0.0, 0.0, 1.0), 60.0 if view == "across" else 8.0, 0.2, W, H)
    P = sun_params(O, cam, 5)
    seeds = O.randseeds(2)
    acc = np.zeros((H, W, 4), np.float32)
    for s in seeds:
        O.pt_pass(chain, cam, W, H, P, s, 1, acc, nthreads=8)
    hold(B, monkeypatch, "sphere chain, " + view, chain, cam, W, H, P, seeds, exp=acc[..., :3])


@gpu
def test_packets_and_per_lane_queries_in_one_launch(B, O, monkeypatch):
    """GPUART_HIP_GEN_WALK=0 with GPUART_HIP_PACKET=2: k_trace walks the closest-hit queries per lane and the Sun-shadow queries of the same
    launch as packets — a wave that still holds queries when its next entries are packet entries waits for them to finish (`hold`: `stay` = 0)."""
    g = golden("frames_scene_d_seg8")
    tree, _ = O.build_bvh(scene("scene_d"))
    variants = (("mode 3, GPUART_HIP_GEN_WALK=0 GPUART_HIP_PACKET=2", 3, {"GPUART_HIP_GEN_WALK": "0", "GPUART_HIP_PACKET": "2"}),) + VARIANTS[1:]
    hold(B, monkeypatch, "scene D, packets and per-lane queries", tree, g["cam"], int(g["W"]), int(g["H"]), frame_golden_params(O, g)(True),
         g["seeds"][:int(g["npasses"])], exp=g["pt_acc"], variants=variants)

