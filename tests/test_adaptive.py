"""Adaptive sampling: passes over an active list of 8x8 blocks (gpuart_hip_set_active_blocks), the per-block estimate, block decision and
normalisation of libgpuart_adaptive.so, and Renderer::RenderAdaptive on top of both.

The contract is exact. A listed pass does for every pixel of a listed block, and for no other, what the plain pass does, so after any
sequence of passes and lists accum[p] is the fp32 sum, in pass order, of the colours of the passes whose list held p's block: the oracle's
pass colours under np.where. The library is NumPy float32 restated (tests/adaptive_ref.py, through tests/converge_ref.py)."""
import functools
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adaptive_ref as AR
from tests import converge_ref
from tests.test_converge_range import E_TOL
from tests.test_kernel_variants import names_of, scene_setup, to_params, tree_of
from tests.util import assert_bits, assert_same_bits, exported, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
FLOOR = 1.0 / 256
F = np.float32


# ---- inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
def growing_accums(rng, h, w, totals, nan_at=None):
    """Raw accumulators after each of `totals` paths: per-pixel means and spreads of several kinds (steady, noisy, dark, black)."""
    mean = rng.uniform(0.0, 2.0, (h, w, 1)) * rng.choice([0.0, 0.002, 1.0], (h, w, 1), p=[0.1, 0.2, 0.7])
    cv = rng.choice([0.0, 0.05, 1.0], (h, w, 1))
    acc, prev, out = np.zeros((h, w, 4), F), 0, []
    for t in totals:
        b = t - prev
        inc = np.maximum(0.0, mean * b * (1.0 + cv * rng.normal(size=(h, w, 3)) / np.sqrt(b)))
        acc = acc.copy()
        acc[..., :3] = acc[..., :3] + inc.astype(F)
        if nan_at is not None:
            acc[nan_at] = np.nan
        out.append(acc)
        prev = t
    return out


PATTERNS = {"equal": [4, 8, 12, 16, 20], "unequal": [100, 103, 104, 111, 211], "one_big": [1, 2, 3, 4, 4096]}


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_library_exports_exactly_its_header(lib):
    hdr = open(os.path.join(ROOT, "include", "gpuart_adaptive.h")).read()
    declared = sorted(set(re.findall(r"\b(gpuart_adaptive_[a-z_0-9]+)\s*\(", hdr)))
    assert len(declared) == 12, declared
    assert exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_adaptive.so")) == declared


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_every_block_active_is_the_uniform_estimator(name):
    """With one count for all blocks the restatement's state and e are converge_ref.Estimator's, bit for bit (33 x 7: ragged blocks)."""
    h, w, totals = 7, 33, PATTERNS[name]
    accums = growing_accums(np.random.default_rng(11), h, w, totals)
    est, uni = AR.Estimator(), converge_ref.Estimator()
    nb = len(AR.block_pixels(h, w))
    for k, (a, t) in enumerate(zip(accums, totals)):
        est.update(a, np.full(nb, t))
        uni.update(a, t)
        assert_same_bits(est.state, uni.state, "%s: state after batch %d" % (name, k))
        if k >= 1:
            assert_same_bits(est.error(FLOOR), uni.error(FLOOR), "%s: e after batch %d" % (name, k))
            blocks, s, _ = AR.Estimator.select(_copy(est), 0.05, FLOOR, 1)
            su, _ = uni.measure(0.05, FLOOR)
            assert {k2: s[k2] for k2 in ("pixels", "above", "non_finite", "max_error")} == {k2: su[k2] for k2 in ("pixels", "above", "non_finite", "max_error")}
            assert s["paths_sum"] == t * h * w and s["paths_min"] == s["paths_max"] == t
    assert (est.batches == len(totals)).all() and (est.seen == totals[-1]).all()


def _copy(est):
    c = AR.Estimator()
    c.state, c.seen, c.batches, c.active = est.state.copy(), est.seen.copy(), est.batches.copy(), est.active.copy()
    return c


def staggered(h, w, totals, seed):
    """Per-block counts after every batch when block t stops after stop[t] batches (at least 2), and masked accumulators to match."""
    rng = np.random.default_rng(seed)
    nb = len(AR.block_pixels(h, w))
    stop = rng.integers(2, len(totals) + 1, nb)
    full = growing_accums(rng, h, w, totals)
    pb = AR.pixel_blocks(h, w)
    accums, counts = [], []
    for k, t in enumerate(totals):
        last = np.minimum(k, stop - 1)
        counts.append(np.array(totals)[last])
        accums.append(np.stack(full)[last[pb], np.arange(h)[:, None], np.arange(w)[None, :]])
    return stop, full, accums, counts


def test_blocks_stopped_at_different_points_against_float64():
    """Each block's e agrees with converge_ref.reference64 fed that block's own luminances and totals, within the uniform estimator's
    tolerance (tests/test_converge_range.py E_TOL plus the accumulator's floor), and a retired block's state stays as it was."""
    h, w, totals = 21, 37, [4, 8, 16, 20, 36, 40]
    stop, full, accums, counts = staggered(h, w, totals, 5)
    est = AR.Estimator()
    frozen = {}
    pb = AR.pixel_blocks(h, w)
    for k in range(len(totals)):
        est.update(accums[k], counts[k])
        for t in np.nonzero(stop == k + 1)[0]:
            frozen[t] = est.state[pb == t].copy()
        for t, st in frozen.items():
            assert_same_bits(est.state[pb == t], st, "block %d after batch %d" % (t, k))
    assert len(frozen) == len(stop) and len(set(stop.tolist())) >= 4
    e = est.error(FLOOR)
    for t in range(len(stop)):
        n = int(stop[t])
        assert est.batches[t] == n and est.seen[t] == totals[n - 1]
        sel = pb == t
        lums = [converge_ref.lum(full[k])[sel] for k in range(n)]
        e64, _, _ = converge_ref.reference64(lums, totals[:n], FLOOR)
        tol = E_TOL + converge_ref.accumulator_floor(totals[n - 1], min(np.diff(totals[:n])))
        d = np.abs(e[sel].astype(np.float64) - e64)
        assert np.isfinite(d).all() and d.max() <= tol, (t, n, d.max(), tol)


def test_the_block_rule():
    h, w = 16, 24   # 2 x 3 blocks
    est = AR.Estimator()
    rng = np.random.default_rng(3)
    accums = growing_accums(rng, h, w, [4, 8])
    for a, t in zip(accums, [4, 8]):
        est.update(a, np.full(6, t))
    e = np.zeros((h, w), F)
    e[3, 9] = 0.3   # one pixel of block 1 above
    blocks, s, _ = _copy(est).select(0.2, FLOOR, 1, e=e)
    assert blocks.tolist() == [1] and s["above"] == 1 and s["active_blocks"] == 1
    blocks, _, _ = _copy(est).select(0.2, FLOOR, 9, e=np.zeros((h, w), F))   # sky: e all zero, but fewer than min_paths
    assert blocks.tolist() == [0, 1, 2, 3, 4, 5]
    blocks, _, _ = _copy(est).select(0.2, FLOOR, 8, e=np.zeros((h, w), F))
    assert blocks.tolist() == []
    one = _copy(est)
    assert one.select(0.2, FLOOR, 1, e=e)[0].tolist() == [1]
    assert one.select(0.2, FLOOR, 1, e=np.full((h, w), 0.5, F))[0].tolist() == [1], "a retired block came back"
    nan = _copy(est)
    nan.state[12, 20, 1] = np.nan   # block 5
    blocks, s, e2 = nan.select(1e9, FLOOR, 1)
    assert blocks.tolist() == [5] and s["non_finite"] == 1 and np.isnan(e2[12, 20])
    young = AR.Estimator()
    young.update(accums[0], np.full(6, 4))
    blocks, s, e3 = young.select(1e9, FLOOR, 1)   # one batch: no estimate, every block stays
    assert blocks.tolist() == [0, 1, 2, 3, 4, 5] and np.isinf(e3).all() and s["above"] == h * w


def plan_active(ops, max_runs=4096):
    """tests/test_run_planner.py `plan` through the second hook (op 7: ACTIVE(blocks)); a record's second word is the run's slots."""
    import ctypes as C
    from gpuart_amd import binding as B
    from tests.test_run_planner import DEFAULTS as c
    cfgv = (C.c_uint32 * 8)(c["batch_limit"], c["lanes"], c["batch_mpaths"], c["min_run_kpaths"], c["small_kpaths"], c["lane_budget_mb"], c["plan_percent"], 0)
    flat = np.ascontiguousarray(np.array(ops, np.uint32).reshape(-1, 3))
    out = np.zeros((max_runs, 6), np.uint32)
    L = B.hip_lib()
    n = L.gpuart_hip_test_planner_active(cfgv, flat.ctypes.data_as(C.POINTER(C.c_uint32)), len(flat), out.ctypes.data_as(C.POINTER(C.c_uint32)), max_runs)
    assert 0 <= n <= max_runs, (n, L.gpuart_hip_last_error().decode())
    return [tuple(int(v) for v in row) for row in out[:n]]


def test_the_planner_plans_from_the_active_slots():
    """1080p in mode 0: 64 planned passes of the whole frame go through the launch pipeline in runs of at most the 8 passes a lane holds;
    with 300 of the 32400 blocks listed the same 64 passes are 1.2 M paths, below small_paths: one k_run launch of 64 x 300 slots per
    pass, still within the lanes' max_batch of the allocation (8: 64 passes are 8 runs); dropping the list brings the first plan back.
    Every pass is launched exactly once, and setting a list flushes."""
    from tests.test_run_planner import FLUSH, MODE, PASS, PLAN, RESIZE
    ACTIVE = 7
    ops = [(RESIZE, 1920, 1080), (MODE, 0, 0), (PLAN, 64, 0), (PASS, 64, 0), (FLUSH, 0, 0),
           (PASS, 3, 0), (ACTIVE, 300, 0), (PLAN, 64, 0), (PASS, 64, 0), (FLUSH, 0, 0),
           (ACTIVE, 0, 0), (PLAN, 64, 0), (PASS, 64, 0), (FLUSH, 0, 0)]
    runs = plan_active(ops)
    whole = [r for r in runs if r[0] in (3, 4)]
    flushed = [r for r in runs if r[0] == 6]
    sparse = [r for r in runs if r[0] in (8, 9)]
    again = [r for r in runs if r[0] in (12, 13)]
    full_slots = 240 * 135 * 64
    assert sum(r[3] for r in whole) == 64 and all(r[1] == full_slots and r[2] == 8 and r[3] <= 8 and r[4] == 0 for r in whole), whole
    assert sum(r[3] for r in flushed) == 3 and all(r[1] == full_slots for r in flushed), flushed   # (the list's own flush: the old slots)
    assert sum(r[3] for r in sparse) == 64 and all(r[1] == 300 * 64 and r[2] == 8 and r[3] <= 8 and r[4] == 1 for r in sparse), sparse
    assert [r[1:5] for r in again] == [r[1:5] for r in whole]
    with pytest.raises(AssertionError):
        plan_active([(RESIZE, 64, 48), (ACTIVE, 49, 0)])   # more blocks than the tile has


@functools.lru_cache(maxsize=None)
def render_inputs(scene, W=64, H=48, passes=64):
    """(tree, camera, oracle params, the Renderer's camera dict, the colours of `passes` one-path passes with the Renderer's RandSeeds)."""
    from gpuart_amd import synth_scenes as S
    from oracle import oracle as O
    from tests.util import default_camera, scene as descs
    cam = default_camera()
    tree, _ = O.build_bvh(descs(scene))
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    colours = []
    for sd in O.randseeds(passes):
        a = np.zeros((H, W, 4), F)
        O.pt_pass(tree, c, W, H, P, sd, 1, a, nthreads=4)
        colours.append(a)
    return tree, c, P, cam, colours


def ref_loop(scene, threshold, min_paths, batch=4, cap=64):
    tree, c, P, cam, colours = render_inputs(scene)
    H, W = colours[0].shape[:2]
    nb = len(AR.block_pixels(H, W))
    return AR.render_adaptive(AR.Estimator(), lambda k, n: colours[k], np.zeros((H, W, 4), F), np.zeros(nb, np.int64), 0, cap, 1, batch,
                              threshold, min_paths, FLOOR)


@pytest.mark.parametrize("min_paths", [1, 10, 16])
def test_the_loop_on_the_box_spends_fewer_paths_than_the_uniform_rule(min_paths):
    """Oracle accumulators of the box at 64 x 48, batches of 4, threshold 0.2: the sky's blocks retire at the first point allowed — the
    first batch end with at least min_paths paths and two batches —, others later, and the paths spent stay below what the uniform stop
    rule (converge_ref.stops_at, no pixel above) spends on the same pass colours."""
    rc, s, accum, counts, issued, active = ref_loop("box", 0.2, min_paths)
    first = max(8, -(-min_paths // 4) * 4)
    print("min_paths %d: converged %d, issued %d, paths %d..%d, sum %d, active %d" % (min_paths, rc, issued, s["paths_min"], s["paths_max"], s["paths_sum"], s["active_blocks"]))
    assert s["paths_min"] == first and s["paths_max"] > s["paths_min"] and s["paths_max"] == issued
    colours = render_inputs("box")[4]
    acc, accums = np.zeros_like(colours[0]), []
    for k, col in enumerate(colours):
        acc = acc + col
        if k % 4 == 3:
            accums.append(acc)
    k, _ = converge_ref.stops_at(accums, [4 * (i + 1) for i in range(len(accums))], 0.2, 0.0, FLOOR)
    uniform = (4 * (k + 1) if k is not None else 64) * acc.shape[0] * acc.shape[1]
    print("  the uniform rule stops at %s: %d paths" % (k, uniform))
    assert s["paths_sum"] < uniform
    assert_same_bits(AR.normalize(accum, counts)[..., :3], accum[..., :3] / counts.astype(F)[AR.pixel_blocks(*accum.shape[:2])][..., None], "normalize")


# ---- GPU: passes over an active list ----------------------------------------------------------------------------------------------
FRAMES = [(40, 24), (37, 21)]
SCENES = ("box", "scene_p", "scene_d")   # all types, round, flat: each k_trace / k_run type class


def lists_of(W, H):
    bh, bw = AR.block_grid(H, W)
    nb = bh * bw
    return {"one": [nb // 2], "corner": [nb - 1], "checker": [t for t in range(nb) if (t // bw + t % bw) % 2 == 0],
            "all_but_one": [t for t in range(nb) if t != 1], "all": list(range(nb)), "empty": []}


@functools.lru_cache(maxsize=None)
def pass_colours(scene, W, H, sun, depth, npaths, n=8):
    """(tree, camera, params, colours of n passes) of a scene as tests/test_kernel_variants.py sets it up."""
    from oracle import oracle as O
    tree = tree_of(scene)
    c, P, _, _, _ = scene_setup(O, tree, W, H)
    P.sunEnabled = 1 if sun else 0
    P.maxSegments = depth
    out = []
    for sd in O.randseeds(n, seed=77 + npaths):
        a = np.zeros((H, W, 4), F)
        O.pt_pass(tree, c, W, H, P, sd, npaths, a)
        out.append(a)
    return tree, c, P, O.randseeds(n, seed=77 + npaths), out


def masked_add(acc, colour, mask):
    new = acc.copy()
    new[..., :3] = acc[..., :3] + colour[..., :3]
    return np.where(mask[..., None], new, acc)


def _cases():
    out = []
    for i, (sc, mode) in enumerate(itertools.product(SCENES, (0, 3, 5))):
        for rep in (0, 1):
            k = 2 * i + rep
            out.append(dict(scene=sc, mode=mode, frame=FRAMES[(i + rep) % 2], runs=(1, 3, 8)[(i // 3 + i + rep) % 3], npaths=1 + (k // 2 + rep) % 2,
                            sun=bool((k // 3) % 2 == 0), depth=(5, 1)[(k // 5 + rep) % 2], packet=(None, "0")[(k // 4) % 2], gen_walk=(None, "0")[(k // 2 + i // 3) % 2]))
    return out


CASES = _cases()


def _case_id(c):
    return "%s-m%d-%dx%d-r%d-p%d-sun%d-d%d-pk%s-gw%s" % (c["scene"], c["mode"], c["frame"][0], c["frame"][1], c["runs"], c["npaths"], c["sun"], c["depth"],
                                                     c["packet"] or "d", c["gen_walk"] or "d")


def test_the_cases_cover_every_setting():
    for key, values in (("mode", {0, 3, 5}), ("runs", {1, 3, 8}), ("npaths", {1, 2}), ("sun", {True, False}), ("depth", {1, 5}), ("packet", {None, "0"}),
                        ("gen_walk", {None, "0"}), ("frame", set(FRAMES)), ("scene", set(SCENES))):
        assert {c[key] for c in CASES} == values, key
    assert {(c["scene"], c["mode"]) for c in CASES} == set(itertools.product(SCENES, (0, 3, 5)))


def _env(monkeypatch, **env):
    for k in ("GPUART_HIP_PACKET", "GPUART_HIP_GEN_WALK", "GPUART_HIP_CHUNK", "GPUART_HIP_TILE_ORDER", "GPUART_HIP_LEAN_KERNELS", "GPUART_HIP_NEAREST_MIN_PRIMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if v is not None:
            monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def backend(B, tree, c, W, H, mode=0):
    b = B.Backend(0)
    b.resize(W, H); b.upload_bvh(tree); b.set_camera(c); b.set_mode(mode)
    return b


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_listed_passes_equal_the_masked_oracle_sum(B, case, monkeypatch):
    """Every list, each from a reset accumulator that first takes one plain pass: the listed blocks gain the run's pass colours in pass
    order, every other pixel keeps its bits, and the block counts are those the test kept."""
    _env(monkeypatch, GPUART_HIP_PACKET=case["packet"], GPUART_HIP_GEN_WALK=case["gen_walk"])
    (W, H), runs, npaths = case["frame"], case["runs"], case["npaths"]
    tree, c, P, seeds, colours = pass_colours(case["scene"], W, H, case["sun"], case["depth"], npaths)
    p = to_params(B, P)
    b = backend(B, tree, c, W, H, case["mode"])
    try:
        for name, blocks in lists_of(W, H).items():
            what = "%s, list %s" % (_case_id(case), name)
            b.pt_reset()
            assert (b.block_paths() == 0).all(), what
            b.pt_pass(p, seeds[0], npaths)
            acc = masked_add(np.zeros((H, W, 4), F), colours[0], np.ones((H, W), bool))
            counts = np.full(b.n_blocks(), npaths, np.uint32)
            b.set_active_blocks(blocks)
            b.pt_plan(runs)
            mask = AR.block_mask(H, W, blocks)
            for k in range(runs):
                b.pt_pass(p, seeds[k % 7 + 1], npaths)
                acc = masked_add(acc, colours[k % 7 + 1], mask)
            counts[blocks] += runs * npaths
            got = b.read(1)
            assert_bits(got[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), what)
            assert (b.block_paths() == counts).all(), (what, b.block_paths(), counts)
            b.pt_plan(0)
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3, 5])
def test_a_sequence_of_lists_on_one_accumulator(B, mode, monkeypatch):
    """List A for 2 passes, B inside A for 3, none for 1, then C, which is no subset of either, for 1; counts exported to the device too."""
    import torch
    _env(monkeypatch)
    W, H = 37, 21
    tree, c, P, seeds, colours = pass_colours("box", W, H, True, 5, 1)
    nb = len(AR.block_pixels(H, W))
    A, Bl, Cl = [0, 2, 3, 5, 7, 8, 11, 14], [2, 5, 8, 14], [1, 2, 4, 13]
    b = backend(B, tree, c, W, H, mode)
    try:
        acc, counts, k = np.zeros((H, W, 4), F), np.zeros(nb, np.uint32), 0
        for blocks, n in ((A, 2), (Bl, 3), (None, 1), (Cl, 1)):
            b.set_active_blocks(blocks)
            listed = list(range(nb)) if blocks is None else blocks
            for _ in range(n):
                b.pt_pass(to_params(B, P), seeds[k], 1)
                acc = masked_add(acc, colours[k], AR.block_mask(H, W, listed))
                k += 1
            counts[listed] += n
            if blocks is Bl:   # a read-back between two lists
                assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "mode %d, after B" % mode)
        dev = torch.zeros(nb, dtype=torch.int32, device="cuda:0")
        b.block_paths(dev.data_ptr())
        b.finish()
        assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "mode %d" % mode)
        assert (dev.cpu().numpy().view(np.uint32) == counts).all() and (b.block_paths() == counts).all()
        b.pt_reset()   # the list and the counts are gone: a plain pass again
        b.pt_pass(to_params(B, P), seeds[0], 1)
        assert_bits(b.read(1)[..., :3].reshape(-1, 3), colours[0][..., :3].reshape(-1, 3), "mode %d, after a reset" % mode)
        assert (b.block_paths() == 1).all()
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tile", "interleaved"])
def test_a_tile_and_an_interleaved_share_with_a_list(B, kind, monkeypatch):
    from oracle import oracle as O
    _env(monkeypatch)
    W, H = 64, 48
    tree, c, P, seeds, colours = pass_colours("box", W, H, True, 5, 1, n=3)
    b = backend(B, tree, c, W, H)
    try:
        if kind == "tile":
            b.set_tile(11, 5, 37, 21)
            rows, cols = np.arange(5, 26), slice(11, 48)
        else:
            g = B.share_of_rank(W, H, 1, 2, 4)
            b.set_share(g)
            rows, cols = g.rows(), slice(g.x0, g.x0 + g.tw)
        _, _, tw, th = b.tile
        blocks = lists_of(tw, th)["checker"]
        mask = AR.block_mask(th, tw, blocks)
        acc = np.zeros((th, tw, 4), F)
        b.pt_reset()
        b.set_active_blocks(blocks)
        for k in range(3):
            b.pt_pass(to_params(B, P), seeds[k], 1)
            acc = masked_add(acc, np.ascontiguousarray(colours[k][rows][:, cols]), mask)
        assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), kind)
        counts = np.zeros(b.n_blocks(), np.uint32)
        counts[blocks] = 3
        assert (b.block_paths() == counts).all()
        b.set_tile(0, 0, 16, 16)   # a new tile drops the list and the counts
        assert (b.block_paths() == 0).all() and b.n_blocks() == 4
    finally:
        b.close()


@pytest.mark.gpu
def test_a_sparse_list_beyond_the_static_chunks(B, monkeypatch):
    """256 x 128, 300 random blocks of 512, 3 passes, chunks of 16: the waves take list entries from the shared cursor."""
    _env(monkeypatch, GPUART_HIP_CHUNK="16")
    W, H = 256, 128
    tree, c, P, seeds, colours = pass_colours("box", W, H, True, 5, 1, n=3)
    blocks = np.sort(np.random.default_rng(8).choice(512, 300, replace=False))
    mask = AR.block_mask(H, W, blocks)
    for mode in (3, 5):
        b = backend(B, tree, c, W, H, mode)
        try:
            b.set_active_blocks(blocks)
            acc = np.zeros((H, W, 4), F)
            for k in range(3):
                b.pt_pass(to_params(B, P), seeds[k], 1)
                acc = masked_add(acc, colours[k], mask)
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "mode %d" % mode)
        finally:
            b.close()


@pytest.mark.gpu
def test_a_bad_list_is_refused_and_changes_nothing(B, monkeypatch):
    _env(monkeypatch)
    W, H = 40, 24
    tree, c, P, seeds, colours = pass_colours("box", W, H, True, 5, 1)
    b = backend(B, tree, c, W, H)
    zero = np.zeros((H, W, 4), F)
    everywhere = np.ones((H, W), bool)
    try:
        for name, bad in (("out of range", [0, 15]), ("not ascending", [3, 2]), ("duplicate", [4, 4]), ("too long", list(range(15)) + [14])):
            # between two plain passes, with nothing reset after the attempt: the sum and the counts of two plain passes
            b.pt_reset()
            b.pt_pass(to_params(B, P), seeds[0], 1)
            with pytest.raises(B.HipError) as ei:
                b.set_active_blocks(bad)
            assert ei.value.code == ERR_ARG and "active blocks" in str(ei.value), name
            b.pt_pass(to_params(B, P), seeds[1], 1)
            two = masked_add(masked_add(zero, colours[0], everywhere), colours[1], everywhere)
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), two[..., :3].reshape(-1, 3), name)
            assert (b.block_paths() == 2).all(), name
            # with a list set: the list stays the one it was, and so do its counts
            kept = [1, 7, 14]
            b.set_active_blocks(kept)
            with pytest.raises(B.HipError) as ei:
                b.set_active_blocks(bad)
            assert ei.value.code == ERR_ARG, name
            b.pt_pass(to_params(B, P), seeds[2], 1)
            three = masked_add(two, colours[2], AR.block_mask(H, W, kept))
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), three[..., :3].reshape(-1, 3), name + ", over a list")
            counts = np.full(15, 2, np.uint32)
            counts[kept] += 1
            assert (b.block_paths() == counts).all(), name
        b.pt_reset()
        b.pt_pass(to_params(B, P), seeds[0], 1)
        b.set_active_blocks([1, 2])
        b.set_mode(2)
        with pytest.raises(B.HipError) as ei:
            b.pt_pass(to_params(B, P), seeds[1], 1)
        assert ei.value.code == ERR_ARG and "mode 2" in str(ei.value)
        b.set_mode(0)
        b.set_active_blocks(None)
        b.pt_pass(to_params(B, P), seeds[1], 1)
        assert_bits(b.read(1)[..., :3].reshape(-1, 3), (colours[0] + colours[1])[..., :3].reshape(-1, 3), "after the refused pass")
        assert (b.block_paths() == 2).all()
    finally:
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 3, 5])
def test_a_listed_pass_launches_only_what_the_plain_pass_launches(B, mode, monkeypatch):
    """The launch ledger of the test build (Backend.launched): no kernel of a listed pass is new, and k_tile_order is not among them."""
    _env(monkeypatch)
    W, H = 40, 24
    tree, c, P, seeds, _ = pass_colours("box", W, H, True, 5, 1)
    b = backend(B, tree, c, W, H, mode)
    try:
        b.launched()
        for k in range(2):   # single-pass runs: the plain ones gather and sort the birth order in modes 0 and 5
            b.pt_pass(to_params(B, P), seeds[k], 1)
            b.read(1)
        plain = names_of(b.launched())
        b.set_active_blocks([0, 3, 7, 14])
        for k in range(2):
            b.pt_pass(to_params(B, P), seeds[k], 1)
            b.read(1)
        b.block_paths()
        listed = names_of(b.launched())
        print("mode %d: plain %s, listed %s" % (mode, sorted(plain), sorted(listed)))
        assert "k_accumulate" in listed and listed <= plain and "k_tile_order" not in listed
    finally:
        b.close()


# ---- GPU: libgpuart_adaptive.so against its restatement -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def library_case(W, H):
    """Staggered accumulators and counts with a NaN pixel and a block that never gets a path, and what the restatement makes of them."""
    totals = [4, 8, 12, 20, 24]
    stop, full, accums, counts = staggered(H, W, totals, 21)
    nb = len(stop)
    pb = AR.pixel_blocks(H, W)
    dead = nb // 3
    nan_at = (H // 2, W // 2)
    for k in range(len(totals)):
        counts[k] = counts[k].copy()
        counts[k][dead] = 0
        accums[k] = accums[k].copy()
        accums[k][pb == dead] = 0
        steady = (np.arange(nb) % 4 == 1)[pb]   # blocks without any spread: they retire as soon as they may
        accums[k][steady] = (counts[k][pb][steady] * F(0.375))[:, None]
        accums[k][nan_at] = np.nan
    est = AR.Estimator()
    steps = []
    for k in range(len(totals)):
        state = est.update(accums[k], counts[k]).copy()
        blocks, s, e = est.select(0.1, FLOOR, 8) if k >= 1 else (None, None, None)
        steps.append(dict(state=state, block_state=est.block_state(), blocks=blocks, summary=s, e=e, norm=AR.normalize(accums[k], counts[k])))
    assert pb[nan_at] != dead and 0 < len(steps[-1]["blocks"]) < nb
    return accums, counts, steps


def assert_summary(got, exp, what):
    g, x = dict(got), dict(exp)
    assert np.float32(g.pop("max_error")).view(np.uint32) == np.float32(x.pop("max_error")).view(np.uint32), what
    assert g == x, what


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("size", [(37, 21), (160, 120)])
def test_the_library_equals_its_restatement(B, size, entry):
    import torch
    W, H = size
    accums, counts, steps = library_case(W, H)
    to = to_device if entry == "device" else (lambda a: a)
    back = (lambda t: t.cpu().numpy()) if entry == "device" else (lambda a: a)
    a = B.Adaptive(0)
    try:
        for k, st in enumerate(steps):
            what = "%d x %d, %s, batch %d" % (W, H, entry, k)
            paths = to(counts[k].astype(np.int32)) if entry == "device" else counts[k]
            a.update(to(accums[k]), paths)
            state, blk = a.state()
            assert_same_bits(state, st["state"], what + ": state")
            if k >= 1:
                emap = torch.full((H, W), 7.0, device="cuda:0")
                blocks, s = a.select(0.1, FLOOR, 8, error_map=emap)
                assert blocks.tolist() == st["blocks"].tolist(), what
                assert_summary(s, st["summary"], what)
                assert_same_bits(emap.cpu().numpy(), st["e"], what + ": error map")
                assert_same_bits(a.error_map(FLOOR).cpu().numpy(), st["e"], what + ": error_map entry point")
            assert (a.state()[1] == st["block_state"]).all(), what + ": block state"
            assert_same_bits(back(a.normalize(to(accums[k]), paths)), st["norm"], what + ": normalize")
        with pytest.raises(B.AdaptiveError) as ei:   # a count that went down: refused, nothing written
            a.update(accums[-1], np.maximum(counts[-1].astype(np.int64) - 1, 0).astype(np.uint32))
        assert ei.value.code == ERR_ARG and "already seen" in str(ei.value)
        with pytest.raises(B.AdaptiveError):
            a.update(accums[-1], np.full(len(counts[-1]), (1 << 24) + 1, np.uint32))
        assert_same_bits(a.state()[0], steps[-1]["state"], "state after the refused updates")
    finally:
        a.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(65536, 1), (1, 65536)])
def test_the_library_at_the_largest_extents(B, size):
    W, H = size
    rng = np.random.default_rng(W)
    nb = len(AR.block_pixels(H, W))
    accums = growing_accums(rng, H, W, [3, 7, 12])
    counts = [np.full(nb, 3), np.where(np.arange(nb) % 3 == 0, 3, 7), np.where(np.arange(nb) % 3 == 0, 3, np.where(np.arange(nb) % 3 == 1, 7, 12))]
    pb = AR.pixel_blocks(H, W)
    for k in (1, 2):   # a block that did not move keeps its accumulator
        keep = (counts[k] == counts[k - 1])[pb]
        accums[k][keep] = accums[k - 1][keep]
    est, a = AR.Estimator(), B.Adaptive(0)
    try:
        for k in range(3):
            est.update(accums[k], counts[k])
            a.update(accums[k], counts[k].astype(np.uint32))
        assert_same_bits(a.state()[0], est.state, "%d x %d: state" % size)
        blocks, s = a.select(0.05, FLOOR, 4)
        xb, xs, _ = est.select(0.05, FLOOR, 4)
        assert blocks.tolist() == xb.tolist()
        assert_summary(s, xs, "%d x %d" % size)
        assert_same_bits(a.normalize(accums[2], counts[2].astype(np.uint32)), AR.normalize(accums[2], counts[2]), "%d x %d: normalize" % size)
    finally:
        a.close()


# ---- GPU: Renderer::RenderAdaptive and gpuart_cli --adaptive ------------------------------------------------------------------------
MIN_PATHS, BATCH, CAP = 10, 4, 64   # (min_paths is no multiple of the batch: the first point a block may retire at is 12 paths)


def same_or_zero(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


def make_renderer(B, scene, cap=CAP):
    from gpuart_amd import synth_scenes as S
    from tests.util import scene as descs
    r = B.Renderer(64, 48, render_inputs(scene)[3])
    if scene == "box":
        r.init_box()
    else:
        r.set_primitives(descs(scene))
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.restart_path_tracing(1, cap)
    assert r.is_ok()
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("threshold", [0.1, 1e9])
@pytest.mark.parametrize("scene", ["box", "scene_p"])
def test_render_adaptive_equals_the_restatement_on_the_oracle(B, scene, threshold, tmp_path, capfd):
    rc, s_exp, accum, counts, issued, active = ref_loop(scene, threshold, MIN_PATHS)
    colours = render_inputs(scene)[4]
    H, W = accum.shape[:2]
    per_pixel = counts[AR.pixel_blocks(H, W)]
    what = "%s, threshold %g" % (scene, threshold)
    print("%s: restatement returns %d after %d paths issued, %d..%d per block, %d of %d blocks active" % (
        what, rc, issued, s_exp["paths_min"], s_exp["paths_max"], s_exp["active_blocks"], s_exp["blocks"]))
    r = make_renderer(B, scene)
    try:
        converged, s = r.render_adaptive(threshold, MIN_PATHS, BATCH, FLOOR)
        assert converged == (rc == 1) and s["paths_max"] == issued, (what, converged, s)
        assert_summary(s, s_exp, what)
        assert (r.read_sample_counts() == per_pixel).all(), what
        acc = r.read_radiance(False)
        assert same_or_zero(acc[..., :3], accum[..., :3]).all(), what
        assert same_or_zero(r.read_radiance(True)[..., :3], AR.normalize(accum, counts)[..., :3]).all(), what + ": normalised"
        assert same_or_zero(r.read_radiance(True)[..., :3], accum[..., :3] / per_pixel.astype(F)[..., None]).all()
        if threshold == 1e9:
            assert converged and (per_pixel == 12).all() and s["active_blocks"] == 0
        else:
            assert len(np.unique(counts)) >= 3, "the case does not stagger the blocks"
        # every block is that block of a plain render stopped at the block's count
        plain = make_renderer(B, scene)
        try:
            for n in range(1, int(counts.max()) + 1):
                plain.path_tracing_pass()
                if (counts == n).any():
                    sel = per_pixel == n
                    assert same_or_zero(acc[sel], plain.read_radiance(False)[sel]).all(), "%s: blocks stopped at %d paths" % (what, n)
        finally:
            plain.close()
        e = r.read_error_map(FLOOR)
        est = AR.Estimator()
        AR.render_adaptive(est, lambda k, n: colours[k], np.zeros_like(accum), np.zeros(len(counts), np.int64), 0, CAP, 1, BATCH, threshold, MIN_PATHS, FLOOR)
        assert same_or_zero(e, est.error(FLOOR)).all(), what + ": error map"
        assert r.read_refined(FLOOR) is not None
        # blocks have been retired: what takes one path count for the frame is refused and changes nothing
        assert s["active_blocks"] < s["blocks"]
        capfd.readouterr()
        with pytest.raises(B.HipError):
            r.render_until(0.1, 0.0, BATCH, FLOOR)
        assert "RenderUntil after adaptive sampling retired blocks" in capfd.readouterr().err
        assert not r.save_checkpoint(str(tmp_path / "ck")) and not os.path.exists(str(tmp_path / "ck"))
        assert "SaveCheckpoint after adaptive sampling retired blocks" in capfd.readouterr().err
        # (one rank: the gather needs no second GPU; the refusal comes before any communicator is made)
        assert B.Renderer.gather_radiance([r], 0, True) is None and B.Renderer.gather_radiance([r], 0, False) is None
        assert capfd.readouterr().err.count("GatherRadiance after adaptive sampling retired blocks") == 2
        with pytest.raises(ValueError):
            r.set_temporal_history(True)
        assert "temporal history after adaptive sampling retired blocks" in capfd.readouterr().err
        assert same_or_zero(r.read_radiance(False), acc).all() and (r.read_sample_counts() == per_pixel).all()
        assert same_or_zero(r.read_radiance(True)[..., :3], AR.normalize(accum, counts)[..., :3]).all(), what + ": normalised, after the refusals"
        # a restart: a plain render again, bit for bit, with uniform counts
        r.set_seed(5489)
        r.restart_path_tracing(1, 4)
        for _ in range(4):
            r.path_tracing_pass()
        four = functools.reduce(lambda a, c: a + c, colours[:4], np.zeros_like(accum))
        assert same_or_zero(r.read_radiance(False)[..., :3], four[..., :3]).all() and (r.read_sample_counts() == 4).all()
        assert same_or_zero(r.read_radiance(True)[..., :3], four[..., :3] / F(4)).all()
        assert r.read_error_map(FLOOR) is None and r.render_until(0.0, 0.0, 4, FLOOR)[0] is False
    finally:
        r.close()


@pytest.mark.gpu
def test_render_adaptive_at_the_cap_and_its_refusals(B):
    """min_paths above the cap: nothing retires, the call returns 0 with the accumulator of 64 plain passes and uniform counts, and
    RenderUntil still works; paths rendered before the call are the first batch; arguments out of range and temporal history are refused."""
    colours = render_inputs("box")[4]
    total = functools.reduce(lambda a, c: a + c, colours, np.zeros_like(colours[0]))
    r = make_renderer(B, "box")
    try:
        for _ in range(6):
            r.path_tracing_pass()
        converged, s = r.render_adaptive(0.1, 1000, BATCH, FLOOR)
        assert converged is False and s["active_blocks"] == s["blocks"] == 48 and s["paths_min"] == s["paths_max"] == CAP
        assert same_or_zero(r.read_radiance(False)[..., :3], total[..., :3]).all() and (r.read_sample_counts() == CAP).all()
        assert same_or_zero(r.read_radiance(True)[..., :3], total[..., :3] / F(CAP)).all()
        nb = 48
        est = AR.Estimator()   # batches of 6, 4, 4, ...: the first is what the plain passes left
        rc, s_exp, _, _, _, _ = AR.render_adaptive(est, lambda k, n: colours[k], functools.reduce(lambda a, c: a + c, colours[:6], np.zeros_like(total)),
                                                   np.full(nb, 6), 6, CAP, 1, BATCH, 0.1, 1000, FLOOR)
        assert rc == 0
        assert_summary(s, s_exp, "after six plain passes")
        assert r.render_until(0.0, 0.0, BATCH, FLOOR)[0] is False and r.save_checkpoint(os.devnull)
        for bad in (dict(threshold=-1.0), dict(threshold=float("nan")), dict(min_paths=0), dict(batch_paths=0), dict(lum_floor=0.0)):
            with pytest.raises(B.HipError):
                r.render_adaptive(**dict(dict(threshold=0.1, min_paths=1, batch_paths=4, lum_floor=FLOOR), **bad))
        r.set_temporal_history(True)
        with pytest.raises(B.HipError):
            r.render_adaptive(0.1, 1, 4, FLOOR)
        assert same_or_zero(r.read_radiance(False)[..., :3], total[..., :3]).all()
    finally:
        r.close()


@pytest.mark.gpu
def test_the_error_map_is_that_of_the_estimate_that_saw_the_last_batch(B):
    """RenderUntil, RenderAdaptive, RenderUntil on one accumulation: read_error_map and read_refined take the adaptive estimate's map
    after the second call and the uniform estimate's again after the third, bit for bit, and the two maps differ."""
    from tests.test_refine import expected_refined
    colours = render_inputs("box")[4]
    sums = {n: functools.reduce(lambda a, c: a + c, colours[:n], np.zeros_like(colours[0])) for n in (4, 8, CAP)}
    r = make_renderer(B, "box")
    try:
        converged, s = r.render_until(1e9, 0.0, BATCH, FLOOR)
        assert converged and s["total"] == 8 and s["batches"] == 2
        converged, s = r.render_adaptive(0.1, 1000, BATCH, FLOOR)   # the 8 paths are its first batch, of their own weight
        assert converged is False and s["active_blocks"] == s["blocks"] == 48 and s["paths_min"] == s["paths_max"] == CAP
        est = AR.Estimator()
        rc = AR.render_adaptive(est, lambda k, n: colours[k], sums[8], np.full(48, 8), 8, CAP, 1, BATCH, 0.1, 1000, FLOOR)[0]
        assert rc == 0 and est.updates == 15
        e_adaptive = est.error(FLOOR)
        assert_same_bits(r.read_error_map(FLOOR), e_adaptive, "error map after RenderAdaptive")
        assert_same_bits(r.read_refined(FLOOR), expected_refined(r, B), "read_refined after RenderAdaptive")
        converged, s = r.render_until(1e9, 0.0, BATCH, FLOOR)   # nothing left to render: the 56 paths are its third batch
        assert converged and s["batches"] == 3 and s["total"] == CAP
        uni = converge_ref.Estimator()
        for n in (4, 8, CAP):
            uni.update(sums[n], n)
        e_uniform = uni.error(FLOOR)
        assert_same_bits(r.read_error_map(FLOOR), e_uniform, "error map after RenderUntil took the turn back")
        assert_same_bits(r.read_refined(FLOOR), expected_refined(r, B), "read_refined after RenderUntil took the turn back")
        differ = e_adaptive.view(np.uint32) != e_uniform.view(np.uint32)
        assert np.isfinite(e_adaptive).all() and np.isfinite(e_uniform).all() and differ.sum() > differ.size // 2, int(differ.sum())
        r.restart_path_tracing(1, CAP)
        assert r.read_error_map(FLOOR) is None and r.read_refined(FLOOR) is None
    finally:
        r.close()


@pytest.mark.gpu
def test_render_adaptive_after_a_loaded_checkpoint(B, tmp_path):
    """A loaded checkpoint's six paths are the first batch, of their own weight, and part of every count: the counts, the summary and the
    accumulator are the restatement's on the oracle's colours from pass 6 on (the checkpoint restores the generator), whatever the
    Renderer had rendered before the load, and the normalised frame divides by checkpoint plus new paths."""
    colours = render_inputs("box")[4]
    six = functools.reduce(lambda a, c: a + c, colours[:6], np.zeros_like(colours[0]))
    ck = str(tmp_path / "six.ck")
    r = make_renderer(B, "box")
    try:
        for _ in range(6):
            r.path_tracing_pass()
        assert r.save_checkpoint(ck)
    finally:
        r.close()
    rc, s_exp, accum, counts, issued, _ = AR.render_adaptive(AR.Estimator(), lambda k, n: colours[k], six, np.full(48, 6), 6, CAP, 1, BATCH, 0.1, MIN_PATHS, FLOOR)
    per_pixel = counts[AR.pixel_blocks(48, 64)]
    assert s_exp["paths_min"] == 10 and len(np.unique(counts)) >= 3, "the case does not stagger the blocks"
    r = make_renderer(B, "box")
    try:
        for _ in range(3):   # paths of another accumulation, which the load discards with their counts
            r.path_tracing_pass()
        assert r.load_checkpoint(ck)
        assert (r.read_sample_counts() == 6).all() and same_or_zero(r.read_radiance(False)[..., :3], six[..., :3]).all()
        converged, s = r.render_adaptive(0.1, MIN_PATHS, BATCH, FLOOR)
        assert converged == (rc == 1) and s["paths_max"] == issued
        assert_summary(s, s_exp, "after a checkpoint of six paths")
        assert (r.read_sample_counts() == per_pixel).all()
        assert same_or_zero(r.read_radiance(False)[..., :3], accum[..., :3]).all()
        assert same_or_zero(r.read_radiance(True)[..., :3], AR.normalize(accum, counts)[..., :3]).all()
        # every block is that block of the plain sum of the first n colours
        acc, plain = r.read_radiance(False), np.zeros_like(six)
        for n in range(1, int(counts.max()) + 1):
            plain = plain + colours[n - 1]
            sel = per_pixel == n
            assert same_or_zero(acc[sel][..., :3], plain[sel][..., :3]).all(), "blocks stopped at %d paths" % n
    finally:
        r.close()


def read_pfm(path, w, h, grey=False):
    raw = open(path, "rb").read()
    head = b"P%s\n%d %d\n-1.0\n" % (b"f" if grey else b"F", w, h)
    assert raw.startswith(head), raw[:32]
    return np.frombuffer(raw[len(head):], F).reshape((h, w) if grey else (h, w, 3))


@pytest.mark.gpu
def test_cli_adaptive(B, tmp_path):
    """gpuart_cli --adaptive: its line, its frame and --samples-pfm are the Python path's; --refine writes read_refined; the refusals."""
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", "64", "--height", "48", "--per-pass", "1", "--spp", str(CAP)]
    ad = ["--adaptive", "0.1", "--adaptive-min", str(MIN_PATHS), "--until-batch", str(BATCH), "--until-floor", "%.9g" % FLOOR]
    pfm, spfm, rpfm = str(tmp_path / "a.pfm"), str(tmp_path / "s.pfm"), str(tmp_path / "r.pfm")
    out = subprocess.run(base + ad + ["--pfm", pfm, "--samples-pfm", spfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and "adaptive" in lines[0], out.stdout
    out = subprocess.run(base + ad + ["--refine", "--pfm", rpfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    r = make_renderer(B, "box")
    try:
        converged, s = r.render_adaptive(0.1, MIN_PATHS, BATCH, FLOOR)
        u = lines[0]
        assert u["converged"] is converged and u["paths_issued"] == s["paths_max"] == lines[1]["paths_per_pixel"]
        assert (u["paths_min"], u["paths_max"], u["active_blocks"], u["blocks"]) == (s["paths_min"], s["paths_max"], s["active_blocks"], s["blocks"])
        assert u["paths_mean"] == pytest.approx(s["paths_sum"] / s["pixels"], rel=1e-8) and F(u["max_error"]).view(np.uint32) == F(s["max_error"]).view(np.uint32)
        assert (read_pfm(spfm, 64, 48, grey=True) == r.read_sample_counts().astype(F)).all()
        assert same_or_zero(read_pfm(pfm, 64, 48), r.read_radiance(True)[..., :3]).all()
        assert same_or_zero(read_pfm(rpfm, 64, 48), r.read_refined(FLOOR)[..., :3]).all()
    finally:
        r.close()
    for extra, word in ((["--until", "0.1"], "--adaptive"), (["--denoise"], "--adaptive"), (["--checkpoint", str(tmp_path / "ck")], "--adaptive"),
                        (["--gpus", "2"], "--adaptive")):
        out = subprocess.run(base + ad + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and word in out.stderr and not out.stdout, (extra, out.returncode, out.stdout, out.stderr)
    out = subprocess.run(base + ["--refine"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--refine" in out.stderr and not out.stdout
