"""Neighbour lists: every primitive within r of a point (include/gpuart_nearest.h "Neighbour lists", libgpuart_nearest.so:
gpuart_nearest_within_*; Backend.within, Renderer::PrimitivesWithin). On the CPU: the definition (gpuart_nearest_within_brute_host) is the
restatement's (tests/within_ref.py) byte for byte on every rule case under eight radii per query, the restated pruned walk with the lower
child first is the definition, the upper child first gives the same sets in another order, and five named wrong rules are told from the
right one. On the GPU: offsets and items of k_within_count and k_within_fill are the restatement's over the device's own arrays, in the
order of the device's own tree, byte for byte — through the scene's life, for query counts around the wave and the chunk, under every grid
and spill limit, through every input kind; the capacity protocol never writes outside what it was given; and what must be refused is
refused with nothing written. There is no tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nearest_cases as NC
from tests import nearest_ref as NR
from tests import within_cases as WC
from tests import within_ref as WR

F = np.float32
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
US = NC.USER_SPHERES[1]
INF = float("inf")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def brute_host(B, recs, prims, boxes, root_ref, points, us=None):
    """gpuart_nearest_within_brute_host by its two-call protocol, with no device: (offsets, items)."""
    L = B.nearest_lib()
    recs, prims, boxes = np.ascontiguousarray(recs, F), np.ascontiguousarray(prims, F), np.ascontiguousarray(boxes, F)
    points = np.ascontiguousarray(points, F)
    offsets = np.full(len(points) + 1, 0xdddddddd, np.uint32)
    total = C.c_uint64(123)
    usp = None if us is None else (C.c_float * 4)(*us)
    args = (_p(recs), C.c_size_t(len(recs)), C.c_uint32(int(root_ref)), _p(prims), _p(boxes), C.c_size_t(len(prims)), _p(points), C.c_size_t(len(points)), usp,
            _p(offsets))
    assert L.gpuart_nearest_within_brute_host(*args, None, C.c_size_t(0), C.byref(total)) == 0, L.gpuart_nearest_last_error().decode()
    assert offsets[0] == 0 and offsets[-1] == total.value
    first = offsets.copy()
    items = np.zeros(total.value, NR.HIT)
    assert L.gpuart_nearest_within_brute_host(*args, _p(items), C.c_size_t(len(items)), C.byref(total)) == 0, L.gpuart_nearest_last_error().decode()
    assert (offsets == first).all() and total.value == len(items)
    return offsets, items


def assert_lists(got, exp, what):
    (go, gi), (eo, ei) = got, exp
    go, eo = np.ascontiguousarray(go).view(np.uint32), np.ascontiguousarray(eo).view(np.uint32)
    assert go.shape == eo.shape, what
    assert (go == eo).all(), "%s: offsets differ; first at %d: got %s expected %s" % (what, int(np.argmax(go != eo)), go[go != eo][:4], eo[go != eo][:4])
    gi, ei = np.ascontiguousarray(gi), np.ascontiguousarray(ei)
    assert gi.dtype.itemsize == 32 and ei.dtype.itemsize == 32 and gi.shape == ei.shape, (what, gi.shape, ei.shape)
    a, b = gi.view(np.uint32).reshape(-1, 8), ei.view(np.uint32).reshape(-1, 8)
    bad = (a != b).any(1)
    assert not bad.any(), "%s: %d of %d items differ; first %d: got %s expected %s" % (what, int(bad.sum()), len(bad), int(np.argmax(bad)),
                                                                                       gi.reshape(-1)[bad][0], ei.reshape(-1)[bad][0])


def lists_of(res):
    """The lists as Python lists of ordinals."""
    o, it = res
    return [it["prim"][o[i]:o[i + 1]].tolist() for i in range(len(o) - 1)]


# ---- CPU: the definition against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("us", NC.USER_SPHERES, ids=["no user sphere", "user sphere"])
@pytest.mark.parametrize("name", NC.RULE_CASES)
def test_the_definition_is_the_restatements(B, name, us):
    c = WC.rule_case(name)
    exp = WR.brute(c["recs"], c["prims"], c["boxes"], c["root"], c["points"], us)
    got = brute_host(B, c["recs"], c["prims"], c["boxes"], c["root"][2], c["points"], us)
    assert_lists(got, exp, name)
    ln = np.diff(exp[0].astype(np.int64)).reshape(-1, WC.RADII_PER_QUERY)
    valid = np.isfinite(c["points"][::WC.RADII_PER_QUERY, :3]).all(1)
    every = len(c["prims"]) + (us is not None)
    assert (ln[valid, 5] == every).all(), "%s: r = +inf lists everything" % name
    assert (ln[:, 6:] == 0).all() and (ln[~valid] == 0).all(), "%s: an invalid query has an empty list" % name
    if name != "misses" and us is None:
        # the query's own nearest distance lists its nearest primitive where r r rounds to no less than its d2; one ulp less never lists more
        assert (ln[valid, 3] <= ln[valid, 2]).all() and (ln[valid, 2] >= 1).any() and (ln[valid, 2] <= ln[valid, 5]).all(), name
    for i, l in enumerate(lists_of(exp)):
        assert l == sorted(l, key=lambda k: (k != -2, k)), "%s: a root leaf's order is the user sphere, then the ordinals" % name


# ---- CPU: the restated pruned walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["morton", "clustered"])
@pytest.mark.parametrize("name", list(WC.TREE_SCENES))
def test_the_pruned_walk_is_the_definition_and_the_order_clause_bites(B, name, kind):
    recs, prims, boxes, root = WC.tree_arrays(name, kind)
    points = WC.query_set(boxes, 96 if len(prims) > 100 else 48, seed=len(prims))
    order = WR.tree_order(recs, prims, root[2])
    assert sorted(order) == list(range(len(prims)))
    for us in NC.USER_SPHERES:
        what = "%s %s%s" % (name, kind, ", user sphere" if us else "")
        exp = WR.brute(recs, prims, boxes, root, points, us)
        assert_lists(brute_host(B, recs, prims, boxes, root[2], points, us), exp, what + ": the definition derives the tree's order from the records")
        assert_lists(WR.walk(recs, prims, boxes, root, points, us, "lower"), exp, what + ": lower child first")
        rank = {k: i for i, k in enumerate([-2] + order)}
        assert all(l == sorted(l, key=rank.get) for l in lists_of(exp)), what
        upper = WR.walk(recs, prims, boxes, root, points, us, "upper")
        assert (upper[0] == exp[0]).all(), what
        a, b = lists_of(upper), lists_of(exp)
        assert [sorted(l) for l in a] == [sorted(l) for l in b], what + ": upper child first lists the same sets"
        assert a != b, what + ": ... in another order"


# ---- CPU: the wrong rules, each caught by its named case ---------------------------------------------------------------------------------------
def duplicates_case():
    """The Morton tree of nearest_cases.duplicates() and the query p = (3, 0, 0), r = 2: the six coincident spheres have d2 = r2 = box_d2 = 4."""
    from tests import build_ref as BR
    tree = BR.build(NC.duplicates()[0])[0]
    return tree, NR.from_tree(tree), np.array([[3, 0, 0, 2]], F)


def test_pruning_at_exactly_r_loses_items(B):
    tree, (recs, dprims, boxes, root), points = duplicates_case()
    copies = [k for k in WR.tree_order(recs, dprims, root[2]) if (dprims[k, 0, :3] == 0).all()]
    assert len(copies) == 6
    exp = WR.brute(recs, dprims, boxes, root, points)
    assert lists_of(exp) == [copies] and (exp[1]["d2"] == 4).all() and (exp[1]["dist"] == 2).all()
    lo, hi = boxes[copies[0], :3], boxes[copies[0], 3:]
    assert NR.box_d2(lo, hi, points[:, :3])[0] == 4, "box_d2 = d2 = r2"
    assert_lists(brute_host(B, recs, dprims, boxes, root[2], points), exp, "duplicates: the definition")
    assert_lists(WR.walk(recs, dprims, boxes, root, points), exp, "duplicates")
    wrong = WR.walk(recs, dprims, boxes, root, points, mutant="prune_ge")
    assert len(wrong[1]) < 6


def test_a_primitive_at_exactly_r_is_listed(B):
    prims, points = NC.at_radius()
    recs, boxes = NC.device_list(prims)
    recs0, dprims, root_ref = WC.root_leaf(recs)
    root = (boxes[0, :3], boxes[0, 3:], root_ref)
    exp = WR.brute(recs0, dprims, boxes, root, points)
    assert lists_of(exp) == [[0], [0], []]
    assert_lists(brute_host(B, recs0, dprims, boxes, root_ref, points), exp, "at the radius")
    assert lists_of(WR.brute(recs0, dprims, boxes, root, points, mutant="strict_accept")) == [[], [], []]


def test_the_second_primitive_of_a_pair_is_listed(B):
    from tests import build_ref as BR
    prims, points = NC.second_of_two()
    recs, dprims, boxes, root = NR.from_tree(BR.build(prims)[0])
    assert len(recs) == 0 and root[2] & NR.REF_LEAF and root[2] & NR.REF_TWO, "the root is a leaf of two"
    exp = WR.brute(recs, dprims, boxes, root, points)
    assert lists_of(exp) == [[0, 1]] * 3
    assert_lists(brute_host(B, recs, dprims, boxes, root[2], points), exp, "second of two")
    assert_lists(WR.walk(recs, dprims, boxes, root, points), exp, "second of two, walked")
    assert lists_of(WR.walk(recs, dprims, boxes, root, points, mutant="skip_second")) == [[0]] * 3


def test_without_the_clamp_the_item_is_another(B):
    prims, points = NC.unclamped()
    recs, boxes = NC.device_list(prims)
    recs0, dprims, root_ref = WC.root_leaf(recs)
    root = (boxes[0, :3], boxes[0, 3:], root_ref)
    clamped = NR.brute(dprims, boxes, points)
    r = clamped["dist"][0]          # the clamped distance, or the float above it where its square rounds below d2
    if r * r < clamped["d2"][0]:
        r = np.nextafter(r, F(INF))
    points = np.array([[*points[0, :3], r]], F)
    exp = WR.brute(recs0, dprims, boxes, root, points)
    assert lists_of(exp) == [[0]] and exp[1]["q"][0, 0] == boxes[0, 3]
    assert_lists(brute_host(B, recs0, dprims, boxes, root_ref, points), exp, "unclamped")
    wrong = WR.brute(recs0, dprims, boxes, root, points, mutant="no_clamp")
    assert wrong[1].tobytes() != exp[1].tobytes() and wrong[1]["q"][0, 0] > boxes[0, 3]


def test_a_best_so_far_loses_items(B):
    recs, prims, boxes, root = WC.tree_arrays("mixed300", "morton")
    points = WC.query_set(boxes, 48, seed=3)
    exp = WR.brute(recs, prims, boxes, root, points)
    assert_lists(brute_host(B, recs, prims, boxes, root[2], points), exp, "mixed300: the definition")
    wrong = WR.walk(recs, prims, boxes, root, points, mutant="best_so_far")
    assert wrong[0][-1] < exp[0][-1] and all(set(a) <= set(b) for a, b in zip(lists_of(wrong), lists_of(exp)))


# ---- CPU: the definition's arguments, and the library as built ----------------------------------------------------------------------------------
def test_brute_host_refuses_null_arrays_and_a_short_capacity_leaves_items_alone(B):
    L = B.nearest_lib()
    c = WC.rule_case("box faces")
    recs, prims, boxes, points = (np.ascontiguousarray(c[k], F) for k in ("recs", "prims", "boxes", "points"))
    n, P = len(points), len(prims)
    offsets = np.zeros(n + 1, np.uint32)
    total = C.c_uint64(0)
    call = lambda prims_p, boxes_p, points_p, offsets_p, items_p, cap, total_p: L.gpuart_nearest_within_brute_host(
        None, C.c_size_t(0), C.c_uint32(int(c["root"][2])), prims_p, boxes_p, C.c_size_t(P), points_p, C.c_size_t(n), None, offsets_p, items_p, C.c_size_t(cap), total_p)
    assert call(None, _p(boxes), _p(points), _p(offsets), None, 0, C.byref(total)) == ERR_ARG
    assert L.gpuart_nearest_last_error().decode().startswith("nearest:")
    assert call(_p(prims), None, _p(points), _p(offsets), None, 0, C.byref(total)) == ERR_ARG
    assert call(_p(prims), _p(boxes), None, _p(offsets), None, 0, C.byref(total)) == ERR_ARG
    assert call(_p(prims), _p(boxes), _p(points), None, None, 0, C.byref(total)) == ERR_ARG
    assert call(_p(prims), _p(boxes), _p(points), _p(offsets), None, 0, None) == ERR_ARG
    # records that do not reach every primitive once: a root leaf of one where there are three
    one = prims.copy()
    one.view(np.uint32)[0, 0, 3] = (one.view(np.uint32)[0, 0, 3] & 3) | 1 << 2
    assert call(_p(one), _p(boxes), _p(points), _p(offsets), None, 0, C.byref(total)) == ERR_ARG
    exp = WR.brute(recs, prims, boxes, c["root"], points)
    assert len(exp[1]) > 8
    items = np.full(len(exp[1]), 7.0, F).repeat(8).view(NR.HIT)
    before = items.tobytes()
    assert call(_p(prims), _p(boxes), _p(points), _p(offsets), _p(items), len(items) - 1, C.byref(total)) == 0
    assert items.tobytes() == before and total.value == len(exp[1]) and (offsets == exp[0]).all()
    assert call(_p(prims), _p(boxes), _p(points), _p(offsets), _p(items), len(items), C.byref(total)) == 0
    assert_lists((offsets, items), exp, "with room")
    # no queries and no primitives
    assert L.gpuart_nearest_within_brute_host(None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_size_t(0), None, C.c_size_t(0), None, _p(offsets), None,
                                              C.c_size_t(0), C.byref(total)) == 0 and total.value == 0


def test_the_kernels_have_no_scratch_and_the_library_exports_its_header(B, tmp_path):
    from tests.test_product_library import _code_object, _kernel_metadata
    from tests.util import exported
    lib = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    meta = _kernel_metadata(_code_object(lib, str(tmp_path)))
    kernels = sorted(k for k in meta if "k_within" in k)
    assert len(kernels) == 2 and "k_within_count" in kernels[1] and "k_within_fill" in kernels[0], sorted(meta)
    for k in kernels:
        text = "\n".join(meta[k])
        assert ".private_segment_fixed_size: 0" in text and ".vgpr_spill_count: 0" in text, text
        assert ".group_segment_fixed_size: %d" % (4 * 256 * B.NEAREST_RING) in text, text
        # 5 waves per SIMD (DESIGN.md "Neighbour lists"): a SIMD's 512 registers per lane over 5 waves are 102, and registers are allocated
        # in eights: 96. No AGPRs (they come out of the same 512) and nothing spilled
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= 96, text
        assert re.search(r"\.agpr_count:\s+0\b", text) and ".sgpr_spill_count: 0" in text, text
    names = exported(lib)
    assert sum(n.startswith("gpuart_nearest_within_") for n in names) == 9 and all(n.startswith("gpuart_nearest_") for n in names), names
    with open(os.path.join(ROOT, "include", "gpuart_nearest.h")) as f:
        header = f.read()
    assert all(n + "(" in header for n in names), [n for n in names if n + "(" not in header]


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
CHUNKS = 2 * 64 + 7   # twice GPUART_NEAREST_CHUNK plus 7


@pytest.fixture
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


def device_scene(b):
    """(recs, prims, boxes, root) the device holds now."""
    from tests.test_edit import device_arrays
    recs, prims, boxes = device_arrays(b)
    s = b.scene_device()
    return recs, prims, boxes, (np.array(s.root_min[:], F), np.array(s.root_max[:], F), int(s.root_ref))


def expected(b, points, us=None):
    """The restatement's definition over the arrays the device holds now, in the order of the device's own tree."""
    return WR.brute(*device_scene(b), points, us)


def scene_queries(b, n, seed=0, spread=True):
    """The query set for the uploaded scene; by the restatement it holds empty lists, lists of one, long lists and a very long one."""
    _, prims, boxes, _ = device_scene(b)
    points = WC.query_set(boxes, n, seed)
    if spread:
        WC.assert_spread(expected(b, points)[0], len(prims))
    return points


def as_numpy(res):
    o, it = res
    if type(o).__module__.startswith("torch"):
        o, it = o.cpu().numpy().view(np.uint32), it.cpu().numpy().view(NR.HIT).reshape(-1)
    return o, it


def check(b, points, what, us=None, device=False):
    from tests.util import to_device
    got = as_numpy(b.within(to_device(points) if device else points, user_sphere=us))
    assert_lists(got, expected(b, points, us), what)
    return got


def upload_scene(b, name):
    s = NC.scene(name)
    b.upload_bvh(s["tree"])
    return s


def limits(B, be, max_blocks=0, spill_bytes=0, host_chunk=0):
    h = be._nearest_handle(be.scene_device())
    assert B.nearest_lib().gpuart_nearest_set_limits(h, C.c_uint32(max_blocks), C.c_size_t(spill_bytes), C.c_size_t(host_chunk)) == 0
    return h


def last_launch(B, h):
    blocks, launches = C.c_uint32(), C.c_uint32()
    assert B.nearest_lib().gpuart_nearest_last_launch(h, C.byref(blocks), C.byref(launches)) == 0
    return blocks.value, launches.value


@gpu
@pytest.mark.parametrize("name", ["box", "mixed300"])
def test_every_list_is_the_definitions_through_the_scenes_life(B, be, name):
    """After the upload, a refit, a Morton rebuild, a clustered rebuild and an edit that removes three and adds five: the handle follows
    the generation by itself; the refit changes the lists and keeps the order rule (the expectation walks the device's own records)."""
    from tests import refit_ref as RR
    s = upload_scene(be, name)
    n_prims = len(s["prims"])
    points = scene_queries(be, CHUNKS, seed=1)
    got = check(be, points, name + ": uploaded")
    check(be, points, name + ": uploaded, user sphere", US)
    check(be, points, name + ": uploaded, device tensors", US, device=True)
    order = WR.tree_order(*device_scene(be)[:2], be.scene_device().root_ref)
    ordinals, payloads = RR.random_update(s["tree"], np.random.default_rng(5), 0.3, 0.3)
    bound = be._nearest.generation
    be.refit(ordinals, payloads)
    assert be.scene_device().generation == bound
    assert WR.tree_order(*device_scene(be)[:2], be.scene_device().root_ref) == order, "a refit keeps the order"
    moved = check(be, points, name + ": refitted")
    assert moved[1].tobytes() != got[1].tobytes()
    check(be, points, name + ": refitted, user sphere", US)
    for mode in ("morton", "clustered"):
        be.rebuild(mode=mode)
        check(be, points, "%s: rebuilt, %s" % (name, mode))
        check(be, points, "%s: rebuilt, %s, user sphere" % (name, mode), US, device=True)
    added = [(t, RR.payload_of((t, f))) for t, f in NC.mixed(5, seed=41)]
    be.edit(np.array([0, n_prims // 2, n_prims - 1], np.uint32), np.array([t for t, _ in added], np.uint32),
            np.array([d for _, d in added], F), mode="clustered", out=False)
    assert be.scene_device().n_prims == n_prims + 2
    points = scene_queries(be, CHUNKS, seed=2)
    check(be, points, name + ": edited")
    check(be, points, name + ": edited, user sphere", US)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNKS])
def test_query_counts_around_the_wave_and_the_chunk(be, n):
    import torch
    upload_scene(be, "mixed300")
    points = scene_queries(be, CHUNKS, seed=7)[:n]
    check(be, points, "%d queries" % n, device=True)
    check(be, points, "%d queries, user sphere" % n, US, device=True)
    check(be, points, "%d queries, host" % n, US)
    if n == 1:
        o, it = be.within(torch.zeros((0, 4), dtype=torch.float32, device="cuda:0"))
        assert o.cpu().tolist() == [0] and tuple(it.shape) == (0, 8)
        o, it = be.within(np.zeros((0, 4), F))
        assert o.tolist() == [0] and len(it) == 0


def chain_tree():
    return WC.tree("chain", "clustered")


@gpu
@pytest.mark.parametrize("n, blocks", [(300, 1), (1000, 1), (1000, 2)])
@pytest.mark.parametrize("name", ["mixed300", "chain"])
def test_lanes_refill_the_cursor_hands_out_chunks_and_deep_stacks_spill(B, be, name, n, blocks):
    """More queries than the launch has lanes, asserted from the handle: chunks from the cursor, idle lanes that take new queries while
    their neighbours walk on, and on the chain — deeper than the LDS ring, asserted from the restated walk — the lane's spill column. The
    answers are those of the unlimited handle."""
    from tests.util import to_device
    if name == "chain":
        be.upload_bvh(chain_tree())
        stats = {}
        WR.walk(*device_scene(be), np.array([[0, 0, 0, INF], [0.1, 0, 0, 3.0]], F), stats=stats)
        assert stats["deepest"] >= B.NEAREST_RING + 4, stats
    else:
        upload_scene(be, name)
    points = scene_queries(be, n, seed=n + blocks, spread=name != "chain")
    if name == "chain":
        points[::7, :3] *= 0.01
        points[::7, 3] = INF     # from near the centre with no radius: the walk stacks the whole chain
        WC.assert_spread(expected(be, points)[0], 24)     # (24 spheres: its longest lists hold them all)
    free = [as_numpy(be.within(to_device(points), user_sphere=us)) for us in (None, US)]
    h = limits(B, be, max_blocks=blocks)
    for us, unlimited in zip((None, US), free):
        got = as_numpy(be.within(to_device(points), user_sphere=us))
        got_blocks, launches = last_launch(B, h)
        assert got_blocks == blocks and launches == 1 and n > got_blocks * 256, (got_blocks, launches)
        assert_lists(got, expected(be, points, us), "%s, %d on %d" % (name, n, blocks))
        assert_lists(got, unlimited, "%s, %d on %d against the unlimited run" % (name, n, blocks))
    if blocks == 1 and n == 300:
        limits(B, be, spill_bytes=100)
        got = as_numpy(be.within(to_device(points)))
        assert last_launch(B, h) == (1, 1)
        assert_lists(got, free[0], name + ": a tiny spill budget still runs one workgroup")


@gpu
@pytest.mark.parametrize("us", NC.USER_SPHERES, ids=["no user sphere", "user sphere"])
def test_every_list_is_complete_without_a_radius(be, us):
    upload_scene(be, "mixed7")
    recs, prims, boxes, root = device_scene(be)
    points = np.array(NC.points_for(boxes, 70, seed=3))
    special = np.arange(70) % 16 == 5
    points[~special, 3] = INF
    got = check(be, points, "mixed7, r = +inf", us)
    order = ([-2] if us else []) + WR.tree_order(recs, prims, root[2])
    valid = NR.query_ok(points) & ~special
    assert valid.sum() > 60
    for i, l in enumerate(lists_of(got)):
        if valid[i]:
            assert l == order, (i, l)


@gpu
def test_a_box_at_exactly_r_is_entered(be):
    """The named case of the prune: the six coincident spheres, in three leaves of different subtrees, at d2 = r2 = box_d2 = 4 from p. A
    walk that skips a child at box_d2 == r2 lists fewer than six; the device lists the six in the order of its own tree — the uploaded
    Morton tree's, and a clustered rebuild's."""
    tree, _, points = duplicates_case()
    points = np.concatenate([points, [[0, -3, 0, 2], [0, 0, 3, 2], [-3, 0, 0, 2], [3, 0, 0, 1.9999999], [3, 0, 0, 2.0000002]]]).astype(F)
    be.upload_bvh(tree)
    for what in ("uploaded", "rebuilt"):
        recs, prims, boxes, root = device_scene(be)
        copies = [k for k in WR.tree_order(recs, prims, root[2]) if (prims[k, 0, :3] == 0).all()]
        assert len(copies) == 6
        assert (NR.box_d2(boxes[copies[0], :3], boxes[copies[0], 3:], points[:4, :3]) == 4).all() and (points[:4, 3] ** 2 == 4).all()
        if what == "uploaded":
            assert len({k // 2 for k in copies}) >= 3, "the copies lie in at least three leaves"
            wrong = WR.walk(recs, prims, boxes, root, points, mutant="prune_ge")
            assert all(len(l) < 6 for l in lists_of(wrong)[:4]), "the wrong rule loses copies here"
        for us in NC.USER_SPHERES:
            for device in (False, True):
                got = check(be, points, "duplicates, " + what, us, device=device)
                assert [[k for k in l if k >= 0] for l in lists_of(got)] == [copies] * 4 + [[], copies]
        be.rebuild(mode="clustered")


@gpu
def test_a_total_of_zero(B, be):
    import torch
    from tests.util import to_device
    upload_scene(be, "mixed300")
    _, _, boxes, _ = device_scene(be)
    points = np.array(NC.points_for(boxes, CHUNKS, seed=5))
    points[:, 3] = 0.0
    points[:, :3] += F(1e-3)
    exp = expected(be, points)
    assert exp[0][-1] == 0, "off the surface"
    o, it = be.within(to_device(points))
    assert (o == 0).all() and tuple(it.shape) == (0, 8)
    items = torch.full((64, 8), 7.0, dtype=torch.float32, device="cuda:0")
    o, it = be.within(to_device(points), out=(torch.full((CHUNKS + 1,), 9, dtype=torch.int32, device="cuda:0"), items))
    assert (o == 0).all() and it is items and bool((items == 7.0).all()), "the fill writes nothing"
    o, it = be.within(points)
    assert (o == 0).all() and len(it) == 0


@gpu
def test_the_capacity_is_never_exceeded_and_wrong_offsets_are_reported(B, be):
    """items lies between 64 canary records on either side. A capacity below the total is refused before any launch. A fill handed the
    offsets of a smaller-radius count of the same points completes — every store is guarded, in bounds —, writes each list's first items
    into the room those offsets leave it and nothing at or beyond the next list's, and finish reports the mismatch."""
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    upload_scene(be, "mixed300")
    points = scene_queries(be, CHUNKS, seed=4)
    small = points.copy()
    small[:, 3] *= F(0.5)
    exp, exp_small = expected(be, points, US), expected(be, small, US)
    total, total_small = int(exp[0][-1]), int(exp_small[0][-1])
    assert 0 < total_small < total
    scene = be.scene_device()
    h = be._nearest_handle(scene)
    tp, ts = to_device(points), to_device(small)
    off, off_small = (torch.zeros(CHUNKS + 1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    CANARY = 64
    buf = torch.full((CANARY + total + CANARY, 8), 7.0, dtype=torch.float32, device="cuda:0")
    items_ptr = buf.data_ptr() + CANARY * 32
    torch.cuda.synchronize()
    usp = (C.c_float * 4)(*US)
    count = lambda pts, o: N.gpuart_nearest_within_count(h, C.byref(scene), C.c_void_p(pts.data_ptr()), C.c_size_t(CHUNKS), usp, C.c_void_p(o.data_ptr()))
    fill = lambda pts, o, cap: N.gpuart_nearest_within_fill(h, C.byref(scene), C.c_void_p(pts.data_ptr()), C.c_size_t(CHUNKS), usp, C.c_void_p(o.data_ptr()),
                                                           C.c_void_p(items_ptr), C.c_size_t(cap))
    t = C.c_uint64(0)
    assert count(ts, off_small) == 0 and N.gpuart_nearest_within_total(h, C.byref(t)) == 0 and t.value == total_small
    assert count(tp, off) == 0 and N.gpuart_nearest_within_total(h, C.byref(t)) == 0 and t.value == total
    assert (off.cpu().numpy().view(np.uint32) == exp[0]).all() and (off_small.cpu().numpy().view(np.uint32) == exp_small[0]).all()
    # a short capacity: refused before any launch
    assert fill(tp, off, total - 1) == ERR_ARG and str(total) in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_finish(h) == 0 and bool((buf == 7.0).all())
    # the right offsets: the lists, between intact canaries
    assert fill(tp, off, total) == 0 and N.gpuart_nearest_finish(h) == 0
    host = buf.cpu().numpy()
    assert (host[:CANARY] == 7.0).all() and (host[CANARY + total:] == 7.0).all()
    assert_lists((exp[0], host[CANARY:CANARY + total].copy().view(NR.HIT).reshape(-1)), exp, "between the canaries")
    # the offsets of the smaller radius
    buf.fill_(7.0)
    torch.cuda.synchronize()
    assert fill(tp, off_small, total) == 0
    assert N.gpuart_nearest_finish(h) == ERR_ARG
    assert "the offsets are not this query set's count: the results are void" in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_finish(h) == 0, "reported once"
    host = buf.cpu().numpy()
    assert (host[:CANARY] == 7.0).all() and (host[CANARY + total_small:] == 7.0).all(), "nothing beyond the last offset"
    written = host[CANARY:CANARY + total_small].copy().view(NR.HIT).reshape(-1)
    for i in range(CHUNKS):
        a, b = int(exp_small[0][i]), int(exp_small[0][i + 1])
        first = exp[1][int(exp[0][i]):int(exp[0][i]) + (b - a)]
        assert written[a:b].tobytes() == first.tobytes(), "list %d: its first %d items, and nothing at or beyond offsets[%d]" % (i, b - a, i + 1)
    # a bind forgets the last count: a fill wants a count of this binding
    buf.fill_(7.0)
    torch.cuda.synchronize()
    assert count(tp, off) == 0 and N.gpuart_nearest_bind(h, C.byref(scene)) == 0
    assert fill(tp, off, total) == ERR_ARG and "the last count was of 0 queries" in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_finish(h) == 0 and bool((buf == 7.0).all())
    check(be, points, "after the mismatch", US, device=True)


@gpu
def test_a_lowered_cap_refuses_the_total(B, be):
    from tests.util import to_device
    N = B.nearest_lib()
    upload_scene(be, "box")
    points = scene_queries(be, CHUNKS, seed=1)
    total = int(expected(be, points)[0][-1])
    assert 200 < total < 1000
    scene = be.scene_device()
    h = be._nearest_handle(scene)
    assert N.gpuart_nearest_within_set_max_items(h, C.c_uint64(100)) == 0
    tp = to_device(points)
    off = to_device(np.zeros(CHUNKS + 1, np.int32))
    t = C.c_uint64(0)
    assert N.gpuart_nearest_within_count(h, C.byref(scene), C.c_void_p(tp.data_ptr()), C.c_size_t(CHUNKS), None, C.c_void_p(off.data_ptr())) == 0
    assert N.gpuart_nearest_within_total(h, C.byref(t)) == ERR_ARG and t.value == total
    assert str(total) in N.gpuart_nearest_last_error().decode()
    for pts in (tp, points):
        with pytest.raises(B.HipError, match=str(total)):
            be.within(pts)
    assert N.gpuart_nearest_within_set_max_items(h, C.c_uint64(0)) == 0
    check(be, points, "the default cap again", device=True)
    for pts in (tp, points):
        with pytest.raises(ValueError, match=str(total)):
            be.within(pts, max_items=total - 1)
    assert len(be.within(points, max_items=total)[1]) == total


@gpu
def test_every_input_kind_gives_the_same_bytes(B, be):
    import torch
    from tests.util import to_device
    upload_scene(be, "mixed300")
    points = scene_queries(be, CHUNKS, seed=6)
    exp = expected(be, points, US)
    total = int(exp[0][-1])
    tp = to_device(points)
    unstaged = as_numpy(be.within(tp, user_sphere=US))
    assert_lists(unstaged, exp, "torch")
    assert_lists(as_numpy(be.within(tp, user_sphere=US)), unstaged, "the same call again")
    h = limits(B, be, host_chunk=64)
    staged = be.within(points, user_sphere=US)
    assert last_launch(B, h)[1] == 3, "the fill alone: three staged launches of 64, 64 and 7 queries"
    assert staged[0].dtype == np.uint32 and staged[1].dtype == B.NEAREST_HIT
    assert_lists(staged, unstaged, "NumPy, staged in chunks of 64, against the unstaged run")
    # gpuart_nearest_within_host by its two-call protocol: offsets and the total always, items only with room for them
    N, scene = B.nearest_lib(), be.scene_device()
    off, t = np.full(CHUNKS + 1, 9, np.uint32), C.c_uint64(0)
    items = np.full(total * 8, 7.0, F).view(NR.HIT)
    host = lambda it, cap: N.gpuart_nearest_within_host(h, C.byref(scene), _p(points), C.c_size_t(CHUNKS), (C.c_float * 4)(*US), _p(off), it, C.c_size_t(cap), C.byref(t))
    assert host(None, 0) == 0 and t.value == total and (off == exp[0]).all() and last_launch(B, h)[1] == 3
    assert host(_p(items), total - 1) == 0 and t.value == total and (items.view(F) == 7.0).all(), "a short capacity is no error and writes no item"
    assert host(_p(items), total) == 0 and last_launch(B, h)[1] == 2 * 3, "three staged launches per pass"
    assert_lists((off, items), unstaged, "gpuart_nearest_within_host, staged, against the unstaged run")
    # gpuart_nearest_within_fill_host: the fill alone for those offsets; what it must refuse, and offsets of another radius
    items[:] = np.full(total * 8, 7.0, F).view(NR.HIT)
    fill = lambda o, cap, pts=points: N.gpuart_nearest_within_fill_host(h, C.byref(scene), _p(pts), C.c_size_t(CHUNKS), (C.c_float * 4)(*US), _p(o), _p(items), C.c_size_t(cap))
    assert fill(off, total - 1) == ERR_ARG and fill(off[::-1].copy(), total) == ERR_ARG and (items.view(F) == 7.0).all()
    assert fill(off, total) == 0
    assert_lists((off, items), unstaged, "gpuart_nearest_within_fill_host")
    wider = points.copy()
    wider[:, 3] *= F(1.5)
    assert fill(off, total, wider) == ERR_ARG and "not this query set's count" in N.gpuart_nearest_last_error().decode()
    limits(B, be)
    assert_lists(be.within(points, user_sphere=US), unstaged, "NumPy, one chunk")
    offsets = torch.full((CHUNKS + 1,), 9, dtype=torch.int32, device="cuda:0")
    items = torch.full((total + 5, 8), 7.0, dtype=torch.float32, device="cuda:0")
    o, it = be.within(tp, user_sphere=US, out=(offsets, items))
    assert o is offsets and it is items and bool((items[total:] == 7.0).all())
    assert_lists((offsets.cpu().numpy().view(np.uint32), items[:total].cpu().numpy().view(NR.HIT).reshape(-1)), exp, "out=")
    with pytest.raises(ValueError, match=str(total)):
        be.within(tp, user_sphere=US, out=(offsets, torch.zeros((total - 1, 8), dtype=torch.float32, device="cuda:0")))
    with pytest.raises(ValueError, match="GPU"):
        be.within(tp.cpu())
    with pytest.raises(ValueError):
        be.within(tp.double())
    with pytest.raises(ValueError):
        be.within(torch.zeros((CHUNKS, 8), dtype=torch.float32, device="cuda:0")[:, :4])
    with pytest.raises(ValueError):
        be.within(tp, out=(offsets.to(torch.int64), items))
    with pytest.raises(ValueError):
        be.within(tp, out=(offsets, items.cpu()))


@gpu
def test_five_queries_through_host_memory_in_chunks_of_two_are_the_unchunked_bytes(B, be):
    """host_chunk = 2: three staged launches per pass, the last one short; offsets rebased by the running total, items at the chunk's place."""
    upload_scene(be, "mixed7")
    points = scene_queries(be, 5, seed=3, spread=False)
    h = limits(B, be)
    whole = be.within(points, user_sphere=US)
    assert last_launch(B, h)[1] == 1 and whole[0][-1] > 0
    limits(B, be, host_chunk=2)
    staged = be.within(points, user_sphere=US)
    assert last_launch(B, h)[1] == 3, "the fill alone: chunks of 2, 2 and 1"
    assert_lists(staged, whole, "in chunks of two")
    assert_lists(staged, expected(be, points, US), "in chunks of two, the definition")


@gpu
def test_the_renderer_lists_what_the_backend_does(B):
    from gpuart_amd import synth_scenes as S
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        with pytest.raises(B.HipError, match="stderr"):
            r.primitives_within(np.zeros((4, 4), F))
        r.set_user_sphere(US[:3], US[3], 0.0)
        r.set_primitives(NC.scene("box")["descs"])
        assert r.rebuild_tree("clustered") is not None
        rb = r.backend
        points = scene_queries(rb, CHUNKS, seed=21)
        exp, exp_us = expected(rb, points), expected(rb, points, US)
        assert exp_us[0][-1] > exp[0][-1] > 0
        assert_lists(r.primitives_within(points, with_user_sphere=False), exp, "Renderer::PrimitivesWithin")
        assert_lists(r.primitives_within(points, with_user_sphere=True), exp_us, "Renderer::PrimitivesWithin, user sphere")
        assert_lists(rb.within(points, user_sphere=US), exp_us, "its context")
        # gpuart_renderer_primitives_within by its two-call protocol
        off, t = np.zeros(CHUNKS + 1, np.uint32), C.c_uint64(0)
        call = lambda it, cap: r.L.gpuart_renderer_primitives_within(r.h, _p(points), C.c_size_t(CHUNKS), C.c_int(1), _p(off), it, C.c_size_t(cap), C.byref(t))
        assert call(None, 0) == 1 and t.value == len(exp_us[1]) and (off == exp_us[0]).all()
        items = np.zeros(t.value, NR.HIT)
        assert call(_p(items), len(items)) == 1
        assert_lists((off, items), exp_us, "gpuart_renderer_primitives_within, the second call")
        nearest = r.closest_points(np.concatenate([points[:, :3], np.full((CHUNKS, 1), INF, F)], 1), user_sphere=False)
        assert set(exp[1]["prim"].tolist()) <= set(range(len(NC.scene("box")["descs"]))) and nearest["prim"].max() < len(NC.scene("box")["descs"])
        o, it = r.primitives_within(np.zeros((0, 4), F))
        assert o.tolist() == [0] and len(it) == 0
    finally:
        r.close()


@gpu
def test_what_must_be_refused_is_refused_with_nothing_written(B, be):
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    s = upload_scene(be, "mixed7")
    points = to_device(scene_queries(be, 16, seed=4, spread=False))
    off = torch.full((17,), 9, dtype=torch.int32, device="cuda:0")
    items = torch.full((64, 8), 7.0, dtype=torch.float32, device="cuda:0")
    untouched = lambda: bool((off == 9).all()) and bool((items == 7.0).all())
    torch.cuda.synchronize()
    count = lambda h, sc, p=points.data_ptr(), n=16, o=off.data_ptr(): N.gpuart_nearest_within_count(h, C.byref(sc), C.c_void_p(p), C.c_size_t(n), None, C.c_void_p(o))
    fill = lambda h, sc: N.gpuart_nearest_within_fill(h, C.byref(sc), C.c_void_p(points.data_ptr()), C.c_size_t(16), None, C.c_void_p(off.data_ptr()),
                                                     C.c_void_p(items.data_ptr()), C.c_size_t(64))
    msg = lambda: N.gpuart_nearest_last_error().decode()
    # an unbound handle
    fresh = B._NearestHandle(0)
    try:
        assert count(fresh, be.scene_device()) == ERR_ARG and "not bound" in msg()
        assert fill(fresh, be.scene_device()) == ERR_ARG and "not bound" in msg()
        assert N.gpuart_nearest_finish(fresh) == 0
    finally:
        fresh.close()
    # a stale generation: bound to the first upload, given the second one's
    be.within(points)
    h = be._nearest
    be.upload_bvh(s["tree"])
    new = be.scene_device()
    assert count(h, new) == ERR_ARG and "bind again" in msg()
    assert fill(h, new) == ERR_ARG and "bind again" in msg()
    # misaligned pointers, offsets overlapping points, too many queries
    assert N.gpuart_nearest_bind(h, C.byref(new)) == 0
    assert count(h, new, p=points.data_ptr() + 4, n=15) == ERR_ARG and "misaligned" in msg()
    assert count(h, new, o=off.data_ptr() + 2, n=15) == ERR_ARG and "misaligned" in msg()
    assert count(h, new, o=points.data_ptr() + 64) == ERR_ARG and "overlaps" in msg()
    assert count(h, new, n=0x80000000) == ERR_ARG and "too many" in msg()
    assert count(h, new, p=None) == ERR_ARG
    assert count(h, new, p=None, n=0, o=None) == 0
    assert N.gpuart_nearest_finish(h) == 0 and untouched()
    before = points.clone()
    h.generation = new.generation
    check(be, points.cpu().numpy(), "after the refusals", device=True)
    assert bool((points == before).all())
