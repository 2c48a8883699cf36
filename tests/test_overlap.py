"""Box overlap: every primitive whose box meets a query box, and the overlapping pairs of the scene's own primitives (include/gpuart_nearest.h
"Box overlap", libgpuart_nearest.so: gpuart_nearest_overlap_*, gpuart_nearest_pairs_*; Backend.overlaps, Backend.overlapping_pairs,
Renderer::PrimitivesOverlapping, Renderer::OverlappingPairs). On the CPU: the definitions (the two brute_host functions) are the
restatement's (tests/overlap_ref.py) byte for byte on every rule case and tree under four margins, the restated pruned walk with the lower
child first is the definition, the pairs are the box query filtered, and five named wrong rules are told from the right one. On the GPU:
offsets and items of k_overlap_count and k_overlap_fill are the restatement's over the device's own arrays, in the order of the device's own
tree — through the scene's life, for query counts around the wave and the chunk, under every grid and spill limit, through every input kind;
the capacity protocol never writes outside what it was given; and what must be refused is refused with nothing written. Every comparison is
byte for byte; there is no tolerance anywhere."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nearest_cases as NC
from tests import nearest_ref as NR
from tests import overlap_cases as OC
from tests import overlap_ref as OR
from tests import within_cases as WC
from tests import within_ref as WR

F = np.float32
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
US = NC.USER_SPHERES[1]
INF, NAN = float("inf"), float("nan")
OVERLAP_NAMES = ["gpuart_nearest_overlap_" + s for s in ("brute_host", "count", "counts", "fill", "fill_host", "host", "step_ms", "total")]
PAIRS_NAMES = ["gpuart_nearest_pairs_" + s for s in ("brute_host", "count", "fill", "host")]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def _two_calls(call, n, what):
    """The two-call protocol of a host function call(offsets_p, items_p, capacity, total_p): (offsets, items)."""
    offsets = np.full(n + 1, 0xdddddddd, np.uint32)
    total = C.c_uint64(123)
    assert call(_p(offsets), None, C.c_size_t(0), C.byref(total)) == 0, what
    assert offsets[0] == 0 and offsets[-1] == total.value
    first = offsets.copy()
    items = np.full(total.value, -7, np.int32)
    assert call(_p(offsets), _p(items), C.c_size_t(len(items)), C.byref(total)) == 0, what
    assert (offsets == first).all() and total.value == len(items)
    return offsets, items


def brute_host(B, recs, prims, boxes, root_ref, queries, margin, us=None):
    """gpuart_nearest_overlap_brute_host by its two-call protocol, with no device: (offsets, items)."""
    L = B.nearest_lib()
    recs, prims, boxes = np.ascontiguousarray(recs, F), np.ascontiguousarray(prims, F), np.ascontiguousarray(boxes, F)
    queries = np.ascontiguousarray(queries, F)
    usp = None if us is None else (C.c_float * 4)(*us)
    head = (_p(recs), C.c_size_t(len(recs)), C.c_uint32(int(root_ref)), _p(prims), _p(boxes), C.c_size_t(len(prims)), _p(queries), C.c_size_t(len(queries)),
            C.c_float(margin), usp)
    return _two_calls(lambda *tail: L.gpuart_nearest_overlap_brute_host(*head, *tail), len(queries), L.gpuart_nearest_last_error().decode())


def pairs_brute_host(B, recs, prims, boxes, root_ref, margin):
    L = B.nearest_lib()
    recs, prims, boxes = np.ascontiguousarray(recs, F), np.ascontiguousarray(prims, F), np.ascontiguousarray(boxes, F)
    head = (_p(recs), C.c_size_t(len(recs)), C.c_uint32(int(root_ref)), _p(prims), _p(boxes), C.c_size_t(len(prims)), C.c_float(margin))
    return _two_calls(lambda *tail: L.gpuart_nearest_pairs_brute_host(*head, *tail), len(prims), L.gpuart_nearest_last_error().decode())


def assert_lists(got, exp, what):
    (go, gi), (eo, ei) = got, exp
    go, eo = np.ascontiguousarray(go).view(np.uint32), np.ascontiguousarray(eo).view(np.uint32)
    assert go.shape == eo.shape, what
    assert (go == eo).all(), "%s: offsets differ; first at %d: got %s expected %s" % (what, int(np.argmax(go != eo)), go[go != eo][:4], eo[go != eo][:4])
    gi, ei = np.ascontiguousarray(gi), np.ascontiguousarray(ei)
    assert gi.dtype.itemsize == 4 and ei.dtype.itemsize == 4 and gi.shape == ei.shape, (what, gi.shape, ei.shape)
    assert gi.tobytes() == ei.tobytes(), "%s: %d of %d items differ; first at %d" % (what, int((gi.view(np.int32) != ei.view(np.int32)).sum()), len(ei),
                                                                                     int(np.argmax(gi.view(np.int32) != ei.view(np.int32))))


lists_of = OR.lists_of


# ---- CPU 1: the definitions against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("us", NC.USER_SPHERES, ids=["no user sphere", "user sphere"])
@pytest.mark.parametrize("name", NC.RULE_CASES)
def test_the_definition_is_the_restatements_on_the_rule_cases(B, name, us):
    c = OC.rule_case(name)
    n_special = len(OC.INVALID)
    for margin in OC.margins(c["boxes"]):
        what = "%s, margin %g" % (name, margin)
        exp = OR.brute(c["recs"], c["prims"], c["boxes"], c["root"], c["queries"], margin, us)
        assert_lists(brute_host(B, c["recs"], c["prims"], c["boxes"], c["root"][2], c["queries"], margin, us), exp, what)
        ln = np.diff(exp[0].astype(np.int64))
        invalid = ~OR.box_ok(c["queries"])
        assert invalid.sum() >= n_special and (ln[invalid] == 0).all(), what + ": an invalid box has an empty list"
        for l in lists_of(exp):
            assert l == sorted(l, key=lambda k: (k != -2, k)), what + ": a root leaf's order is the user sphere, then the ordinals"
        if us is None:
            exp = OR.pairs(c["recs"], c["prims"], c["boxes"], c["root"], margin)
            assert_lists(pairs_brute_host(B, c["recs"], c["prims"], c["boxes"], c["root"][2], margin), exp, what + ": pairs")
    # a primitive's own box lists that primitive, the root box every primitive, at every margin
    P, own = len(c["prims"]), c["queries"]
    finite = int(np.isfinite(NC.rule_case(name)["points"][:, :3]).all(1).sum())
    lists = lists_of(OR.brute(c["recs"], c["prims"], c["boxes"], c["root"], own, 0.0))
    assert all(k in lists[finite + k] for k in range(P)) and sorted(lists[finite + P]) == list(range(P)) and lists[finite + P + 1] == []


# ---- CPU 1 and 2: the trees, and the restated pruned walk ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["morton", "clustered"])
@pytest.mark.parametrize("name", list(WC.TREE_SCENES))
def test_the_pruned_walk_is_the_definition_and_the_order_clause_bites(B, name, kind):
    recs, prims, boxes, root, queries = OC.tree_case(name, kind)
    order = WR.tree_order(recs, prims, root[2])
    assert sorted(order) == list(range(len(prims)))
    rank = {k: i for i, k in enumerate([-2] + order)}
    differs = False
    for margin in OC.margins(boxes):
        for us in NC.USER_SPHERES:
            what = "%s %s, margin %g%s" % (name, kind, margin, ", user sphere" if us else "")
            exp = OR.brute(recs, prims, boxes, root, queries, margin, us)
            assert_lists(brute_host(B, recs, prims, boxes, root[2], queries, margin, us), exp, what + ": the definition derives the tree's order from the records")
            assert_lists(OR.walk(recs, prims, boxes, root, queries, margin, us, "lower"), exp, what + ": lower child first")
            assert all(l == sorted(l, key=rank.get) for l in lists_of(exp)), what
            upper = OR.walk(recs, prims, boxes, root, queries, margin, us, "upper")
            assert (upper[0] == exp[0]).all(), what
            a, b = lists_of(upper), lists_of(exp)
            assert [sorted(l) for l in a] == [sorted(l) for l in b], what + ": upper child first lists the same sets"
            differs = differs or a != b
        assert_lists(pairs_brute_host(B, recs, prims, boxes, root[2], margin), OR.pairs(recs, prims, boxes, root, margin), "%s %s, margin %g: pairs" % (name, kind, margin))
    assert differs, "... in another order"


# ---- CPU 3: pairs are the box query filtered ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["morton", "clustered"])
@pytest.mark.parametrize("name", list(WC.TREE_SCENES))
def test_pairs_are_the_box_query_filtered(B, name, kind):
    recs, prims, boxes, root = WC.tree_arrays(name, kind)
    for margin in OC.margins(boxes):
        got = pairs_brute_host(B, recs, prims, boxes, root[2], margin)
        full = lists_of(brute_host(B, recs, prims, boxes, root[2], boxes, margin))
        lists = lists_of(got)
        assert lists == [[j for j in l if j > i] for i, l in enumerate(full)], "%s %s, margin %g" % (name, kind, margin)
        seen = [(i, j) for i, l in enumerate(lists) for j in l]
        assert len(set(seen)) == len(seen) and all(i < j for i, j in seen), "every unordered pair at most once, in the lower ordinal's list"
        assert all(i in l for i, l in enumerate(full)), "a box overlaps itself"
    assert len(seen) > 0, "at a quarter of the extent there are pairs"


# ---- CPU 4: the wrong rules, each caught by its named case ---------------------------------------------------------------------------------------
def test_strict_comparisons_lose_a_box_that_touches_at_one_face(B):
    (recs, prims, boxes, root), queries, margin = OC.touching()
    exp = OR.brute(recs, prims, boxes, root, queries, margin)
    assert lists_of(exp) == [[0]] and queries[0, 0] == boxes[0, 3], "the query's lower face is the box's upper face"
    assert_lists(brute_host(B, recs, prims, boxes, root[2], queries, margin), exp, "touching")
    assert_lists(OR.walk(recs, prims, boxes, root, queries, margin), exp, "touching, walked")
    assert lists_of(OR.brute(recs, prims, boxes, root, queries, margin, mutant="strict")) == [[]]
    assert lists_of(OR.walk(recs, prims, boxes, root, queries, margin, mutant="strict")) == [[]]


def test_the_uninflated_box_at_a_child_loses_what_only_the_margin_reaches(B):
    (recs, prims, boxes, root), queries, margin = OC.margin_reaches()
    copies = [k for k in WR.tree_order(recs, prims, root[2]) if (prims[k, 0, :3] == 0).all()]
    exp = OR.brute(recs, prims, boxes, root, queries, margin)
    assert lists_of(exp) == [copies] and len(copies) == 6
    assert lists_of(OR.brute(recs, prims, boxes, root, queries, 0.0)) == [[]], "only the margin reaches them"
    assert_lists(brute_host(B, recs, prims, boxes, root[2], queries, margin), exp, "margin reaches: the definition")
    assert_lists(OR.walk(recs, prims, boxes, root, queries, margin), exp, "margin reaches, walked")
    wrong = lists_of(OR.walk(recs, prims, boxes, root, queries, margin, mutant="uninflated_child"))[0]
    assert len(wrong) < 6 and set(wrong) <= set(copies)


def test_the_lower_ordinals_box_is_the_inflated_one(B):
    one, swapped, margin = OC.asymmetry()
    m = F(margin)
    lo_i, hi_j = F(1), F(1) - F(2.0 ** -24)
    assert not (lo_i - m <= hi_j) and (lo_i <= hi_j + m), "the fp32 example: the two forms disagree"
    for (recs, prims, boxes, root), right, wrong in ((one, [[], []], [[1], []]), (swapped, [[1], []], [[], []])):
        exp = OR.pairs(recs, prims, boxes, root, margin)
        assert lists_of(exp) == right
        assert_lists(pairs_brute_host(B, recs, prims, boxes, root[2], margin), exp, "asymmetry")
        assert lists_of(OR.pairs(recs, prims, boxes, root, margin, mutant="inflate_higher")) == wrong
        # the box query says the same: box 0 inflated against box 1
        assert lists_of(brute_host(B, recs, prims, boxes, root[2], boxes[:1], margin))[0] == [0] + right[0]


def test_a_leafs_box_in_place_of_its_primitives_boxes_lists_too_much(B):
    (recs, prims, boxes, root), queries, margin = OC.second_misses()
    assert len(recs) == 0 and root[2] & NR.REF_LEAF and root[2] & NR.REF_TWO, "the root is a leaf of two"
    exp = OR.brute(recs, prims, boxes, root, queries, margin)
    assert len(exp[1]) == 1
    assert_lists(brute_host(B, recs, prims, boxes, root[2], queries, margin), exp, "second misses")
    assert_lists(OR.walk(recs, prims, boxes, root, queries, margin), exp, "second misses, walked")
    assert lists_of(OR.walk(recs, prims, boxes, root, queries, margin, mutant="leaf_box")) == [[0, 1]]


def test_pairs_listing_j_at_or_above_i_list_every_primitive_with_itself(B):
    (recs, prims, boxes, root), margin = OC.coincident()
    copies = sorted(k for k in range(len(prims)) if (prims[k, 0, :3] == 0).all())
    exp = OR.pairs(recs, prims, boxes, root, margin)
    assert len(exp[1]) == 15 and all(sorted(l) == [j for j in copies if j > i] for i, l in enumerate(lists_of(exp)) if i in copies)
    assert_lists(pairs_brute_host(B, recs, prims, boxes, root[2], margin), exp, "coincident")
    wrong = OR.pairs(recs, prims, boxes, root, margin, mutant="pairs_ge")
    assert len(wrong[1]) == 15 + len(prims) and all(i in l for i, l in enumerate(lists_of(wrong)))


# ---- CPU 5: the definitions' arguments ---------------------------------------------------------------------------------------------------------
def test_brute_host_refuses_null_arrays_a_bad_margin_and_a_short_capacity_leaves_items_alone(B):
    L = B.nearest_lib()
    recs, prims, boxes, root, queries = OC.tree_case("mixed300", "morton")
    recs, prims, boxes, queries = (np.ascontiguousarray(a, F) for a in (recs, prims, boxes, queries))
    n, P, R = len(queries), len(prims), len(recs)
    margin = OC.margins(boxes)[3]
    offsets = np.zeros(n + 1, np.uint32)
    total = C.c_uint64(0)
    call = lambda recs_p, prims_p, boxes_p, queries_p, offsets_p, items_p, cap, total_p, m=margin: L.gpuart_nearest_overlap_brute_host(
        recs_p, C.c_size_t(R), C.c_uint32(int(root[2])), prims_p, boxes_p, C.c_size_t(P), queries_p, C.c_size_t(n), C.c_float(m), None, offsets_p, items_p,
        C.c_size_t(cap), total_p)
    good = (_p(recs), _p(prims), _p(boxes), _p(queries), _p(offsets))
    for k in range(5):
        args = list(good)
        args[k] = None
        assert call(*args, None, 0, C.byref(total)) == ERR_ARG, k
        assert L.gpuart_nearest_last_error().decode().startswith("nearest:")
    assert call(*good, None, 0, None) == ERR_ARG
    for m in (NAN, INF, -INF, -1e-30, -1.0):
        assert call(*good, None, 0, C.byref(total), m=m) == ERR_ARG and "margin" in L.gpuart_nearest_last_error().decode(), m
    exp = OR.brute(recs, prims, boxes, root, queries, margin)
    assert len(exp[1]) > 8
    items = np.full(len(exp[1]), -7, np.int32)
    assert call(*good, _p(items), len(items) - 1, C.byref(total)) == 0
    assert (items == -7).all() and total.value == len(exp[1]) and (offsets == exp[0]).all(), "a short capacity is no error and writes no item"
    assert call(*good, _p(items), len(items), C.byref(total)) == 0
    assert_lists((offsets, items), exp, "with room")
    # the pairs
    poff = np.zeros(P + 1, np.uint32)
    pcall = lambda recs_p, prims_p, boxes_p, offsets_p, items_p, cap, total_p, m=margin: L.gpuart_nearest_pairs_brute_host(
        recs_p, C.c_size_t(R), C.c_uint32(int(root[2])), prims_p, boxes_p, C.c_size_t(P), C.c_float(m), offsets_p, items_p, C.c_size_t(cap), total_p)
    pgood = (_p(recs), _p(prims), _p(boxes), _p(poff))
    for k in range(4):
        args = list(pgood)
        args[k] = None
        assert pcall(*args, None, 0, C.byref(total)) == ERR_ARG, k
    assert pcall(*pgood, None, 0, None) == ERR_ARG
    for m in (NAN, INF, -1.0):
        assert pcall(*pgood, None, 0, C.byref(total), m=m) == ERR_ARG and "margin" in L.gpuart_nearest_last_error().decode(), m
    pexp = OR.pairs(recs, prims, boxes, root, margin)
    assert len(pexp[1]) > 2
    pitems = np.full(len(pexp[1]), -7, np.int32)
    assert pcall(*pgood, _p(pitems), len(pitems) - 1, C.byref(total)) == 0 and (pitems == -7).all() and total.value == len(pitems) and (poff == pexp[0]).all()
    assert pcall(*pgood, _p(pitems), len(pitems), C.byref(total)) == 0
    assert_lists((poff, pitems), pexp, "pairs, with room")
    # no queries and no primitives
    assert L.gpuart_nearest_overlap_brute_host(None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_size_t(0), None, C.c_size_t(0), C.c_float(0), None, _p(offsets), None,
                                               C.c_size_t(0), C.byref(total)) == 0 and total.value == 0
    assert L.gpuart_nearest_pairs_brute_host(None, C.c_size_t(0), C.c_uint32(0), None, None, C.c_size_t(0), C.c_float(0), _p(poff), None, C.c_size_t(0),
                                             C.byref(total)) == 0 and total.value == 0 and poff[0] == 0


# ---- CPU 6: the library as built ------------------------------------------------------------------------------------------------------------------
def test_the_kernels_have_no_scratch_and_the_library_exports_its_header(B, tmp_path):
    from tests.test_product_library import _code_object, _kernel_metadata
    from tests.util import exported
    lib = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    meta = _kernel_metadata(_code_object(lib, str(tmp_path)))
    kernels = sorted(k for k in meta if "k_overlap" in k)
    assert len(kernels) == 2 and "k_overlap_fill" in kernels[0] and "k_overlap_count" in kernels[1], sorted(meta)
    assert not [k for k in kernels if "k_nearest" in k or "k_within" in k or "k_knn" in k], kernels
    for k in kernels:
        text = "\n".join(meta[k])
        assert ".private_segment_fixed_size: 0" in text and ".vgpr_spill_count: 0" in text and ".sgpr_spill_count: 0" in text, text
        assert ".group_segment_fixed_size: %d" % (4 * 256 * B.NEAREST_RING) in text, text
        # 5 waves per SIMD as the sibling kernels: at most 96 registers, no AGPRs (they come out of the same file)
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= 96 and re.search(r"\.agpr_count:\s+0\b", text), text
    names = exported(lib)
    with open(os.path.join(ROOT, "include", "gpuart_nearest.h")) as f:
        header = f.read()
    assert all(n.startswith("gpuart_nearest_") for n in names) and all(n + "(" in header for n in names), [n for n in names if n + "(" not in header]
    assert sorted(n for n in names if n.startswith("gpuart_nearest_overlap_")) == OVERLAP_NAMES
    assert sorted(n for n in names if n.startswith("gpuart_nearest_pairs_")) == PAIRS_NAMES
    section = header[header.index("Box overlap: every primitive whose box meets a box"):]
    declared = sorted(set(re.findall(r"\b(gpuart_nearest_(?:overlap|pairs)_\w+)\(", section)))
    assert declared == sorted(OVERLAP_NAMES + PAIRS_NAMES) == sorted(set(re.findall(r"\b(gpuart_nearest_(?:overlap|pairs)_\w+)\(", header))), declared


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


def expected(b, queries, margin, us=None):
    """The restatement's definition over the arrays the device holds now, in the order of the device's own tree."""
    return OR.brute(*device_scene(b), queries, margin, us)


def expected_pairs(b, margin):
    return OR.pairs(*device_scene(b), margin)


def scene_margin(b):
    """The margin of the device tests: 0.02 times the root extent of what the device holds."""
    return OC.margins(device_scene(b)[2])[2]


def scene_queries(b, n, seed=0, spread=True, margin=None):
    """The query set for the uploaded scene; by the restatement it holds empty lists, lists of one, long lists and a very long one."""
    _, prims, boxes, _ = device_scene(b)
    margin = scene_margin(b) if margin is None else margin
    queries = OC.query_set(boxes, n, seed, margin)
    if spread:
        OC.assert_spread(expected(b, queries, margin)[0], len(prims))
    return queries, margin


def as_numpy(res):
    o, it = res
    if type(o).__module__.startswith("torch"):
        o, it = o.cpu().numpy().view(np.uint32), it.cpu().numpy().view(np.int32).reshape(-1)
    return o, it


def check(b, queries, margin, what, us=None, device=False):
    from tests.util import to_device
    got = as_numpy(b.overlaps(to_device(np.array(queries)) if device else queries, margin, user_sphere=us))
    assert_lists(got, expected(b, queries, margin, us), what)
    return got


def check_pairs(b, margin, what):
    exp = expected_pairs(b, margin)
    host = b.overlapping_pairs(margin)
    assert host[0].dtype == np.uint32 and host[1].dtype == np.int32
    assert_lists(host, exp, what + ": pairs, host")
    assert_lists(as_numpy(b.overlapping_pairs(margin, device=True)), exp, what + ": pairs, device")
    return host


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


# ---- GPU 8 ------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["box", "mixed300"])
def test_every_list_is_the_definitions_through_the_scenes_life(B, be, name):
    """After the upload, a refit, a Morton rebuild, a clustered rebuild and an edit that removes three and adds five: the handle follows
    the generation by itself; the refit changes the pair lists and keeps the order (the expectation walks the device's own records)."""
    from tests import refit_ref as RR
    s = upload_scene(be, name)
    n_prims = len(s["prims"])
    queries, margin = scene_queries(be, CHUNKS, seed=1)

    def stage(what):
        got = check(be, queries, margin, what)
        check(be, queries, margin, what + ", user sphere", US)
        check(be, queries, margin, what + ", device tensors", device=True)
        check(be, queries, margin, what + ", device tensors, user sphere", US, device=True)
        return got, check_pairs(be, margin, what)

    got, pairs = stage(name + ": uploaded")
    assert pairs[0][-1] > 0
    order = WR.tree_order(*device_scene(be)[:2], be.scene_device().root_ref)
    ordinals, payloads = RR.random_update(s["tree"], np.random.default_rng(5), 0.3, 0.3)
    bound = be._nearest.generation
    be.refit(ordinals, payloads)
    assert be.scene_device().generation == bound
    assert WR.tree_order(*device_scene(be)[:2], be.scene_device().root_ref) == order, "a refit keeps the order"
    moved, moved_pairs = stage(name + ": refitted")
    assert moved_pairs[1].tobytes() != pairs[1].tobytes() or moved_pairs[0].tobytes() != pairs[0].tobytes(), "the refit changes the pair lists"
    for mode in ("morton", "clustered"):
        be.rebuild(mode=mode)
        stage("%s: rebuilt, %s" % (name, mode))
    added = [(t, RR.payload_of((t, f))) for t, f in NC.mixed(5, seed=41)]
    be.edit(np.array([0, n_prims // 2, n_prims - 1], np.uint32), np.array([t for t, _ in added], np.uint32),
            np.array([d for _, d in added], F), mode="clustered", out=False)
    assert be.scene_device().n_prims == n_prims + 2
    queries, margin = scene_queries(be, CHUNKS, seed=2)
    stage(name + ": edited")


# ---- GPU 9 ------------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNKS])
def test_query_counts_around_the_wave_and_the_chunk(be, n):
    import torch
    upload_scene(be, "mixed300")
    queries, margin = scene_queries(be, CHUNKS, seed=7)
    queries = queries[:n]
    check(be, queries, margin, "%d queries" % n, device=True)
    check(be, queries, margin, "%d queries, user sphere" % n, US, device=True)
    check(be, queries, margin, "%d queries, host" % n, US)
    if n == 1:
        o, it = be.overlaps(torch.zeros((0, 6), dtype=torch.float32, device="cuda:0"))
        assert o.cpu().tolist() == [0] and tuple(it.shape) == (0,)
        o, it = be.overlaps(np.zeros((0, 6), F))
        assert o.tolist() == [0] and len(it) == 0


# ---- GPU 10 -----------------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n, blocks", [(300, 1), (1000, 1), (1000, 2)])
@pytest.mark.parametrize("name", ["mixed300", "chain"])
def test_lanes_refill_the_cursor_hands_out_chunks_and_deep_stacks_spill(B, be, name, n, blocks):
    """More queries than the launch has lanes, asserted from the handle: chunks from the cursor, idle lanes that take new queries while
    their neighbours walk on, and on the chain — deeper than the LDS ring, asserted from the restated walk — the lane's spill column, under
    a spill budget of one workgroup. The staged paths make several launches. The answers are those of the unlimited handle."""
    from tests.util import to_device
    if name == "chain":
        be.upload_bvh(WC.tree("chain", "clustered"))
        recs, prims, boxes, root = device_scene(be)
        stats = {}
        OR.walk(recs, prims, boxes, root, np.array([[*root[0], *root[1]]], F), 0.0, stats=stats)
        assert stats["deepest"] >= B.NEAREST_RING + 4, stats
    else:
        upload_scene(be, name)
    queries, margin = scene_queries(be, n, seed=n + blocks, spread=name != "chain")
    if name == "chain":
        queries = np.array(queries)
        lo, hi = device_scene(be)[3][:2]
        queries[::7] = [*lo, *hi]     # the root box: the walk stacks the whole chain
        OC.assert_spread(expected(be, queries, margin)[0], 24)     # (24 spheres: its longest lists hold them all)
    free = [as_numpy(be.overlaps(to_device(np.array(queries)), margin, user_sphere=us)) for us in (None, US)]
    free_pairs = as_numpy(be.overlapping_pairs(margin, device=True))
    n_prims = be.scene_device().n_prims
    # one workgroup's spill columns and no more: (max_depth + 2) levels of 1 KiB
    h = limits(B, be, max_blocks=blocks, spill_bytes=100 if blocks == 1 else 0)
    for us, unlimited in zip((None, US), free):
        got = as_numpy(be.overlaps(to_device(np.array(queries)), margin, user_sphere=us))
        got_blocks, launches = last_launch(B, h)
        assert got_blocks == blocks and launches == 1 and n > got_blocks * 256, (got_blocks, launches)
        assert_lists(got, expected(be, queries, margin, us), "%s, %d on %d" % (name, n, blocks))
        assert_lists(got, unlimited, "%s, %d on %d against the unlimited run" % (name, n, blocks))
    got = as_numpy(be.overlapping_pairs(margin, device=True))
    assert last_launch(B, h) == (min(blocks, -(-n_prims // 256)), 1)
    assert_lists(got, free_pairs, name + ": pairs under the limits")
    assert_lists(got, expected_pairs(be, margin), name + ": pairs under the limits, the definition")
    if blocks == 2:
        # the staged paths: chunks of 100 queries and of 100 ordinals
        limits(B, be, max_blocks=blocks, host_chunk=100)
        staged = be.overlaps(np.array(queries), margin, user_sphere=US)
        assert last_launch(B, h)[1] == n // 100, "the fill alone: ten staged launches"
        assert_lists(staged, free[1], name + ": staged box queries")
        staged = be.overlapping_pairs(margin)
        assert last_launch(B, h)[1] == 2 * -(-n_prims // 100), "count and fill, a launch per range of 100 ordinals"
        assert_lists(staged, free_pairs, name + ": staged pairs")


# ---- GPU 11 -----------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_primitive_moved_into_contact_becomes_a_pair(B, be):
    from tests import refit_ref as RR
    s = upload_scene(be, "mixed300")
    recs, prims, boxes, root = device_scene(be)
    before = lists_of(expected_pairs(be, 0.0))
    # two spheres (type 0) that are no pair at margin 0, by the restatement
    spheres = [k for k in range(len(prims)) if NR._type(prims[k]) == 0]
    i, j = next((a, b) for a in spheres for b in spheres if a < b and b not in before[a])
    assert_lists(be.overlapping_pairs(0.0), expected_pairs(be, 0.0), "before")
    there = prims[i, 0, :3].astype(np.float64)
    home = prims[j, 0, :3].astype(np.float64)
    radius = float(prims[j, 1, 0])

    def move(c):
        payload = RR.payload_of((0, [*[float(x) for x in c], radius]))
        be.refit(np.array([j], np.uint32), np.array([payload], F))

    move(there)
    got = be.overlapping_pairs(0.0)
    assert_lists(got, expected_pairs(be, 0.0), "moved onto the other")
    lists = lists_of(got)
    assert lists[i].count(j) == 1 and i not in lists[j], "listed once, in the lower ordinal's list"
    pairs = be.overlapping_pairs(0.0, as_pairs=True)
    assert ((pairs[:, 0] == i) & (pairs[:, 1] == j)).sum() == 1 and not ((pairs[:, 0] == j) & (pairs[:, 1] == i)).any()
    move(home)
    got = be.overlapping_pairs(0.0)
    assert_lists(got, expected_pairs(be, 0.0), "moved away")
    assert j not in lists_of(got)[i] and lists_of(got) == before


# ---- GPU 12 -----------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_capacity_is_never_exceeded_and_wrong_offsets_are_reported(B, be):
    """items lies between 64 canary words on either side. A capacity below the total is refused before any launch; one above it leaves the
    rows behind the total untouched. A fill handed the offsets of a smaller-margin count of the same boxes completes — every store is
    guarded —, writes nothing outside [0, capacity) and nothing at or beyond the next list's start, and finish reports the mismatch. A fill
    of one kind after a count of another is refused."""
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    upload_scene(be, "mixed300")
    queries, margin = scene_queries(be, CHUNKS, seed=4)
    exp, exp_small = expected(be, queries, margin, US), expected(be, queries, 0.0, US)
    total, total_small = int(exp[0][-1]), int(exp_small[0][-1])
    assert 0 < total_small < total
    scene = be.scene_device()
    n_prims = int(scene.n_prims)
    h = be._nearest_handle(scene)
    tq = to_device(np.array(queries))
    off, off_small = (torch.zeros(CHUNKS + 1, dtype=torch.int32, device="cuda:0") for _ in range(2))
    CANARY, SPARE = 64, 16
    buf = torch.full((CANARY + total + SPARE + CANARY,), -7, dtype=torch.int32, device="cuda:0")
    items_ptr = buf.data_ptr() + CANARY * 4
    torch.cuda.synchronize()
    usp = (C.c_float * 4)(*US)
    count = lambda m, o: N.gpuart_nearest_overlap_count(h, C.byref(scene), C.c_void_p(tq.data_ptr()), C.c_size_t(CHUNKS), C.c_float(m), usp, C.c_void_p(o.data_ptr()))
    fill = lambda o, cap: N.gpuart_nearest_overlap_fill(h, C.byref(scene), C.c_void_p(tq.data_ptr()), C.c_size_t(CHUNKS), C.c_float(margin), usp,
                                                        C.c_void_p(o.data_ptr()), C.c_void_p(items_ptr), C.c_size_t(cap))
    msg = lambda: N.gpuart_nearest_last_error().decode()
    t = C.c_uint64(0)
    assert count(0.0, off_small) == 0 and N.gpuart_nearest_overlap_total(h, C.byref(t)) == 0 and t.value == total_small
    assert count(margin, off) == 0 and N.gpuart_nearest_overlap_total(h, C.byref(t)) == 0 and t.value == total
    assert (off.cpu().numpy().view(np.uint32) == exp[0]).all() and (off_small.cpu().numpy().view(np.uint32) == exp_small[0]).all()
    # a short capacity: refused before any launch
    assert fill(off, total - 1) == ERR_ARG and str(total) in msg()
    assert N.gpuart_nearest_finish(h) == 0 and bool((buf == -7).all())
    # a capacity above the total: the lists, the rows behind the total untouched, between intact canaries
    assert fill(off, total + SPARE) == 0 and N.gpuart_nearest_finish(h) == 0
    host = buf.cpu().numpy()
    assert (host[:CANARY] == -7).all() and (host[CANARY + total:] == -7).all()
    assert_lists((exp[0], host[CANARY:CANARY + total].copy()), exp, "between the canaries")
    # the offsets of the smaller margin, and a capacity of their total: nothing outside [0, capacity)
    buf.fill_(-7)
    torch.cuda.synchronize()
    assert fill(off_small, total) == 0
    assert N.gpuart_nearest_finish(h) == ERR_ARG
    assert "the offsets are not this query set's count: the results are void" in msg()
    assert N.gpuart_nearest_finish(h) == 0, "reported once"
    host = buf.cpu().numpy()
    assert (host[:CANARY] == -7).all() and (host[CANARY + total_small:] == -7).all(), "nothing beyond the last offset"
    written = host[CANARY:CANARY + total_small]
    for i in range(CHUNKS):
        a, b = int(exp_small[0][i]), int(exp_small[0][i + 1])
        first = exp[1][int(exp[0][i]):int(exp[0][i]) + (b - a)]
        assert written[a:b].tobytes() == first.tobytes(), "list %d: its first %d items, and nothing at or beyond offsets[%d]" % (i, b - a, i + 1)
    # a fill of one kind after a count of another is refused, in every direction, with nothing written
    buf.fill_(-7)
    torch.cuda.synchronize()
    points = to_device(np.concatenate([np.array(queries)[:, :3], np.full((CHUNKS, 1), margin, F)], 1).astype(F))
    hits = torch.full((total + 64, 8), 7.0, dtype=torch.float32, device="cuda:0")
    wcount = lambda: N.gpuart_nearest_within_count(h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(CHUNKS), usp, C.c_void_p(off_small.data_ptr()))
    wfill = lambda: N.gpuart_nearest_within_fill(h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(CHUNKS), usp, C.c_void_p(off_small.data_ptr()),
                                                 C.c_void_p(hits.data_ptr()), C.c_size_t(hits.shape[0]))
    ofill = lambda: fill(off, total + SPARE)
    assert wcount() == 0
    assert ofill() == ERR_ARG and "the last count was of neighbour lists" in msg()
    assert count(margin, off) == 0
    assert wfill() == ERR_ARG and "the last count was of box queries" in msg()
    assert N.gpuart_nearest_finish(h) == 0 and bool((buf == -7).all()) and bool((hits == 7.0).all())
    # box queries and pairs of the same n — the scene's own boxes as the queries —, so that the kind alone refuses
    bq = to_device(np.array(device_scene(be)[2]))
    o2 = torch.zeros(n_prims + 1, dtype=torch.int32, device="cuda:0")
    i2 = torch.full((n_prims * 64,), -7, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    ocount2 = lambda: N.gpuart_nearest_overlap_count(h, C.byref(scene), C.c_void_p(bq.data_ptr()), C.c_size_t(n_prims), C.c_float(0), None, C.c_void_p(o2.data_ptr()))
    ofill2 = lambda: N.gpuart_nearest_overlap_fill(h, C.byref(scene), C.c_void_p(bq.data_ptr()), C.c_size_t(n_prims), C.c_float(0), None, C.c_void_p(o2.data_ptr()),
                                                   C.c_void_p(i2.data_ptr()), C.c_size_t(i2.shape[0]))
    pcount2 = lambda: N.gpuart_nearest_pairs_count(h, C.byref(scene), C.c_float(0), C.c_void_p(o2.data_ptr()))
    pfill2 = lambda: N.gpuart_nearest_pairs_fill(h, C.byref(scene), C.c_float(0), C.c_void_p(o2.data_ptr()), C.c_void_p(i2.data_ptr()), C.c_size_t(i2.shape[0]))
    assert ocount2() == 0 and pfill2() == ERR_ARG and "the last count was of box queries (overlap), this fill is of pairs" in msg()
    assert pcount2() == 0 and ofill2() == ERR_ARG and "the last count was of pairs, this fill is of box queries (overlap)" in msg()
    assert N.gpuart_nearest_finish(h) == 0 and bool((i2 == -7).all())
    assert pfill2() == 0 and N.gpuart_nearest_finish(h) == 0
    assert_lists((o2.cpu().numpy().view(np.uint32), i2[:int(o2[-1])].cpu().numpy()), expected_pairs(be, 0.0), "pairs after the refusals")
    check(be, queries, margin, "after the mismatch", US, device=True)


COUNTS = (("within", 0), ("within", 3), ("overlap", 0), ("overlap", 3), ("pairs", 7))
FILLS = (("within_fill", 0), ("within_fill", 3), ("overlap_fill", 0), ("overlap_fill", 3), ("pairs_fill", 7), ("within_fill_host", 0), ("within_fill_host", 3),
         ("overlap_fill_host", 0), ("overlap_fill_host", 3))
KIND = "nearest: the last count was of %s, this fill is of %s"
WITHIN, OVERLAP, PAIRS = "neighbour lists (within)", "box queries (overlap)", "pairs"
NOT_OF = "nearest: the last count was of %d queries, not of %d"
# (count, its n) -> per fill of FILLS: (return code, the last error where it failed, (blocks, launches) of the last launch where it did not),
# as a run of the library before the list protocol was stated once gave them.
FILL_TABLE = {
    ("within", 0): (
        (0, "", (0, 0)), (-1, NOT_OF % (0, 3), None),
        (-1, KIND % (WITHIN, OVERLAP), None), (-1, NOT_OF % (0, 3), None), (-1, NOT_OF % (0, 7), None),
        (0, "", (0, 0)), (0, "", (1, 1)), (0, "", (1, 0)), (0, "", (1, 1))),
    ("within", 3): (
        (-1, NOT_OF % (3, 0), None), (0, "", (1, 1)),
        (-1, NOT_OF % (3, 0), None), (-1, KIND % (WITHIN, OVERLAP), None), (-1, NOT_OF % (3, 7), None),
        (0, "", (1, 0)), (0, "", (1, 1)), (0, "", (1, 0)), (0, "", (1, 1))),
    ("overlap", 0): (
        # a within fill of no queries returns before it looks at whose the last count was; a box-query fill looks first (the next table's row)
        (0, "", (1, 0)), (-1, NOT_OF % (0, 3), None),
        (0, "", (1, 0)), (-1, NOT_OF % (0, 3), None), (-1, NOT_OF % (0, 7), None),
        (0, "", (1, 0)), (0, "", (1, 1)), (0, "", (1, 0)), (0, "", (1, 1))),
    ("overlap", 3): (
        (-1, NOT_OF % (3, 0), None), (-1, KIND % (OVERLAP, WITHIN), None),
        (-1, NOT_OF % (3, 0), None), (0, "", (1, 1)), (-1, NOT_OF % (3, 7), None),
        (0, "", (1, 0)), (0, "", (1, 1)), (0, "", (1, 0)), (0, "", (1, 1))),
    ("pairs", 7): (
        (-1, NOT_OF % (7, 0), None), (-1, NOT_OF % (7, 3), None),
        (-1, NOT_OF % (7, 0), None), (-1, NOT_OF % (7, 3), None), (0, "", (1, 1)),
        (0, "", (1, 0)), (0, "", (1, 1)), (0, "", (1, 0)), (0, "", (1, 1))),
}


def fill_rows(B, be):
    """Every fill of FILLS after every count of COUNTS on the seven primitives of "mixed7": {count: its row of FILL_TABLE}. The device fills
    get the offsets the count left, the two _fill_host entries the restatement's; every items array has room."""
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    upload_scene(be, "mixed7")
    queries, margin = scene_queries(be, 3, seed=4, spread=False)
    queries = np.array(queries)
    points = np.concatenate([queries[:, :3], np.full((3, 1), margin, F)], 1).astype(F)
    scene = be.scene_device()
    assert int(scene.n_prims) == 7
    h = be._nearest_handle(scene)
    tq, tp = to_device(queries), to_device(points)
    off = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    hits = torch.zeros((256, 8), dtype=torch.float32, device="cuda:0")
    items = torch.zeros(256, dtype=torch.int32, device="cuda:0")
    host_off = {("within", 3): np.array(WR.brute(*device_scene(be), points, None)[0], np.uint32), ("overlap", 3): np.array(expected(be, queries, margin)[0], np.uint32),
                ("within", 0): np.zeros(1, np.uint32), ("overlap", 0): np.zeros(1, np.uint32)}
    host_hits, host_items = np.zeros((256, 8), F), np.zeros(256, np.int32)
    torch.cuda.synchronize()
    sc, m, dp = C.byref(scene), C.c_float(margin), lambda t: C.c_void_p(t.data_ptr())
    cap = C.c_size_t(256)
    calls = {
        "within": lambda n: N.gpuart_nearest_within_count(h, sc, dp(tp), C.c_size_t(n), None, dp(off)),
        "overlap": lambda n: N.gpuart_nearest_overlap_count(h, sc, dp(tq), C.c_size_t(n), m, None, dp(off)),
        "pairs": lambda n: N.gpuart_nearest_pairs_count(h, sc, m, dp(off)),
        "within_fill": lambda n: N.gpuart_nearest_within_fill(h, sc, dp(tp), C.c_size_t(n), None, dp(off), dp(hits), cap),
        "overlap_fill": lambda n: N.gpuart_nearest_overlap_fill(h, sc, dp(tq), C.c_size_t(n), m, None, dp(off), dp(items), cap),
        "pairs_fill": lambda n: N.gpuart_nearest_pairs_fill(h, sc, m, dp(off), dp(items), cap),
        "within_fill_host": lambda n: N.gpuart_nearest_within_fill_host(h, sc, _p(points), C.c_size_t(n), None, _p(host_off["within", n]), _p(host_hits), cap),
        "overlap_fill_host": lambda n: N.gpuart_nearest_overlap_fill_host(h, sc, _p(queries), C.c_size_t(n), m, None, _p(host_off["overlap", n]), _p(host_items), cap),
    }
    rows = {}
    for count in COUNTS:
        row = []
        for fill, n in FILLS:
            assert calls[count[0]](count[1]) == 0, (count, N.gpuart_nearest_last_error().decode())
            rc = calls[fill](n)
            row.append((rc, N.gpuart_nearest_last_error().decode() if rc else "", None if rc else last_launch(B, h)))
            assert N.gpuart_nearest_finish(h) == 0, (count, fill, n, N.gpuart_nearest_last_error().decode())
        rows[count] = tuple(row)
    return rows


@gpu
def test_every_fill_after_every_count_answers_as_it_did(B, be):
    """The three kinds of count (neighbour lists, box queries, pairs) times the four fills (those three, and each _fill_host), at no queries
    and at three: the return code, the text where the call fails, the last launch's two numbers where it does not. FILL_TABLE is what the
    library answered before the lists' protocol was stated once for the kinds, the one difference between them included: a within fill of no
    queries succeeds whatever the last count was of, a box-query fill of none is refused after a count of another kind."""
    rows = fill_rows(B, be)
    for count in COUNTS:
        for (fill, n), got, exp in zip(FILLS, rows[count], FILL_TABLE[count]):
            assert got == exp, "after the count of %s, n = %d: %s, n = %d" % (*count, fill, n)


@gpu
def test_five_queries_through_host_memory_in_chunks_of_two_are_the_unchunked_bytes(B, be):
    """host_chunk = 2: three staged launches per pass, the last one short; offsets rebased by the running total, items at the chunk's place."""
    from oracle import oracle
    be.upload_bvh(np.ascontiguousarray(oracle.build_bvh(NC.mixed(5, 1))[0], F))
    assert int(be.scene_device().n_prims) == 5
    queries, margin = scene_queries(be, 5, seed=3, spread=False)
    queries = np.array(queries)
    h = limits(B, be)
    wide = 2 * OC.margins(device_scene(be)[2])[3]   # half the extent: there are pairs in more than one chunk
    whole, whole_pairs = be.overlaps(queries, margin, user_sphere=US), be.overlapping_pairs(wide)
    assert last_launch(B, h)[1] == 2 and whole[0][-1] > 0 and whole_pairs[0][-1] > 0
    limits(B, be, host_chunk=2)
    staged = be.overlaps(queries, margin, user_sphere=US)
    assert last_launch(B, h)[1] == 3, "the fill alone: chunks of 2, 2 and 1"
    assert_lists(staged, whole, "box queries in chunks of two")
    assert_lists(staged, expected(be, queries, margin, US), "box queries in chunks of two, the definition")
    staged = be.overlapping_pairs(wide)
    assert last_launch(B, h)[1] == 2 * 3, "count and fill, chunks of 2, 2 and 1 ordinals"
    assert_lists(staged, whole_pairs, "pairs in chunks of two")
    assert_lists(staged, expected_pairs(be, wide), "pairs in chunks of two, the definition")


@gpu
def test_a_lowered_cap_refuses_the_total_and_a_total_of_zero_works(B, be):
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    upload_scene(be, "box")
    queries, margin = scene_queries(be, CHUNKS, seed=1)
    total = int(expected(be, queries, margin)[0][-1])
    assert total > 200
    scene = be.scene_device()
    h = be._nearest_handle(scene)
    assert N.gpuart_nearest_within_set_max_items(h, C.c_uint64(100)) == 0
    tq = to_device(np.array(queries))
    off = to_device(np.zeros(CHUNKS + 1, np.int32))
    items = torch.full((total,), -7, dtype=torch.int32, device="cuda:0")
    t = C.c_uint64(0)
    assert N.gpuart_nearest_overlap_count(h, C.byref(scene), C.c_void_p(tq.data_ptr()), C.c_size_t(CHUNKS), C.c_float(margin), None, C.c_void_p(off.data_ptr())) == 0
    assert N.gpuart_nearest_overlap_total(h, C.byref(t)) == ERR_ARG and t.value == total
    assert str(total) in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_overlap_fill(h, C.byref(scene), C.c_void_p(tq.data_ptr()), C.c_size_t(CHUNKS), C.c_float(margin), None, C.c_void_p(off.data_ptr()),
                                         C.c_void_p(items.data_ptr()), C.c_size_t(total)) == ERR_ARG
    assert N.gpuart_nearest_finish(h) == 0 and bool((items == -7).all()), "items untouched"
    for q in (tq, queries):
        with pytest.raises(B.HipError, match=str(total)):
            be.overlaps(q, margin)
    ptotal = int(expected_pairs(be, margin)[0][-1])
    assert 0 < ptotal
    assert N.gpuart_nearest_within_set_max_items(h, C.c_uint64(ptotal - 1)) == 0
    for device in (False, True):
        with pytest.raises(B.HipError, match=str(ptotal)):
            be.overlapping_pairs(margin, device=device)
    assert N.gpuart_nearest_within_set_max_items(h, C.c_uint64(0)) == 0
    check(be, queries, margin, "the default cap again", device=True)
    for q in (tq, queries):
        with pytest.raises(ValueError, match=str(total)):
            be.overlaps(q, margin, max_items=total - 1)
    assert len(be.overlaps(queries, margin, max_items=total)[1]) == total
    # a total of zero: boxes beyond the root
    lo, hi = device_scene(be)[3][:2]
    far = (np.zeros((CHUNKS, 3)) + hi + 10).astype(F)
    far = np.concatenate([far, far + 1], 1).astype(F)
    assert expected(be, far, margin)[0][-1] == 0
    o, it = be.overlaps(to_device(far), margin)
    assert bool((o == 0).all()) and tuple(it.shape) == (0,)
    items = torch.full((64,), -7, dtype=torch.int32, device="cuda:0")
    o, it = be.overlaps(to_device(far), margin, out=(torch.full((CHUNKS + 1,), 9, dtype=torch.int32, device="cuda:0"), items))
    assert bool((o == 0).all()) and it is items and bool((items == -7).all()), "the fill writes nothing"
    o, it = be.overlaps(far, margin)
    assert (o == 0).all() and len(it) == 0


# ---- GPU 13 -----------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_every_input_kind_gives_the_same_bytes(B, be):
    import torch
    from tests.util import to_device
    upload_scene(be, "mixed300")
    queries, margin = scene_queries(be, CHUNKS, seed=6)
    queries = np.array(queries)
    exp = expected(be, queries, margin, US)
    total = int(exp[0][-1])
    tq = to_device(queries)
    unstaged = as_numpy(be.overlaps(tq, margin, user_sphere=US))
    assert_lists(unstaged, exp, "torch")
    assert_lists(as_numpy(be.overlaps(tq, margin, user_sphere=US)), unstaged, "the same call again")
    h = limits(B, be, host_chunk=64)
    staged = be.overlaps(queries, margin, user_sphere=US)
    assert last_launch(B, h)[1] == 3, "the fill alone: three staged launches of 64, 64 and 7 queries"
    assert staged[0].dtype == np.uint32 and staged[1].dtype == np.int32
    assert_lists(staged, unstaged, "NumPy, staged in chunks of 64, against the unstaged run")
    # gpuart_nearest_overlap_host by its two-call protocol
    N, scene = B.nearest_lib(), be.scene_device()
    off, t = np.full(CHUNKS + 1, 9, np.uint32), C.c_uint64(0)
    items = np.full(total, -7, np.int32)
    host = lambda it, cap: N.gpuart_nearest_overlap_host(h, C.byref(scene), _p(queries), C.c_size_t(CHUNKS), C.c_float(margin), (C.c_float * 4)(*US), _p(off), it,
                                                         C.c_size_t(cap), C.byref(t))
    assert host(None, 0) == 0 and t.value == total and (off == exp[0]).all() and last_launch(B, h)[1] == 3
    assert host(_p(items), total - 1) == 0 and t.value == total and (items == -7).all(), "a short capacity is no error and writes no item"
    assert host(_p(items), total) == 0 and last_launch(B, h)[1] == 2 * 3, "three staged launches per pass"
    assert_lists((off, items), unstaged, "gpuart_nearest_overlap_host, staged, against the unstaged run")
    # gpuart_nearest_overlap_fill_host: what it must refuse, and offsets of another margin
    items[:] = -7
    fill = lambda o, cap, m=margin: N.gpuart_nearest_overlap_fill_host(h, C.byref(scene), _p(queries), C.c_size_t(CHUNKS), C.c_float(m), (C.c_float * 4)(*US), _p(o),
                                                                      _p(items), C.c_size_t(cap))
    assert fill(off, total - 1) == ERR_ARG and fill(off[::-1].copy(), total) == ERR_ARG and (items == -7).all()
    assert fill(off, total) == 0
    assert_lists((off, items), unstaged, "gpuart_nearest_overlap_fill_host")
    assert fill(off, total, margin * 2) == ERR_ARG and "not this query set's count" in N.gpuart_nearest_last_error().decode()
    limits(B, be)
    assert_lists(be.overlaps(queries, margin, user_sphere=US), unstaged, "NumPy, one chunk")
    offsets = torch.full((CHUNKS + 1,), 9, dtype=torch.int32, device="cuda:0")
    items = torch.full((total + 5,), -7, dtype=torch.int32, device="cuda:0")
    o, it = be.overlaps(tq, margin, user_sphere=US, out=(offsets, items))
    assert o is offsets and it is items and bool((items[total:] == -7).all())
    assert_lists((offsets.cpu().numpy().view(np.uint32), items[:total].cpu().numpy()), exp, "out=")
    # the pairs: host, device, out=, as_pairs
    pexp = expected_pairs(be, margin)
    ptotal, n_prims = int(pexp[0][-1]), int(scene.n_prims)
    assert ptotal > n_prims
    assert_lists(be.overlapping_pairs(margin), pexp, "pairs, NumPy")
    po = torch.full((n_prims + 1,), 9, dtype=torch.int32, device="cuda:0")
    pi = torch.full((ptotal + 5,), -7, dtype=torch.int32, device="cuda:0")
    o, it = be.overlapping_pairs(margin, device=True, out=(po, pi))
    assert o is po and it is pi and bool((pi[ptotal:] == -7).all())
    assert_lists((po.cpu().numpy().view(np.uint32), pi[:ptotal].cpu().numpy()), pexp, "pairs, out=")
    ij = OR.as_pairs(pexp)
    host_pairs = be.overlapping_pairs(margin, as_pairs=True)
    assert host_pairs.dtype == np.int32 and host_pairs.tobytes() == ij.tobytes()
    dev_pairs = be.overlapping_pairs(margin, device=True, as_pairs=True)
    assert dev_pairs.dtype == torch.int32 and dev_pairs.cpu().numpy().tobytes() == ij.tobytes()
    with pytest.raises(ValueError, match=str(total)):
        be.overlaps(tq, margin, user_sphere=US, out=(offsets, torch.zeros((total - 1,), dtype=torch.int32, device="cuda:0")))


@gpu
def test_the_renderer_lists_what_the_backend_does(B):
    from gpuart_amd import synth_scenes as S
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        with pytest.raises(B.HipError, match="stderr"):
            r.primitives_overlapping(np.zeros((4, 6), F))
        r.set_user_sphere(US[:3], US[3], 0.0)
        r.set_primitives(NC.scene("box")["descs"])
        assert r.rebuild_tree("clustered") is not None
        rb = r.backend
        queries, margin = scene_queries(rb, CHUNKS, seed=21)
        queries = np.array(queries)
        exp, exp_us = expected(rb, queries, margin), expected(rb, queries, margin, US)
        assert exp_us[0][-1] > exp[0][-1] > 0
        assert_lists(r.primitives_overlapping(queries, margin, with_user_sphere=False), exp, "Renderer::PrimitivesOverlapping")
        assert_lists(r.primitives_overlapping(queries, margin, with_user_sphere=True), exp_us, "Renderer::PrimitivesOverlapping, user sphere")
        assert_lists(rb.overlaps(queries, margin, user_sphere=US), exp_us, "its context")
        # gpuart_renderer_primitives_overlapping by its two-call protocol
        off, t = np.zeros(CHUNKS + 1, np.uint32), C.c_uint64(0)
        call = lambda it, cap: r.L.gpuart_renderer_primitives_overlapping(r.h, _p(queries), C.c_size_t(CHUNKS), C.c_float(margin), C.c_int(1), _p(off), it, C.c_size_t(cap),
                                                                          C.byref(t))
        assert call(None, 0) == 1 and t.value == len(exp_us[1]) and (off == exp_us[0]).all()
        items = np.zeros(t.value, np.int32)
        assert call(_p(items), len(items)) == 1
        assert_lists((off, items), exp_us, "gpuart_renderer_primitives_overlapping, the second call")
        pexp = expected_pairs(rb, margin)
        assert pexp[0][-1] > 0
        assert_lists(r.overlapping_pairs(margin), pexp, "Renderer::OverlappingPairs")
        assert_lists(rb.overlapping_pairs(margin), pexp, "its context")
        n_descs = len(NC.scene("box")["descs"])
        nearest = r.closest_points(np.concatenate([queries[:, :3], np.full((CHUNKS, 1), INF, F)], 1)[np.isfinite(queries[:, :3]).all(1)], user_sphere=False)
        assert set(exp[1].tolist()) <= set(range(n_descs)) and nearest["prim"].max() < n_descs, "the ordinals are ClosestPoints'"
        with pytest.raises(B.HipError):
            r.primitives_overlapping(queries, -1.0)
        o, it = r.primitives_overlapping(np.zeros((0, 6), F))
        assert o.tolist() == [0] and len(it) == 0
    finally:
        r.close()


# ---- GPU 14 -----------------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_what_must_be_refused_is_refused_with_nothing_written(B, be):
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    s = upload_scene(be, "mixed7")
    queries, margin = scene_queries(be, 16, seed=4, spread=False)
    tq = to_device(np.array(queries))
    n_prims = int(be.scene_device().n_prims)
    off = torch.full((17,), 9, dtype=torch.int32, device="cuda:0")
    items = torch.full((256,), -7, dtype=torch.int32, device="cuda:0")
    untouched = lambda: bool((off == 9).all()) and bool((items == -7).all())
    torch.cuda.synchronize()
    count = lambda h, sc, p=tq.data_ptr(), n=16, o=off.data_ptr(), m=margin, us=None: N.gpuart_nearest_overlap_count(
        h, C.byref(sc), C.c_void_p(p), C.c_size_t(n), C.c_float(m), us, C.c_void_p(o))
    fill = lambda h, sc, it=items.data_ptr(), o=off.data_ptr(): N.gpuart_nearest_overlap_fill(h, C.byref(sc), C.c_void_p(tq.data_ptr()), C.c_size_t(16), C.c_float(margin), None,
                                                                                            C.c_void_p(o), C.c_void_p(it), C.c_size_t(64))
    pcount = lambda h, sc, o=off.data_ptr(), m=margin: N.gpuart_nearest_pairs_count(h, C.byref(sc), C.c_float(m), C.c_void_p(o))
    pfill = lambda h, sc: N.gpuart_nearest_pairs_fill(h, C.byref(sc), C.c_float(margin), C.c_void_p(off.data_ptr()), C.c_void_p(items.data_ptr()), C.c_size_t(64))
    msg = lambda: N.gpuart_nearest_last_error().decode()
    # an unbound handle
    fresh = B._NearestHandle(0)
    try:
        for call in (count, fill, pcount, pfill):
            assert call(fresh, be.scene_device()) == ERR_ARG and "not bound" in msg()
        assert N.gpuart_nearest_finish(fresh) == 0
    finally:
        fresh.close()
    # a stale generation: bound to the first upload, given the second one's
    be.overlaps(tq, margin)
    h = be._nearest
    be.upload_bvh(s["tree"])
    new = be.scene_device()
    for call in (count, fill, pcount, pfill):
        assert call(h, new) == ERR_ARG and "bind again" in msg()
    assert N.gpuart_nearest_bind(h, C.byref(new)) == 0
    # the margin
    for m in (NAN, INF, -INF, -1.0, -1e-30):
        assert count(h, new, m=m) == ERR_ARG and "margin" in msg(), m
        assert pcount(h, new, m=m) == ERR_ARG and "margin" in msg(), m
        for call in (lambda: be.overlaps(tq, m), lambda: be.overlaps(np.array(queries), m), lambda: be.overlapping_pairs(m), lambda: be.overlapping_pairs(m, device=True)):
            with pytest.raises(ValueError, match="margin"):
                call()
    # misaligned pointers, overlapping buffers, too many queries, NULL
    assert count(h, new, p=tq.data_ptr() + 2, n=15) == ERR_ARG and "misaligned" in msg()
    assert count(h, new, o=off.data_ptr() + 2, n=15) == ERR_ARG and "misaligned" in msg()
    assert pcount(h, new, o=off.data_ptr() + 2) == ERR_ARG and "misaligned" in msg()
    assert count(h, new, o=tq.data_ptr() + 64) == ERR_ARG and "overlaps" in msg()
    assert count(h, new, n=0x80000000) == ERR_ARG and "too many" in msg()
    assert count(h, new, p=None) == ERR_ARG
    assert pcount(h, new, o=None) == ERR_ARG
    assert count(h, new, p=None, n=0, o=None) == 0
    # a user sphere with a word that is not finite
    for bad in ((NAN, 0, 0, 1), (0, INF, 0, 1), (0, 0, 0, NAN), (0, 0, 0, -1.0)):
        assert count(h, new, us=(C.c_float * 4)(*bad)) == ERR_ARG and "user sphere" in msg(), bad
        with pytest.raises(B.HipError):
            be.overlaps(tq, margin, user_sphere=bad)
    # the fill: items misaligned, items overlapping the boxes or the offsets
    assert count(h, new) == 0 and N.gpuart_nearest_finish(h) == 0
    counted = off.clone()
    assert fill(h, new, it=items.data_ptr() + 2) == ERR_ARG and "misaligned" in msg()
    assert fill(h, new, it=tq.data_ptr() + 8) == ERR_ARG and "overlaps" in msg()
    assert fill(h, new, it=off.data_ptr() + 8) == ERR_ARG and "overlaps" in msg()
    assert N.gpuart_nearest_finish(h) == 0 and bool((off == counted).all()) and bool((items == -7).all())
    off.fill_(9)
    # wrong shapes, dtypes and devices
    with pytest.raises(ValueError, match="GPU"):
        be.overlaps(tq.cpu(), margin)
    with pytest.raises(ValueError):
        be.overlaps(tq.double(), margin)
    with pytest.raises(ValueError):
        be.overlaps(torch.zeros((16, 8), dtype=torch.float32, device="cuda:0")[:, :6], margin)
    with pytest.raises(ValueError):
        be.overlaps(torch.zeros((16, 4), dtype=torch.float32, device="cuda:0"), margin)
    with pytest.raises(ValueError):
        be.overlaps(np.zeros((16, 4), F), margin)
    with pytest.raises(ValueError):
        be.overlaps(tq, margin, out=(off.to(torch.int64), items))
    with pytest.raises(ValueError):
        be.overlaps(tq, margin, out=(off, items.cpu()))
    with pytest.raises(ValueError):
        be.overlaps(tq, margin, out=(off, items.to(torch.float32)))
    with pytest.raises(ValueError):
        be.overlapping_pairs(margin, device=True, out=(torch.zeros(n_prims, dtype=torch.int32, device="cuda:0"), items))
    with pytest.raises(ValueError):
        be.overlapping_pairs(margin, out=(off, items))
    assert untouched()
    before = tq.clone()
    h.generation = new.generation
    check(be, queries, margin, "after the refusals", device=True)
    check_pairs(be, margin, "after the refusals")
    assert bool((tq == before).all())
