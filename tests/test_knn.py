"""k nearest: the k nearest primitives of a point (include/gpuart_nearest.h "k nearest", libgpuart_nearest.so: gpuart_nearest_knn_*;
Backend.nearest_k, Renderer::NearestPrimitives). On the CPU: the definition (gpuart_nearest_knn_brute_host) is the restatement's
(tests/knn_ref.py) on every rule case for every k, k = 1 is the closest-point definition byte for byte, every found record is the
neighbour list's item for that primitive, the restated pruned walk is the restated definition in all three child orders, and five named
wrong rules are told from the right one. On the GPU: every row k_knn writes is the restatement's over the device's own arrays — through
the scene's life, for query counts around the wave and the chunk, under every grid and spill limit, with fewer primitives than k, for
every kind of radius, through every input kind; and what must be refused is refused with nothing written. There is no tolerance
anywhere: every comparison is on the records' 32-bit words."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import knn_cases as KC
from tests import knn_ref as KR
from tests import nearest_cases as NC
from tests import nearest_ref as NR
from tests import within_cases as WC

F = np.float32
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
US = NC.USER_SPHERES[1]
INF = float("inf")
MISS = np.array([(-1.0, (0, 0, 0), 0.0, -1, -1, 0)], NR.HIT)[0]
CAPACITIES = (4, 8, 16, 32)      # the kernel's specialisations: lists of that many entries in LDS


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def brute_host(B, prims, boxes, points, k, us=None):
    """gpuart_nearest_knn_brute_host on host arrays, with no handle and no device: (n, k) records."""
    L = B.nearest_lib()
    prims, boxes, points = np.ascontiguousarray(prims, F), np.ascontiguousarray(boxes, F), np.ascontiguousarray(points, F)
    hits = np.full((len(points), k, 8), 7.0, F).view(NR.HIT).reshape(len(points), k)
    usp = None if us is None else (C.c_float * 4)(*us)
    rc = L.gpuart_nearest_knn_brute_host(None, None, C.c_size_t(0), _p(prims), _p(boxes), C.c_size_t(len(prims)), _p(points), C.c_size_t(len(points)),
                                         C.c_size_t(k), usp, _p(hits))
    assert rc == 0, L.gpuart_nearest_last_error().decode()
    return hits


def assert_rows(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype.itemsize == 32 and exp.dtype.itemsize == 32, (what, got.shape, exp.shape)
    a, b = got.view(np.uint32).reshape(-1, 8), exp.view(np.uint32).reshape(-1, 8)
    bad = (a != b).any(1)
    k = got.shape[-1]
    assert not bad.any(), "%s: %d of %d records differ; first at query %d slot %d: got %s expected %s" % (
        what, int(bad.sum()), len(bad), int(np.argmax(bad)) // k, int(np.argmax(bad)) % k, got.reshape(-1)[bad][0], exp.reshape(-1)[bad][0])


def differ(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any())


def assert_shape_of_an_answer(rows, what):
    """What every answer shows, whatever it was computed from: found records first, in the contract's order, then misses and only misses."""
    n, k = rows.shape
    found = KR.found(rows)
    for i in range(n):
        row = rows[i]
        assert (row["prim"][:found[i]] != -1).all() and row[found[i]:].tobytes() == np.repeat(MISS, k - found[i]).tobytes(), (what, i)
        keys = [(row["d2"][j], int(row["prim"][j]) & 0xffffffff) for j in range(found[i])]
        assert keys == sorted(keys) and len(set(keys)) == len(keys), (what, i, keys)


# ---- CPU: the definition against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("us", NC.USER_SPHERES, ids=["no user sphere", "user sphere"])
@pytest.mark.parametrize("name", NC.RULE_CASES)
def test_the_definition_is_the_restatements(B, name, us):
    from tests.test_nearest import brute_host as nearest_brute_host
    from tests.test_within import brute_host as within_brute_host
    c = NC.rule_case(name)
    recs0, leaf_prims, root_ref = WC.root_leaf(c["recs"])
    offsets, items = within_brute_host(B, recs0, leaf_prims, c["boxes"], root_ref, c["points"], us)
    for k in KC.KS:
        exp = KR.brute(c["recs"], c["boxes"], c["points"], k, us)
        got = brute_host(B, c["recs"], c["boxes"], c["points"], k, us)
        assert_rows(got, exp, "%s, k = %d" % (name, k))
        assert_shape_of_an_answer(got, "%s, k = %d" % (name, k))
        # a found record is the item the neighbour list of the same query holds for that primitive, and a row holds min(k, the list's length)
        for i in range(len(got)):
            mine = items[offsets[i]:offsets[i + 1]]
            assert KR.found(got)[i] == min(k, len(mine)), (name, k, i)
            for rec in got[i][:KR.found(got)[i]]:
                assert rec.tobytes() == mine[mine["prim"] == rec["prim"]][0].tobytes(), (name, k, i, rec)
        if k == 1:
            assert_rows(got[:, 0], nearest_brute_host(B, c["recs"], c["boxes"], c["points"], us), name + ": k = 1 is the closest-point definition")
    if name == "misses":
        assert (KR.found(got) == 0).any() and (KR.found(got) > 0).any()


# ---- CPU: the restated pruned walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["morton", "clustered"])
@pytest.mark.parametrize("name", list(WC.TREE_SCENES))
def test_the_pruned_walk_is_the_definition_in_every_order(B, name, kind):
    recs, prims, boxes, root, points = KC.tree_queries(name, kind)
    for us in NC.USER_SPHERES:
        ctx = KR.prepare(recs, prims, boxes, root, points, us)
        for k in KC.KS:
            what = "%s %s%s, k = %d" % (name, kind, ", user sphere" if us else "", k)
            exp = KR.brute(prims, boxes, points, k, us)
            assert_rows(brute_host(B, prims, boxes, points, k, us), exp, what + ": the definition")
            for order in KR.ORDERS:
                assert_rows(KR.walk(recs, prims, boxes, root, points, k, us, order, ctx=ctx), exp, what + ", %s child first" % order)
            if k == 8 and name in ("mixed300", "chain"):
                found = KR.found(exp)
                kinds = ((found == k).sum(), ((found > 0) & (found < k)).sum(), (found == 0).sum())
                print(what, "full / short / empty:", kinds)
                assert min(kinds) >= 4, "%s: full, short and empty rows: %s" % (what, kinds)


# ---- CPU: the wrong rules, each caught by its named case ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", ["prune_ge", "d2_only"])
def test_a_tie_at_the_worst_kept_goes_to_the_lower_ordinal(B, mutant):
    recs, prims, boxes, root, points = KC.duplicates()
    copies = [o for o in range(len(prims)) if (prims[o, 0, :3] == 0).all()]
    assert len(copies) == 6 and len({o // 2 for o in copies}) >= 3, "the copies lie in at least three leaves"
    ctx = KR.prepare(recs, prims, boxes, root, points)
    for k in (1, 2, 3, 5):
        exp = KR.brute(prims, boxes, points, k)
        assert (exp["prim"] == copies[:k]).all() and (exp["d2"] == exp["d2"][:, :1]).all(), "the copies of the k lowest ordinals, at one distance"
        assert_rows(brute_host(B, prims, boxes, points, k), exp, "duplicates, k = %d: the definition" % k)
        for order in KR.ORDERS:
            assert_rows(KR.walk(recs, prims, boxes, root, points, k, None, order, ctx=ctx), exp, "duplicates, k = %d, %s first" % (k, order))
        for order in ("upper", "nearer"):
            wrong = KR.walk(recs, prims, boxes, root, points, k, None, order, mutant=mutant, ctx=ctx)
            assert differ(wrong, exp) and (wrong["d2"] == exp["d2"]).all(), "%s, k = %d, %s first: other copies at the same distance" % (mutant, k, order)
    for k in (6, 8):     # all six fit: nothing to tell
        exp = KR.brute(prims, boxes, points, k)
        assert_rows(KR.walk(recs, prims, boxes, root, points, k, None, "nearer", mutant=mutant, ctx=ctx)[:, :6], exp[:, :6], "k = %d" % k)


@pytest.mark.parametrize("kind", ["morton", "clustered"])
def test_the_worst_kept_prunes_only_a_full_list(B, kind):
    recs, prims, boxes, root, points = KC.tree_queries("mixed300", kind)
    exp = KR.brute(prims, boxes, points, 8)
    assert_rows(brute_host(B, prims, boxes, points, 8), exp, "mixed300: the definition")
    ctx = KR.prepare(recs, prims, boxes, root, points)
    assert_rows(KR.walk(recs, prims, boxes, root, points, 8, None, "nearer", ctx=ctx), exp, "mixed300, k = 8")
    wrong = KR.walk(recs, prims, boxes, root, points, 8, None, "nearer", mutant="before_full", ctx=ctx)
    assert differ(wrong, exp) and (KR.found(wrong) <= KR.found(exp)).all() and (KR.found(wrong) < KR.found(exp)).any(), "it loses candidates"
    # at k = 1 the list is full with its first entry: the two rules are one
    assert_rows(KR.walk(recs, prims, boxes, root, points, 1, None, "nearer", mutant="before_full", ctx=ctx), KR.brute(prims, boxes, points, 1), "k = 1")


def test_an_answer_is_sorted(B):
    recs, prims, boxes, root, points, k = KC.unsorted_case()
    exp = KR.brute(prims, boxes, points, k)
    assert (KR.found(exp) == k).all() and (np.diff(exp["d2"], axis=1) > 0).all(), "k found, at k different distances"
    assert_rows(brute_host(B, prims, boxes, points, k), exp, "mixed7: the definition")
    assert_rows(KR.walk(recs, prims, boxes, root, points, k), exp, "mixed7")
    wrong = KR.walk(recs, prims, boxes, root, points, k, mutant="unsorted")
    assert (wrong["d2"][:, 0] == exp["d2"][:, k - 1]).all(), "a heap's first entry is its worst"
    assert (np.sort(wrong["prim"], 1) == np.sort(exp["prim"], 1)).all(), "the same sets"


def test_without_the_clamp_the_record_is_another(B):
    recs, boxes, points, k = KC.unclamped()
    exp = KR.brute(recs, boxes, points, k)
    assert exp["prim"].tolist() == [[0, -1]] and exp["q"][0, 0, 0] == boxes[0, 3]
    assert_rows(brute_host(B, recs, boxes, points, k), exp, "unclamped")
    wrong = KR.brute(recs, boxes, points, k, mutant="no_clamp")
    assert differ(wrong[:, 0], exp[:, 0]) and wrong["q"][0, 0, 0] > boxes[0, 3] and not differ(wrong[:, 1], exp[:, 1])


# ---- CPU: the library as built, and the definition's arguments ---------------------------------------------------------------------------------
def test_the_kernels_have_no_scratch_and_the_library_exports_its_header(B, tmp_path):
    from tests.test_product_library import _code_object, _kernel_metadata
    from tests.util import exported
    lib = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    meta = _kernel_metadata(_code_object(lib, str(tmp_path)))
    kernels = {k: "\n".join(meta[k]) for k in meta if "k_knn" in k}
    assert len(kernels) == len(CAPACITIES) and not [k for k in kernels if "k_nearest" in k or "k_within" in k], sorted(meta)
    lds = []
    for name, text in kernels.items():
        assert ".private_segment_fixed_size: 0" in text and ".vgpr_spill_count: 0" in text and ".sgpr_spill_count: 0" in text, text
        # 5 waves per SIMD where the LDS leaves them (DESIGN.md "k nearest"): at most 96 registers, no AGPRs (they come out of the same file)
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= 96 and re.search(r"\.agpr_count:\s+0\b", text), text
        # the kernel reads some members of its launch from the argument segment by their offsets in the struct: the struct is the only
        # argument, by value, at offset 0
        args = re.findall(r"- \.offset:\s+(\d+)\n\s+\.size:\s+(\d+)\n\s+\.value_kind:\s+(\S+)", text)
        assert args[0][0] == "0" and args[0][2] == "by_value" and all(kind.startswith("hidden_") for _, _, kind in args[1:]), args
        lds.append(int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", text).group(1)))
    # per workgroup of four waves: the ring's 8 bytes x RING entries and the list's 8 bytes x capacity per thread — 512 (RING + capacity) per wave
    assert sorted(lds) == [4 * 512 * (B.NEAREST_RING + cap) for cap in CAPACITIES], lds
    assert max(CAPACITIES) == B.NEAREST_KNN_MAX == KC.KNN_MAX
    names = exported(lib)
    knn = sorted(n for n in names if n.startswith("gpuart_nearest_knn_"))
    assert knn == ["gpuart_nearest_knn_" + s for s in ("brute_host", "counts", "run", "run_host", "step_ms")], knn
    assert all(n.startswith("gpuart_nearest_") for n in names), names
    with open(os.path.join(ROOT, "include", "gpuart_nearest.h")) as f:
        header = f.read()
    assert all(n + "(" in header for n in names), [n for n in names if n + "(" not in header]
    assert "#define GPUART_NEAREST_KNN_MAX %du" % B.NEAREST_KNN_MAX in header


def test_brute_host_refuses_null_arrays_and_a_k_out_of_range(B):
    L = B.nearest_lib()
    c = NC.rule_case("box faces")
    prims, boxes, points = (np.ascontiguousarray(c[k], F) for k in ("recs", "boxes", "points"))
    n, P = len(points), len(prims)
    hits = np.full((n, KC.KNN_MAX + 1, 8), 7.0, F)
    call = lambda prims_p, boxes_p, n_prims, points_p, n, k, hits_p: L.gpuart_nearest_knn_brute_host(
        None, None, C.c_size_t(0), prims_p, boxes_p, C.c_size_t(n_prims), points_p, C.c_size_t(n), C.c_size_t(k), None, hits_p)
    for args in ((None, _p(boxes), P, _p(points), n, 3, _p(hits)), (_p(prims), None, P, _p(points), n, 3, _p(hits)),
                 (_p(prims), _p(boxes), P, None, n, 3, _p(hits)), (_p(prims), _p(boxes), P, _p(points), n, 3, None),
                 (_p(prims), _p(boxes), P, _p(points), n, 0, _p(hits)), (_p(prims), _p(boxes), P, _p(points), n, KC.KNN_MAX + 1, _p(hits))):
        assert call(*args) == ERR_ARG and L.gpuart_nearest_last_error().decode().startswith("nearest:")
        assert (hits == 7.0).all(), "nothing written"
    assert "k is 33" in L.gpuart_nearest_last_error().decode()
    assert call(_p(prims), _p(boxes), P, _p(points), n, KC.KNN_MAX, _p(hits)) == 0
    written = n * KC.KNN_MAX * 8
    assert_rows(hits.reshape(-1)[:written].view(NR.HIT).reshape(n, KC.KNN_MAX), KR.brute(prims, boxes, points, KC.KNN_MAX), "the most k")
    assert (hits.reshape(-1)[written:] == 7.0).all(), "n * k records and no more"
    # no primitives: k misses per query; no queries: nothing
    one = np.full((1, 2, 8), 7.0, F)
    assert call(None, None, 0, _p(points), 1, 2, _p(one)) == 0 and one.view(NR.HIT).tobytes() == np.repeat(MISS, 2).tobytes()
    assert call(None, None, 0, None, 0, 2, None) == 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
CHUNKS = 2 * 64 + 7   # twice GPUART_NEAREST_CHUNK plus 7


@pytest.fixture
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


def device_arrays(b):
    """(prims, boxes) the device holds now."""
    from tests.test_edit import device_arrays as read
    _, prims, boxes = read(b)
    return prims, boxes


def expected(b, points, k, us=None):
    """The restatement's definition over the arrays the device holds now."""
    return KR.brute(*device_arrays(b), points, k, us)


def as_rows(res):
    if type(res).__module__.startswith("torch"):
        n, k, _ = res.shape
        return res.cpu().numpy().view(NR.HIT).reshape(n, k)
    return res


def check(b, points, k, what, us=None, device=False):
    from tests.util import to_device
    got = as_rows(b.nearest_k(to_device(points) if device else points, k, user_sphere=us))
    assert_rows(got, expected(b, points, k, us), what)
    return got


def scene_points(b, n, seed=0):
    from tests.test_nearest import scene_points as make
    return make(b, n, seed)


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
def test_every_row_is_the_definitions_through_the_scenes_life(B, be, name):
    """After the upload, a refit, a Morton rebuild, a clustered rebuild and an edit that removes three and adds five: the handle follows
    the generation by itself, a refit needs no second bind."""
    from tests import refit_ref as RR
    s = upload_scene(be, name)
    n_prims = len(s["prims"])
    points = scene_points(be, 128, seed=1)

    def check_all(what):
        from tests.util import to_device
        for us in (None, US):
            most = expected(be, points, 32, us)      # (the definition's first k are the first k of its first 32)
            for k in (1, 3, 8, 32):
                got = as_rows(be.nearest_k(to_device(points) if k == 8 else points, k, user_sphere=us))
                assert_rows(got, most[:, :k], "%s: %s, k = %d%s" % (name, what, k, ", user sphere" if us else ""))
                if k == 1:
                    assert_rows(got[:, 0], be.closest_points(points, user_sphere=us), "%s: %s: k = 1 is closest_points" % (name, what))
        return got

    got = check_all("uploaded")
    found = KR.found(got)
    assert (found == 0).any() and ((found > 0) & (found < 32)).any() and (found == min(32, n_prims + 1)).any(), found
    ordinals, payloads = RR.random_update(s["tree"], np.random.default_rng(5), 0.3, 0.3)
    bound = be._nearest.generation
    be.refit(ordinals, payloads)
    assert be.scene_device().generation == bound
    assert differ(check_all("refitted"), got)
    for mode in ("morton", "clustered"):
        be.rebuild(mode=mode)
        assert be.scene_device().generation != be._nearest.generation
        check_all("rebuilt, " + mode)
    added = [(t, RR.payload_of((t, f))) for t, f in NC.mixed(5, seed=41)]
    be.edit(np.array([0, n_prims // 2, n_prims - 1], np.uint32), np.array([t for t, _ in added], np.uint32),
            np.array([d for _, d in added], F), mode="clustered", out=False)
    assert be.scene_device().n_prims == n_prims + 2
    points = scene_points(be, 128, seed=2)
    check_all("edited")


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNKS])
def test_query_counts_around_the_wave_and_the_chunk(be, n):
    import torch
    upload_scene(be, "mixed300")
    points = scene_points(be, CHUNKS, seed=7)[:n]
    check(be, points, 3, "%d queries" % n, device=True)
    check(be, points, 3, "%d queries, user sphere" % n, US, device=True)
    check(be, points, 3, "%d queries, host" % n, US)
    if n == 1:
        assert tuple(be.nearest_k(torch.zeros((0, 4), dtype=torch.float32, device="cuda:0"), 3).shape) == (0, 3, 8)
        assert be.nearest_k(np.zeros((0, 4), F), 3).shape == (0, 3)


@gpu
@pytest.mark.parametrize("n, blocks", [(300, 1), (1000, 1), (1000, 2)])
@pytest.mark.parametrize("name", ["mixed300", "chain"])
def test_lanes_refill_the_cursor_hands_out_chunks_and_deep_stacks_spill(B, be, name, n, blocks):
    """More queries than the launch has lanes, asserted from the handle: chunks from the cursor, idle lanes that take new queries — and
    with them a new list in the same column of LDS — while their neighbours walk on, and on the chain — deeper than the LDS ring,
    asserted from the descriptor and the restated closest-point walk — the lane's spill column. The answers are the unlimited handle's."""
    from tests.util import to_device
    if name == "chain":
        be.upload_bvh(WC.tree("chain", "clustered"))
        assert be.scene_device().max_depth >= B.NEAREST_RING + 4
        stats = {}
        from tests.test_within import device_scene
        NR.walk(*device_scene(be), np.array([[0, 0, 0, INF], [0.1, 0, 0, INF]], F), None, "nearer", stats=stats)
        assert stats["deepest"] >= B.NEAREST_RING + 4, stats
    else:
        upload_scene(be, name)
    points = scene_points(be, n, seed=n + blocks)
    if name == "chain":
        points[::7, :3] *= 0.01     # from near the centre every sphere's box is as near as the next: the walk stacks the whole chain
    k = 8
    free = [as_rows(be.nearest_k(to_device(points), k, user_sphere=us)) for us in (None, US)]
    h = limits(B, be, max_blocks=blocks)
    for us, unlimited in zip((None, US), free):
        got = as_rows(be.nearest_k(to_device(points), k, user_sphere=us))
        got_blocks, launches = last_launch(B, h)
        assert got_blocks == blocks and launches == 1 and n > got_blocks * 256, (got_blocks, launches)
        assert_rows(got, expected(be, points, k, us), "%s, %d on %d" % (name, n, blocks))
        assert_rows(got, unlimited, "%s, %d on %d against the unlimited run" % (name, n, blocks))
    found = KR.found(got)
    assert (found == k).any() and (found < k).any()
    if blocks == 1 and n == 1000:
        # a spill budget of two workgroups' columns: four by the work, two by the budget; and of next to nothing: one still runs
        per_block = (be.scene_device().max_depth + 2) * 8 * 256
        limits(B, be, spill_bytes=2 * per_block + 100)
        assert_rows(as_rows(be.nearest_k(to_device(points), k)), free[0], name + ": two workgroups' worth of spill")
        assert last_launch(B, h) == (2, 1)
        limits(B, be, spill_bytes=100)
        assert_rows(as_rows(be.nearest_k(to_device(points), k)), free[0], name + ": a tiny spill budget still runs one workgroup")
        assert last_launch(B, h) == (1, 1)


@gpu
@pytest.mark.parametrize("name", ["one", "two", "duplicates"])
def test_fewer_primitives_than_k_and_ties(B, be, name):
    """Root-leaf scenes of one primitive and of two, and the six coincident spheres, uploaded and rebuilt to the device's own Morton
    tree: ties resolve to the lowest ordinals, the user sphere — here a seventh copy of the spheres — comes last among equals, and the
    slots behind the candidates are misses."""
    from tests import build_ref as BR
    from tests import refit_ref as RR
    if name == "duplicates":
        be.upload_bvh(BR.build(NC.duplicates()[0])[0])
        points = np.array(NC.duplicates()[1])
        us = (0.0, 0.0, 0.0, 1.0)
    else:
        be.upload_bvh(BR.build([(t, RR.payload_of((t, f))) for t, f in NC.mixed(4, seed=8)[2:3 if name == "one" else 4]])[0])
        assert be.scene_device().n_recs == 0 and be.scene_device().root_ref & NR.REF_LEAF
        points = scene_points(be, 70, seed=3)
        us = US
    for what in ("uploaded", "rebuilt"):
        prims, _ = device_arrays(be)
        copies = [o for o in range(len(prims)) if (prims[o, 0, :3] == 0).all() and prims[o, 1, 0] == 1]
        for k in (1, 2, 3, 5, 7, 32):
            for sphere in (None, us):
                got = check(be, points, k, "%s, %s, k = %d%s" % (name, what, k, ", user sphere" if sphere else ""), sphere, device=k in (2, 7))
                assert_shape_of_an_answer(got, name)
                assert KR.found(got).max() <= len(prims) + (sphere is not None)
                if name == "duplicates":
                    assert len(copies) == 6
                    ties = (copies + ([-2] if sphere else []))[:k]
                    assert (got["prim"][:, :len(ties)] == ties).all() and (got["d2"][:, :len(ties)] == got["d2"][:, :1]).all(), (k, got["prim"])
        if name != "duplicates":
            assert (KR.found(got) < 32).all() and (KR.found(got) == len(prims) + 1).any()
        be.rebuild(mode="morton")


@gpu
@pytest.mark.parametrize("name", ["at radius", "mixed300"])
def test_every_kind_of_radius(be, name):
    """r = 0 on a surface and off it, a tiny r, +inf, NaN, negative, -0, and the radius that is exactly the distance of the k-th nearest
    (accepted: the row is full) beside the float below it (not: the row is one short); and points whose words are not finite."""
    from tests import build_ref as BR
    k = 3
    if name == "at radius":
        prims, points = NC.at_radius()
        be.upload_bvh(BR.build(prims + [NC.sphere((0, 0, 0), 0.5), NC.sphere((0, 0, 0), 0.25)])[0])
        rows = [list(p) for p in points]      # the outer sphere at exactly r = 2 (d2 = r r = 4) twice, and at r just below 2
    else:
        upload_scene(be, name)
        base = scene_points(be, 64, seed=9)
        free = np.array(base[:4])
        free[:, 3] = INF
        exact = expected(be, free, k)
        assert (KR.found(exact) == k).all()
        rows = []
        for p, row in zip(free[:, :3], exact):
            kth = row["dist"][k - 1]
            for r in (0.0, 1e-30, 1e-3, INF, float("nan"), -1.0, -0.0, -INF):
                rows.append([*p, r])
            # the k-th nearest's own distance, raised until its square reaches its d2 (the product rounds): accepted; one float below the
            # smallest such radius: not
            r = F(kth)
            while F(r) * F(r) < row["d2"][k - 1]:
                r = np.nextafter(F(r), F(INF))
            while F(np.nextafter(F(r), F(-INF))) ** 2 >= row["d2"][k - 1]:
                r = np.nextafter(F(r), F(-INF))
            rows.append([*p, r])
            rows.append([*p, np.nextafter(F(r), F(-INF))])
            rows.append([*row["q"][0], 0.0])      # on the nearest primitive's surface: r = 0 finds it
        rows += [[INF, 0, 0, INF], [0, float("nan"), 0, INF], [0, 0, -INF, 1.0]]
    points = np.array(rows, F)
    for us in (None, US):
        got = check(be, points, k, name + (", user sphere" if us else ""), us)
        check(be, points, k, name + ", device" + (", user sphere" if us else ""), us, device=True)
    got = check(be, points, k, name)
    found = KR.found(got)
    if name == "at radius":
        assert found.tolist() == [1, 1, 0] and (got["d2"][:2, 0] == 4).all()
    else:
        per = found[:-3].reshape(4, 11)
        assert (per[:, 3] == k).all() and (per[:, [4, 5, 7]] == 0).all() and (per[:, 8] == k).all() and (per[:, 9] == k - 1).all(), per
        assert (found[-3:] == 0).all()


@gpu
def test_every_input_kind_gives_the_same_bytes(B, be):
    import torch
    from gpuart_amd import synth_scenes as S
    from tests.util import to_device
    s = upload_scene(be, "box")
    points = scene_points(be, CHUNKS, seed=6)
    k = 3
    exp = expected(be, points, k, US)
    tp = to_device(points)
    unstaged = as_rows(be.nearest_k(tp, k, user_sphere=US))
    assert_rows(unstaged, exp, "torch")
    h = limits(B, be, host_chunk=64)
    staged = be.nearest_k(points, k, user_sphere=US)
    assert staged.dtype == B.NEAREST_HIT and staged.shape == (CHUNKS, k)
    # 64 // 3 = 21 queries to a chunk, whose 63 records are no more than a chunk of run_host holds: 135 queries in 7 launches
    assert last_launch(B, h)[1] == 7
    assert_rows(staged, unstaged, "NumPy, staged in chunks of 21 queries, against the unstaged run")
    limits(B, be)
    assert_rows(be.nearest_k(points, k, user_sphere=US), unstaged, "NumPy, one chunk")
    assert last_launch(B, h)[1] == 1
    out = torch.full((CHUNKS, k, 8), 7.0, dtype=torch.float32, device=tp.device)
    assert be.nearest_k(tp, k, user_sphere=US, out=out) is out
    assert_rows(as_rows(out), unstaged, "torch, out=")
    for bad in (torch.zeros((CHUNKS, k + 1, 8), dtype=torch.float32, device=tp.device), out.cpu(), out.double(), out.transpose(0, 1)):
        with pytest.raises(ValueError):
            be.nearest_k(tp, k, out=bad)
    with pytest.raises(ValueError, match="GPU"):
        be.nearest_k(tp.cpu(), k)
    with pytest.raises(ValueError):
        be.nearest_k(tp.double(), k)
    with pytest.raises(ValueError):
        be.nearest_k(points, k, out=out)
    for bad_k in (0, B.NEAREST_KNN_MAX + 1):
        with pytest.raises(ValueError):
            be.nearest_k(points, bad_k)
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        with pytest.raises(B.HipError, match="stderr"):
            r.nearest_primitives(points, k)
        r.set_user_sphere(US[:3], US[3], 0.0)
        r.set_primitives(s["descs"])
        rb = r.backend
        assert_rows(r.nearest_primitives(points, k, user_sphere=True), expected(rb, points, k, US), "Renderer::NearestPrimitives, user sphere")
        assert_rows(r.nearest_primitives(points, k, user_sphere=False), expected(rb, points, k), "Renderer::NearestPrimitives")
        assert_rows(rb.nearest_k(points, k, user_sphere=US), expected(rb, points, k, US), "its context")
        assert r.rebuild_tree("clustered") is not None
        assert_rows(r.nearest_primitives(points, 8, user_sphere=False), expected(rb, points, 8), "Renderer::NearestPrimitives after RebuildTree")
        assert r.nearest_primitives(np.zeros((0, 4), F), 2).shape == (0, 2)
        hits = np.full((CHUNKS, 2, 8), 7.0, F)
        for bad_k in (0, B.NEAREST_KNN_MAX + 1):
            assert r.L.gpuart_renderer_nearest_primitives(r.h, _p(points), C.c_size_t(CHUNKS), C.c_size_t(bad_k), C.c_int(1), _p(hits)) == 0
        assert (hits == 7.0).all()
    finally:
        r.close()


@gpu
def test_what_must_be_refused_is_refused_with_nothing_written(B, be):
    import torch
    from tests.util import to_device
    N = B.nearest_lib()
    s = upload_scene(be, "mixed7")
    points = to_device(scene_points(be, 16, seed=4))
    k = 3
    out = torch.full((16 * k + 1, 8), 7.0, dtype=torch.float32, device=points.device)
    untouched = lambda: bool((out == 7.0).all())
    torch.cuda.synchronize()
    run = lambda h, sc, p=points.data_ptr(), n=16, k=k, us=None, o=out.data_ptr(): N.gpuart_nearest_knn_run(
        h, C.byref(sc), C.c_void_p(p), C.c_size_t(n), C.c_size_t(k), us, C.c_void_p(o))
    msg = lambda: N.gpuart_nearest_last_error().decode()
    # an unbound handle
    fresh = B._NearestHandle(0)
    try:
        assert run(fresh, be.scene_device()) == ERR_ARG and "not bound" in msg()
        assert N.gpuart_nearest_finish(fresh) == 0
    finally:
        fresh.close()
    # a stale generation: bound to the first upload, given the second one's; and after a rebuild without a bind
    be.nearest_k(points, k)
    h = be._nearest
    be.upload_bvh(s["tree"])
    assert run(h, be.scene_device()) == ERR_ARG and "bind again" in msg()
    assert N.gpuart_nearest_bind(h, C.byref(be.scene_device())) == 0
    be.rebuild(mode="morton")
    new = be.scene_device()
    assert run(h, new) == ERR_ARG and "bind again" in msg()
    assert N.gpuart_nearest_bind(h, C.byref(new)) == 0
    # k out of range, too many records, NULL and misaligned pointers, overlap, a user sphere that is not finite or negative
    assert run(h, new, k=0) == ERR_ARG and "k is 0" in msg()
    assert run(h, new, k=B.NEAREST_KNN_MAX + 1) == ERR_ARG and "k is 33" in msg()
    assert run(h, new, n=0x7fffffff // 3 + 1) == ERR_ARG and "too many records" in msg()
    assert run(h, new, n=0x80000000, k=1) == ERR_ARG and "too many" in msg()
    assert run(h, new, p=None) == ERR_ARG and run(h, new, o=None) == ERR_ARG
    assert run(h, new, p=points.data_ptr() + 4, n=15) == ERR_ARG and "misaligned" in msg()
    assert run(h, new, o=out.data_ptr() + 8) == ERR_ARG and "misaligned" in msg()
    assert run(h, new, o=points.data_ptr() + 16 * 8) == ERR_ARG and "overlaps" in msg()
    assert run(h, new, p=out.data_ptr() + 16 * k * 32 - 16, n=16) == ERR_ARG and "overlaps" in msg(), "the last of n * k records"
    assert run(h, new, us=(C.c_float * 4)(0, 0, float("inf"), 1)) == ERR_ARG and run(h, new, us=(C.c_float * 4)(0, 0, 0, -1)) == ERR_ARG
    assert run(h, new, p=None, n=0, o=None) == 0
    assert N.gpuart_nearest_finish(h) == 0 and untouched()
    # the same through host memory
    hp, ho = points.cpu().numpy(), np.full((16 * k, 8), 7.0, F)
    host = lambda k: N.gpuart_nearest_knn_run_host(h, C.byref(new), _p(hp), C.c_size_t(16), C.c_size_t(k), None, _p(ho))
    assert host(0) == ERR_ARG and host(B.NEAREST_KNN_MAX + 1) == ERR_ARG and (ho == 7.0).all()
    before = points.clone()
    h.generation = new.generation
    check(be, points.cpu().numpy(), k, "after the refusals", device=True)
    assert bool((points == before).all())
    ms = (C.c_double * 1)(-1.0)
    assert N.gpuart_nearest_knn_step_ms(h, ms) == 0 and ms[0] > 0
