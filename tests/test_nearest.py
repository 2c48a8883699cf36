"""Closest-point queries over the uploaded scene's tree (include/gpuart_nearest.h, libgpuart_nearest.so; Backend.closest_points,
Renderer::ClosestPoints). On the CPU: the rule (csrc/hip/nearest_rule.h through gpuart_nearest_brute_host) is the restatement's
(tests/nearest_ref.py) bit for bit on every region of every type, the restatement agrees with a float64 statement of the same distances,
the pruned walk returns the brute force's record in every child order, and four named cases tell four wrong rules from the right one. On
the GPU: every record k_nearest writes is the restatement's brute force over the device's own arrays, bit for bit — after an upload, a
refit, both rebuilds and an edit, on root leaves, on leaves of many primitives, on a chain deeper than the LDS ring, for query counts
around the wave and the cursor's chunk, every kind of radius, with and without the user sphere, through every input kind; and what must
be refused is refused with nothing written."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import nearest_cases as NC
from tests import nearest_ref as NR

F = np.float32
ERR_ARG = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest |dist32 - dist64| / (scene extent + |p|) of the restatement over the non-degenerate rule cases, as measured
# (profiles/nearest.txt lists it per case): the geometry test asserts four times that. A mistaken region is wrong by many orders more.
MEASURED_REL_ERROR = 3.81e-8


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def brute_host(B, recs, boxes, points, us=None):
    """gpuart_nearest_brute_host on host arrays, with no handle and no device."""
    L = B.nearest_lib()
    recs, boxes = np.ascontiguousarray(recs, F), np.ascontiguousarray(boxes, F)
    points = np.ascontiguousarray(points, F)
    hits = np.zeros(len(points), NR.HIT)
    usp = None if us is None else (C.c_float * 4)(*us)
    rc = L.gpuart_nearest_brute_host(None, None, C.c_size_t(0), _p(recs), _p(boxes), C.c_size_t(len(recs)), _p(points), C.c_size_t(len(points)), usp, _p(hits))
    assert rc == 0, L.gpuart_nearest_last_error().decode()
    return hits


def assert_hits(got, exp, what):
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype.itemsize == 32 and exp.dtype.itemsize == 32, what
    a, b = got.view(np.uint32).reshape(-1, 8), exp.view(np.uint32).reshape(-1, 8)
    bad = (a != b).any(1)
    assert not bad.any(), "%s: %d of %d records differ; first %d: got %s expected %s" % (what, int(bad.sum()), len(bad), int(np.argmax(bad)),
                                                                                         got.reshape(-1)[bad][0], exp.reshape(-1)[bad][0])


def differ(a, b):
    return bool((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).any())


# ---- CPU: the rule against the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("us", NC.USER_SPHERES, ids=["no user sphere", "user sphere"])
@pytest.mark.parametrize("name", NC.RULE_CASES)
def test_the_rule_is_the_restatements(B, name, us):
    c = NC.rule_case(name)
    exp = NR.brute(c["recs"], c["boxes"], c["points"], us)
    assert_hits(brute_host(B, c["recs"], c["boxes"], c["points"], us), exp, name)
    if us is None and name != "misses":
        finite = np.isfinite(c["points"]).all(1)
        assert (exp["prim"][finite] >= 0).all(), "%s: a query with r = +inf met no primitive" % name


@pytest.mark.parametrize("name", [n for n in NC.RULE_CASES if NC.rule_case(n)["degenerate"]])
def test_a_degenerate_primitive_yields_a_finite_point_of_its_box(name):
    c = NC.rule_case(name)
    p = c["points"][:, :3]
    for rec, box in zip(c["recs"], c["boxes"]):
        q, d2 = NR.closest_on_prim(rec, box, p)
        assert np.isfinite(q).all() and np.isfinite(d2).all(), name
        assert ((q >= box[:3]) & (q <= box[3:])).all(), name


def test_every_region_of_the_triangle_is_met():
    """The first seven queries of "triangle regions" lie in the seven Voronoi regions, in the rule's order: their nearest points are the
    vertex, the point of the edge or the projection that region names."""
    c = NC.rule_case("triangle regions")
    q, _ = NR.closest_on_prim(c["recs"][0], c["boxes"][0], c["points"][:7, :3])
    assert (q == np.array([(0, 0, 0), (2, 0, 0), (1, 0, 0), (0, 2, 0), (0, 1, 0), (1, 1, 0), (0.5, 0.5, 0)], F)).all()


def test_the_cut_over_to_the_fixed_perpendicular_is_met_from_both_sides(B):
    """The case's records put the second pass' length n just below, at and just above 0.5 for points along their axes: both branches of
    the rule are taken within 1e-6 of the threshold, and (test_the_rule_is_the_restatements) header and restatement agree there."""
    c = NC.rule_case("fixed perpendicular threshold")
    along = c["points"][:4, :3]
    n = np.stack([NR.cone_radial(rec, along)[1] for rec in c["recs"]])
    assert (n[0] > 0.5).all() and (n[2] < 0.5).all() and (np.abs(n[:3] - 0.5) < 0.02).all(), n
    assert (n[3] >= 0.5).all() and (n[4] < 0.5).all() and (np.abs(n[3:] - 0.5) < 1e-6).all(), n
    exp = NR.brute(c["recs"][3:], c["boxes"][3:], c["points"])
    assert_hits(brute_host(B, c["recs"][3:], c["boxes"][3:], c["points"]), exp, "either side of n = 0.5")


# ---- CPU: the restatement against geometry, in float64 and written independently -----------------------------------------------------------
def _seg64(p, a, b):
    d = b - a
    t = np.clip(((p - a) @ d) / (d @ d), 0.0, 1.0)
    return np.linalg.norm(p - (a + t[:, None] * d), axis=1)


def dist64(t, d, p):
    """The distance of the points p (n, 3) to the surface of the primitive with data quads d, in float64."""
    d, p = np.asarray(d, np.float64), np.asarray(p, np.float64)
    if t == 0:
        return np.abs(np.linalg.norm(p - d[0:3], axis=1) - d[3])
    if t == 1:
        n = d[4:7] / np.linalg.norm(d[4:7])
        h = (p - d[0:3]) @ n
        radial = np.linalg.norm((p - d[0:3]) - h[:, None] * n, axis=1)
        return np.where(radial <= d[3], np.abs(h), np.hypot(h, radial - d[3]))
    if t == 2:
        a, b, c = d[0:3], d[4:7], d[8:11]
        out = np.minimum(np.minimum(_seg64(p, a, b), _seg64(p, b, c)), _seg64(p, c, a))
        nrm = np.cross(b - a, c - a)
        nrm = nrm / np.linalg.norm(nrm)
        h = (p - a) @ nrm
        foot = p - h[:, None] * nrm
        inside = np.ones(len(p), bool)
        for u, v in ((a, b), (b, c), (c, a)):
            inside &= np.cross(v - u, foot - u) @ nrm >= 0
        return np.where(inside, np.abs(h), out)
    c1, c2, r1, r2 = d[0:3], d[4:7], d[3], d[7]
    ax = (c2 - c1) / np.linalg.norm(c2 - c1)
    t_ = (p - c1) @ ax
    rho = np.linalg.norm((p - c1) - t_[:, None] * ax, axis=1)
    return _seg64(np.stack([t_, rho], 1), np.array([0.0, r1]), np.array([np.linalg.norm(c2 - c1), r2]))


def geometry_errors():
    """name -> the largest |dist32 - dist64| / (scene extent + |p|) over the case's primitives and finite queries."""
    out = {}
    for name in NC.RULE_CASES:
        c = NC.rule_case(name)
        if c["degenerate"]:
            continue
        pts = c["points"][np.isfinite(c["points"][:, :3]).all(1) & (np.abs(c["points"][:, :3]) < 1e30).all(1)][:, :3]
        lo, hi = c["boxes"][:, :3].min(0).astype(np.float64), c["boxes"][:, 3:].max(0).astype(np.float64)
        scale = np.linalg.norm(hi - lo) + np.linalg.norm(pts.astype(np.float64), axis=1)
        worst = 0.0
        for (t, d), rec, box in zip(c["prims"], c["recs"], c["boxes"]):
            _, d2 = NR.closest_on_prim(rec, box, pts)
            err = np.abs(np.sqrt(d2.astype(np.float64)) - dist64(t, d, pts)) / scale
            worst = max(worst, float(err.max()))
        out[name] = worst
    return out


def test_the_restatement_agrees_with_float64_geometry():
    errors = geometry_errors()
    for name, e in errors.items():
        print("%-36s %.3e" % (name, e))
    print("largest: %.3e" % max(errors.values()))
    assert len(errors) >= 10
    assert max(errors.values()) <= 4 * MEASURED_REL_ERROR, errors


# ---- CPU: the lemma — the pruned walk is the brute force, in every child order ------------------------------------------------------------
def trees_of(B, name):
    """name -> the host library's tree of the scene (what SetPrimitives uploads), the Morton restatement's and the clustered one's."""
    from tests import build_ref as BR
    from tests import ploc_ref as PR
    from tests.test_ray_queries import tree_prims
    s = NC.scene(name)
    host = np.ascontiguousarray(B.compile_bvh(s["descs"])[0], F)
    prims = tree_prims(host)
    return {"host library": host, "morton": BR.build(prims)[0], "clustered": PR.build(prims)[0]}


@pytest.mark.parametrize("name", list(NC.SCENES))
def test_the_pruned_walk_is_the_brute_force_in_every_order(B, name):
    for kind, tree in trees_of(B, name).items():
        recs, prims, boxes, root = NR.from_tree(tree)
        types = {int(t) & 3 for t in prims.view(np.uint32)[:, 0, 3]}
        assert name in ("mixed2",) or types == {0, 1, 2, 3}, (name, types)
        points = NC.points_for(boxes, 96 if len(prims) > 100 else 48, seed=len(prims))
        for us in NC.USER_SPHERES:
            exp = NR.brute(prims, boxes, points, us)
            assert (exp["prim"] >= 0).any() and (exp["prim"] == -1).any()
            assert_hits(brute_host(B, prims, boxes, points, us), exp, "%s %s: the rule" % (name, kind))
            for order in NR.ORDERS:
                assert_hits(NR.walk(recs, prims, boxes, root, points, us, order), exp, "%s %s, %s child first" % (name, kind, order))


# ---- CPU: the wrong rules, each caught by its named case ------------------------------------------------------------------------------------
def test_pruning_on_equality_loses_the_lowest_ordinal(B):
    from tests import build_ref as BR
    prims, points = NC.duplicates()
    tree, order = BR.build(prims)
    recs, dprims, boxes, root = NR.from_tree(tree)
    copies = [k for k in range(len(dprims)) if (dprims[k, 0, :3] == 0).all()]
    leaves = {k // 2 for k in copies}
    assert len(copies) == 6 and len(leaves) >= 3, "the copies lie in at least three leaves"
    exp = NR.brute(dprims, boxes, points)
    assert (exp["prim"] == copies[0]).all()
    assert_hits(brute_host(B, dprims, boxes, points), exp, "duplicates")
    for o in NR.ORDERS:
        assert_hits(NR.walk(recs, dprims, boxes, root, points, None, o), exp, "duplicates, %s first" % o)
    wrong = NR.walk(recs, dprims, boxes, root, points, None, "upper", mutant="prune_ge")
    assert differ(wrong, exp) and (wrong["prim"] != copies[0]).any() and (wrong["d2"] == exp["d2"]).all()


def test_without_the_clamp_the_point_leaves_its_box(B):
    prims, points = NC.unclamped()
    recs, boxes = NC.device_list(prims)
    exp = NR.brute(recs, boxes, points)
    assert_hits(brute_host(B, recs, boxes, points), exp, "unclamped")
    wrong = NR.brute(recs, boxes, points, mutant="no_clamp")
    assert differ(wrong, exp) and wrong["q"][0, 0] > boxes[0, 3] and exp["q"][0, 0] == boxes[0, 3]
    # ... and the lemma with it: the box is nearer than the clamped point is never, but nearer than the unclamped point it need not be
    assert NR.box_d2(boxes[0, :3], boxes[0, 3:], points[:, :3])[0] <= exp["d2"][0]


def test_a_primitive_at_exactly_r_is_accepted(B):
    prims, points = NC.at_radius()
    recs, boxes = NC.device_list(prims)
    exp = NR.brute(recs, boxes, points)
    assert exp["prim"].tolist() == [0, 0, -1] and (exp["d2"][:2] == 4).all() and (exp["dist"][:2] == 2).all()
    assert_hits(brute_host(B, recs, boxes, points), exp, "at the radius")
    wrong = NR.brute(recs, boxes, points, mutant="strict_accept")
    assert wrong["prim"].tolist() == [-1, -1, -1]


def test_the_second_primitive_of_a_pair_is_tested(B):
    from tests import build_ref as BR
    prims, points = NC.second_of_two()
    tree, order = BR.build(prims)
    recs, dprims, boxes, root = NR.from_tree(tree)
    assert len(recs) == 0 and root[2] & NR.REF_LEAF and root[2] & NR.REF_TWO, "the root is a leaf of two"
    exp = NR.brute(dprims, boxes, points)
    assert exp["prim"].tolist() == [1, 1, 0]
    assert_hits(brute_host(B, dprims, boxes, points), exp, "second of two")
    for o in NR.ORDERS:
        assert_hits(NR.walk(recs, dprims, boxes, root, points, None, o), exp, "second of two, %s first" % o)
    assert NR.walk(recs, dprims, boxes, root, points, None, "nearer", mutant="skip_second")["prim"].tolist() == [0, 0, 0]


# ---- CPU: the library as built ---------------------------------------------------------------------------------------------------------------
def test_the_kernel_has_no_scratch_and_the_library_exports_its_header(B, tmp_path):
    from tests.test_product_library import _code_object, _kernel_metadata
    from tests.util import exported
    lib = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    meta = _kernel_metadata(_code_object(lib, str(tmp_path)))
    kernels = [k for k in meta if "k_nearest" in k]
    assert len(kernels) == 1, sorted(meta)
    text = "\n".join(meta[kernels[0]])
    assert ".private_segment_fixed_size: 0" in text and ".vgpr_spill_count: 0" in text, text
    assert ".group_segment_fixed_size: %d" % (8 * 256 * B.NEAREST_RING) in text, text
    # 5 waves per SIMD (DESIGN.md "Closest points"): a SIMD's 512 registers per lane over 5 waves are 102, and registers are allocated in
    # eights: 96. No AGPRs (they come out of the same 512) and nothing spilled
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", text).group(1)) <= 96, text
    assert re.search(r"\.agpr_count:\s+0\b", text) and ".sgpr_spill_count: 0" in text, text
    names = exported(lib)
    assert names and all(n.startswith("gpuart_nearest_") for n in names), names
    with open(os.path.join(ROOT, "include", "gpuart_nearest.h")) as f:
        header = f.read()
    assert all(n + "(" in header for n in names), [n for n in names if n + "(" not in header]


def test_brute_host_refuses_null_arrays(B):
    L = B.nearest_lib()
    hits = np.zeros(1, NR.HIT)
    pts = np.zeros((1, 4), F)
    assert L.gpuart_nearest_brute_host(None, None, C.c_size_t(0), None, None, C.c_size_t(1), _p(pts), C.c_size_t(1), None, _p(hits)) == ERR_ARG
    assert L.gpuart_nearest_last_error().decode().startswith("nearest:")
    assert L.gpuart_nearest_brute_host(None, None, C.c_size_t(0), None, None, C.c_size_t(0), _p(pts), C.c_size_t(1), None, _p(hits)) == 0
    assert hits["prim"][0] == -1 and hits["dist"][0] == -1


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu
CHUNKS = 2 * 64 + 7   # twice GPUART_NEAREST_CHUNK plus 7
US = (0.4, 0.3, 0.2, 0.5)


@pytest.fixture
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


def device_arrays(b):
    from tests.test_edit import device_arrays as read
    return read(b)


def expected(b, points, us=None):
    """The restatement's brute force over the arrays the device holds now."""
    _, prims, boxes = device_arrays(b)
    return NR.brute(prims, boxes, points, us)


def scene_points(b, n, seed=0):
    """n interleaved queries for the uploaded scene, a tenth of them ON a surface (a former answer's q) with r = 0 or tiny."""
    _, prims, boxes = device_arrays(b)
    points = NC.points_for(boxes, n, seed)
    first = NR.brute(prims, boxes, points)
    for i in range(3, n, 10):
        if first["prim"][i - 1] >= 0:
            points[i, :3], points[i, 3] = first["q"][i - 1], (0.0 if i % 20 < 10 else 1e-30)
    return points


def check(b, points, what, us=None):
    got = b.closest_points(points, user_sphere=us)
    assert_hits(got, expected(b, points, us), what)
    return got


def upload_scene(b, name):
    s = NC.scene(name)
    b.upload_bvh(s["tree"])
    return s


@gpu
@pytest.mark.parametrize("name", ["box", "mixed300"])
def test_every_record_is_the_brute_forces_through_the_scenes_life(B, be, name):
    """After the upload, a refit, a Morton rebuild, a clustered rebuild and an edit that removes and adds: the handle follows the
    generation by itself, a refit needs no second bind."""
    from tests import refit_ref as RR
    s = upload_scene(be, name)
    n_prims = len(s["prims"])
    points = scene_points(be, CHUNKS, seed=1)
    got = check(be, points, name + ": uploaded")
    assert (got["prim"] >= 0).sum() > CHUNKS // 3 and (got["prim"] == -1).any() and (got["d2"][got["prim"] >= 0] == 0).any()
    check(be, points, name + ": uploaded, user sphere", US)
    bound = be._nearest.generation
    ordinals, payloads = RR.random_update(s["tree"], np.random.default_rng(5), 0.3, 0.3)
    be.refit(ordinals, payloads)
    assert be.scene_device().generation == bound
    moved = check(be, points, name + ": refitted")
    assert differ(moved, got)
    for mode in ("morton", "clustered"):
        be.rebuild(mode=mode)
        assert be.scene_device().generation != be._nearest.generation
        check(be, points, "%s: rebuilt, %s" % (name, mode))
        check(be, points, "%s: rebuilt, %s, user sphere" % (name, mode), US)
    added = [(t, RR.payload_of((t, f))) for t, f in NC.mixed(5, seed=41)]
    be.edit(np.array([0, n_prims // 2, n_prims - 1], np.uint32), np.array([t for t, _ in added], np.uint32),
            np.array([d for _, d in added], F), mode="clustered", out=False)
    assert be.scene_device().n_prims == n_prims + 2
    check(be, scene_points(be, CHUNKS, seed=2), name + ": edited", US)


@gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, CHUNKS])
def test_query_counts_around_the_wave_and_the_chunk(be, n):
    upload_scene(be, "mixed300")
    points = scene_points(be, n, seed=n)
    check(be, points, "%d queries" % n)
    check(be, points, "%d queries, user sphere" % n, US)


def limits(B, be, max_blocks=0, spill_bytes=0, host_chunk=0):
    """gpuart_nearest_set_limits on the context's handle (made and bound here if need be)."""
    h = be._nearest_handle(be.scene_device())
    assert B.nearest_lib().gpuart_nearest_set_limits(h, C.c_uint32(max_blocks), C.c_size_t(spill_bytes), C.c_size_t(host_chunk)) == 0
    return h


def last_launch(B, h):
    blocks, launches = C.c_uint32(), C.c_uint32()
    assert B.nearest_lib().gpuart_nearest_last_launch(h, C.byref(blocks), C.byref(launches)) == 0
    return blocks.value, launches.value


def chain_tree():
    from tests import ploc_ref as PR
    from tests import refit_ref as RR
    return PR.build([(t, RR.payload_of((t, f))) for t, f in NC.chain(24)])[0]


@gpu
@pytest.mark.parametrize("n, blocks", [(300, 1), (1000, 1), (1000, 2)])
@pytest.mark.parametrize("name", ["mixed300", "chain"])
def test_lanes_refill_and_the_cursor_hands_out_chunks(B, be, name, n, blocks):
    """More queries than the launch has lanes — asserted from the handle —, so that every wave goes on past its first chunk: chunks from
    the cursor (300 on one workgroup: a last chunk of 44), idle lanes that take new queries while their neighbours walk on (near, far and
    radius-limited points interleaved), a lane's stack begun anew, on the chain with its spill column in use."""
    from tests.util import to_device
    if name == "chain":
        be.upload_bvh(chain_tree())
    else:
        upload_scene(be, name)
    h = limits(B, be, max_blocks=blocks)
    points = scene_points(be, n, seed=n + blocks)
    if name == "chain":
        points[::7, :3] *= 0.01     # from near the centre every sphere's box is as near as the next: the walk stacks the whole chain
    for us in (None, US):
        assert_hits(be.closest_points(to_device(points), user_sphere=us).cpu().numpy().view(NR.HIT).reshape(-1), expected(be, points, us), "%s, %d on %d" % (name, n, blocks))
        got_blocks, launches = last_launch(B, h)
        assert got_blocks == blocks and launches == 1 and n > got_blocks * 256, (got_blocks, launches)


@gpu
def test_a_small_spill_budget_shrinks_the_grid_and_run_host_stages_in_chunks(B, be):
    be.upload_bvh(chain_tree())
    per_block = (be.scene_device().max_depth + 2) * 8 * 256
    h = limits(B, be, spill_bytes=2 * per_block + 100, host_chunk=100)
    points = scene_points(be, 2000, seed=12)
    points[::5, :3] *= 0.01
    from tests.util import to_device
    assert_hits(be.closest_points(to_device(points)).cpu().numpy().view(NR.HIT).reshape(-1), expected(be, points), "two workgroups' worth of spill")
    assert last_launch(B, h) == (2, 1)      # (eight workgroups by the work, two by the budget)
    check(be, points[:1000], "staged in chunks of 100", US)
    assert last_launch(B, h) == (1, 10)
    check(be, points[:250], "staged in chunks of 100, the last of 50")
    assert last_launch(B, h)[1] == 3
    limits(B, be)
    check(be, points[:1000], "the defaults again")
    assert last_launch(B, h) == (4, 1)


@gpu
@pytest.mark.parametrize("name", ["box", "mixed300"])
def test_a_set_primitives_tree_answers(B, name):
    """The scene through Renderer::SetPrimitives — the host library's build, compilation and upload —, queried through the renderer, and
    through its context with NumPy arrays and device tensors."""
    from gpuart_amd import synth_scenes as S
    from tests.util import to_device
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        r.set_user_sphere(US[:3], US[3], 0.0)
        r.set_primitives(NC.scene(name)["descs"])
        rb = r.backend
        assert rb.scene_device().n_prims == len(NC.scene(name)["descs"])
        points = scene_points(rb, CHUNKS, seed=21)
        exp = expected(rb, points)
        assert (exp["prim"] >= 0).sum() > CHUNKS // 3
        assert_hits(r.closest_points(points, user_sphere=False), exp, name + ": Renderer::ClosestPoints")
        assert_hits(r.closest_points(points, user_sphere=True), expected(rb, points, US), name + ": Renderer::ClosestPoints, user sphere")
        assert_hits(rb.closest_points(points), exp, name + ": Backend, NumPy")
        assert_hits(rb.closest_points(to_device(points)).cpu().numpy().view(NR.HIT).reshape(-1), exp, name + ": Backend, torch")
    finally:
        r.close()


@gpu
def test_every_kind_of_radius(be):
    upload_scene(be, "mixed300")
    base = scene_points(be, 64, seed=9)
    surface = expected(be, base)["q"][0]
    rows = []
    for r in (0.0, 1e-30, 1e-3, 0.25, np.inf, np.nan, -1.0, -0.0, -np.inf):
        for p in (base[0, :3], base[1, :3], base[2, :3], surface):
            rows.append([*p, r])
    points = np.array(rows, F)
    got = check(be, points, "radii")
    by_r = got["prim"].reshape(-1, 4)
    assert (by_r[4] >= 0).all() and (by_r[5] == -1).all() and (by_r[6] == -1).all() and (by_r[8] == -1).all() and by_r[0, 3] >= 0
    check(be, points, "radii, user sphere", US)


@gpu
@pytest.mark.parametrize("name", ["one", "two", "many", "chain", "duplicates"])
def test_root_leaves_long_leaves_a_deep_chain_and_ties(B, be, name):
    """A scene of one primitive and of two (the root is a leaf), a tree whose leaves hold more than two primitives, a chain deeper than
    the LDS ring by at least four levels — asserted from the descriptor, so that the walk spills —, and coincident primitives."""
    from tests import build_ref as BR
    from tests import converter_ref as CR
    from tests import refit_ref as RR
    if name in ("one", "two"):
        tree = BR.build([(t, RR.payload_of((t, f))) for t, f in NC.mixed(4, seed=8)[2:3 if name == "one" else 4]])[0]
    elif name == "many":
        tree = np.ascontiguousarray(B.compile_bvh(NC.mixed(40, seed=4), 1024, 6)[0], F)
    elif name == "chain":
        from tests import ploc_ref as PR     # (the Morton rule balances equal keys by index; clustering nests the spheres one by one)
        tree = PR.build([(t, RR.payload_of((t, f))) for t, f in NC.chain(24)])[0]
    else:
        tree = BR.build(NC.duplicates()[0])[0]
    be.upload_bvh(tree)
    s = be.scene_device()
    cv = CR.convert(tree)
    if name in ("one", "two"):
        assert s.n_recs == 0 and s.root_ref & NR.REF_LEAF
    if name == "many":
        counts = [len(NR.leaf_members(cv["prims"], int(r))) for r in cv["refs"] if int(r) & NR.REF_LEAF]
        assert max(counts) > 2, counts
    if name == "chain":
        assert s.max_depth >= B.NEAREST_RING + 4, s.max_depth
        stats = {}
        centre = np.array([[0, 0, 0, np.inf], [0.1, 0, 0, np.inf]], F)
        NR.walk(*NR.from_tree(tree), centre, None, "nearer", stats=stats)
        assert stats["deepest"] >= B.NEAREST_RING + 4, stats
    points = NC.duplicates()[1] if name == "duplicates" else scene_points(be, 70, seed=3)
    if name == "chain":
        points[:2] = [[0, 0, 0, np.inf], [0.1, 0, 0, np.inf]]
    got = check(be, points, name)
    check(be, points, name + ", user sphere", US)
    if name == "duplicates":
        assert (got["prim"] == got["prim"].min()).all() and got["prim"].min() >= 0


@gpu
def test_every_input_kind_gives_the_same_records(B, be):
    import torch
    from tests.util import to_device
    s = upload_scene(be, "box")
    points = scene_points(be, CHUNKS, seed=6)
    exp = expected(be, points, US)
    assert_hits(be.closest_points(points, user_sphere=US), exp, "NumPy")
    tp = to_device(points)
    out = torch.full((len(points), 8), 7.0, dtype=torch.float32, device=tp.device)
    got = be.closest_points(tp, user_sphere=US, out=out)
    assert got is out
    assert_hits(out.cpu().numpy().view(NR.HIT).reshape(-1), exp, "torch, in place")
    assert_hits(be.closest_points(tp, user_sphere=US).cpu().numpy().view(NR.HIT).reshape(-1), exp, "torch")
    assert be.closest_points(to_device(np.zeros((0, 4), F))).shape == (0, 8) and len(be.closest_points(np.zeros((0, 4), F))) == 0
    cam = dict(__import__("gpuart_amd.synth_scenes", fromlist=["x"]).DEFAULT_CAMERA)
    cam["dir"] = __import__("gpuart_amd.synth_scenes", fromlist=["x"]).camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        r.set_user_sphere(US[:3], US[3], 0.0)
        r.set_primitives(s["descs"])
        rb = r.backend
        assert_hits(r.closest_points(points, user_sphere=True), expected(rb, points, US), "Renderer::ClosestPoints")
        assert_hits(r.closest_points(points, user_sphere=False), expected(rb, points), "Renderer::ClosestPoints, no user sphere")
        assert r.rebuild_tree("clustered") is not None
        assert_hits(r.closest_points(points, user_sphere=False), expected(rb, points), "Renderer::ClosestPoints after RebuildTree")
    finally:
        r.close()


@gpu
def test_what_must_be_refused_is_refused_with_nothing_written(B, be):
    import torch
    from tests import converter_ref as CR
    from tests.util import to_device
    N = B.nearest_lib()
    s = upload_scene(be, "mixed7")
    points = to_device(scene_points(be, 16, seed=4))
    out = torch.full((16, 8), 7.0, dtype=torch.float32, device=points.device)
    untouched = lambda: bool((out == 7.0).all())
    # a stale descriptor: bound to the first upload, given the second one's
    be.closest_points(points)
    h = be._nearest
    old = be.scene_device()
    be.upload_bvh(s["tree"])
    new = be.scene_device()
    assert new.generation != old.generation
    args = lambda sc: (h, C.byref(sc), C.c_void_p(points.data_ptr()), C.c_size_t(16), None, C.c_void_p(out.data_ptr()))
    assert N.gpuart_nearest_run(*args(new)) == ERR_ARG and "bind again" in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_finish(h) == 0 and untouched()
    # NULL and misaligned pointers, too many queries, a bad user sphere
    assert N.gpuart_nearest_bind(h, C.byref(new)) == 0
    assert N.gpuart_nearest_run(h, C.byref(new), None, C.c_size_t(16), None, C.c_void_p(out.data_ptr())) == ERR_ARG
    assert N.gpuart_nearest_run(h, C.byref(new), C.c_void_p(points.data_ptr() + 4), C.c_size_t(15), None, C.c_void_p(out.data_ptr())) == ERR_ARG
    assert N.gpuart_nearest_run(h, C.byref(new), C.c_void_p(points.data_ptr()), C.c_size_t(0x80000000), None, C.c_void_p(out.data_ptr())) == ERR_ARG
    assert N.gpuart_nearest_run(h, C.byref(new), C.c_void_p(points.data_ptr()), C.c_size_t(16), (C.c_float * 4)(0, 0, 0, -1), C.c_void_p(out.data_ptr())) == ERR_ARG
    assert N.gpuart_nearest_run(h, C.byref(new), None, C.c_size_t(0), None, None) == 0
    assert N.gpuart_nearest_finish(h) == 0 and untouched()
    # a hand-compiled tree with one interior box shrunk by an ulp. The uploader itself classifies it disorderly (every child box is
    # held to its parent's there: tests/converter_ref.py), so bind refuses the descriptor it hands out ...
    tree = np.array(NC.scene("mixed7")["tree"], F)
    lay = CR.layout(tree)
    inner = [k for k in range(1, len(lay["addr"])) if not lay["leaf"][k] and not lay["leaf"][lay["parent"][k]]]
    assert inner, "an interior node below the root"
    a = int(lay["addr"][inner[0]])
    tree[a + 1, 0] = np.nextafter(tree[a + 1, 0], F(-np.inf))     # its upper x plane, one ulp inwards
    be.upload_bvh(tree)
    shrunk = be.scene_device()
    assert shrunk.exact_boxes == 1, "the uploader classifies the shrunk tree disorderly"
    with pytest.raises(B.HipError) as e:
        be.closest_points(points, out=out)
    assert e.value.code == ERR_ARG and "irregular" in str(e.value) and untouched()
    # ... and so that the nesting launch itself is held to the case: the same descriptor with the uploader's verdict struck out
    shrunk.exact_boxes = 0
    assert N.gpuart_nearest_bind(h, C.byref(shrunk)) == ERR_ARG
    msg = N.gpuart_nearest_last_error().decode()
    assert "record" in msg and "do not lie inside" in msg, msg
    assert N.gpuart_nearest_run(*args(shrunk)) == ERR_ARG and "not bound" in N.gpuart_nearest_last_error().decode()
    assert N.gpuart_nearest_finish(h) == 0 and untouched()
    # a descriptor that claims a deeper tree than any upload or rebuild accepts: a clear refusal, not an allocation of that size
    be.upload_bvh(s["tree"])
    deep = be.scene_device()
    deep.max_depth = B.NEAREST_MAX_DEPTH + 1
    assert N.gpuart_nearest_bind(h, C.byref(deep)) == ERR_ARG and "levels" in N.gpuart_nearest_last_error().decode()
    # a renderer without a scene refuses, and says where its reason is
    from gpuart_amd import synth_scenes as S
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    r = B.Renderer(32, 24, cam, device=0)
    try:
        with pytest.raises(B.HipError, match="stderr"):
            r.closest_points(points.cpu().numpy())
    finally:
        r.close()
    with pytest.raises(ValueError, match="GPU"):
        be.closest_points(points.cpu())
    # the honest tree binds again and answers
    be.upload_bvh(s["tree"])
    check(be, points.cpu().numpy(), "after the refusals")
