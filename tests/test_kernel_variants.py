"""Every product kernel specialisation held to the oracle, with the launch ledger of the test build as evidence of which one ran.

The device code is a few kernels compiled many times over: the host picks the instantiation from the tree's class (types present, exact
boxes), the visiting order, the execution mode, GPUART_HIP_LEAN_KERNELS and, for queries, the ray source. The library states that rule
once, `kernel_choice` in csrc/hip/gpuart_hip.hip, and one dispatcher there (`with_types`, with a list of the instantiations each kernel
has) turns its answer into the launch. A bug in one instantiation is invisible on every scene that does not select it. Each row of the
matrix below is a (scene, entry point, setting) triple; it compares the output with the oracle bit for bit, and asserts that the kernels
the ledger saw (Backend.launched, gpuart_hip_test_launches) are those `expected_kernels` — a restatement of the host's rule — names for
the row. The CPU tests check that the rows together name every kernel of the product's code object, so a new instantiation without a row
fails by name, and that the restatement and the library's rule (gpuart_hip_test_kernel_choice: no device) agree on every input.
"""
import os
import zlib

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests.test_product_library import PRODUCT_DIR, _code_object, _demangled, _kernel_metadata
from tests.test_ray_queries import assert_same_bits, hook_record, random_rays, rays8, tree_prims, words
from tests.util import assert_bits, golden, pad4

FLAT, ROUND, ALL, EXACT, REF = 0x6, 0x3, 0xF, 0x10, 0x20   # csrc/hip: GD_FLAT_TYPES, GD_ROUND_TYPES, GD_ALL_TYPES, GD_EXACT_BOXES, GD_REF_ORDER
RQ_RAYS, RQ_PIXELS = 0, 1
W, H = 40, 24
COUNTS = (1, 63, 64, 65, 3000)   # queries: one ray, around one wave, and a batch long enough for the thin-wave regroup
PASSES = 3
STAGE = 1 << 21                  # GD_QUERY_STAGE of gpuart_hip.hip: queries per staged chunk of the host-memory entry points

# Kernels no row reaches, each with the existing test that compares its output (test_every_exemption_names_an_existing_test checks it).
EXEMPT = {"k_scatter_rows": "tests.test_gather_inprocess::test_frames_gathered_from_n_contexts_equal_the_frame_of_one"}


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _disorderly():
    """Scene P with the root's lower child pushed outside its parent (test_uploader_classifies_trees_for_the_visiting_order)."""
    from oracle import oracle as O
    tree, _ = O.build_bvh(S.scene_p())
    tree = tree.copy()
    tree[3, 0] -= 100.0
    return tree


def _one_each():
    return [(S.SPHERE, [0.3, 0.2, 0.4, 0.3]), (S.DISC, [-0.5, 0.1, 0.2, 0.2, 0.3, 0.9, 0.4]),
            (S.TRIANGLE, [-0.6, -0.4, 0.1, 0.7, -0.3, 0.3, 0.1, 0.6, 0.9]), (S.CONE, [0.5, -0.5, 0.0, 0.6, -0.4, 0.7, 0.2, 0.05])]


def _descs(f):
    def build():
        from oracle import oracle as O
        return O.build_bvh(f())[0]
    return build


SCENES = {   # name -> compiled tree; the comment is the class the uploader gives it (type mask, or 31: exact boxes)
    "spheres": _descs(lambda: S.cluster_scene(n=2000)[:-1]),                          # 1 -> round (the cluster without its floor)
    "scene_p": _descs(S.scene_p),                                                     # 3 -> round
    "discs": _descs(lambda: S.scene_p(nspheres=0)),                                   # 2 -> flat
    "triangles": _descs(lambda: [d for d in S.scene_d(24, 24) if d[0] == S.TRIANGLE]),  # 4 -> flat
    "scene_d": _descs(lambda: S.scene_d(48, 48)),                                     # 6 -> flat
    "cones": _descs(lambda: S.scene_p(seed=3, nspheres=0, ndiscs=0, ncones=64)[1:]),  # 8 -> all
    "tree": _descs(lambda: S.tree_scene(depth=5)),                                    # 11 -> all
    "lattice": _descs(S.lattice_scene),                                               # 7 -> all
    "box": _descs(S.box_scene),                                                       # 15 -> all
    "one_each": _descs(_one_each),                                                    # 15 -> all
    "wild": lambda: golden("traverse_wild_wild_42874")["tree"],                       # irregular -> 31
    "disorderly": _disorderly,                                                        # disorderly -> 31
    "empty": _descs(lambda: []),                                                      # irregular box, mask 0 -> 31
}


def tree_of(name):
    return np.ascontiguousarray(SCENES[name](), np.float32)


# ---- the host's dispatch rules, restated ----------------------------------------------------------------------------------------
def leaf_types(cls, lean):
    """The type specialisation of the lean-capable kernels (k_direct_persistent, k_ray_query, and k_trace / k_run before the order bit)."""
    if cls["irregular"] or cls["disorderly"]:
        return ALL | EXACT
    mask = cls["type_mask"]
    if lean and mask & ~FLAT == 0:
        return FLAT
    if lean and mask & ~ROUND == 0:
        return ROUND
    return ALL


def expected_kernels(entry, cls, mode=0, lean=True, nearest=False, source=RQ_RAYS):
    """(alternatives, optional): the ledger of a row must equal one of the alternative kernel sets, plus any subset of `optional`."""
    exact = cls["irregular"] or cls["disorderly"]
    T = leaf_types(cls, lean)
    order = 0 if exact or nearest else REF   # every walk keeps the reference's order unless nearest-first is opted into
    if entry == "direct":
        return [{"k_direct<true>"} if mode == 1 else {"k_direct<false>"} if mode == 2 else {"k_direct_persistent<%d>" % T}], set()
    if entry == "query":
        return [{"k_ray_query<%d, %d>" % (T, source)}], set()
    assert entry == "pt"
    read = {"k_scale_copy"}   # every pt row reads its accumulator divided by the pass count too
    run = lambda c, r, t: {"k_run<%s, %s, %d>" % ("true" if c else "false", "true" if r else "false", t), "k_accumulate"} | read
    pipeline = {"k_gen", "k_trace<false, %d>" % (T | order), "k_shade<false>", "k_accumulate"} | read
    sorting = {"k_tile_order"}   # the birth-order sort behind a run of one pass (modes 0 and 5)
    if mode == 1:
        return [run(True, True, ALL | EXACT if exact else ALL)], set()
    if mode == 2:
        return [{"k_pt_mega<false>"} | read], set()
    if mode == 3:
        return [pipeline], set()
    if mode == 4:
        return [run(True, False, ALL | EXACT if exact else (FLAT if T == FLAT else ALL) | order)], set()
    persistent = run(False, False, T | order)
    if mode == 5:
        return [persistent], sorting
    return [persistent, pipeline], sorting   # mode 0: the planner picks the persistent kernel or the launch pipeline


def _clean_env(monkeypatch, env=None):
    for k in ("GPUART_HIP_NEAREST_MIN_PRIMS", "GPUART_HIP_LEAN_KERNELS", "GPUART_HIP_CHUNK", "GPUART_HIP_REFILL_LANES", "GPUART_HIP_LEAF_LANES",
              "GPUART_HIP_LEAF_SHARE", "GPUART_HIP_DIRECT_WAVES_PER_CU", "GPUART_HIP_TILE_ORDER"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


# ---- the matrix ---------------------------------------------------------------------------------------------------------------
KNOBS = [
    {"GPUART_HIP_CHUNK": "16", "GPUART_HIP_REFILL_LANES": "1", "GPUART_HIP_LEAF_LANES": "64"},
    {"GPUART_HIP_CHUNK": "4096", "GPUART_HIP_REFILL_LANES": "64", "GPUART_HIP_LEAF_LANES": "1"},
    {"GPUART_HIP_LEAF_SHARE": "1", "GPUART_HIP_DIRECT_WAVES_PER_CU": "1"},
    {"GPUART_HIP_LEAF_SHARE": "64", "GPUART_HIP_DIRECT_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "16"},
]
LEAN_SCENES = ("spheres", "scene_p", "discs", "triangles", "scene_d")   # every flat and round scene


def _rows():
    """(id, scene, entry, setting) of every row; setting: mode, lean, nearest, env."""
    rows = []
    for sc in SCENES:
        for m in (0, 1, 2):
            rows.append(("%s-direct-m%d" % (sc, m), sc, "direct", dict(mode=m)))
        for m in range(6):
            rows.append(("%s-pt-m%d" % (sc, m), sc, "pt", dict(mode=m)))
        for m in (0, 3, 4, 5):
            rows.append(("%s-pt-m%d-nearest" % (sc, m), sc, "pt", dict(mode=m, nearest=True)))
        rows.append(("%s-query" % sc, sc, "query", {}))
    for sc in LEAN_SCENES:
        rows.append(("%s-direct-m0-lean0" % sc, sc, "direct", dict(mode=0, lean=False)))
        for m in (3, 4, 5):
            rows.append(("%s-pt-m%d-lean0" % (sc, m), sc, "pt", dict(mode=m, lean=False)))
        rows.append(("%s-query-lean0" % sc, sc, "query", dict(lean=False)))
    for sc in ("scene_p", "tree"):   # one round and one all-types scene under the scheduling knobs
        for k, env in enumerate(KNOBS):
            rows.append(("%s-direct-m0-knobs%d" % (sc, k), sc, "direct", dict(mode=0, env=env)))
            rows.append(("%s-query-knobs%d" % (sc, k), sc, "query", dict(env=env)))
    return rows


ROWS = _rows()


def row_expectation(sc, entry, setting, cls):
    """Every kernel set a row must see: for a query row the union over its two sources (trace_rays and pick)."""
    kw = dict(mode=setting.get("mode", 0), lean=setting.get("lean", True), nearest=setting.get("nearest", False))
    if entry == "query":
        alts = [expected_kernels("query", cls, source=RQ_RAYS, **kw)[0][0] | expected_kernels("query", cls, source=RQ_PIXELS, **kw)[0][0]]
        return alts, set()
    return expected_kernels(entry, cls, **kw)


# ---- CPU: the matrix reaches every product kernel -----------------------------------------------------------------------------
def test_the_matrix_reaches_every_product_kernel(tmp_path):
    """The union of what the rows require (from their definitions and B.tree_class of their scenes: host code only) equals the product
    code object's kernel list, less the exemptions. With the ledger check of every GPU row, each product kernel ran in a row that matched
    the oracle; a new instantiation without a row fails here by name."""
    from gpuart_amd import binding as B
    classes = {sc: B.tree_class(tree_of(sc)) for sc in SCENES}
    required = set()
    for _, sc, entry, setting in ROWS:
        alts, _ = row_expectation(sc, entry, setting, classes[sc])
        required |= set.intersection(*alts)
    required |= {"k_tile_order"}   # test_pt_run_of_one_pass_sorts_the_birth_order requires it
    required |= {"k_ray_query<%d, %d>" % (leaf_types(classes["box"], True), RQ_RAYS)}   # test_host_staging_with_a_ragged_last_chunk
    co = _code_object(os.path.join(PRODUCT_DIR, "libgpuart_hip.so"), str(tmp_path))
    product = set(_demangled(sorted(_kernel_metadata(co))))
    assert len(product) >= 40, sorted(product)
    unknown = sorted(required - product)
    assert not unknown, "rows expect kernels the product does not have: %s" % unknown
    missing = sorted(product - required - set(EXEMPT))
    assert not missing, "product kernels no row of tests/test_kernel_variants.py runs: %s" % missing
    assert not set(EXEMPT) & required, "an exempt kernel is reached by a row: drop its exemption"
    print("%d product kernels, %d matched by rows, exempt: %s\n  %s" % (len(product), len(required), sorted(EXEMPT), "\n  ".join(sorted(required))))


def test_the_host_rule_and_its_restatement_agree(tmp_path):
    """The library's kernel choice (B.kernel_choice: gpuart_hip_test_kernel_choice, pure host code) against `leaf_types` / `expected_kernels`
    over every tree class (type mask 0-15 x regular / irregular / disorderly), visiting order, GPUART_HIP_LEAN_KERNELS, mode, launch site and
    query source: wherever the restatement names a kernel of the launch site's family, the rule names the same one, and every answer is a
    kernel of the product's code object. The quirks of the rule (mode 1: all types, never the order bit; mode 4: flat but no round variant;
    no order bit on the direct frame and the queries) fail here by name if either side is tidied alone."""
    from gpuart_amd import binding as B
    co = _code_object(os.path.join(PRODUCT_DIR, "libgpuart_hip.so"), str(tmp_path))
    product = set(_demangled(sorted(_kernel_metadata(co))))
    tf = lambda v: "true" if v else "false"
    checked = named = 0
    for mask in range(16):
        for kind in ("regular", "irregular", "disorderly"):
            cls = dict(irregular=kind == "irregular", disorderly=kind == "disorderly", type_mask=mask)
            for ref_order in (0, 1):
                for lean in (0, 1):
                    for mode in range(6):
                        kw = dict(mode=mode, lean=bool(lean), nearest=not ref_order)
                        for entry in B.KERNEL_ENTRIES:
                            T, count, refwork = B.kernel_choice(mask, int(kind != "regular"), ref_order, lean, mode, entry)
                            what = "%s, mask %d, ref_order %d, lean %d, mode %d, %s" % (kind, mask, ref_order, lean, mode, entry)
                            assert (count, refwork) == (entry == "run" and mode in (1, 4), entry == "run" and mode == 1), what
                            if entry == "direct":
                                got = ["k_direct_persistent<%d>" % T]
                                want = [set.union(*expected_kernels("direct", cls, **kw)[0])] if mode not in (1, 2) else [None]   # k_direct<.> there
                                assert T == leaf_types(cls, bool(lean)), what
                            elif entry == "query":
                                got = ["k_ray_query<%d, %d>" % (T, src) for src in (RQ_RAYS, RQ_PIXELS)]
                                want = [expected_kernels("query", cls, source=src, **kw)[0][0] for src in (RQ_RAYS, RQ_PIXELS)]
                            else:
                                got = ["k_run<%s, %s, %d>" % (tf(count), tf(refwork), T) if entry == "run" else "k_trace<false, %d>" % T]
                                family = got[0].split("<")[0] + "<"
                                alts = expected_kernels("pt", cls, **kw)[0]
                                want = [next((a for a in alts if any(k.startswith(family) for k in a)), None)]   # None: the mode never launches it
                            for g, w in zip(got, want):
                                assert g in product, "%s: the rule names %s, which the product does not have" % (what, g)
                                checked += 1
                                if w is not None:
                                    family = g.split("<")[0] + "<"
                                    assert {k for k in w if k.startswith(family)} == {g}, "%s: the rule names %s, the restatement %s" % (what, g, sorted(w))
                                    named += 1
    assert checked == 16 * 3 * 2 * 2 * 6 * 5 and named >= checked * 2 // 3, (checked, named)


def test_every_exemption_names_an_existing_test():
    import importlib
    for kernel, test_id in EXEMPT.items():
        mod, name = test_id.split("::")
        assert callable(getattr(importlib.import_module(mod), name, None)), "%s is exempt in favour of %s, which does not exist" % (kernel, test_id)


def test_dispatch_rules_name_the_issue_classes():
    """The restated rules on the classes that matter: sphere and disc scenes take the round kernels, the empty scene (mask 0, but an irregular
    box) the exact ones, mode 4 has no round variant, nearest-first drops the order bit except on exact trees."""
    c = lambda mask, irr=False, dis=False: dict(irregular=irr, disorderly=dis, type_mask=mask)
    assert [leaf_types(c(m), True) for m in (1, 2, 3, 4, 6, 7, 8, 11, 15)] == [3, 6, 3, 6, 6, 15, 15, 15, 15]
    assert leaf_types(c(0, irr=True), True) == 31 and leaf_types(c(3, dis=True), True) == 31 and leaf_types(c(3), False) == 15
    assert expected_kernels("pt", c(3), mode=4)[0] == [{"k_run<true, false, 47>", "k_accumulate", "k_scale_copy"}]
    assert expected_kernels("pt", c(3), mode=5, nearest=True)[0][0] >= {"k_run<false, false, 3>"}
    assert expected_kernels("pt", c(3, dis=True), mode=5, nearest=True)[0][0] >= {"k_run<false, false, 31>"}
    assert expected_kernels("query", c(3), source=RQ_PIXELS)[0] == [{"k_ray_query<3, 1>"}]


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


def scene_setup(O, tree, W=W, H=H):
    """Camera looking at the tree's root box from the front, a user sphere beside its centre, the reference's sun; (cam, params, lo, hi, us)."""
    lo, hi = tree[0, :3].astype(np.float64), tree[1, :3].astype(np.float64)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()):
        lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    pos = centre + ext * np.array([0.15, -1.3, 0.55])
    c = O.camera(pos.tolist(), (centre - pos).tolist(), (0.0, 0.0, 1.0), 60.0, 0.2, W, H)
    us = tuple(float(v) for v in (centre + ext * np.array([0.1, -0.2, 0.05]))) + (0.12 * ext,)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, us, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    return c, P, lo, hi, us


def to_params(B, op):
    import ctypes as C
    p = B.Params()
    C.memmove(C.byref(p), C.byref(op), C.sizeof(p))
    return p


def names_of(launched):
    return set(_demangled(sorted(launched)))


def check_ledger(got, alts, optional, what):
    """The kernels a row launched are one alternative of its expectation, plus optional ones only."""
    for want in alts:
        if want <= got and not (got - want - optional):
            return
    raise AssertionError("%s: launched %s, expected one of %s (optional %s)" % (what, sorted(got), [sorted(a) for a in alts], sorted(optional)))


def tmax_set(rng, pos):
    """Test 4's tmax set around the oracle's closest-hit pos: 0, NaN, +inf, negative, = pos, nextafter up and down, random."""
    n = len(pos)
    pick = rng.integers(0, 8, n)
    t = np.where(pick == 0, 0.0, np.where(pick == 1, np.nan, np.where(pick == 2, np.inf, np.where(pick == 3, -1.0, np.where(pick == 4, pos,
        rng.uniform(0, 50, n)))))).astype(np.float32)
    up, down = (pick == 5) & (pos > 0), (pick == 6) & (pos > 0)
    t[up] = np.nextafter(pos[up], np.float32(np.inf))
    t[down] = np.nextafter(pos[down], np.float32(0))
    return t


def oracle_records(O, tree, rays, us):
    """The oracle's closest hits of rays (n, 8) as the words of gpuart_ray_hit, and which of them are the user sphere's."""
    o0, o1 = O.traverse(tree, pad4(rays[:, 0:3]), pad4(rays[:, 4:7]), us)
    return hook_record(o0, o1)


def prim_hits(O, tree, rays):
    """(n rays, primitives) parameters of every ray against every primitive of the tree, each intersected alone by the oracle (-1: none)."""
    plist = [p for p in tree_prims(tree) if p[0] >= 0]
    out = np.full((len(rays), len(plist)), -1.0, np.float32)
    types = np.array([t for t, _ in plist])
    for t in np.unique(types):
        cols = np.nonzero(types == t)[0]
        q = np.tile(np.stack([plist[k][1] for k in cols]).reshape(-1, 4, 4), (len(rays), 1, 1))
        rs, rd = np.repeat(pad4(rays[:, 0:3]), len(cols), 0), np.repeat(pad4(rays[:, 4:7]), len(cols), 0)
        o0, _ = (O.sphere(rs, rd, q[:, 0]) if t == S.SPHERE else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == S.DISC else
                 O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == S.TRIANGLE else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
        out[:, cols] = o0[:, 0].reshape(len(rays), len(cols))
    return out


def through_the_box(rng, n, lo, hi):
    """Rays (n, 8) from outside the box [lo, hi] towards random points inside it (tmax +inf): most cross several primitives."""
    centre, ext = (lo + hi) / 2, max(float((hi - lo).max()), 1e-3)
    u = rng.normal(size=(n, 3))
    rs = centre + 1.5 * ext * u / np.linalg.norm(u, axis=1, keepdims=True)
    rd = lo + rng.uniform(0, 1, (n, 3)) * (hi - lo) - rs
    return rays8(rs.astype(np.float32), (rd / np.linalg.norm(rd, axis=1, keepdims=True)).astype(np.float32))


def behind_the_closest(O, tree, rays, closest):
    """tmax = the parameter of a hit BEHIND the closest one (the next one, or the farthest), where a ray has one: an occlusion walk that
    meets that primitive first must not stop there as if the ray were unoccluded (the early-out is strict: parameter < tmax)."""
    tmax = rays[:, 3].copy()
    hits = prim_hits(O, tree, rays)
    for i in range(len(rays)):
        behind = np.unique(hits[i][hits[i] > closest[i]]) if closest[i] > 0 else []
        if len(behind):
            tmax[i] = behind[0] if i % 2 == 0 else behind[-1]
    return tmax


def check_ordinals(O, tree, rays, hits, prims, what):
    """Every ordinal names, through the tree's leaf order (tree_prims), the primitive whose oracle intersection gives the hit's pos, p and n."""
    plist = tree_prims(tree)
    idx = np.nonzero(prims >= 0)[0]
    types = np.array([plist[k][0] for k in prims[idx]], np.int64)
    assert (types == hits["type"][idx]).all(), what
    w = words(hits)
    for t in np.unique(types):
        sel = idx[types == t]
        q = np.stack([plist[k][1] for k in prims[sel]]).reshape(-1, 4, 4)
        rs, rd = pad4(rays[sel, 0:3]), pad4(rays[sel, 4:7])
        o0, o1 = (O.sphere(rs, rd, q[:, 0]) if t == S.SPHERE else O.disc(rs, rd, q[:, 0], q[:, 1]) if t == S.DISC else
                  O.triangle(rs, rd, q[:, 0], q[:, 1], q[:, 2]) if t == S.TRIANGLE else O.cone(rs, rd, q[:, 0], q[:, 1], q[:, 2], q[:, 3]))
        assert_same_bits(w[sel, :7], np.concatenate([o0, o1[:, :3]], 1), "%s, ordinals of type %d" % (what, t))


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_variant_row(B, O, row, monkeypatch, record_property):
    rid, sc, entry, setting = row
    mode, lean, nearest = setting.get("mode", 0), setting.get("lean", True), setting.get("nearest", False)
    env = dict(setting.get("env", {}))
    if not lean:
        env["GPUART_HIP_LEAN_KERNELS"] = "0"
    _clean_env(monkeypatch, env)
    tree = tree_of(sc)
    cls = B.tree_class(tree)
    alts, optional = row_expectation(sc, entry, setting, cls)
    info = "%s: class %s, entry %s, setting %s, expects %s" % (rid, cls, entry, setting, [sorted(a) for a in alts])
    print(info)
    record_property("row", info)
    c, P, lo, hi, us = scene_setup(O, tree)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(c)
        if nearest:
            b.set_nearest_first(0)
        b.set_mode(mode)
        assert b.launched() == set(), "setting up a context launched a kernel"
        if entry == "direct":
            b.render_direct(to_params(B, P))
            got = b.read(0)
            exp, _ = O.render_direct(tree, c, W, H, P)
            assert_bits(got[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), rid)
        elif entry == "pt":
            seeds = O.randseeds(2 * PASSES)
            for npaths in (1, 2):
                b.pt_reset()
                acc = np.zeros((H, W, 4), np.float32)
                for k in range(PASSES):
                    sd = seeds[(npaths - 1) * PASSES + k]
                    b.pt_pass(to_params(B, P), sd, npaths)
                    O.pt_pass(tree, c, W, H, P, sd, npaths, acc)
                assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "%s, %d paths" % (rid, npaths))
                scaled = b.read(1, divide_by=PASSES)
                assert_bits(scaled[..., :3].reshape(-1, 3), (acc[..., :3] / np.float32(PASSES)).reshape(-1, 3), "%s, %d paths, divided" % (rid, npaths))
        else:
            query_row(B, O, b, tree, c, lo, hi, us, rid)
        got = names_of(b.launched())
        record_property("kernels", sorted(got))
        print("  launched %s" % sorted(got))
        check_ledger(got, alts, optional, info)
        assert b.launched() == set(), "the ledger was not reset"
    finally:
        b.close()


def query_row(B, O, b, tree, c, lo, hi, us, rid):
    """trace_rays (closest hit and occlusion, with and without the user sphere, host memory and a torch tensor) and pick, at every count."""
    import torch
    rng = np.random.default_rng(zlib.crc32(rid.encode()))
    rs, rd = random_rays(rng, COUNTS[-1], lo, hi)
    for sphere in (us, None):
        rays = rays8(rs, rd)
        exp, ush = oracle_records(O, tree, rays, sphere)
        rays[:, 3] = tmax_set(rng, exp[:, 0].copy())
        for n in COUNTS:
            what = "%s, n = %d, user sphere %s" % (rid, n, sphere)
            hits, prims = b.trace_rays(rays[:n], user_sphere=sphere, want_prims=True)
            assert_same_bits(words(hits), exp[:n], "closest hit, " + what)
            is_us = prims == -2
            assert (is_us == ush[:n]).all(), "user-sphere ordinals, " + what
            assert ((prims == -1) == (hits["type"] == -1)).all(), what
            check_ordinals(O, tree, rays[:n][~is_us], hits[~is_us], prims[~is_us], what)
            occ, oprims = b.trace_rays(rays[:n], occlusion=True, user_sphere=sphere, want_prims=True)
            pos, tmax = exp[:n, 0], rays[:n, 3]
            want = (pos > 0) & (pos < tmax)
            got = occ["pos"] > 0
            assert (got == want).all(), "occlusion, %s: %d of %d answers differ from the oracle's closest hit" % (what, int((got != want).sum()), n)
            assert (occ["pos"][got] < tmax[got]).all() and (occ["p"] == 0).all() and (occ["n"] == 0).all(), what
            assert (((oprims >= 0) | (oprims == -2)) == got).all() and (occ["type"][~got] == -1).all(), what
            if n == COUNTS[-1]:   # tmax at the parameter of a primitive hit behind the closest one, on rays aimed into the tree's box
                far = through_the_box(rng, 1024, lo, hi)
                fexp, _ = oracle_records(O, tree, far, sphere)
                far[:, 3] = behind_the_closest(O, tree, far, fexp[:, 0])
                got = b.trace_rays(far, occlusion=True, user_sphere=sphere)["pos"] > 0
                want = (fexp[:, 0] > 0) & (fexp[:, 0] < far[:, 3])
                assert (got == want).all(), "occlusion, tmax behind the closest hit, %s: %d answers differ" % (what, int((got != want).sum()))
            if n in (65, COUNTS[-1]):   # the device path: the same bits from a torch tensor
                t = torch.from_numpy(np.ascontiguousarray(rays[:n])).to("cuda:0")
                for occl, ref in ((False, hits), (True, occ)):
                    dev = b.trace_rays(t, occlusion=occl, user_sphere=sphere)
                    assert_same_bits(dev.cpu().numpy(), words(ref), "device path, occlusion %s, %s" % (occl, what))
    # pick: the oracle's camera rays of the frame's pixels, all of them and a seeded sample at the counts
    crs, crd = O.cam_rays(c, W, H)
    crays = rays8(crs.reshape(-1, 4)[:, :3], crd.reshape(-1, 4)[:, :3])
    y, x = np.divmod(np.arange(W * H), W)
    xy = np.stack([x, y], 1)
    for sphere in (us, None):
        exp, _ = oracle_records(O, tree, crays, sphere)
        assert_same_bits(words(b.pick(xy, user_sphere=sphere)), exp, "pick, %s, user sphere %s" % (rid, sphere))
        for n in COUNTS[:-1]:
            sel = rng.choice(W * H, n, replace=False)
            assert_same_bits(words(b.pick(xy[sel], user_sphere=sphere)), exp[sel], "pick, %s, n = %d" % (rid, n))


@pytest.mark.gpu
def test_pt_run_of_one_pass_sorts_the_birth_order(B, O, monkeypatch, record_property):
    """Passes observed one by one in mode 5 (the reference's interactive loop): every run holds one pass, the first counts the blocks' cost
    and k_tile_order sorts them; the later passes are born in that order. The accumulator equals the oracle's after every pass."""
    _clean_env(monkeypatch)
    tree = tree_of("scene_p")
    cls = B.tree_class(tree)
    c, P, _, _, _ = scene_setup(O, tree)
    b = B.Backend(0)
    try:
        b.resize(W, H); b.upload_bvh(tree); b.set_camera(c)
        b.set_mode(5)
        b.pt_reset()
        acc = np.zeros((H, W, 4), np.float32)
        for k, sd in enumerate(O.randseeds(4)):
            b.pt_pass(to_params(B, P), sd, 1)
            O.pt_pass(tree, c, W, H, P, sd, 1, acc)
            assert_bits(b.read(1)[..., :3].reshape(-1, 3), acc[..., :3].reshape(-1, 3), "pass %d" % k)
        got = names_of(b.launched())
        record_property("kernels", sorted(got))
        want = expected_kernels("pt", cls, mode=5)[0][0] - {"k_scale_copy"} | {"k_tile_order"}
        assert got == want, (sorted(got), sorted(want))
    finally:
        b.close()


@pytest.mark.gpu
def test_host_staging_with_a_ragged_last_chunk(B, O, monkeypatch, record_property):
    """gpuart_hip_trace_rays_host stages 2^21 queries at a time: 2^21 + 3 rays end in a chunk of 3. The host path equals the device path
    bit for bit (records and ordinals, both modes), and the oracle on a seeded sample of 65 536 rays that includes the whole last chunk."""
    import torch
    _clean_env(monkeypatch)
    tree = tree_of("box")
    cls = B.tree_class(tree)
    _, _, lo, hi, us = scene_setup(O, tree)
    n = STAGE + 3
    rng = np.random.default_rng(21)
    rs, rd = random_rays(rng, n, lo, hi)
    rays = rays8(rs, rd, rng.uniform(0, 8, n).astype(np.float32))
    b = B.Backend(0)
    try:
        b.upload_bvh(tree)
        t = torch.from_numpy(rays).to("cuda:0")
        for occl in (False, True):
            hits, prims = b.trace_rays(rays, occlusion=occl, user_sphere=us, want_prims=True)
            dh, dp = b.trace_rays(t, occlusion=occl, user_sphere=us, want_prims=True)
            assert_same_bits(words(hits), dh.cpu().numpy(), "host vs device path, occlusion %s" % occl)
            assert (prims == dp.cpu().numpy()).all()
            sub = np.unique(np.concatenate([rng.choice(n, 65536, replace=False), np.arange(STAGE - 5, n)]))
            exp, _ = oracle_records(O, tree, rays[sub], us)
            if not occl:
                assert_same_bits(words(hits)[sub], exp, "host path vs oracle")
            else:
                want = (exp[:, 0] > 0) & (exp[:, 0] < rays[sub, 3])
                assert ((hits["pos"][sub] > 0) == want).all(), "occlusion vs oracle"
        got = names_of(b.launched())
        record_property("kernels", sorted(got))
        assert got == expected_kernels("query", cls, source=RQ_RAYS)[0][0], sorted(got)
    finally:
        b.close()


CURSOR_W, CURSOR_H = 160, 120   # 19 200 pixel slots: beyond three static chunks of 16 per wave at one wave per CU


@pytest.mark.gpu
@pytest.mark.parametrize("sc", ["scene_p", "box", "wild"])   # round, all types, exact boxes (no thin path: the cursor is still there)
def test_waves_take_chunks_from_the_shared_cursor(B, O, sc, monkeypatch, record_property):
    """The chunk cursor the direct frame and the ray queries share (kernels_pipeline.h ChunkCursor), behind its static part: the matrix
    above never gets there — with the default grid of 16 waves per CU every wave's static first chunk covers its 40x24 frames and 3000
    queries. Here the knobs are at their minima (one wave per CU, chunks of 16), so the static part is CUs x 16 entries and a 160x120
    frame, 19 200 + 37 rays and a pick of every pixel take most of their chunks through the atomic cursor. Each against the oracle, bit
    for bit, and the ledger names the instantiations `expected_kernels` names."""
    import torch
    _clean_env(monkeypatch, {"GPUART_HIP_DIRECT_WAVES_PER_CU": "1", "GPUART_HIP_CHUNK": "16"})
    n_rays = CURSOR_W * CURSOR_H + 37
    static = torch.cuda.get_device_properties(0).multi_processor_count * 16
    assert min(n_rays, CURSOR_W * CURSOR_H) >= 3 * static, "%d entries do not reach past the static chunks (%d) of this device" % (CURSOR_W * CURSOR_H, static)
    tree = tree_of(sc)
    cls = B.tree_class(tree)
    c, P, lo, hi, us = scene_setup(O, tree, CURSOR_W, CURSOR_H)
    rng = np.random.default_rng(zlib.crc32(sc.encode()))
    b = B.Backend(0)
    try:
        b.resize(CURSOR_W, CURSOR_H); b.upload_bvh(tree); b.set_camera(c)
        b.render_direct(to_params(B, P))
        exp, _ = O.render_direct(tree, c, CURSOR_W, CURSOR_H, P)
        assert_bits(b.read(0)[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "direct frame, " + sc)
        rs, rd = random_rays(rng, n_rays, lo, hi)
        rays = rays8(rs, rd)
        exp, ush = oracle_records(O, tree, rays, us)
        rays[:, 3] = tmax_set(rng, exp[:, 0].copy())
        hits, prims = b.trace_rays(rays, user_sphere=us, want_prims=True)
        assert_same_bits(words(hits), exp, "closest hit, " + sc)
        assert ((prims == -2) == ush).all() and ((prims == -1) == (hits["type"] == -1)).all(), sc
        occ = b.trace_rays(rays, occlusion=True, user_sphere=us)
        want = (exp[:, 0] > 0) & (exp[:, 0] < rays[:, 3])
        got = occ["pos"] > 0
        assert (got == want).all(), "occlusion, %s: %d of %d answers differ from the oracle's closest hit" % (sc, int((got != want).sum()), n_rays)
        assert (occ["pos"][got] < rays[got, 3]).all() and (occ["type"][~got] == -1).all(), sc
        crs, crd = O.cam_rays(c, CURSOR_W, CURSOR_H)
        crays = rays8(crs.reshape(-1, 4)[:, :3], crd.reshape(-1, 4)[:, :3])
        y, x = np.divmod(np.arange(CURSOR_W * CURSOR_H), CURSOR_W)
        pexp, _ = oracle_records(O, tree, crays, us)
        assert_same_bits(words(b.pick(np.stack([x, y], 1), user_sphere=us)), pexp, "pick, " + sc)
        got = names_of(b.launched())
        record_property("kernels", sorted(got))
        want = set.union(*[expected_kernels(e, cls, source=src)[0][0] for e, src in (("direct", 0), ("query", RQ_RAYS), ("query", RQ_PIXELS))])
        assert got == want, (sorted(got), sorted(want))
    finally:
        b.close()
