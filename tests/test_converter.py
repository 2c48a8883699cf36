"""The tree uploader (csrc/hip/converter.h, behind gpuart_hip_upload_bvh) held to a restatement, record by record.

gpuart_hip_test_convert runs the upload's own Converter::convert without a device and copies the two device arrays out;
tests/converter_ref.py restates the conversion from the two formats. Every comparison is byte equality. All but the last test run on the
CPU; tools/sanitize_converter.sh runs the same corpus under AddressSanitizer / UBSan / ThreadSanitizer in a stand-alone program.
"""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from gpuart_amd import binding as B
from gpuart_amd import synth_scenes as S
from tests import converter_cases as K
from tests import converter_ref as R
from tests.util import GOLDEN, assert_bits, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ("irregular", "disorderly", "subnormal")
ARRAYS = ("recs", "prims", "root_min", "root_max")
SCALARS = ("root_ref", "num_nodes", "max_depth", "type_mask")


def hook(tree, nquads=None, threads=1, top_depth=0):
    """The hook's outputs, or the uploader's reason for rejecting the tree (a str)."""
    try:
        return B.convert_tree(tree, nquads, threads, top_depth)
    except B.HipError as e:
        m = re.search(r"malformed compiled BVH: (.*)$", str(e))
        assert m, str(e)
        return m.group(1)


def ref(tree, nquads=None, top_depth=0):
    try:
        return R.convert(tree, nquads, top_depth)
    except R.Rejected as e:
        return str(e)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, exp, what, flags=True):
    """Two conversions are equal to the byte (flags: the three classifications too)."""
    assert not isinstance(got, str) and not isinstance(exp, str), (what, got if isinstance(got, str) else "accepted", exp if isinstance(exp, str) else "accepted")
    for k in SCALARS + (FLAGS if flags else ()):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ARRAYS:
        a, b = bits(got[k]), bits(exp[k])
        assert a.shape == b.shape, (what, k, a.shape, b.shape)
        bad = np.flatnonzero((a != b).reshape(len(a), a[0].size if len(a) else 1).any(1))
        assert not len(bad), "%s: %s differs in %d of %d records, first %d: %s against %s" % (what, k, len(bad), len(a), bad[0], got[k][bad[0]], exp[k][bad[0]])


def check(tree, what, **kw):
    """Hook == restatement for an accepted tree; returns the restatement."""
    h, r = hook(tree, **kw), ref(tree, kw.get("nquads"), kw.get("top_depth", 0))
    assert_same(h, r, what)
    return r


def ref_kinds(r):
    """The (TRIS, SMALL, TWO) combinations among a conversion's leaf refs."""
    leaf = r["refs"][(r["refs"] & np.uint32(R.REF_LEAF)) != 0]
    return {(bool(x & R.REF_TRIS), bool(x & R.REF_SMALL), bool(x & R.REF_TWO)) for x in leaf.tolist()}


# ---- a. honest trees, record for record ------------------------------------------------------------------------------------------
def honest_trees():
    for name in ("box", "scene_d", "scene_p", "scene_pc", "tree", "cluster", "lattice"):
        yield name, B.compile_bvh(scene(name))[0]
    for seed in range(200):
        yield "random_case %d" % seed, B.compile_bvh(S.random_case(seed)["prims"])[0]
        yield "random_lattice_case %d" % seed, B.compile_bvh(S.random_lattice_case(seed)["prims"])[0]
    yield "the empty scene", B.compile_bvh([])[0]
    yield "a root that is a leaf", K.piece(K.SPH, K.CON)
    for n in (0, 1, 2, 3, 5):
        tris = [K.TRI, K.TRI2, K.TRI3, K.TRI, K.TRI2][:n]
        mixed = [K.TRI, K.SPH, K.DSC, K.CON, K.TRI2][:n]
        other = [K.CON, K.DSC, K.SPH, K.SPH2, K.TRI][:n]
        yield "leaves of %d" % n, K.assemble(((K.piece(*tris), K.piece(*mixed)), (K.piece(*other), K.piece(K.SPH))))
    yield "a chain of 1024 levels", K.chain(1024)
    for name, t in zip(("root leaf", "two leaves", "mixed"), K.small_trees()):
        yield "small tree: " + name, t
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))):
        g = np.load(path)
        for key in g.files:
            if re.fullmatch(r"tree\d*", key):
                yield "%s:%s" % (os.path.basename(path), key), g[key]


def test_honest_trees_convert_as_the_formats_say():
    """Every scene the suite renders, 400 random cases, the empty scene, leaves of 0, 1, 2, 3 and 5 primitives (all triangles and mixed), the
    deepest chain the uploader takes, and every tree stored under tests/golden/ (hostile and adversary ones): arrays, root, counts and flags
    equal the restatement's. The inputs cover every ref kind and every primitive type (a condition on the inputs, read from the restatement)."""
    kinds, types, n, stored = set(), 0, 0, 0
    for what, tree in honest_trees():
        r = check(tree, what)
        kinds |= ref_kinds(r)
        types |= r["type_mask"]
        n += 1
        stored += ".npz:" in what
    assert n >= 420 and stored >= 25, (n, stored)
    assert types == 15
    #                 one triangle          two triangles        one, not a triangle   two, not all triangles  none or more than two
    assert kinds == {(True, False, False), (True, False, True), (False, True, False), (False, True, True), (False, False, False)}, kinds
    assert check(K.chain(1024), "chain")["max_depth"] == 1024


# ---- b. every rejection --------------------------------------------------------------------------------------------------------------
def test_every_rejection_is_reached_and_writes_nothing():
    """One minimal mutation per message of scan(): the hook returns that message, the restatement agrees, and no output is touched. The table
    reaches every `err = "..."` of converter.h but the two capacity limits, which need tens of millions of entries."""
    table = K.rejections()
    L = B.hip_lib()
    base = hook(K.small_trees()[1])
    for name, (tree, nq, message) in table.items():
        assert ref(tree, nq) == message, (name, ref(tree, nq))
        assert hook(tree, nq) == message, (name, hook(tree, nq))
        for threads, top in ((8, 0), (1, 4)):
            assert hook(tree, nq, threads, top) == message, name
        q = np.ascontiguousarray(tree, np.float32)
        recs, prims = np.full((len(tree), 4, 4), 7.0, np.float32), np.full((len(tree), 3, 4), 7.0, np.float32)
        info, box = (C.c_uint32 * 8)(*[77] * 8), (C.c_float * 6)(*[7.0] * 6)
        rc = L.gpuart_hip_test_convert(q.ctypes.data_as(C.c_void_p), C.c_size_t(len(q) if nq is None else nq), C.c_uint32(1), C.c_uint32(0),
                                       recs.ctypes.data_as(C.c_void_p), C.c_size_t(len(recs)), prims.ctypes.data_as(C.c_void_p), C.c_size_t(len(prims)), info, box)
        assert rc != 0 and (recs == 7.0).all() and (prims == 7.0).all() and list(info) == [77] * 8 and list(box) == [7.0] * 6, name
    assert_same(hook(K.small_trees()[1]), base, "the tree the table edits, afterwards")
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "hip", "converter.h")).read()
    declared = set(re.findall(r'err\s*=\s*"([^"]+)"', src))
    assert len(declared) == 10 and K.NOT_REACHED <= declared, declared
    assert {m for _, _, m in table.values()} == declared - K.NOT_REACHED


# ---- c. mutants stay inside the arrays -------------------------------------------------------------------------------------------
def device_safe(h, what):
    """What the kernels rely on when they index recs[4 * ref] and prims[3 * first ...] (device_scene.h: leaf_tests reads the count from the first
    primitive's T >> 2)."""
    n_recs, n_prims = len(h["recs"]), len(h["prims"])
    ru, pu = bits(h["recs"]), bits(h["prims"])
    refs = np.concatenate([[np.uint32(h["root_ref"])], ru[:, 0, 3], ru[:, 1, 3]]).astype(np.uint32)
    leaf = (refs & np.uint32(R.REF_LEAF)) != 0
    assert (refs[~leaf] < n_recs).all(), what
    T = pu[:, 0, 3]
    covered = np.zeros(n_prims, np.int64)
    for x in refs[leaf].tolist():
        first = x & R.REF_INDEX
        assert first < n_prims, what
        count = int(T[first]) >> 2
        assert first + max(count, 1) <= n_prims, (what, first, count, n_prims)
        covered[first:first + max(count, 1)] += 1
        types = [int(T[first + k]) & 3 for k in range(count)]
        assert all(int(T[first + k]) <= 3 for k in range(1, count)), what   # a bare type: only the first primitive carries the count
        tris, small, two = bool(x & R.REF_TRIS), bool(x & R.REF_SMALL), bool(x & R.REF_TWO)
        assert two == (count == 2), (what, hex(x), count)
        assert tris == (count in (1, 2) and all(t == 2 for t in types)), (what, hex(x), types)
        assert small == (count in (1, 2) and not all(t == 2 for t in types)), (what, hex(x), types)
    assert (covered == 1).all(), what   # every primitive record belongs to exactly one leaf


def test_mutants_are_rejected_or_stay_inside_the_arrays():
    """20 000 seeded one- and two-word mutants of three small trees (one in eight also cut short): hook and restatement agree on accept /
    reject and on the message; an accepted mutant converts to the restatement's bytes, and every ref and leaf count stays inside the arrays.
    Flags: `irregular` and `subnormal` equal the restatement's; `disorderly` equals it on trees without cones, and is implied by it otherwise (the
    uploader also holds a cone's derived constants to its centres, which the restatement leaves out)."""
    verdicts = {}
    accepted = 0
    for i, (tree, nq) in enumerate(K.mutants()):
        what = "mutant %d" % i
        r = ref(tree, nq)
        h = hook(tree, nq)
        if isinstance(r, str):
            verdicts[r] = verdicts.get(r, 0) + 1
            assert h == r, (what, h, r)
            continue
        accepted += 1
        assert_same(h, r, what, flags=False)
        assert h["irregular"] == r["irregular"] and h["subnormal"] == r["subnormal"], what
        assert h["disorderly"] == r["disorderly"] if not r["type_mask"] & 8 else h["disorderly"] >= r["disorderly"], what
        device_safe(h, what)
    # the condition on the mutant set, from the restatement alone
    n = K.N_MUTANTS
    assert accepted >= n // 10 and n - accepted >= n // 10, (accepted, verdicts)
    expected = {m for _, _, m in K.rejections().values()} - {"tree deeper than 1024 levels"}
    assert set(verdicts) == expected, verdicts


# ---- d. thread counts ----------------------------------------------------------------------------------------------------------------
THREADS = (1, 2, 3, 8, 64)


def planted(tree, lay, node, defect):
    """The big tree with one defect in the box of one node (a lower child other than the root: its parent is the entry before it)."""
    t = tree.copy()
    a = int(lay["addr"][node])
    if defect == "inverted box":
        t[a, 0], t[a + 1, 0] = tree[a + 1, 0], tree[a, 0]
        assert t[a, 0] > t[a + 1, 0]
    elif defect == "infinite bound":
        t[a + 1, 1] = np.inf
    elif defect == "child outside its parent":
        t[a, 2] = tree[int(lay["addr"][lay["parent"][node]]), 2] - np.float32(0.25)
    elif defect == "plane of 2^-70":   # (on the side that keeps the box ordered)
        if tree[a + 1, 0] > 0:
            t[a, 0] = np.float32(2.0 ** -70)
        else:
            t[a + 1, 0] = np.float32(-2.0 ** -70)
    return t


def test_every_thread_count_fills_the_same_arrays_and_raises_the_same_flags():
    """A tree whose node table has at least 8 x 16384 entries (the fill pass takes min(threads, entries / 16384) parts): 1, 2, 3, 8 and 64
    threads give identical bytes, equal to the restatement's. Then one defect in one node, once in the first eighth of the table and once in
    the last (node and parent both: the parent's part is the one that sees a child's box): the flags are the restatement's at every thread
    count — the matching flag always, and with it only what the same edit implies (an edited box no longer nests: disorderly)."""
    tree = K.big_tree()
    r = ref(tree)
    n = r["num_nodes"]
    assert n >= 8 * 16384 and r["type_mask"] == 15 and not any(r[k] for k in FLAGS), (n, r["type_mask"])
    for threads in THREADS:
        assert_same(hook(tree, threads=threads), r, "%d threads" % threads)
    lay = R.layout(tree)
    lower = np.flatnonzero(lay["parent"] == np.arange(n) - 1)
    first, last = int(lower[lower >= n // 16][0]), int(lower[lower >= n - n // 16][0])
    assert 0 < first < n // 8 and n - n // 8 < last - 1 < n
    matching = {"inverted box": "irregular", "infinite bound": "irregular", "child outside its parent": "disorderly", "plane of 2^-70": "subnormal"}
    never = {"inverted box": ("subnormal",), "infinite bound": ("subnormal",), "child outside its parent": ("irregular", "subnormal"),
             "plane of 2^-70": ("irregular",)}
    for defect, flag in matching.items():
        for node in (first, last):
            t = planted(tree, lay, node, defect)
            rr = ref(t)
            assert rr[flag] and not any(rr[k] for k in never[defect]), (defect, node, [rr[k] for k in FLAGS])
            for threads in THREADS:
                assert_same(hook(t, threads=threads), rr, "%s in node %d, %d threads" % (defect, node, threads))


# ---- e. top_depth ------------------------------------------------------------------------------------------------------------------------
def record_depths(h):
    """The level of every record's node, walked from the root through the arrays themselves."""
    ru = bits(h["recs"])
    depth = np.full(len(ru), -1, np.int64)
    todo = [(h["root_ref"], 0)]
    while todo:
        x, d = todo.pop()
        if not x & R.REF_LEAF:
            depth[x] = d
            todo += [(int(ru[x, 0, 3]), d + 1), (int(ru[x, 1, 3]), d + 1)]
    assert (depth >= 0).all()
    return depth


def test_top_depth_marks_the_records_above_that_level_and_nothing_else():
    tree = B.compile_bvh(scene("scene_pc"))[0]
    plain = hook(tree)
    depth = record_depths(plain)
    assert plain["max_depth"] > 5 and (bits(plain["recs"])[:, 2, 3] == 0).all()
    for top in (0, 1, 4, plain["max_depth"] + 1, 1 << 20):
        h = hook(tree, top_depth=top)
        assert_same(h, ref(tree, top_depth=top), "top_depth %d" % top)
        assert (bits(h["recs"])[:, 2, 3] == (depth < top)).all(), top
        assert 0 < (depth < top).sum() < len(depth) or top in (0, plain["max_depth"] + 1, 1 << 20)
        unmarked = bits(h["recs"]).copy()
        unmarked[:, 2, 3] = 0
        assert (unmarked == bits(plain["recs"])).all() and (bits(h["prims"]) == bits(plain["prims"])).all(), top
        assert all(h[k] == plain[k] for k in SCALARS + FLAGS), top


# ---- f. boundary values of the classification ---------------------------------------------------------------------------------
def point_sphere(x, y=0.5):
    """A root leaf of one sphere of radius 0 at (x, y, 0.5): its box is that point (min == max)."""
    t = K.piece((S.SPHERE, [1.0, 0.5, 0.5, 0.0])).copy()
    for quad in (0, 1, 4):
        t[quad, 0], t[quad, 1] = x, y
    return t


def flags_of(tree, what):
    r = check(tree, what)
    return tuple(r[k] for k in FLAGS)


def test_classification_at_its_boundary_values():
    f32, up, down = np.float32, lambda v: np.nextafter(np.float32(v), np.float32(np.inf)), lambda v: np.nextafter(np.float32(v), np.float32(0))
    clean = (False, False, False)
    assert flags_of(point_sphere(f32(0.25)), "a box with min == max") == clean
    # coordinates: 2^20 is in, the next float is out
    assert flags_of(point_sphere(f32(1048576.0)), "2^20") == clean
    assert flags_of(point_sphere(up(1048576.0)), "above 2^20") == (False, True, False)
    assert flags_of(point_sphere(f32(-1048576.0)), "-2^20") == clean
    assert flags_of(point_sphere(-up(1048576.0)), "below -2^20") == (False, True, False)
    # planes: zero or at least 2^-60
    tiny = f32(2.0 ** -60)
    assert flags_of(point_sphere(tiny), "2^-60") == clean
    assert flags_of(point_sphere(down(tiny)), "below 2^-60") == (False, False, True)
    assert flags_of(point_sphere(-tiny), "-2^-60") == clean
    assert flags_of(point_sphere(-down(tiny)), "above -2^-60") == (False, False, True)
    assert flags_of(point_sphere(f32(1e-45)), "the smallest subnormal") == (False, False, True)
    assert flags_of(point_sphere(f32(0.0)), "0") == clean
    assert flags_of(point_sphere(f32(-0.0)), "-0") == clean
    # NaN and +-inf in a box (the primitive untouched), and in a primitive (the box untouched)
    for v, irregular in ((f32(np.nan), True), (f32(np.inf), True), (f32(-np.inf), True)):
        for quad in (0, 1):
            t = point_sphere(f32(0.25)); t[quad, 1] = v
            got = flags_of(t, "%s in box quad %d" % (v, quad))
            bounds = (quad == 0 and v == -np.inf) or (quad == 1 and v == np.inf)     # an infinite box still bounds the sphere
            assert got[0] == irregular and got[1] == (not bounds), (v, quad, got)
            assert got[2] == bool(np.isnan(v)), (v, quad, got)               # a NaN plane is neither zero nor at least 2^-60
        t = point_sphere(f32(0.25)); t[4, 1] = v
        assert flags_of(t, "%s in a primitive" % v) == (False, True, False)
        t = point_sphere(f32(0.25)); t[4, 3] = v
        assert flags_of(t, "%s as a radius" % v) == (False, True, False)
    # the same in an interior node's children, where the boxes travel in a record
    two = K.small_trees()[1]
    for v in (f32(np.nan), f32(np.inf), f32(-np.inf), up(1048576.0), down(tiny)):
        for quad in (3, 4, 8, 9):
            t = two.copy(); t[quad, 2] = v
            flags_of(t, "%s in quad %d of the two-leaf tree" % (v, quad))
    t = two.copy(); t[4, :3] = t[3, :3]          # an inverted-to-a-point child box: ordered, but the sphere is outside
    assert flags_of(t, "a child box shrunk to a point") == (False, True, False)


# ---- g. words the device never reads -----------------------------------------------------------------------------------------------
def test_words_the_device_never_reads_change_nothing():
    """Parent addresses, IS_ROOT / IS_LOWER, and every pad word of the canonical layout: trees that differ only there convert to identical
    arrays and get identical flags."""
    junk = np.array([0xffffffff, 0x7fc00000, 0x7f800000, 0x7149f2ca, 0x80000001, 12345, 0xff800000], np.uint32)   # all ones, NaN, inf, 1e30, ...
    n_trees = 0
    for name, tree in (("box", B.compile_bvh(scene("box"))[0]), ("scene_pc", B.compile_bvh(scene("scene_pc"))[0]), ("mixed", K.small_trees()[2]),
                       ("root leaf", K.small_trees()[0])):
        base = check(tree, name)
        lay = R.layout(tree)
        rs = np.random.RandomState(5)
        pick = lambda size=None: junk[rs.randint(len(junk), size=size)]
        words = {}
        t = tree.copy(); u = t.view(np.uint32)
        u[lay["addr"] + 2, 3] = pick(len(lay["addr"]))
        words["parent addresses"] = t
        t = tree.copy(); u = t.view(np.uint32)
        u[lay["addr"] + 2, 0] ^= rs.randint(1, 4, size=len(lay["addr"])).astype(np.uint32) << np.uint32(29)
        words["IS_ROOT / IS_LOWER"] = t
        t = tree.copy(); u = t.view(np.uint32)
        u[lay["addr"], 3] = pick(len(lay["addr"])); u[lay["addr"] + 1, 3] = pick(len(lay["addr"]))
        leaves = lay["addr"][lay["leaf"]]
        u[leaves + 2, 1] = pick(len(leaves)); u[leaves + 2, 2] = pick(len(leaves))
        for a, ty in zip(lay["prim_addr"].tolist(), lay["prim_type"].tolist()):
            u[a, 1:4] = pick(3)
            if ty == S.DISC:
                u[a + 2, 3] = pick()
            elif ty == S.TRIANGLE:
                u[a + 1:a + 4, 3] = pick(3)
            elif ty == S.CONE:
                u[a + 4, 3] = pick()
        words["pad words"] = t
        for what, t in words.items():
            assert (bits(t) != bits(tree)).any(), what
            assert_same(hook(t), base, "%s: %s" % (name, what))
            assert_same(ref(t), base, "%s: %s (restatement)" % (name, what))
        n_trees += 1
    assert n_trees == 4


# ---- the uploader on a device ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_upload_threads_and_top_depth_render_the_same_frames(monkeypatch):
    """The big tree at 64 x 48, mode 0, one direct-lighting frame and one path-traced pass, on fresh contexts with GPUART_HIP_UPLOAD_THREADS =
    1, 3, 8 crossed with GPUART_HIP_TOP_DEPTH unset and 4 (the upload reads both each time): all six pairs of accumulators are bit-identical
    and equal the oracle's. Then a rejected tree: HipError "malformed", and the context renders the scene it had bit for bit as before."""
    from oracle import oracle as O
    from tests.test_gpu_parity import to_params
    W, H = 64, 48
    tree = K.big_tree()
    cam = dict(S.DEFAULT_CAMERA); cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    seed = O.randseeds(1)[0]
    exp_direct, _ = O.render_direct(tree, c, W, H, P)
    exp_pt = np.zeros((H, W, 4), np.float32)
    O.pt_pass(tree, c, W, H, P, seed, 1, exp_pt)
    assert len(np.unique(bits(exp_direct[..., :3]))) > 100 and len(np.unique(bits(exp_pt[..., :3]))) > 100   # frames of the tree, not of the sky

    def frames(be):
        be.render_direct(to_params(B, P))
        direct = be.read(0).copy()
        be.pt_reset(); be.pt_pass(to_params(B, P), seed, 1)
        return direct, be.read(1).copy()

    be, first = None, None
    for threads in (1, 3, 8):
        for top in (None, 4):
            monkeypatch.setenv("GPUART_HIP_UPLOAD_THREADS", str(threads))
            if top is None:
                monkeypatch.delenv("GPUART_HIP_TOP_DEPTH", raising=False)
            else:
                monkeypatch.setenv("GPUART_HIP_TOP_DEPTH", str(top))
            if be is not None:
                be.close()
            be = B.Backend(0)
            be.set_mode(0); be.resize(W, H); be.upload_bvh(tree); be.set_camera(c)
            direct, pt = frames(be)
            what = "%d threads, top depth %s" % (threads, top)
            assert_bits(direct[..., :3].reshape(-1, 3), exp_direct[..., :3].reshape(-1, 3), what + ": direct")
            assert_bits(pt[..., :3].reshape(-1, 3), exp_pt[..., :3].reshape(-1, 3), what + ": path-traced")
            first = first or (direct, pt)
            assert (bits(direct) == bits(first[0])).all() and (bits(pt) == bits(first[1])).all(), what
    with pytest.raises(B.HipError, match="malformed.*upper child does not start"):
        be.upload_bvh(K.rejections()["upper child one quad late"][0])
    direct, pt = frames(be)
    assert (bits(direct) == bits(first[0])).all() and (bits(pt) == bits(first[1])).all(), "after the rejected upload"
    be.close()
