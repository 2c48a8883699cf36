"""The history blend (libgpuart_temporal.so) and the denoiser (libgpuart_denoise.so) on every branch and edge value: synthetic cases
(tests/filter_cases.py) that reach every entry of the branch ledgers of the two restatements, a history of another share or frame than
the current tile, kept fp32 denormals, the largest legal shapes, counts that (float)spp rounds, out_rgba == rgba, stray non-finite
inputs, and the back-projection against a float64 solve. profiles/filter_edges.txt holds the measurements and what the tests catch."""
import hashlib

import numpy as np
import pytest

from tests import denoise_ref as R
from tests import filter_cases as FC
from tests import temporal_ref as T
from tests.test_temporal import TRACK, assert_same_bits, cpu_camera, cpu_gbuffer, radiance, run_chain, same_bits

FLOOR = 20     # every ledger entry, over the set of cases: a condition on the inputs, met by the restatements alone
_CACHE = {}


def temporal_cases():
    if "tp" not in _CACHE:
        _CACHE["tp"] = FC.temporal_cases()
    return _CACHE["tp"]


def denoise_cases():
    if "dn" not in _CACHE:
        _CACHE["dn"] = FC.denoise_cases()
    return _CACHE["dn"]


def add_to(total, led):
    for k, v in led.items():
        total[k] = total.get(k, 0) + v


def expected_chain(case, ledger=None):
    """The restatement's (out, len) of every call run_chain makes for a case, in order."""
    kw = dict(T.DEFAULTS, **(case["params"] or {}))
    hist, res = None, []
    for i, (rgba, spp, words, prims, v) in enumerate(case["steps"]):
        for _ in range(2 if i == case["preview_at"] else 1):
            out, ln, new, led = T.accumulate(hist, rgba, spp, words, prims, v, want_ledger=True, **kw)
            if ledger is not None:
                add_to(ledger, led)
            res.append((out, ln))
        hist = new
    return res


def denoise_kw(case):
    return dict(R.DEFAULTS, **(case["params"] or {}))


# ---- CPU: the ledgers ---------------------------------------------------------------------------------------------------------------
def restatement_digests(Tm, Rm):
    """SHA-256 of what the two restatements return on the CPU cases of tests/test_temporal.py and tests/test_denoise.py."""
    from tests.test_denoise import synthetic_gbuffer
    from tests.test_temporal import P_A, P_B, SPHERE
    dig = {}
    for name in ("box", "scene_p"):
        h = hashlib.sha256()
        hist = None
        for i, pos in enumerate(TRACK):
            words, prims, c = cpu_gbuffer(name, pos, SPHERE)
            v = Tm.view(c, Tm.full_frame(words.shape[1], words.shape[0]), SPHERE, 0)
            res = Tm.accumulate(hist, radiance(10 + i), 1 + i, words, prims, v, want_coords=True, **(P_A, P_B, Tm.DEFAULTS, P_A)[i])
            hist = res[2]
            for a in (res[0], res[1], hist["col"], hist["cls"], hist["n"], hist["p"]) + (res[3] or ()):
                h.update(np.ascontiguousarray(a).tobytes())
        dig["temporal " + name] = h.hexdigest()
    rng = np.random.default_rng(5)
    words, prims = synthetic_gbuffer(rng, 23, 37)
    rgba = rng.uniform(0, 3, (23, 37, 4)).astype(np.float32)
    h = hashlib.sha256()
    for flags in (0, 1, 2):
        for p in (dict(iterations=0), Rm.DEFAULTS, FC.DN_A, FC.DN_B):
            h.update(Rm.denoise(rgba, words, prims, flags, **dict(Rm.DEFAULTS, **p)).tobytes())
    dig["denoise"] = h.hexdigest()
    return dig


# what restatement_digests gave with the two restatements as they were before they grew a ledger
DIGESTS_BEFORE_THE_LEDGER = {
    "temporal box": "309aa86712968304bdab007cbbfeebaa9badef34a41646ae762f10105de22f11",
    "temporal scene_p": "0c424d45cd112494ab3ed2c108c426f2ee3e82a2c6c75439bd02f4453af2d3cc",
    "denoise": "1111c04e1b8f57f696fc6832b3a95c77b6feb6c2daaa03a868da2e306b3d9af7",
}


def test_the_ledger_leaves_the_restatements_values_alone():
    """On the existing CPU cases the two restatements return, bit for bit, what they returned before the ledger was built into them,
    and asking for the ledger changes no value."""
    assert restatement_digests(T, R) == DIGESTS_BEFORE_THE_LEDGER
    words, prims, c = cpu_gbuffer("box", TRACK[0])
    w1, p1, c1 = cpu_gbuffer("box", TRACK[1])
    g = T.full_frame(words.shape[1], words.shape[0])
    _, _, hist = T.accumulate(None, radiance(1), 3, words, prims, T.view(c, g))
    plain = T.accumulate(hist, radiance(2), 2, w1, p1, T.view(c1, g))
    asked = T.accumulate(hist, radiance(2), 2, w1, p1, T.view(c1, g), want_coords=True, want_ledger=True)
    assert len(plain) == 3 and len(asked) == 5 and set(asked[4]) == set(T.LEDGER_KEYS)
    assert same_bits(plain[0], asked[0]) and same_bits(plain[1], asked[1]) and same_bits(plain[2]["col"], asked[2]["col"])
    case = denoise_cases()[5]
    out, led = R.denoise(case["rgba"], case["words"], case["prims"], case["flags"], want_ledger=True, **denoise_kw(case))
    assert same_bits(out, R.denoise(case["rgba"], case["words"], case["prims"], case["flags"], **denoise_kw(case)))
    assert set(led) == set(R.LEDGER_KEYS)


def test_the_cases_reach_every_branch():
    """Over the set of cases every entry of both ledgers is at least FLOOR; the geometry pairs the kernel has lines for are all there;
    nothing the restatements expect from these in-contract inputs is non-finite."""
    assert np.float32(1e-39) * np.float32(0.5) != 0, "this host flushes fp32 denormals: the denormal cases would be trivial"
    tl, dl = {}, {}
    pairs = set()
    for case in temporal_cases():
        for out, ln in expected_chain(case, tl):
            assert np.isfinite(out).all() and np.isfinite(ln).all(), case["name"]
        for a, b in zip(case["steps"], case["steps"][1:]):
            ga, gb = a[4]["geom"], b[4]["geom"]
            full = lambda g: g[2:6] == (0, 0, g[0], g[1])
            banded = lambda g: g[7] > g[6]
            pairs.add(("banded" if banded(ga) else "full" if full(ga) else "tile", "banded" if banded(gb) else "full" if full(gb) else "tile",
                       "same" if ga == gb else "other frame" if ga[:2] != gb[:2] else "larger" if gb[4] * gb[5] > ga[4] * ga[5] else "smaller or equal"))
    for case in denoise_cases():
        out, led = R.denoise(case["rgba"], case["words"], case["prims"], case["flags"], want_ledger=True, **denoise_kw(case))
        assert np.isfinite(out).all(), case["name"]
        add_to(dl, led)
    print("temporal ledger:", tl)
    print("denoiser ledger:", dl)
    assert set(tl) == set(T.LEDGER_KEYS) and set(dl) == set(R.LEDGER_KEYS)
    assert min(tl.values()) >= FLOOR, {k: v for k, v in tl.items() if v < FLOOR}
    assert min(dl.values()) >= FLOOR, {k: v for k, v in dl.items() if v < FLOOR}
    for want in (("banded", "full", "other frame"), ("full", "banded", "other frame"), ("tile", "tile", "larger"), ("tile", "tile", "smaller or equal"),
                 ("full", "tile", "smaller or equal"), ("tile", "full", "larger")):
        assert want in pairs, (want, sorted(pairs))
    assert sorted(set(s[1] for c in temporal_cases() for s in c["steps"]) & {1, 2 ** 24 + 1, 2 ** 32 - 1}) == [1, 2 ** 24 + 1, 2 ** 32 - 1]
    assert np.float32(2 ** 24 + 1) == 2 ** 24 and np.float32(2 ** 32 - 1) == 2 ** 32      # the counts that (float)spp rounds
    shapes = set(s[0].shape[:2] for c in temporal_cases() for s in c["steps"]), set(c["rgba"].shape[:2] for c in denoise_cases())
    for w, h in FC.SMALL_SHAPES + FC.LONG_SHAPES:
        assert (h, w) in shapes[0] and (h, w) in shapes[1], (w, h)


def test_pixels_behind_the_old_camera_hang_on_k_alone():
    """The ledger counts the pixels behind the old camera, but a count is no value: were all their taps rejected anyway, a blend that
    forgot "k > 0" would give the same bits. A restatement without that condition (ignore_k) differs from the right one on at least
    FLOOR pixels, in chains of both directions (share -> full, full -> share); the pixels are those plant_mirrored makes. Not so for
    "dn != 0": dn = 0 makes u and v NaN or infinite, which fail the range tests by themselves, so dropping it changes no value and its
    count in the ledger stands for a branch taken, not for a value covered."""
    differ = {}
    for case in temporal_cases():
        kw = dict(T.DEFAULTS, **(case["params"] or {}))
        hist = None
        for rgba, spp, words, prims, v in case["steps"]:
            out, ln, new = T.accumulate(hist, rgba, spp, words, prims, v, **kw)
            wrong, wrong_len, _ = T.accumulate(hist, rgba, spp, words, prims, v, ignore_k=True, **kw)
            assert np.isfinite(wrong).all()
            n = int(((out.view(np.uint32) != wrong.view(np.uint32)).any(-1) | (ln != wrong_len)).sum())
            if n:
                differ[case["name"]] = differ.get(case["name"], 0) + n
            hist = new
    print("pixels that differ without k > 0:", differ)
    assert differ.get("share->full", 0) >= FLOOR and differ.get("full->share", 0) >= FLOOR, differ


def test_a_narrower_view_reads_a_history_of_another_pitch():
    """The tap address is row * (the HISTORY's width) + column. A blend that took the current width instead stays inside the history
    only where the current tile is not the wider one; `narrower` marks those chains, and at least one of them reads a history whose
    width differs from its own and finds history there, so that such a mistake shows as wrong values."""
    hit = []
    for case in temporal_cases():
        if not case["narrower"]:
            continue
        res = expected_chain(dict(case, preview_at=-1))
        for i in range(1, len(case["steps"])):
            a, b = case["steps"][i - 1], case["steps"][i]
            assert b[4]["geom"][4] <= a[4]["geom"][4]
            if b[4]["geom"][4] < a[4]["geom"][4] and int((res[i][1] > b[1]).sum()) >= FLOOR:
                hit.append(case["name"])
    assert "full->share" in hit, hit


def test_the_cases_hold_denormals():
    """The history blend of the denormal chain holds at least FLOOR denormal values, among them sums of products w * hist that are
    denormal themselves; the denoiser's outputs and states hold them too (its ledger counts them). A host that flushes denormals would
    make all of this trivial without saying so."""
    assert np.float32(1e-39) * np.float32(0.5) != 0
    case = [c for c in temporal_cases() if c["name"] == "denormals"][0]
    res = expected_chain(case)
    assert all(R.denormals(s[0][..., :3]) >= FLOOR for s in case["steps"])     # the radiance that goes in
    blended = [R.denormals(out[..., :3][ln > s[1]]) for (out, ln), s in zip(res[1:], [case["steps"][1]] * 2 + [case["steps"][2]])]
    print("denormal values in the blends of pixels that found history:", blended)
    assert min(blended) >= FLOOR, blended
    # w * hist: a history colour below 1e-39 times a bilinear weight below 1 is a denormal again
    hist_col = res[0][0][..., :3]
    assert R.denormals(hist_col) >= FLOOR and float(np.abs(hist_col).max()) <= 1e-39
    dl = {}
    for c in denoise_cases():
        add_to(dl, R.denoise(c["rgba"], c["words"], c["prims"], c["flags"], want_ledger=True, **denoise_kw(c))[1])
    assert dl["denormal_out"] >= FLOOR and dl["denormal_state"] >= FLOOR, dl


# ---- CPU: the back-projection against a float64 solve ------------------------------------------------------------------------------
# Measured maxima of |fx - (u W' - 1/2)| and |fy - (v H' - 1/2)| over the points below, in units of W' 2^-23 and H' 2^-23 pixel
# (profiles/filter_edges.txt); the test asserts twice the measured maximum.
BACKPROJECT_MEASURED = {(160, 120): (2.96, 3.16), (1920, 1080): (2.57, 2.93)}


def backproject_errors(W, H, uniform=False):
    """For 20000 hit points per camera of TRACK, spread over and around the old view's frustum (u, v in -0.2..1.2, 0.3..30 from the old
    camera): the fp32 fx, fy of T.backproject against u W' - 1/2, v H' - 1/2 of a float64 solve of
    u DH' + v DV' - m (p - pos') = -(BL' - pos'). -> (error in x, error in y, both in pixels, float64 fx, fy, the fp32 fx, fy, and
    whether k > 0 agrees with the sign of m)."""
    rng = np.random.default_rng(3)
    ex, ey, f64x, f64y, f32x, f32y, agree = [], [], [], [], [], [], []
    for pos in TRACK:
        c0 = cpu_camera(pos, W, H)
        v = T.view(c0, T.full_frame(W, H))
        c = c0.astype(np.float64)
        n = 20000
        # fx = u W' - 1/2 keeps 0.05 away from the integers, so that few floors are in doubt: of points uniform in u and v, 2 (bx + by)
        # would lie within the bound of an integer, which is 0.4 % at 1920 x 1080
        u = (np.floor(rng.uniform(-0.2, 1.2, n) * W) + 0.5 + rng.uniform(0.05, 0.95, n)) / W
        vv = (np.floor(rng.uniform(-0.2, 1.2, n) * H) + 0.5 + rng.uniform(0.05, 0.95, n)) / H
        if uniform:
            u, vv = rng.uniform(-0.2, 1.2, n), rng.uniform(-0.2, 1.2, n)
        dist = np.exp(rng.uniform(np.log(0.3), np.log(30), n))
        d = (c[3:6] + u[:, None] * c[6:9] + vv[:, None] * c[9:12]) - c[0:3]
        sign = np.where(rng.random(n) < 0.1, -1.0, 1.0)      # a tenth of the points lie behind the old camera
        p = (c[0:3] + (sign * dist)[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        with np.errstate(all="ignore"):
            fx, fy, k, dn, _ = T.backproject(p, v)
        P = p.astype(np.float64) - c[0:3]
        M = np.stack([np.broadcast_to(c[6:9], P.shape), np.broadcast_to(c[9:12], P.shape), -P], 2)
        sol = np.linalg.solve(M, np.broadcast_to(-(c[3:6] - c[0:3]), P.shape)[..., None])[..., 0]
        gx, gy = sol[:, 0] * W - 0.5, sol[:, 1] * H - 0.5
        ex.append(np.abs(fx - gx)); ey.append(np.abs(fy - gy))
        f64x.append(gx); f64y.append(gy); f32x.append(fx); f32y.append(fy)
        agree.append((k > 0) == (sol[:, 2] > 0))
    return tuple(np.concatenate(a) for a in (ex, ey, f64x, f64y, f32x, f32y, agree))


@pytest.mark.parametrize("W,H", [(160, 120), (1920, 1080)])
def test_backprojection_agrees_with_a_float64_solve(W, H):
    """Step 3 of the header between different views and outside the old frustum, against arithmetic that shares nothing with the kernel's
    formulas. The bound is twice the maximum measured against the float64 solve — a property of the header's fp32 formula, to which
    the GPU tests tie the kernel bit for bit — stated in units of W' 2^-23 (fx) and H' 2^-23 (fy) pixel. Where the float64 coordinate
    lies within the bound of an integer the floor may fall on the other side; those points are left out of the comparison of x0, y0
    and must be fewer than 0.1 % of all."""
    ex, ey, gx, gy, fx, fy, agree = backproject_errors(W, H)
    ux, uy = W * 2.0 ** -23, H * 2.0 ** -23
    print("%d x %d: max |fx - f64| %.3e pixel = %.2f W'2^-23, max |fy - f64| %.3e pixel = %.2f H'2^-23, %d points"
          % (W, H, ex.max(), ex.max() / ux, ey.max(), ey.max() / uy, ex.size))
    bx, by = 2 * BACKPROJECT_MEASURED[(W, H)][0] * ux, 2 * BACKPROJECT_MEASURED[(W, H)][1] * uy
    assert ex.max() <= bx and ey.max() <= by, (ex.max() / ux, ey.max() / uy)
    assert agree.all(), int((~agree).sum())
    near = (np.abs(gx - np.round(gx)) <= bx) | (np.abs(gy - np.round(gy)) <= by)
    assert near.mean() < 0.001, near.mean()
    assert (np.floor(fx)[~near] == np.floor(gx)[~near]).all() and (np.floor(fy)[~near] == np.floor(gy)[~near]).all()
    # The same with points uniform in u and v, which do come close to the cell borders: a share of 2 (bx + by) of them is expected within
    # the bound of an integer (0.43 % at 1920 x 1080, above the 0.1 % held above, which is why the first sample keeps away from the
    # borders); twice that share is allowed here, and every floor that is not in doubt agrees.
    ex, ey, gx, gy, fx, fy, agree = backproject_errors(W, H, uniform=True)
    print("%d x %d, uniform points: max %.2f W'2^-23, %.2f H'2^-23" % (W, H, ex.max() / ux, ey.max() / uy))
    assert ex.max() <= bx and ey.max() <= by and agree.all(), (ex.max() / ux, ey.max() / uy)
    near = (np.abs(gx - np.round(gx)) <= bx) | (np.abs(gy - np.round(gy)) <= by)
    assert 0 < near.mean() < 2 * 2 * (bx + by), (near.mean(), 2 * (bx + by))
    assert (np.floor(fx)[~near] == np.floor(gx)[~near]).all() and (np.floor(fy)[~near] == np.floor(gy)[~near]).all()


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def tp(B):
    handles = [B.Temporal(0), B.Temporal(0)]   # one fed through the host entry point, one through the device entry point
    yield handles
    for t in handles:
        t.close()


@pytest.fixture(scope="module")
def dn(B):
    d = B.Denoiser(0)
    yield d
    d.close()


def binding_view(B, v):
    return B.temporal_view(np.concatenate([v["pos"], v["bl"], v["dh"], v["dv"]]), v["geom"], tuple(v["user_sphere"]), v["us_flags"])


def chain_data(B, steps):
    return [(rgba, spp, words, prims, binding_view(B, v), v) for rgba, spp, words, prims, v in steps]


_RAN = {"temporal": {}, "denoise": {}, "cases": set()}


def run_temporal_case(tp, B, case):
    run_chain(tp, chain_data(B, case["steps"]), case["params"], case["name"], preview_at=case["preview_at"], ledger=_RAN["temporal"],
              alias_at=case["alias_at"])
    _RAN["cases"].add(case["name"])


def run_denoise_case(dn, case):
    from tests.test_denoise import check_entry_points
    check_entry_points(dn, case["rgba"], case["words"], case["prims"], case["flags"], case["params"], case["name"])
    add_to(_RAN["denoise"], R.denoise(case["rgba"], case["words"], case["prims"], case["flags"], want_ledger=True, **denoise_kw(case))[1])
    _RAN["cases"].add(case["name"])


def pick(cases, what):
    return [c for c in cases if (c["name"][0].isdigit()) == (what == "shapes")]


@pytest.mark.gpu
def test_history_of_another_geometry_equals_the_restatement(tp, B):
    """The chains whose history is another share, tile or frame than the current tile, with pixels behind and at the old camera, a moved
    user sphere, a long window, denormal colours, counts that (float)spp rounds and one device call whose out_rgba is its rgba: every
    blend and length of both entry points has the restatement's bits."""
    cases = pick(temporal_cases(), "branches")
    assert any(c["alias_at"] is not None for c in cases)
    for case in cases:
        run_temporal_case(tp, B, case)


@pytest.mark.gpu
def test_history_blend_at_the_edge_shapes(tp, B):
    """65536 x 1, 1 x 65536 and one below, at and one above the block's 64 x 4."""
    for case in pick(temporal_cases(), "shapes"):
        run_temporal_case(tp, B, case)


@pytest.mark.gpu
def test_denoiser_on_the_edge_patches_equals_the_restatement(dn):
    """Zero normals, pos = 1e-7 and 0, a flat patch, denormal and 1e15 radiance, for iterations 0 to 8 and two other settings, with and
    without the user-sphere pixels taken out: both entry points have the restatement's bits."""
    for case in pick(denoise_cases(), "branches"):
        run_denoise_case(dn, case)


@pytest.mark.gpu
def test_denoiser_at_the_edge_shapes(dn):
    """65536 x 1, 1 x 65536 and one below, at and one above the blocks' 64 x 4 and 16 x 16."""
    for case in pick(denoise_cases(), "shapes"):
        run_denoise_case(dn, case)


@pytest.mark.gpu
def test_the_gpu_ran_the_cases_that_reach_every_branch(tp, dn, B):
    """Prints the ledger totals of what the tests above ran on the device (it runs whatever they have not) and holds them to the floor
    the CPU check holds the cases to."""
    for case in temporal_cases():
        if case["name"] not in _RAN["cases"]:
            run_temporal_case(tp, B, case)
    for case in denoise_cases():
        if case["name"] not in _RAN["cases"]:
            run_denoise_case(dn, case)
    print("temporal ledger of the GPU run:", _RAN["temporal"])
    print("denoiser ledger of the GPU run:", _RAN["denoise"])
    assert set(_RAN["temporal"]) == set(T.LEDGER_KEYS) and min(_RAN["temporal"].values()) >= FLOOR, _RAN["temporal"]
    assert set(_RAN["denoise"]) == set(R.LEDGER_KEYS) and min(_RAN["denoise"].values()) >= FLOOR, _RAN["denoise"]
    assert _RAN["cases"] == set(c["name"] for c in temporal_cases() + denoise_cases())


@pytest.mark.gpu
def test_stray_non_finite_inputs_stay_inside_their_buffers(tp, B):
    """Outside the contract, but a caller's stray NaN must not take a tap out of its buffer: every data-dependent index of k_tp_accumulate
    is range-checked as a float before its (int) cast, and a NaN fails those comparisons. NaN, +-inf and 3e38 over the radiance, the hit
    points and so the history: every call returns 0, the guard elements before and after the outputs are untouched, every output the
    restatement expects finite has its bits, and every other one is non-finite."""
    import torch
    steps = FC.nonfinite_case()
    G = 64     # guard elements on either side (256 bytes: the device outputs stay 16-byte aligned)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def check(got, exp, what):
        fin = np.isfinite(exp)
        assert (got.view(np.uint32)[fin] == exp.view(np.uint32)[fin]).all(), what
        assert not np.isfinite(got[~fin]).any(), what
        return int((~fin).sum())

    for h in tp:
        h.reset()
    hist, odd = None, 0
    for i, (rgba, spp, words, prims, v) in enumerate(steps):
        view = binding_view(B, v)
        th, tw = rgba.shape[:2]
        for commit in (False, True):
            with np.errstate(all="ignore"):
                exp, exp_len, new = T.accumulate(hist, rgba, spp, words, prims, v)
            hbuf, hlen = np.full(2 * G + th * tw * 4, 7.0, np.float32), np.full(2 * G + th * tw, 7.0, np.float32)
            out, ln = hbuf[G:-G].reshape(th, tw, 4), hlen[G:-G].reshape(th, tw)
            tp[0].accumulate(rgba, spp, words, prims, view, commit=commit, out=out, out_len=ln)     # raises unless the call returns 0
            assert (hbuf[:G] == 7).all() and (hbuf[-G:] == 7).all() and (hlen[:G] == 7).all() and (hlen[-G:] == 7).all()
            odd += check(out, exp, "host") + check(ln, exp_len, "host length")
            dbuf, dlen = torch.full((2 * G + th * tw * 4,), 7.0, device="cuda:0"), torch.full((2 * G + th * tw,), 7.0, device="cuda:0")
            dout, dln = dbuf[G:-G].view(th, tw, 4), dlen[G:-G].view(th, tw)
            tp[1].accumulate(t(rgba), spp, t(words), t(prims), view, commit=commit, out=dout, out_len=dln)
            hb, hl = dbuf.cpu().numpy(), dlen.cpu().numpy()
            assert (hb[:G] == 7).all() and (hb[-G:] == 7).all() and (hl[:G] == 7).all() and (hl[-G:] == 7).all()
            odd += check(hb[G:-G].reshape(th, tw, 4), exp, "torch") + check(hl[G:-G].reshape(th, tw), exp_len, "torch length")
        hist = new
    assert odd >= FLOOR     # the non-finite values did reach the outputs
