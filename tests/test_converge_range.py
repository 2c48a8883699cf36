"""The convergence estimate where it is used and where it had not been tested (include/gpuart_converge.h):
A. against a float64 reference of another form (tests/converge_ref.reference64) at thousands to 2^24 paths per pixel: the fp32 arithmetic of
   the update, the floor the fp32 accumulator puts under e, two wrong variants that the comparison catches, and the same accumulators
   through the kernels;
B. against the variance real paths really have: E[se^2] = Var(mean) over independent replicate renders of the CPU oracle;
C. Renderer::RenderUntil in every state DESIGN.md describes, against the restatement on the oracle's accumulators.
The measured figures behind every tolerance are in profiles/convergence.txt, sections 4 and 5."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from gpuart_amd import sharding
from gpuart_amd import synth_scenes as S
from tests import converge_cases as K
from tests import converge_ref as R
from tests import test_converge as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
LUM_FLOOR = K.LUM_FLOOR

# ---- A. the float64 reference -------------------------------------------------------------------------------------------------
# Twice the largest differences measured over the case table (24 kinds of pixel x 128, six batch patterns, seed 17) between the
# restatement and reference64 on the same fp32 luminances: measured against the float64 reference, not against the kernels
# (profiles/convergence.txt, section 4, names the cases).
E_TOL = 2 * 1.251e-8       # |e32 - e64|: 4096x64, mean 0.01, cv 0, coloured
MEAN_TOL = 2 * 1.574e-5    # |mean32 - L_last / total| / (L_last / total): 4096x64, mean 0.01, cv 0, coloured
PER_KIND = 128
N_CPU = len(K.COMBOS) * PER_KIND


@pytest.fixture(scope="module")
def table():
    """Every batch pattern once: the restatement's e and mean, reference64 on the fp32 luminances and on the unrounded sums."""
    out = {}
    for name, sizes in K.PATTERNS.items():
        est = R.Estimator()
        mutants = {k: K.Mutant(k) for k in ("prev_mean", "r_batches")} if name in ("unequal", "64x64") else {}
        l32, l64, totals = [], [], []
        for acc, s64, total in K.batches(sizes, N_CPU, seed=17):
            a = acc.reshape(1, N_CPU, 4)
            est.update(a, total)
            for m in mutants.values():
                m.update(a, total)
            l32.append(R.lum(acc).astype(np.float64))
            l64.append(R.lum64(s64))
            totals.append(total)
        e64, mean64, _ = R.reference64(l32, totals, LUM_FLOOR)
        e_exact, mean_exact, _ = R.reference64(l64, totals, LUM_FLOOR)
        out[name] = dict(e32=est.error(LUM_FLOOR).reshape(-1).astype(np.float64), mean32=est.state[0, :, 0].astype(np.float64), e64=e64, mean64=mean64,
                         e_exact=e_exact, mean_exact=mean_exact, l_last=l32[-1], total=totals[-1], nb=len(totals),
                         mutants={k: m.error(LUM_FLOOR).reshape(-1).astype(np.float64) for k, m in mutants.items()})
    return out


def kind(i):
    return "mean %g cv %g %s" % (K.COMBOS[i % len(K.COMBOS)][:2] + ("coloured" if K.COMBOS[i % len(K.COMBOS)][2] else "grey",))


@pytest.mark.parametrize("name", sorted(K.PATTERNS))
def test_fp32_arithmetic_against_the_float64_reference(table, name):
    """Comparison 1: the restatement (which the kernels equal bit for bit) against reference64 on the same fp32 luminances: the
    update's own rounding, over up to 4096 batches and up to 2^24 paths, changes e by at most E_TOL and the mean by MEAN_TOL."""
    t = table[name]
    assert np.isfinite(t["e64"]).all() and np.isfinite(t["e32"]).all()
    de = np.abs(t["e32"] - t["e64"])
    i = int(de.argmax())
    print("%s (%d batches, %d paths): largest |e32 - e64| = %.3e at %s (e64 = %.3e)" % (name, t["nb"], t["total"], de[i], kind(i), t["e64"][i]))
    assert de[i] <= E_TOL, (name, kind(i), de[i])
    exact_mean = t["l_last"] / t["total"]
    assert np.allclose(t["mean64"], exact_mean, rtol=1e-12, atol=0)   # (the weighted mean of batch means telescopes)
    dm = np.abs(t["mean32"] - exact_mean) / exact_mean
    j = int(dm.argmax())
    print("%s: largest relative |mean32 - L/total| = %.3e at %s" % (name, dm[j], kind(j)))
    assert dm[j] <= MEAN_TOL, (name, kind(j), dm[j])


@pytest.mark.parametrize("mutant", ["prev_mean", "r_batches"])
def test_the_reference_catches_a_wrong_update(table, mutant):
    """Teeth: prevL kept as a rounded mean, and r = 1/batches, pass for 64 equal batches of 64 (where a steady pixel hides both: the
    tolerance is not loose there, it is the pattern that cannot tell) or fail, but must fail on the unequal pattern."""
    e64 = table["unequal"]["e64"]
    de = np.abs(table["unequal"]["mutants"][mutant] - e64)
    good = np.abs(table["unequal"]["e32"] - e64)
    print("mutant %s on [100, 3, 1, 7] repeated to 2^16: largest |e - e64| = %.3e (the restatement: %.3e, tolerance %.3e): caught" % (
        mutant, de.max(), good.max(), E_TOL))
    assert good.max() <= E_TOL < de.max() / 10, (mutant, de.max())


@pytest.mark.parametrize("name", sorted(K.PATTERNS))
def test_the_accumulator_floor(table, name):
    """Comparison 2: reference64 on the fp32-rounded luminances against reference64 on the unrounded float64 sums: what the fp32
    accumulator alone adds to e stays within 2^-22 sqrt(total / b_min), the formula include/gpuart_converge.h states
    (converge_ref.accumulator_floor). A luminance carries a relative error of about 2^-24 of the whole sum from its roundings; a batch mean
    is a difference of two of them over b paths, so its error is up to 2 * 2^-24 * total * mean / b; sqrt(m2) is a norm of the batch
    means' deviations with weights b, so it changes by at most sqrt(sum b_k err_k^2) <= 2^-23 total mean sqrt(batches / b_min), and
    e = sqrt(m2 / (batches - 1) / total) / mean by 2^-23 sqrt(total / b_min) sqrt(batches / (batches - 1)); the stated bound is twice
    that, for the extra roundings of L(a). Below the floor e is divided by more than the mean, so the bound holds there a fortiori."""
    t = table[name]
    bound = R.accumulator_floor(t["total"], K.b_min(K.PATTERNS[name]))
    assert bound == 2.0 ** -22 * np.sqrt(t["total"] / K.b_min(K.PATTERNS[name]))
    d = np.abs(t["e64"] - t["e_exact"])
    i = int(d.argmax())
    steady = np.array([K.COMBOS[k % len(K.COMBOS)][1] == 0 for k in range(N_CPU)])
    lit = t["mean_exact"] >= LUM_FLOOR
    print("%s: bound %.3e; largest |e64(fp32 L) - e64(exact L)| = %.3e (%.2f of it) at %s; steady pixels at or above the floor report e = %.1e .. %.1e" % (
        name, bound, d[i], d[i] / bound, kind(i), t["e32"][steady & lit].min(), t["e32"][steady & lit].max()))
    assert (t["e_exact"][steady] < 1e-10).all()    # (with unrounded sums a steady pixel has no error)
    assert d[lit].max() <= bound and d.max() <= bound, (name, kind(i), d[i], bound)


# ---- B. calibration on real paths (CPU oracle) ----------------------------------------------------------------------------------
W0, H0 = 64, 48
REPLICATES = 64
CAL_PATTERNS = {"16x4": [4] * 16, "8+6x4": [8, 4, 4, 4, 4, 4, 4], "8x1": [1] * 8}
TEETH = [32, 4, 4, 4, 4, 4, 4, 4]
BAND = (0.85, 1.15)


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def scene(O):
    """The box scene at 64 x 48 as the Renderer sets it up by default (tests/test_converge.py's)."""
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    tree, _ = O.build_bvh(S.box_scene())
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)

    def view(w, h):
        c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], w, h)
        return c, O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    c, P = view(W0, H0)
    return dict(cam=cam, tree=tree, c=c, P=P, view=view)


def calibrate(O, tree, c, P, w, h, patterns, replicates, seed0, nthreads=4):
    """Per pattern name {variant: sum over pixels of the estimated variance of the mean, averaged over the replicates} and "actual": the
    sum over pixels of the variance (ddof 1) of the replicates' means. Variants: "weighted" (the estimator), "unweighted"
    (Estimator(weighted=False)), "by_batches" (the weighted m2 divided by batches instead of total)."""
    marks = sorted({t for sizes in patterns.values() for t in np.cumsum(sizes)})
    v_est = {n: dict(weighted=0.0, unweighted=0.0, by_batches=0.0) for n in patterns}
    means = {n: [] for n in patterns}
    for rep in range(replicates):
        seeds = O.randseeds(marks[-1], seed=seed0 + rep)
        acc = np.zeros((h, w, 4), F)
        at = {}
        for k in range(marks[-1]):
            O.pt_pass(tree, c, w, h, P, seeds[k], 1, acc, nthreads=nthreads)
            if k + 1 in marks:
                at[k + 1] = acc.copy()
        for n, sizes in patterns.items():
            ests = dict(weighted=R.Estimator(), unweighted=R.Estimator(weighted=False))
            for t in np.cumsum(sizes):
                for e in ests.values():
                    e.update(at[int(t)], int(t))
            nb, total = len(sizes), int(sum(sizes))
            for v, e in ests.items():
                v_est[n][v] += float((np.maximum(e.state[..., 1].astype(np.float64), 0) / (nb - 1) / total).sum()) / replicates
            v_est[n]["by_batches"] += float((np.maximum(ests["weighted"].state[..., 1].astype(np.float64), 0) / (nb - 1) / nb).sum()) / replicates
            means[n].append(R.lum64(at[total]) / total)
    return {n: dict(v_est[n], actual=float(np.var(np.stack(means[n]), axis=0, ddof=1).sum())) for n in patterns}


@pytest.fixture(scope="module")
def calibration(O, scene):
    return calibrate(O, scene["tree"], scene["c"], scene["P"], W0, H0, dict(CAL_PATTERNS, teeth=TEETH), REPLICATES, 1000)


@pytest.mark.parametrize("name", sorted(CAL_PATTERNS))
def test_the_estimate_is_the_variance_real_paths_have(calibration, name):
    """For independent passes E[m2 / (batches - 1) / total] = Var(mean) whatever the paths' distribution (they are heavy-tailed: no
    Gaussian assumption). 64 replicate renders of the box, seeds 1000 + rep: the estimated variance of the pixel means, averaged over the
    replicates and summed over the frame, over the variance the 64 means really have. The band [0.85, 1.15] is about three standard
    deviations of that ratio (disjoint quarters of the replicates spread from 0.95 to 1.22)."""
    c = calibration[name]
    ratio = c["weighted"] / c["actual"]
    print("box %dx%d, batches %s, %d replicates: sum V_est / sum V_actual = %.4f" % (W0, H0, CAL_PATTERNS[name], REPLICATES, ratio))
    assert BAND[0] <= ratio <= BAND[1], (name, ratio)


def test_the_calibration_catches_a_wrong_estimator(calibration):
    """Teeth: ignoring the batch weights on a first batch of 32 and batches of 4, and dividing by batches instead of total, fall
    outside the band that the estimator itself meets on the same passes."""
    c = calibration["teeth"]
    good, unweighted = c["weighted"] / c["actual"], c["unweighted"] / c["actual"]
    print("batches %s: weighted %.4f, weights ignored %.4f: caught" % (TEETH, good, unweighted))
    assert BAND[0] <= good <= BAND[1] and not BAND[0] <= unweighted <= BAND[1], (good, unweighted)
    for name in CAL_PATTERNS:
        by_batches = calibration[name]["by_batches"] / calibration[name]["actual"]
        print("batches %s: divided by batches instead of total %.4f%s" % (CAL_PATTERNS[name], by_batches, "" if name == "8x1" else ": caught"))
        # (batches of one path: batches == total, the same number)
        assert (BAND[0] <= by_batches <= BAND[1]) == (name == "8x1"), (name, by_batches)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


GW, GH = 33, 7   # ragged: neither a multiple of the 64 x 4 block
# planted pixels (tests/test_converge.py's scheme): copies of one pixel, whose mean is the floor and whose e is the threshold
AT_FLOOR, FLOOR_SOURCE = [200, 201, 202], 16          # mean 1, cv 1, grey
AT_THRESHOLD, THRESHOLD_SOURCE = [210, 211, 212], 9   # mean 0.01, cv 0.05, coloured
GPU_PATTERNS = {"2^23+64x1": (K.PATTERNS["2^23+64x1"], True), "256x65536": (K.PATTERNS["256x65536"], True), "2048x64": ([64] * 2048, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GPU_PATTERNS))
def test_kernels_equal_the_restatement_on_long_renders(B, name):
    """b and total up to 2^24, r down to 2^-24, b * d large: the state after updates 1, 2, 3, every 256th and the last, then the error map
    and the summary, bit for bit, through the device entry points and (for the shorter patterns) the host ones."""
    import torch
    sizes, with_host = GPU_PATTERNS[name]
    n = GW * GH
    ref = R.Estimator()
    dev = B.Converge(0)
    host = B.Converge(0) if with_host else None
    try:
        for k, (acc, _, total) in enumerate(K.batches(sizes, n, seed=23, copies=((AT_FLOOR, FLOOR_SOURCE), (AT_THRESHOLD, THRESHOLD_SOURCE)))):
            acc = acc.reshape(GH, GW, 4)
            exp = ref.update(acc, total)
            dev.update(torch.from_numpy(acc).to("cuda:0"), total)
            if host:
                host.update(acc, total)
            if k < 3 or (k + 1) % 256 == 0 or k == len(sizes) - 1:
                T.assert_same(dev.state(), exp, "%s: state after update %d, device" % (name, k + 1))
                if host:
                    T.assert_same(host.state(), exp, "%s: state after update %d, host" % (name, k + 1))
        assert ref.total == sum(sizes) and ref.batches == len(sizes)
        flat = ref.state.reshape(-1, 4)
        floor = float(flat[FLOOR_SOURCE, 0])
        e0 = ref.error(floor).reshape(-1)
        thr = float(e0[THRESHOLD_SOURCE])
        below = float(np.nextafter(F(thr), F(-1)))
        assert (flat[AT_FLOOR, 0] == F(floor)).all() and (e0[AT_THRESHOLD] == F(thr)).all() and np.isfinite(thr) and thr > 0
        assert (flat[:, 0] > F(floor)).any() and np.isfinite(e0).all()
        for t, tag in ((thr, "at"), (below, "below"), (0.0, "zero")):
            s_exp, e_exp = ref.measure(t, floor)
            what = "%s threshold %s" % (name, tag)
            s, m = dev.measure(t, floor, error_map=torch.full((GH, GW), 7.0, device="cuda:0"))
            cs = B.ConvergeSummary()
            assert dev.L.gpuart_converge_measure(dev.h, C.c_float(t), C.c_float(floor), None, C.byref(cs)) == 0
            T.assert_summary(s, s_exp, what + " device+map")
            T.assert_summary(cs.as_dict(), s_exp, what + " device")
            T.assert_same(m.cpu().numpy(), e_exp, what + ": error map, device")
            if host:
                s1, m1 = host.measure(t, floor, error_map=True)
                T.assert_summary(s1, s_exp, what + " host+map")
                T.assert_summary(host.measure(t, floor), s_exp, what + " host")
                T.assert_same(m1, e_exp, what + ": error map, host")
        at, bel = ref.measure(thr, floor)[0], ref.measure(below, floor)[0]
        assert bel["above"] - at["above"] == int((e0 == F(thr)).sum()) >= len(AT_THRESHOLD) + 1, (at, bel)
    finally:
        dev.close()
        if host:
            host.close()


# ---- C. Renderer::RenderUntil, every state ----------------------------------------------------------------------------------------
CAP, BATCH = 32, 4
NPASS = 72   # one-path passes of the oracle: the longest scenario uses 28 + 40


@pytest.fixture(scope="module")
def one_path(O, scene):
    """The oracle's raw accumulator after every one-path pass (the RandSeeds of a never re-seeded Renderer), read-only."""
    seeds = O.randseeds(NPASS)
    acc = np.zeros((H0, W0, 4), F)
    at = {}
    for k in range(40):
        O.pt_pass(scene["tree"], scene["c"], W0, H0, scene["P"], seeds[k], 1, acc)
        at[k + 1] = acc.copy()
        at[k + 1].setflags(write=False)
    return dict(at=at, seeds=seeds)


class Until:
    """A Renderer beside the restatement of what its render_until calls must do (converge_ref.render_until on accum_at)."""

    def __init__(self, B, scene, accum_at, per_pass=1, cap=CAP, setup=None):
        self.B, self.scene, self.setup, self.per_pass, self.cap = B, scene, setup, per_pass, cap
        self.r = self.fresh()
        self.est = R.Estimator()
        self.accum_at = accum_at
        self.rendered = 0
        self.shown = []   # the path totals at which the restatement was shown the accumulator

    def fresh(self):
        r = T.make_renderer(self.B, self.scene, self.per_pass, self.cap)
        if self.setup:
            self.setup(r)
        return r

    def _at(self, total):
        self.shown.append(total)
        return self.accum_at(total)

    def plain(self, passes):
        for _ in range(passes):
            self.rendered = self.r.path_tracing_pass()

    def call(self, threshold, share=0.0, batch=BATCH, what=""):
        """One render_until on both; asserts the three things every scenario asserts; returns (converged, summary)."""
        converged, s = self.r.render_until(threshold, share, batch, LUM_FLOOR)
        exp_conv, exp_s, self.rendered = R.render_until(self.est, self._at, self.rendered, self.cap, self.per_pass, batch, threshold, share, LUM_FLOOR)
        assert converged == exp_conv, (what, converged, s, exp_s)
        if exp_s is None:
            assert s is None, (what, s)
        else:
            T.assert_summary(s, exp_s, what + ": summary")
        self.check(what)
        return converged, s

    def check(self, what=""):
        m = self.r.read_error_map(LUM_FLOOR)
        if self.est.batches >= 2:
            exp = self.est.error(LUM_FLOOR)
            assert m is not None and m.shape == exp.shape and T.same_or_zero(m, exp).all(), what + ": error map"
        else:
            assert m is None, what + ": an error map before the second batch"
        acc = self.r.read_radiance(False)
        if self.rendered:
            assert T.same_or_zero(acc[..., :3], self.accum_at(self.rendered)[..., :3]).all(), what + ": accumulator against the oracle"
        return acc

    def check_plain(self, passes, what=""):
        """The accumulator is that of `passes` plain passes of a fresh Renderer, bit for bit."""
        p = self.fresh()
        try:
            for _ in range(passes):
                p.path_tracing_pass()
            T.assert_same(self.r.read_radiance(False), p.read_radiance(False), what + ": accumulator after render_until and after plain passes")
        finally:
            p.close()

    def close(self):
        self.r.close()


def stopping_threshold(at, totals, share, first=1):
    """(threshold, j): the restatement, shown at[t] for t in totals, first has at most `share` of its pixels above the threshold after
    batch j + 1 >= first + 1, and batches follow it."""
    est = R.Estimator()
    q = []
    pixels = at[totals[0]].shape[0] * at[totals[0]].shape[1]
    allowed = int(np.floor(float(F(share)) * pixels))
    for t in totals:
        est.update(at[t], t)
        q.append(np.sort(est.error(LUM_FLOOR).reshape(-1))[pixels - allowed - 1] if est.batches >= 2 else np.inf)
    j = next(j for j in range(max(first, 2), len(totals) - 1) if q[j] < min(q[1:j]))
    return float(q[j]), j


@pytest.mark.gpu
def test_render_until_with_passes_that_do_not_divide_the_batch_or_the_cap(B, O, scene):
    """Passes of 3 paths, batches of at least 4, a cap of 32: every batch is two passes (6 paths), the last pass is clamped to 2 paths."""
    seeds = O.randseeds(11)
    acc = np.zeros((H0, W0, 4), F)
    at, total = {}, 0
    for k in range(11):
        n = min(3, 32 - total)
        O.pt_pass(scene["tree"], scene["c"], W0, H0, scene["P"], seeds[k], n, acc)
        total += n
        at[total] = acc.copy()
    u = Until(B, scene, at.__getitem__, per_pass=3, cap=32)
    try:
        converged, s = u.call(0.0, 0.0, 4, "ragged passes")
        assert not converged and u.shown == [6, 12, 18, 24, 30, 32] and s["total"] == 32 and s["batches"] == 6 and s["pixels"] == W0 * H0, (s, u.shown)
        assert u.r.path_tracing_pass() == 32
        u.check_plain(11, "ragged passes")
    finally:
        u.close()


@pytest.mark.gpu
def test_render_until_after_a_loaded_checkpoint(B, scene, one_path, tmp_path):
    """8 plain passes saved and loaded into a fresh Renderer are the first batch, of weight 8; a load resets an estimate that exists."""
    ck = str(tmp_path / "eight.ck")
    u = Until(B, scene, one_path["at"].__getitem__)
    try:
        u.plain(8)
        assert u.r.save_checkpoint(ck)
        u.close()
        u.r = u.fresh()
        assert u.r.load_checkpoint(ck) and u.r.read_error_map() is None
        converged, s = u.call(0.0, 0.0, BATCH, "checkpoint")
        assert not converged and u.shown == [8, 12, 16, 20, 24, 28, 32] and s["batches"] == 7 and s["total"] == CAP, (s, u.shown)
        u.check_plain(CAP, "checkpoint")
        # the same Renderer, which now holds an estimate, loads it again
        assert u.r.read_error_map() is not None and u.r.load_checkpoint(ck)
        assert u.r.read_error_map() is None
        u.est.reset()
        u.rendered, u.shown = 8, []
        thr, j = stopping_threshold(one_path["at"], [8, 12, 16, 20, 24, 28, 32], 0.1)
        converged, s = u.call(thr, 0.1, BATCH, "checkpoint, loaded again")
        assert converged and u.shown == [8 + 4 * k for k in range(j + 1)] and s["batches"] == j + 1 and s["total"] == 8 + 4 * j < CAP, (s, j, u.shown)
    finally:
        u.close()


@pytest.mark.gpu
def test_render_until_with_the_cap_inside_the_first_batch(B, scene, one_path, tmp_path):
    """A cap of 3 paths and batches of 4: one batch, no measure; the three paths are rendered; the CLI says so."""
    u = Until(B, scene, one_path["at"].__getitem__, per_pass=1, cap=3)
    try:
        assert u.call(0.5, 1.0, 4, "cap inside the first batch") == (False, None)
        assert u.shown == [3] and u.r.path_tracing_pass() == 3 and u.r.read_error_map() is None
        u.check_plain(3, "cap inside the first batch")
    finally:
        u.close()
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    cmd = [exe, "--scene", "box", "--width", str(W0), "--height", str(H0), "--per-pass", "1", "--spp", "3", "--until", "0.5", "--until-batch", "4"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 2 and lines[0]["batches"] == 0 and lines[0]["converged"] is False and lines[0]["paths_rendered"] == 3 == lines[1]["paths_per_pixel"], out.stdout
    epfm = tmp_path / "error.pfm"
    out = subprocess.run(cmd + ["--error-pfm", str(epfm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 1 and "no error map" in out.stderr and not epfm.exists(), (out.returncode, out.stderr)


@pytest.mark.gpu
def test_render_until_at_the_cap_only_measures_again(B, scene, one_path):
    """After a run that ended at the cap a call renders nothing and updates nothing: the same total, batches and accumulator, under the
    new threshold; and the comparison above <= share * pixels is made in double on the float share, at its boundary."""
    u = Until(B, scene, one_path["at"].__getitem__)
    try:
        converged, s0 = u.call(0.0, 0.0, BATCH, "to the cap")
        assert not converged and s0["total"] == CAP and s0["batches"] == CAP // BATCH and s0["non_finite"] == 0
        before = u.r.read_radiance(False)
        u.shown = []
        converged, s = u.call(2 * s0["max_error"], 0.0, BATCH, "at the cap")
        assert converged and s["above"] == 0 and (s["total"], s["batches"], s["max_error"]) == (s0["total"], s0["batches"], s0["max_error"]) and u.shown == []
        T.assert_same(u.r.read_radiance(False), before, "accumulator after the call at the cap")
        assert u.r.path_tracing_pass() == CAP
        # the share boundary: a threshold that leaves A > 0 pixels above; shares at float32(A / pixels) and its two neighbours
        e = np.sort(u.est.error(LUM_FLOOR).reshape(-1))
        seen = set()
        for thr in (float(e[e.size // 2]), float(e[(9 * e.size) // 10]), float(e[e.size // 3])):
            A = u.est.measure(thr, LUM_FLOOR)[0]["above"]
            assert 0 < A < e.size
            mid = F(A / e.size)
            for share in (np.nextafter(mid, F(0)), mid, np.nextafter(mid, F(1))):
                expect = float(A) <= float(F(share)) * float(e.size)
                converged, s = u.call(thr, float(share), BATCH, "share boundary")
                assert converged == expect and s["above"] == A and s["total"] == CAP and s["batches"] == CAP // BATCH, (A, share, converged, expect)
                seen.add(expect)
        assert seen == {True, False} and u.shown == []
    finally:
        u.close()


@pytest.mark.gpu
def test_render_until_counts_plain_passes_in_between(B, scene, one_path):
    """Stopped after batch j + 1, three plain passes, called again: the next batch has weight 3 + 4."""
    cap = 40
    thr, j = stopping_threshold(one_path["at"], list(range(4, cap + 1, 4)), 0.1, first=3)
    u = Until(B, scene, one_path["at"].__getitem__, cap=cap)
    try:
        converged, s = u.call(thr, 0.1, BATCH, "first call")
        stop = 4 * (j + 1)
        assert converged and s["total"] == stop and stop + 7 < cap, (s, j)
        u.plain(3)
        u.shown = []
        converged, s = u.call(0.0, 0.0, BATCH, "after three plain passes")
        rest = list(range(stop + 7, cap, 4)) + [cap]
        assert not converged and u.shown == rest and s["total"] == cap and s["batches"] == j + 1 + len(rest), (s, u.shown)
        u.check_plain(cap, "plain passes in between")
    finally:
        u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["tile", "share"])
def test_render_until_on_a_tile_and_on_an_interleaved_share(B, scene, one_path, geom):
    """The estimate is of the tile's pixels: set_tile(5, 7, 37, 23) and share 1 of 3 (bands of 8 rows): the oracle frame's rows and
    columns of that tile, and `pixels` is the tile's count."""
    if geom == "tile":
        x0, y0, tw, th = 5, 7, 37, 23
        rows = np.arange(y0, y0 + th)
        setup = lambda r: r.set_tile(x0, y0, tw, th) or pytest.fail("set_tile")
    else:
        y0, th, band, stride, rows = sharding.interleaved_rows(1, 3, H0)
        x0, tw = 0, W0
        assert th == 16 and list(rows[[0, 7, 8, 15]]) == [8, 15, 32, 39]
        setup = lambda r: r.set_interleaved_tile(0, y0, W0, th, band, stride) or pytest.fail("set_interleaved_tile")
    cut = {t: np.ascontiguousarray(a[rows, x0:x0 + tw]) for t, a in one_path["at"].items()}
    thr, j = stopping_threshold(cut, list(range(4, CAP + 1, 4)), 0.1)
    u = Until(B, scene, cut.__getitem__, setup=setup)
    try:
        converged, s = u.call(thr, 0.1, BATCH, geom)
        assert converged and s["pixels"] == tw * th and s["total"] == 4 * (j + 1) and s["batches"] == j + 1, (s, j)
        assert u.r.read_error_map(LUM_FLOOR).shape == (th, tw)
        u.check_plain(4 * (j + 1), geom)
        converged, s = u.call(0.0, 0.0, BATCH, geom + ", on to the cap")
        assert not converged and s["pixels"] == tw * th and s["total"] == CAP and s["batches"] == CAP // BATCH
    finally:
        u.close()


@pytest.mark.gpu
def test_render_until_after_a_viewport_resize(B, O, scene, one_path):
    """A converged call at 64 x 48, the viewport updated to 40 x 24, a second call: it succeeds on 960 pixels and the estimate started
    again at its first batch (the RandSeed draws go on: the generator is never re-seeded)."""
    thr, j = stopping_threshold(one_path["at"], list(range(4, CAP + 1, 4)), 0.1)
    u = Until(B, scene, one_path["at"].__getitem__)
    try:
        converged, s = u.call(thr, 0.1, BATCH, "before the resize")
        used = 4 * (j + 1)
        assert converged and s["total"] == used and s["pixels"] == W0 * H0
        w, h = 40, 24
        assert u.r.update_viewport(w, h) and u.r.read_error_map() is None
        c, P = scene["view"](w, h)
        acc = np.zeros((h, w, 4), F)
        small = {}
        for k in range(CAP):
            O.pt_pass(scene["tree"], c, w, h, P, one_path["seeds"][used + k], 1, acc)
            small[k + 1] = acc.copy()
        u.accum_at, u.rendered, u.shown = small.__getitem__, 0, []
        u.est.reset()
        converged, s = u.call(0.0, 0.0, BATCH, "after the resize")
        assert not converged and s["pixels"] == w * h == 960 and s["batches"] == CAP // BATCH and s["total"] == CAP and u.shown == list(range(4, CAP + 1, 4)), (s, u.shown)
        assert u.r.read_error_map(LUM_FLOOR).shape == (h, w)
    finally:
        u.close()
