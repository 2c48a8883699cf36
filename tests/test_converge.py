"""The convergence estimate (include/gpuart_converge.h, libgpuart_converge.so): the weighted batch-means estimator as statistics (CPU, on
its NumPy restatement tests/converge_ref.py), the kernels against that restatement bit for bit on synthetic accumulators with planted
edge values and on rendered ones, Renderer::RenderUntil / ReadErrorMap, gpuart_cli --until and the argument checks."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import converge_ref as R
from tests.util import exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
FLOOR = 20           # every ledger entry over the synthetic case set (as tests/test_filter_edges.py)
LUM_FLOOR = 1.0 / 256


def same(a, b):
    """Bit for bit; a NaN equals a NaN (the sign and payload of a generated NaN are the processor's choice: x86 and gfx950 differ)."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def assert_same(got, exp, what):
    got, exp = np.ascontiguousarray(got, F), np.ascontiguousarray(exp, F)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = ~same(got, exp)
    assert not bad.any(), "%s: %d of %d values differ; first at %s: got %r expected %r" % (
        what, int(bad.sum()), bad.size, np.argwhere(bad)[0], got[bad][0], exp[bad][0])


def assert_summary(got, exp, what):
    g, e = dict(got), dict(exp)
    gm, em = F(g.pop("max_error")), F(e.pop("max_error"))
    assert g == e and gm.view(np.uint32) == em.view(np.uint32), (what, got, exp)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_converge_library_exports_exactly_its_header(lib):
    names = sorted(set(re.findall(r"\b(gpuart_converge_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "gpuart_converge.h")).read())))
    assert len(names) == 10, names
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_converge.so")
    assert exported(path) == names
    # the estimator knows nothing of the scene: it links the HIP runtime, not the renderer's back end
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart_hip.so" not in dyn and "libamdhip64" in dyn, dyn
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    assert "gpuart_renderer_render_until" in host and "gpuart_renderer_read_error_map" in host


def test_summary_record_matches_the_header(tmp_path):
    from gpuart_amd import binding as B
    fields = ["pixels", "above", "non_finite", "max_error", "batches", "total"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_converge.h"\n'
                   'int main(void) { printf("%zu ' + "%zu " * len(fields) + '%u %u\\n", sizeof(gpuart_converge_summary), '
                   + ", ".join("offsetof(gpuart_converge_summary, %s)" % f for f in fields)
                   + ', GPUART_CONVERGE_MAX_PATHS, GPUART_CONVERGE_DEFAULT_BATCH); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = B.ConvergeSummary
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in fields] + [B.CONVERGE_MAX_PATHS, B.CONVERGE_DEFAULT_BATCH]
    assert got[:7] == [40, 0, 8, 16, 24, 28, 32] and got[7] == R.MAX_PATHS


SIZES = {"equal": [4] * 16, "doubling": [1, 2, 4, 8] * 4, "first100": [100] + [3] * 15}


def gaussian_run(sizes, seed, weighted=True, n=64):
    """Grey per-path radiance 1 + 0.5 N(0, 1) on n x n pixels, accumulated path by path in fp32, shown to the estimator batch by batch."""
    rng = np.random.default_rng(seed)
    est = R.Estimator(weighted)
    acc = np.zeros((n, n, 4), F)
    total = 0
    for b in sizes:
        for _ in range(b):
            acc[..., :3] += (F(1) + F(0.5) * rng.standard_normal((n, n)).astype(F))[..., None]
        total += b
        est.update(acc, total)
    return est


@pytest.mark.parametrize("name", sorted(SIZES))
def test_estimator_is_unbiased(name):
    """E[m2] = (batches - 1) sigma^2 whatever the batch sizes: over 64 x 64 pixels the mean of m2 / (batches - 1) over sigma^2 = 0.25 lies
    in [0.97, 1.03]. For Gaussian data m2 / sigma^2 is chi-squared with 15 degrees of freedom, so the relative standard deviation of
    that mean is sqrt(2/15) / 64 = 0.57 %: the bound is 5 sigma."""
    for seed in range(5):
        est = gaussian_run(SIZES[name], 100 + seed)
        ratio = float(est.variance().mean() / 0.25)
        print("%s seed %d: mean variance estimate / 0.25 = %.4f" % (name, seed, ratio))
        assert 0.97 <= ratio <= 1.03, (name, seed, ratio)
        # and the mean is the accumulator's: total paths, whatever their grouping
        assert np.allclose(est.state[..., 0], est.state[..., 2] / est.total, rtol=1e-5)


def test_ignoring_the_batch_weight_is_wrong_for_unequal_batches():
    """The variant that counts every batch as one sample: the same numbers for batches of one path, a variance estimate far outside the
    bound above for a first batch of 100 followed by batches of 3 (a batch mean's variance is sigma^2 / b: it estimates about
    sigma^2 (1/100 + 15/3) / 16 = 0.31 sigma^2)."""
    ones = gaussian_run([1] * 8, 7, weighted=False).variance().mean() / gaussian_run([1] * 8, 7).variance().mean()
    assert abs(ones - 1) < 1e-5, ones
    good, bad = gaussian_run(SIZES["first100"], 7), gaussian_run(SIZES["first100"], 7, weighted=False)
    assert 0.97 <= good.variance().mean() / 0.25 <= 1.03
    ratio = float(bad.variance().mean() / 0.25)
    assert 0.25 <= ratio <= 0.4, ratio
    assert not same(good.state[..., 1], bad.state[..., 1]).any()


def test_constant_image_has_no_error():
    """A constant per-path radiance gives m2 == 0 and e == 0 everywhere when every step is exact: path totals that double, so that the
    accumulator and its luminance scale by a power of two and every batch mean is the same float. With other totals the three roundings
    of L (relative 2^-24 each, in both luminances of a difference: 6 * 2^-24 * total / b relative to a batch mean) are all that is left:
    for 8 batches of 4 paths e stays below 6 * 2^-24 * 8 = 2.9e-6."""
    est = R.Estimator()
    img = np.zeros((5, 7, 4), F)
    img[..., :3] = [0.5, 0.25, 2.0]
    for total in [4, 8, 16, 32, 64]:
        est.update(img * F(total), total)
    assert (est.state[..., 1] == 0).all()
    s, e = est.measure(0.0, LUM_FLOOR)
    assert (e == 0).all() and s["above"] == 0 and s["non_finite"] == 0 and s["max_error"] == 0.0 and s["batches"] == 5 and s["total"] == 64
    est.reset()
    for total in range(4, 36, 4):
        est.update(img * F(total), total)
    s, e = est.measure(0.0, LUM_FLOOR)
    assert s["non_finite"] == 0 and s["max_error"] < 6 * 2.0 ** -24 * 8, s


def test_python_wrapper_checks_its_arguments():
    """The checks binding.Converge and binding.Renderer make before they call the library (on objects without a handle: no call is made)."""
    from gpuart_amd import binding as B
    c = object.__new__(B.Converge)
    c.h, c.shape, c.device = None, None, 0
    good = np.zeros((2, 3, 4), F)
    for accum, total in ((good, 0), (good, -1), (good, 1.5), (good, (1 << 24) + 1), (np.zeros((2, 3, 3), F), 1), (np.zeros((6, 4), F), 1)):
        with pytest.raises(ValueError):
            c.update(accum, total)
    with pytest.raises(ValueError):
        c.measure(0.1)          # before the first update
    with pytest.raises(ValueError):
        c.state()
    c.shape = (2, 3)
    for m in (np.zeros((3, 2), F), np.zeros((2, 3), np.float64), np.zeros((2, 6), F)[:, ::2]):
        with pytest.raises(ValueError):
            c.measure(0.1, error_map=m)
    r = object.__new__(B.Renderer)
    r.h = None
    for args in ((-1.0,), (float("nan"),), (float("inf"),), (0.1, -0.5), (0.1, float("nan")), (0.1, 0.0, 0), (0.1, 0.0, 2.5), (0.1, 0.0, 4, 0.0),
                 (0.1, 0.0, 4, float("inf"))):
        with pytest.raises(ValueError):
            r.render_until(*args)


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


# One size below, at and above each block dimension (64 x 4): 63x3, 64x4, 65x5; 3x8197 and 130x2735: more rows than k_cv_measure's grid
# has (2048 blocks of 4 rows for up to 64 columns, 682 for 130), so its waves walk several rows.
SHAPES = [(1, 1), (37, 23), (63, 3), (64, 4), (65, 5), (257, 3), (1920, 2), (3, 8197), (130, 2735)]
BATCHES = {"equal": [4, 4, 4, 4], "unequal": [100, 3, 1, 7]}
# The frame-size limits and two sizes one past a multiple of the block: at 65536 columns k_cv_measure's grid cap (2048 blocks / 1024
# column blocks) is 2 with a single row of blocks, at 1 x 65536 every wave walks 8 rows; 4097 and 2049 columns leave one pixel in the
# last column block. A smaller loop: equal batches, the device update, one device measure and one host measure with a map.
EDGE_SHAPES = [(65536, 1), (1, 65536), (4097, 3), (2049, 5)]


def synthetic(w, h, sizes, seed):
    """Accumulators of a made-up render, one per batch, with planted pixels; returns (accums, totals, groups): groups names the planted
    pixels (flat indices). Pixels of one group are copies of each other."""
    rng = np.random.default_rng(seed)
    n = w * h
    mu = rng.uniform(0.02, 2.0, (n, 3)).astype(F)
    sg = (mu * rng.uniform(0.05, 1.5, (n, 1))).astype(F)
    k = min(6, n // 9)   # pixels per planted group (none in a tile of fewer than 9 pixels)
    names = ["black", "dim", "at_floor", "at_threshold", "nan", "inf", "overflow", "denormal", "steady"]
    pick = rng.permutation(n)[:k * len(names)].reshape(len(names), k) if k else np.zeros((len(names), 0), np.int64)
    groups = dict(zip(names, pick))
    accums, totals = [], []
    acc = np.zeros((n, 4), F)
    total = 0
    for j, b in enumerate(sizes):
        step = np.maximum(F(b) * mu + np.sqrt(F(b)) * sg * rng.standard_normal((n, 3)).astype(F), F(0)).astype(F)
        for g in ("at_floor", "at_threshold"):   # copies of the group's first pixel
            step[groups[g]] = step[groups[g][:1]]
        step[groups["black"]] = 0
        step[groups["dim"]] = F(b) * F(0.001) * (1 + (j & 1))           # luminance below the floor, with a spread
        step[groups["steady"]] = F(b) * F(0.5)                           # no spread: m2 = 0 or rounding noise of either sign
        step[groups["denormal"]] = F(b) * F(1e-41) * (1 + (j & 1))
        step[groups["overflow"]] = F(3e25) * (j & 1)                     # b d^2 overflows: m2 = +inf, e = +inf
        acc = acc.copy()
        acc[:, :3] += step
        acc[:, 3] = F(total + b)
        if j >= 1:
            acc[groups["nan"], 1] = np.nan
        acc[groups["inf"], 0] = np.inf
        total += b
        accums.append(acc.reshape(h, w, 4))
        totals.append(total)
    return accums, totals, groups


@pytest.mark.gpu
def test_kernels_equal_the_restatement_on_synthetic_accumulators(B):
    """read_state after every update, the error map and the summary, bit for bit, through the host entry points (NumPy) and the device
    ones (torch), with and without a map; thresholds and floors taken from the restatement's own values for planted pixels."""
    import torch
    ledger, edge_ledger = R.new_ledger(), R.new_ledger()   # (each loop meets the floor on its own)
    host, dev = B.Converge(0), B.Converge(0)
    try:
        for w, h in SHAPES:
            for bname, sizes in BATCHES.items():
                what = "%dx%d %s" % (w, h, bname)
                accums, totals, groups = synthetic(w, h, sizes, seed=w * 131 + h)
                ref = R.Estimator()
                host.reset()
                dev.reset()
                for k, (acc, total) in enumerate(zip(accums, totals)):
                    exp = ref.update(acc, total)
                    host.update(acc, total)
                    dev.update(torch.from_numpy(acc).to("cuda:0"), total)
                    assert_same(host.state(), exp, "%s: state after update %d, host" % (what, k))
                    assert_same(dev.state(), exp, "%s: state after update %d, device" % (what, k))
                    if k == 0:
                        continue
                    # the floor: the mean of the at_floor pixels (they are not above it); the threshold: the e of the at_threshold pixels
                    # under that floor (they are not above it), and the float below it (now they are: their e is the next float up)
                    flat = ref.state.reshape(-1, 4)
                    floor = float(flat[groups["at_floor"][0], 0]) if len(groups["at_floor"]) else LUM_FLOOR
                    e0 = ref.error(floor).reshape(-1)
                    thr = float(e0[groups["at_threshold"][0]]) if len(groups["at_threshold"]) else 0.05
                    below = float(np.nextafter(F(thr), F(-1)))
                    for t, tag in ((thr, "at"), (below, "below"), (0.0, "zero")):
                        if t < 0:
                            continue
                        s_exp, e_exp = ref.measure(t, floor, ledger)
                        s1, m1 = host.measure(t, floor, error_map=True)
                        s2 = host.measure(t, floor)
                        s3, m3 = dev.measure(t, floor, error_map=torch.full((h, w), 7.0, device="cuda:0"))
                        cs = B.ConvergeSummary()   # the call Renderer::RenderUntil makes: device entry point, no map
                        assert dev.L.gpuart_converge_measure(dev.h, C.c_float(t), C.c_float(floor), None, C.byref(cs)) == 0
                        s4 = cs.as_dict()
                        for s, tg in ((s1, "host+map"), (s2, "host"), (s3, "device+map"), (s4, "device")):
                            assert_summary(s, s_exp, "%s update %d threshold %s %s" % (what, k, tag, tg))
                        assert_same(m1, e_exp, "%s update %d: error map, host" % (what, k))
                        assert_same(m3.cpu().numpy(), e_exp, "%s update %d: error map, device" % (what, k))
                    if len(groups["at_threshold"]):
                        g = groups["at_threshold"]
                        at, bel = ref.measure(thr, floor)[0], ref.measure(below, floor)[0]
                        assert (e0[g] == F(thr)).all() and np.isfinite(thr) and thr > 0
                        assert bel["above"] - at["above"] == int((e0 == F(thr)).sum()) >= len(g), (what, k, at, bel)
                        # the planted values did what they were planted for
                        st = flat
                        assert (st[groups["at_floor"], 0] == F(floor)).all() and (st[groups["dim"], 0] < F(floor)).all()
                        assert np.isnan(e0[groups["nan"]]).all() and np.isnan(e0[groups["inf"]]).all() and np.isinf(e0[groups["overflow"]]).all()
                        assert at["non_finite"] == len(groups["nan"]) + len(groups["inf"]) + len(groups["overflow"])
                        assert at["above"] >= at["non_finite"] and np.isfinite(at["max_error"])
                        assert ((st[groups["denormal"], 2] != 0) & (np.abs(st[groups["denormal"], 2]) < np.finfo(F).tiny)).all()
                        assert (e0[groups["black"]] == 0).all()
        for w, h in EDGE_SHAPES:
            what = "%dx%d equal" % (w, h)
            accums, totals, groups = synthetic(w, h, BATCHES["equal"], seed=w * 131 + h)
            ref = R.Estimator()
            dev.reset()
            for k, (acc, total) in enumerate(zip(accums, totals)):
                exp = ref.update(acc, total)
                dev.update(torch.from_numpy(acc).to("cuda:0"), total)
                assert_same(dev.state(), exp, "%s: state after update %d, device" % (what, k))
            flat = ref.state.reshape(-1, 4)
            floor = float(flat[groups["at_floor"][0], 0])
            e0 = ref.error(floor).reshape(-1)
            thr = float(e0[groups["at_threshold"][0]])
            assert (e0[groups["at_threshold"]] == F(thr)).all() and np.isfinite(thr) and thr > 0
            for t, tag in ((thr, "at"), (float(np.nextafter(F(thr), F(-1))), "below")):
                s_exp, e_exp = ref.measure(t, floor, edge_ledger)
                cs = B.ConvergeSummary()
                assert dev.L.gpuart_converge_measure(dev.h, C.c_float(t), C.c_float(floor), None, C.byref(cs)) == 0
                assert_summary(cs.as_dict(), s_exp, "%s threshold %s device" % (what, tag))
                s1, m1 = dev.measure(t, floor, error_map=True)
                assert_summary(s1, s_exp, "%s threshold %s host+map" % (what, tag))
                assert_same(m1, e_exp, "%s: error map, host" % what)
            assert s_exp["non_finite"] == len(groups["nan"]) + len(groups["inf"]) + len(groups["overflow"]) > 0
    finally:
        host.close()
        dev.close()
    print("ledger:", ledger)
    print("ledger of the edge shapes:", edge_ledger)
    assert min(ledger.values()) >= FLOOR, ledger
    assert min(edge_ledger.values()) >= FLOOR, edge_ledger


W0, H0 = 64, 48
NBATCH, PER = 8, 4   # the oracle's accumulators: 8 batches of 4 one-path passes


@pytest.fixture(scope="module")
def box(O):
    """The box scene at 64 x 48 as the Renderer sets it up by default, and the oracle's raw accumulator after every batch of 4 passes
    (the RandSeeds of a never re-seeded Renderer), computed once."""
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    tree, _ = O.build_bvh(S.box_scene())
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W0, H0)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    seeds = O.randseeds(NBATCH * PER)
    acc = np.zeros((H0, W0, 4), F)
    accums = []
    for k in range(NBATCH * PER):
        O.pt_pass(tree, c, W0, H0, P, seeds[k], 1, acc)
        if k % PER == PER - 1:
            accums.append(acc.copy())
    for a in accums:
        a.setflags(write=False)
    return dict(cam=cam, tree=tree, c=c, P=P, seeds=seeds, accums=accums, totals=[PER * (k + 1) for k in range(NBATCH)])


def same_or_zero(a, b):
    """As tests.util.bit_mismatch: bit for bit, +0 = -0."""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [3, 5])
def test_state_of_rendered_batches_equals_the_restatement_on_the_oracle(B, O, box, mode):
    """Four batches of four passes through Backend (the launch pipeline, then the persistent run kernel), the raw accumulator exported
    on the device after each: the state is the restatement's on the oracle's accumulators."""
    import torch
    be, cv = B.Backend(0), B.Converge(0)
    try:
        be.upload_bvh(box["tree"])
        be.resize(W0, H0)
        be.set_camera(box["c"])
        be.set_mode(mode)
        P = B.Params()
        C.memmove(C.byref(P), C.byref(box["P"]), C.sizeof(P))
        be.pt_reset()
        ref = R.Estimator()
        buf = torch.zeros((H0, W0, 4), device="cuda:0")
        torch.cuda.synchronize()
        for k in range(4):
            be.pt_plan(PER)
            for s in box["seeds"][PER * k:PER * (k + 1)]:
                be.pt_pass(P, s, 1)
            be.export(1, buf.data_ptr(), 1.0)
            be.finish()
            assert same_or_zero(buf.cpu().numpy()[..., :3], box["accums"][k][..., :3]).all(), "accumulator after batch %d" % k
            cv.update(buf, PER * (k + 1))
            exp = ref.update(box["accums"][k], PER * (k + 1))
            assert same_or_zero(cv.state(), exp).all(), "state after batch %d, mode %d" % (k, mode)
        s_exp, e_exp = ref.measure(0.1, LUM_FLOOR)
        s, m = cv.measure(0.1, LUM_FLOOR, error_map=True)
        assert_summary(s, s_exp, "summary")
        assert same_or_zero(m, e_exp).all() and s["above"] > 0 and s["non_finite"] == 0
    finally:
        cv.close()
        be.close()


SHARE = 0.1


def predicted(box):
    """A threshold that the restatement, on the oracle's accumulators, first meets after batch j + 1, 3 <= j < NBATCH - 1: for every
    batch the smallest threshold at which at most SHARE of the pixels are above, then the first j whose value is below all earlier ones."""
    est = R.Estimator()
    q = []
    allowed = int(np.floor(float(F(SHARE)) * W0 * H0))
    for a, t in zip(box["accums"], box["totals"]):
        est.update(a, t)
        q.append(np.sort(est.error(LUM_FLOOR).reshape(-1))[W0 * H0 - allowed - 1] if est.batches >= 2 else np.inf)
    j = next(j for j in range(3, NBATCH - 1) if q[j] < min(q[1:j]))
    thr = float(q[j])
    k, s = R.stops_at(box["accums"], box["totals"], thr, SHARE, LUM_FLOOR)
    assert k == j and s["above"] <= allowed
    return thr, j, s


def make_renderer(B, box, per_pass, cap):
    r = B.Renderer(W0, H0, box["cam"])
    r.init_box()
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.restart_path_tracing(per_pass, cap)
    return r


@pytest.mark.gpu
def test_render_until_stops_where_the_restatement_predicts(B, box):
    thr, j, s_exp = predicted(box)
    cap = NBATCH * PER
    r = make_renderer(B, box, 1, cap)
    try:
        assert r.read_error_map() is None
        converged, s = r.render_until(thr, SHARE, PER, LUM_FLOOR)
        assert converged and s["total"] == PER * (j + 1) < cap, (s, j)
        assert_summary(s, s_exp, "render_until's last measure")
        acc = r.read_radiance(False)
        assert same_or_zero(acc[..., :3], box["accums"][j][..., :3]).all()
        est = R.Estimator()
        for a, t in zip(box["accums"][:j + 1], box["totals"]):
            est.update(a, t)
        assert same_or_zero(r.read_error_map(LUM_FLOOR), est.error(LUM_FLOOR)).all()
        # the same number of plain passes: the same bits
        p = make_renderer(B, box, 1, cap)
        try:
            for _ in range(PER * (j + 1)):
                p.path_tracing_pass()
            assert_same(acc, p.read_radiance(False), "accumulator after render_until and after plain passes")
        finally:
            p.close()
        # it goes on from where it stopped; a threshold nothing reaches ends at the cap
        converged, s = r.render_until(0.0, 0.0, PER, LUM_FLOOR)
        assert not converged and s["total"] == cap and s["batches"] == NBATCH and s["above"] > 0
        assert same_or_zero(r.read_radiance(False)[..., :3], box["accums"][-1][..., :3]).all()
        # a setter restarts the accumulation and with it the estimate
        assert r.read_error_map() is not None
        r.set_sun(float(S.SUN_AZIMUTH) + 0.5, float(S.SUN_ALTITUDE))
        assert r.read_error_map() is None
        converged, s = r.render_until(0.0, 0.0, PER, LUM_FLOOR)
        assert not converged and s["total"] == cap and s["batches"] == NBATCH
    finally:
        r.close()


@pytest.mark.gpu
def test_render_until_leaves_the_denoised_preview_alone(B, box):
    """ReadDenoised before and after RenderUntil, and the accumulator, are those of a run that renders the same passes without it; paths
    rendered before the first RenderUntil are its first batch."""
    def run(with_until):
        r = make_renderer(B, box, 1, 16)
        try:
            for _ in range(8):
                r.path_tracing_pass()
            d1 = r.read_denoised()
            if with_until:
                assert r.render_until(0.0, 0.0, PER, LUM_FLOOR)[0] is False
            else:
                for _ in range(8):
                    r.path_tracing_pass()
            return d1, r.read_denoised(), r.read_radiance(False), r.read_error_map(LUM_FLOOR)
        finally:
            r.close()
    a, b = run(False), run(True)
    for x, y, what in zip(a[:3], b[:3], ("denoised before", "denoised after", "accumulator")):
        assert_same(y, x, what)
    assert same_or_zero(b[2][..., :3], box["accums"][3][..., :3]).all()
    # the 8 paths rendered before the call were the estimate's first batch, of weight 8: batches of 8, 4 and 4 paths
    est = R.Estimator()
    for k in (1, 2, 3):
        est.update(box["accums"][k], box["totals"][k])
    assert a[3] is None and same_or_zero(b[3], est.error(LUM_FLOOR)).all()


def read_pfm(path, w, h, grey=False):
    raw = open(path, "rb").read()
    head = b"P%s\n%d %d\n-1.0\n" % (b"f" if grey else b"F", w, h)
    assert raw.startswith(head), raw[:32]
    return raw, np.frombuffer(raw[len(head):], F).reshape((h, w) if grey else (h, w, 3))


@pytest.mark.gpu
def test_cli_until(B, box, tmp_path):
    """gpuart_cli --until: its line, its frame byte-equal to a plain --spp run of the path count it reports, --error-pfm = read_error_map,
    and the refusal of --gpus 2."""
    thr, j, s_exp = predicted(box)
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", str(W0), "--height", str(H0), "--per-pass", "1"]
    pfm, epfm, plain = str(tmp_path / "until.pfm"), str(tmp_path / "error.pfm"), str(tmp_path / "plain.pfm")
    until = ["--until", "%.9g" % thr, "--until-share", "%.9g" % SHARE, "--until-batch", str(PER), "--until-floor", "%.9g" % LUM_FLOOR]
    out = subprocess.run(base + ["--spp", str(NBATCH * PER)] + until + ["--pfm", pfm, "--error-pfm", epfm], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]   # (the scene set-up prints its own lines)
    assert len(lines) == 2 and "until" in lines[0], out.stdout
    u = lines[0]
    assert u["converged"] is True and u["paths_rendered"] == PER * (j + 1) == lines[1]["paths_per_pixel"], (u, j)
    assert u["batches"] == j + 1 and u["above"] == s_exp["above"] and u["pixels"] == W0 * H0, (u, s_exp)
    assert F(u["max_error"]).view(np.uint32) == F(s_exp["max_error"]).view(np.uint32) and F(u["until"]) == F(thr)
    out = subprocess.run(base + ["--spp", str(u["paths_rendered"]), "--pfm", plain], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and len([l for l in out.stdout.splitlines() if l.startswith("{")]) == 1, (out.stdout, out.stderr)
    assert open(pfm, "rb").read() == open(plain, "rb").read()
    r = make_renderer(B, box, 1, NBATCH * PER)
    try:
        assert r.render_until(thr, SHARE, PER, LUM_FLOOR)[0]
        assert_same(read_pfm(epfm, W0, H0, grey=True)[1], r.read_error_map(LUM_FLOOR), "--error-pfm")
    finally:
        r.close()
    out = subprocess.run(base + ["--spp", "8", "--gpus", "2"] + until, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--until" in out.stderr and not out.stdout, (out.returncode, out.stdout, out.stderr)


@pytest.mark.gpu
def test_argument_errors(B):
    """Every GPUART_HIP_ERR_ARG case of the header returns the error with a message, and nothing is written or counted."""
    import torch
    cv = B.Converge(0)
    L = cv.L
    try:
        h, w = 4, 6
        rng = np.random.default_rng(3)
        acc = rng.uniform(0, 2, (h * w + 1, 4)).astype(F)
        ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
        summary = B.ConvergeSummary()
        err = lambda: L.gpuart_converge_last_error().decode()

        def update(fn="gpuart_converge_update_host", accum=ptr(acc), total=8, ww=w, hh=h):
            return getattr(L, fn)(cv.h, accum, C.c_uint32(total), C.c_uint32(ww), C.c_uint32(hh))

        def measure(fn="gpuart_converge_measure_host", thr=0.1, floor=LUM_FLOOR, m=None, s=C.byref(summary)):
            return getattr(L, fn)(cv.h, C.c_float(thr), C.c_float(floor), m, s)

        state = np.full((h, w, 4), 7.0, F)
        assert L.gpuart_converge_read_state(cv.h, ptr(state)) == ERR_ARG and "first update" in err() and (state == 7.0).all()
        assert L.gpuart_converge_create(C.c_int(0), None) == ERR_ARG and L.gpuart_converge_reset(None) == ERR_ARG
        assert L.gpuart_converge_finish(None) == ERR_ARG and L.gpuart_converge_read_state(None, ptr(state)) == ERR_ARG
        assert update(total=4) == 0
        emap = np.full(h * w + 1, 7.0, F)
        assert measure(m=ptr(emap)) == ERR_ARG and "2 batches" in err()     # before the second update
        assert update(total=8) == 0
        cv.shape = (h, w)   # (the updates above went past the wrapper)
        before = cv.state()
        d = torch.zeros(h * w * 4 + 8, device="cuda:0")
        dp = lambda k=0: C.c_void_p(d.data_ptr() + k)
        cases = [(dict(total=8), "not above"), (dict(total=3), "not above"), (dict(total=0), "not above"), (dict(total=(1 << 24) + 1), "2^24"),
                 (dict(ww=w + 1), "state's"), (dict(hh=h - 1), "state's"), (dict(ww=h, hh=w), "state's"), (dict(accum=None), "NULL"),
                 (dict(accum=ptr(acc, 2)), "misaligned"), (dict(ww=0), "bad size"), (dict(hh=0), "bad size"), (dict(ww=65537), "bad size"),
                 (dict(hh=65537), "bad size"),
                 (dict(fn="gpuart_converge_update", accum=dp(4)), "misaligned"), (dict(fn="gpuart_converge_update", accum=dp(8)), "misaligned"),
                 (dict(fn="gpuart_converge_update", accum=None), "NULL"), (dict(fn="gpuart_converge_update", accum=dp(), total=8), "not above"),
                 (dict(fn="gpuart_converge_update", accum=dp(), ww=w + 1), "state's")]
        for kw, msg in cases:
            kw = dict(dict(total=12), **kw)
            rc = update(**kw)
            assert rc == ERR_ARG and msg in err(), (kw, msg, rc, err())
        mcases = [(dict(thr=float("nan"), m=ptr(emap)), "threshold"), (dict(thr=-0.5), "threshold"), (dict(thr=float("inf")), "threshold"),
                  (dict(floor=0.0, m=ptr(emap)), "lum_floor"), (dict(floor=-1.0), "lum_floor"), (dict(floor=float("nan")), "lum_floor"),
                  (dict(floor=float("inf")), "lum_floor"), (dict(m=ptr(emap, 2)), "misaligned"), (dict(s=None, m=ptr(emap)), "summary is NULL"),
                  (dict(fn="gpuart_converge_measure", m=dp(2)), "misaligned"), (dict(fn="gpuart_converge_measure", thr=float("nan")), "threshold"),
                  (dict(fn="gpuart_converge_measure", s=None), "summary is NULL")]
        for kw, msg in mcases:
            rc = measure(**kw)
            assert rc == ERR_ARG and msg in err(), (kw, msg, rc, err())
        assert (emap == 7.0).all() and (d == 0).all() and summary.pixels == 0 and summary.batches == 0
        # nothing was written or counted: the state, the batches and the total are those of the two good updates
        assert_same(cv.state(), before, "state after the rejected calls")
        ref = R.Estimator()
        ref.update(acc[:h * w].reshape(h, w, 4), 4)
        ref.update(acc[:h * w].reshape(h, w, 4), 8)
        assert_same(before, ref.state, "state")
        assert measure(m=ptr(emap)) == 0 and (emap[h * w] == 7.0) and not (emap[:h * w] == 7.0).any()
        assert_summary(summary.as_dict(), ref.measure(0.1, LUM_FLOOR)[0], "summary after the rejected calls")
        # another size is accepted after a reset, and 2^24 paths are
        cv.reset()
        assert update(total=1 << 24, ww=h, hh=w) == 0
    finally:
        cv.close()
