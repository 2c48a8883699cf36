"""The firefly clamp (include/gpuart_despeckle.h, libgpuart_despeckle.so): the argument checks, the NumPy restatement
(tests/despeckle_ref.py) against a second statement in plain loops, its ledger over the planted cases (tests/despeckle_cases.py), its
properties and its quality on the CPU oracle; on the GPU gpuart_despeckle_run and _run_host against the restatement, bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import denoise_ref as D
from tests import despeckle_cases as P
from tests import despeckle_ref as DS
from tests.util import assert_same_bits, exported, same_bits, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
FLOOR = 20   # every ledger entry over the planted cases (as tests/test_moments.py)
ENTRY_POINTS = ["gpuart_despeckle_" + n for n in ("create", "defaults", "destroy", "finish", "last_error", "read_summary", "run", "run_host")]
# R = clamped-then-denoised over denoised surface RMSE that tools/despeckle_quality.py measured with the defaults on scene P with the
# radius-0.1, emittance-30 sphere (profiles/despeckle.txt), by paths per pixel
CPU_RATIO = {1: 0.3582, 4: 0.4960}


# ---- CPU: the library's surface ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_library_exports_exactly_its_header(lib):
    header = open(os.path.join(ROOT, "include", "gpuart_despeckle.h")).read()
    assert sorted(set(re.findall(r"\b(gpuart_despeckle_[a-z_0-9]+)\s*\(", header))) == ENTRY_POINTS
    assert exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_despeckle.so")) == ENTRY_POINTS
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    for name in ("set_firefly_clamp", "get_firefly_clamp", "read_firefly_summary"):
        assert "gpuart_renderer_" + name in host
    for other in ("hip", "denoise", "temporal", "converge", "refine", "adaptive", "moments", "display", "antilag", "edges"):
        assert not [s for s in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % other)) if "despeckle" in s or "firefly" in s]


def test_defaults_and_the_record():
    from gpuart_amd import binding as B
    L = B.despeckle_lib()
    p = B.DespeckleParams()
    assert L.gpuart_despeckle_defaults(C.byref(p)) == 0
    got = dict(radius=p.radius, rank=p.rank, k=p.k, floor=p.floor, min_count=p.min_count)
    assert got == dict(DS.DEFAULTS, floor=float(F(1e-3))) and B.DESPECKLE_DEFAULTS == DS.DEFAULTS
    assert C.sizeof(B.DespeckleParams) == 20 and C.sizeof(B.DespeckleSummary) == 24
    assert L.gpuart_despeckle_defaults(None) == ERR_ARG and "params is NULL" in L.gpuart_despeckle_last_error().decode()
    with pytest.raises(ValueError):
        B.despeckle_params(dict(sigma=1))


def test_parameter_and_argument_errors_need_no_device():
    """Every check but the handle's is made before the handle is looked at: without a device (a NULL handle) each field out of range
    names the field, and NULL pointers, misaligned pointers, sizes beyond 65536 and partial overlap are refused; nothing is written."""
    from gpuart_amd import binding as B
    L = B.despeckle_lib()
    h, w = 4, 4
    n = h * w
    rgba = np.ones((2 * n + 1, 4), np.float32)
    hits = np.zeros((n + 1, 8), np.float32)
    prims = np.zeros(n + 2, np.int32)
    out = np.full((n + 1, 4), 7.0, np.float32)
    scale = np.full(n + 2, 7.0, np.float32)
    assert all(a.ctypes.data % 16 == 0 for a in (rgba, hits, out))
    ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
    good = dict(rgba=ptr(rgba), hits=ptr(hits), prims=ptr(prims), w=w, h=h, p=None, out=ptr(out), scale=ptr(scale))
    par = lambda **kw: C.byref(B.despeckle_params(kw))

    def call(fn, **kw):
        a = dict(good, **kw)
        rc = getattr(L, fn)(None, a["rgba"], a["hits"], a["prims"], C.c_uint32(0), C.c_uint32(a["w"]), C.c_uint32(a["h"]), a["p"], a["out"], a["scale"])
        return rc, L.gpuart_despeckle_last_error().decode()

    fields = [(dict(radius=0), "radius"), (dict(radius=3), "radius"), (dict(rank=0), "rank"), (dict(rank=5), "rank"), (dict(k=0.5), "k must"),
              (dict(k=float("inf")), "k must"), (dict(k=float("nan")), "k must"), (dict(floor=-1e-9), "floor"), (dict(floor=float("inf")), "floor"),
              (dict(floor=float("nan")), "floor"), (dict(min_count=0), "min_count"), (dict(min_count=25), "min_count")]
    args = [(dict(rgba=None), "NULL"), (dict(hits=None), "NULL"), (dict(prims=None), "NULL"), (dict(out=None), "NULL"), (dict(w=0), "bad size"),
            (dict(h=0), "bad size"), (dict(w=65537), "bad size"), (dict(h=65537), "bad size"), (dict(prims=ptr(prims, 2)), "misaligned"),
            (dict(scale=ptr(scale, 1)), "misaligned")]
    dev_args = [(dict(rgba=ptr(rgba, 4)), "misaligned"), (dict(hits=ptr(hits, 8)), "misaligned"), (dict(out=ptr(out, 4)), "misaligned"),
                (dict(out=ptr(rgba, 16)), "overlaps"), (dict(rgba=ptr(rgba, n * 16), out=ptr(rgba, n * 16 - 16)), "overlaps"),
                (dict(scale=ptr(rgba, 32)), "scale overlaps"), (dict(scale=ptr(out, 16)), "scale overlaps")]
    host_args = [(dict(rgba=ptr(rgba, 2)), "misaligned"), (dict(out=ptr(out, 1)), "misaligned"), (dict(out=ptr(rgba, 4)), "overlaps")]
    for fn in ("gpuart_despeckle_run", "gpuart_despeckle_run_host"):
        for kw, msg in fields:
            rc, said = call(fn, p=par(**kw))
            assert rc == ERR_ARG and said.startswith("despeckle: ") and msg in said, (fn, kw, rc, said)
        for kw, msg in args + (dev_args if fn.endswith("run") else host_args):
            rc, said = call(fn, **kw)
            assert rc == ERR_ARG and msg in said, (fn, kw, rc, said)
        # a bad field is named even where a pointer is bad too; with everything else in order the handle is what is missing
        rc, said = call(fn, p=par(rank=9), rgba=None)
        assert rc == ERR_ARG and "rank" in said
        rc, said = call(fn)
        assert rc == ERR_ARG and "handle is NULL" in said
        rc, said = call(fn, out=good["rgba"])   # in place is no overlap error
        assert rc == ERR_ARG and "handle is NULL" in said
    assert L.gpuart_despeckle_read_summary(None, None) == ERR_ARG and L.gpuart_despeckle_finish(None) == ERR_ARG
    assert L.gpuart_despeckle_create(C.c_int(0), None) == ERR_ARG and L.gpuart_despeckle_destroy(None) == 0
    assert (out == 7.0).all() and (scale == 7.0).all() and (rgba == 1.0).all()


# ---- CPU: the restatement against a second statement -----------------------------------------------------------------------------------
def lum1(x):
    return (F(0.2126) * x[0] + F(0.7152) * x[1]) + F(0.0722) * x[2]


def loop_clamp(rgba, words, prims, flags, radius, rank, k, floor, min_count):
    """The header again, pixel by pixel in plain loops, sharing nothing with tests/despeckle_ref.py but the colour table:
    -> (out, scale, summary, cnt (h, w), ref (h, w))."""
    h, w = rgba.shape[:2]
    t = words[..., 7].view(np.int32)
    out, scale = rgba.copy(), np.ones((h, w), np.float32)
    cnts, refs = np.zeros((h, w), np.int32), np.full((h, w), np.nan, np.float32)
    summary = dict(surface=0, clamped=0, too_few=0)

    def surf(y, x):
        return t[y, x] >= 0 and not (prims[y, x] == -2 and flags & 3)

    def demod(y, x):
        a = D.PRIMITIVE_COLOR[t[y, x] & 3]
        v = np.array([rgba[y, x, j] / a[j] for j in range(3)], np.float32)
        return v, a

    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if not surf(y, x):
                    continue
                summary["surface"] += 1
                vals = []
                for dy in range(-radius, radius + 1):
                    for dx in range(-radius, radius + 1):
                        qy, qx = y + dy, x + dx
                        if (dy == 0 and dx == 0) or not (0 <= qy < h and 0 <= qx < w) or not surf(qy, qx):
                            continue
                        Lq = lum1(demod(qy, qx)[0])
                        if Lq == Lq:
                            vals.append(Lq)
                cnts[y, x] = len(vals)
                if len(vals) < max(min_count, rank):
                    summary["too_few"] += 1
                    continue
                for _ in range(rank - 1):          # strike the largest rank - 1 times: the rank-th largest is then the largest
                    vals.remove(max(vals))
                ref = max(vals)
                refs[y, x] = ref
                cap = F(F(k) * ref) + F(floor)
                v, a = demod(y, x)
                L = lum1(v)
                if L > cap:
                    summary["clamped"] += 1
                    s = cap / L
                    scale[y, x] = s
                    for j in range(3):
                        out[y, x, j] = F(v[j] * s) * a[j]
    return out, scale, summary, cnts, refs


def small_frame(seed, levels=None, sky=0.35, zeros=False):
    """A 9 x 7 frame: much sky (neighbour counts of every size), a user-sphere pixel or two, and, with `levels`, radiance from that
    many values and one type (ties at every rank); with `zeros` most of it black."""
    rng = np.random.default_rng(seed)
    h, w = 7, 9
    t = rng.integers(0, 4, (h, w)).astype(np.int32) if levels is None else np.full((h, w), 2, np.int32)
    t[rng.random((h, w)) < sky] = -1
    prims = rng.integers(0, 50, (h, w)).astype(np.int32)
    us = (rng.random((h, w)) < 0.05) & (t >= 0)
    t[us], prims[us] = 0, -2
    rgba = rng.uniform(0.05, 1.0, (h, w, 4)).astype(np.float32)
    if levels is not None:
        rgba[..., :3] = (rng.integers(1, levels + 1, (h, w, 1)) * F(0.25)).astype(np.float32)
    if zeros:
        rgba[rng.random((h, w)) < 0.7, :3] = 0
    hot = rng.random((h, w)) < 0.15
    rgba[hot, :3] *= F(40)
    rgba[0, 0, :3] = rgba[h - 1, w - 1, :3] = F(30)      # corners
    rgba[0, w // 2, :3] = rgba[h // 2, 0, :3] = F(30)    # borders
    words = np.zeros((h, w, 8), np.float32)
    words[..., 7] = t.view(np.float32)
    return rgba, words, prims


def test_restatement_equals_a_second_statement_in_loops():
    """Every rank and radius on 9 x 7 frames: random ones, ones with ties at the rank, black ones with floor = 0 (ref = 0, cap = 0).
    Among them are windows with exactly max(min_count, rank) - 1 and exactly that many valid neighbours, clamped corner and border
    pixels, and a ref that ties with its neighbours in the order."""
    seen = dict(below=0, at=0, corner=0, border=0, tied=0, ref_zero=0, flagged=0)
    for radius in (1, 2):
        for rank in (1, 2, 3, 4):
            for seed, kw, params in ((1, {}, {}), (2, dict(levels=3), {}), (3, dict(zeros=True, sky=0.1), dict(floor=0.0)),
                                     (4, dict(sky=0.6), dict(min_count=1)), (5, dict(levels=2, sky=0.2), dict(k=1.0, min_count=6))):
                for flags in (0, D.EM_NONZERO):
                    rgba, words, prims = small_frame(10 * seed + rank, **kw)
                    p = dict(DS.DEFAULTS, radius=radius, rank=rank, **params)
                    out, scale, summary, led = DS.clamp(rgba, words, prims, flags, want_ledger=True, **p)
                    exp_out, exp_scale, exp_summary, cnt, ref = loop_clamp(rgba, words, prims, flags, **p)
                    what = "radius %d rank %d seed %d flags %d" % (radius, rank, seed, flags)
                    assert_same_bits(out, exp_out, what)
                    assert_same_bits(scale, exp_scale, what + ", scale")
                    assert summary == exp_summary, what
                    need = max(p["min_count"], rank)
                    surf = D.surface(words, prims, flags)[0]
                    hit = scale != 1
                    seen["below"] += int((surf & (cnt == need - 1)).sum())
                    seen["at"] += int((surf & (cnt == need)).sum())
                    seen["corner"] += int(hit[0, 0]) + int(hit[-1, -1])
                    seen["border"] += int(hit[0, 4]) + int(hit[3, 0])
                    seen["tied"] += led["ref_tied"]
                    seen["ref_zero"] += int((surf & (ref == 0) & (cnt >= need)).sum()) if p["floor"] == 0 else 0
                    seen["flagged"] += int(((prims == -2) & ~surf).sum())
    assert min(seen.values()) >= 8, seen


# ---- CPU: the ledger and the properties --------------------------------------------------------------------------------------------
def test_cases_take_every_branch():
    """Over the planted cases every ledger key reaches the floor, the ledger adds up, and the summary is the ledger's counts."""
    total = dict.fromkeys(DS.LEDGER_KEYS, 0)
    for i, (what, rgba, words, prims, flags, params) in enumerate(P.cases()):
        _, _, summary, led = P.expected(i)
        for key in DS.LEDGER_KEYS:
            total[key] += led[key]
        h, w = prims.shape
        assert led["not_surface"] + led["too_few"] + led["not_above_cap"] + led["clamped"] == h * w, what
        assert summary == dict(surface=h * w - led["not_surface"], clamped=led["clamped"], too_few=led["too_few"]), what
        assert led["neighbour_outside"] + led["neighbour_invalid"] <= summary["surface"] * len(DS.offsets(params["radius"])), what
    assert min(total.values()) >= FLOOR, total
    assert {p["radius"] for *_, p in P.cases()} == {1, 2} and {p["rank"] for *_, p in P.cases()} == {1, 2, 3, 4}


def test_properties():
    """Unclamped pixels are the input bit for bit (alpha everywhere); a frame with no pixel above its cap comes back whole; no channel of
    a clamped pixel exceeds the input's; k = 1e30 is the identity wherever no ref is 0; with floor = 0, radiance scaled by 2^n gives the output scaled by 2^n."""
    for i, (what, rgba, words, prims, flags, params) in enumerate(P.cases()):
        out, scale, summary, _ = P.expected(i)
        hit = scale != 1
        assert int(hit.sum()) == summary["clamped"] > 0, what
        assert same_bits(out[~hit], rgba[~hit]) and same_bits(out[..., 3], rgba[..., 3]), what
        assert (out[hit][:, :3] <= rgba[hit][:, :3]).all() and (scale[hit] < 1).all() and (scale[hit] >= 0).all(), what
        assert (out[hit][:, :3] < rgba[hit][:, :3]).any(1).all(), what
        surf = D.surface(words, prims, flags)[0]
        assert not hit[~surf].any(), what
        lit = np.where(rgba == 0, F(0.01), rgba)   # (where ref = 0 the cap is the floor, whatever k is)
        again = DS.clamp(lit, words, prims, flags, **dict(params, k=1e30))
        assert same_bits(again[0], lit) and (again[1] == 1).all() and again[2]["clamped"] == 0, what
        # a frame whose demodulated radiance is 0.25 everywhere (but for the NaN pixels) has no pixel above a cap of at least twice that
        smooth = rgba.copy()
        smooth[..., :3] = np.where(np.isnan(rgba[..., :3]), np.nan, F(0.25) * D.PRIMITIVE_COLOR[words[..., 7].view(np.int32) & 3])
        whole = DS.clamp(smooth, words, prims, flags, **dict(params, k=max(params["k"], 2.0)))
        assert same_bits(whole[0], smooth) and whole[2]["clamped"] == 0, what
        for n in (-3, 5):
            p0 = dict(params, floor=0.0)
            a = DS.clamp(rgba, words, prims, flags, **p0)
            b = DS.clamp(rgba * F(2.0 ** n), words, prims, flags, **p0)
            assert same_bits(b[0][..., :3], a[0][..., :3] * F(2.0 ** n)) and same_bits(a[1], b[1]) and a[2] == b[2], (what, n)


# ---- CPU: quality on the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paths", [1, 4])
def test_the_clamp_helps_the_denoised_frame_where_fireflies_are(paths):
    """Scene P with the radius-0.1, emittance-30 sphere, 160 x 120: the surface RMSE of the clamped, then denoised frame over that of the
    denoised frame, both against the oracle's 1024-path reference, is at most r + (1 - r)/4, r the ratio tools/despeckle_quality.py
    measured with the defaults (tests/test_edges.py's rule: a quarter of the gain is the margin a seed change may use)."""
    r = CPU_RATIO[paths]
    got = P.ratio("scene_p_firefly", paths)
    _, summary = P.clamped_error("scene_p_firefly", paths)
    print("%d paths: clamped / plain = %.4f (recorded %.4f, bound %.4f); %s" % (paths, got, r, r + (1 - r) / 4, summary))
    assert got <= r + (1 - r) / 4, (got, r)
    assert 0 < summary["clamped"] < 0.05 * summary["surface"], summary


@pytest.mark.parametrize("name", ["scene_p", "box"])
@pytest.mark.parametrize("paths", [1, 64])
def test_the_clamp_is_neutral_where_none_are(name, paths):
    """The two scenes without a sphere: the same ratio is at most 1.02, the project's "within 2 %"."""
    got = P.ratio(name, paths)
    _, summary = P.clamped_error(name, paths)
    print("%s, %d paths: clamped / plain = %.4f; %s" % (name, paths, got, summary))
    assert got <= 1.02, got


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def ds(B):
    h = B.Despeckle(0)
    yield h
    h.close()


@pytest.fixture(autouse=True)
def bounded(request):
    """Every GPU test of this file runs as one phase of the library's watchdog (gpuart_hip_phase_begin): a test that hangs ends the
    process after two minutes instead of waiting for ever."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    from gpuart_amd import binding
    was = binding.phase_log(False)
    with binding.phase("tests/test_despeckle.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)


def check(ds, rgba, words, prims, flags, params, exp, what):
    """gpuart_despeckle_run_host, and gpuart_despeckle_run with separate buffers and in place, against `exp` = (out, scale, summary):
    out, scale and the three counts, bit for bit; the inputs stay as they were."""
    keep = rgba.copy()
    out, scale = ds.run_host(rgba, words, prims, flags, params, want_scale=True)
    assert_same_bits(out, exp[0], what + ": run_host")
    assert_same_bits(scale, exp[1], what + ": run_host, scale")
    assert ds.summary() == exp[2], what
    assert same_bits(rgba, keep)
    d_rgba, d_words, d_prims = to_device(rgba), to_device(words), to_device(prims)
    out, scale = ds.run(d_rgba, d_words, d_prims, flags, params, want_scale=True)
    assert_same_bits(out.cpu().numpy(), exp[0], what + ": run")
    assert_same_bits(scale.cpu().numpy(), exp[1], what + ": run, scale")
    assert ds.summary() == exp[2], what
    assert same_bits(d_rgba.cpu().numpy(), keep)
    assert ds.run(d_rgba, d_words, d_prims, flags, params, out=d_rgba) is d_rgba
    assert_same_bits(d_rgba.cpu().numpy(), exp[0], what + ": run in place")
    assert ds.summary() == exp[2], what + ": in place"


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(P.cases())))
def test_kernel_equals_the_restatement_on_the_planted_cases(ds, i):
    """The ledger's case set: both radii, every rank, the three user-sphere flags."""
    what, rgba, words, prims, flags, params = P.cases()[i]
    check(ds, rgba, words, prims, flags, params, P.expected(i)[:3], what)


SEAMS = (15, 16, 17, 31, 32, 33)   # one below, at and one above the block and two blocks: the apron's seams
SIZES = [(1, 1), (1, 64), (64, 1)] + [(w, h) for w in SEAMS for h in SEAMS]


@pytest.mark.gpu
@pytest.mark.parametrize("radius", [1, 2])
def test_kernel_equals_the_restatement_at_the_seams(ds, radius):
    for k, (w, h) in enumerate(SIZES):
        rgba, words, prims = P.plant(300 + k, w, h)
        params = dict(DS.DEFAULTS, radius=radius, rank=1 + k % 4, min_count=1 + k % 3)
        check(ds, rgba, words, prims, 0, params, DS.clamp(rgba, words, prims, 0, **params), "%d x %d" % (w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65536, 1), (1, 65536)])
def test_kernel_equals_the_restatement_at_the_limit_shapes(ds, w, h):
    rgba, words, prims = P.plant(11, w, h)
    exp = DS.clamp(rgba, words, prims, 0, **dict(DS.DEFAULTS, radius=2, min_count=3))   # (four neighbours at most)
    assert exp[2]["clamped"] > 100 and exp[2]["too_few"] > 100, exp[2]
    check(ds, rgba, words, prims, 0, dict(radius=2, min_count=3), exp, "%d x %d" % (w, h))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_one_handle_grows_and_the_summary_is_per_run(B, entry):
    """A smaller, then a larger frame through one fresh handle: the staging memory regrows, and the counts are the last run's alone."""
    h = B.Despeckle(0)
    try:
        assert h.summary() == dict(surface=0, clamped=0, too_few=0)
        for k, (w, hh) in enumerate(((19, 9), (64, 48), (19, 9))):
            rgba, words, prims = P.plant(40 + k, w, hh)
            exp = DS.clamp(rgba, words, prims, 0, **DS.DEFAULTS)
            if entry == "host":
                out = h.run_host(rgba, words, prims)
            else:
                t = to_device(rgba)
                out = h.run(t, to_device(words), to_device(prims), out=t).cpu().numpy()   # in place: through the handle's memory
            assert_same_bits(out, exp[0], "%s, run %d" % (entry, k))
            assert h.summary() == exp[2], (entry, k)
    finally:
        h.close()


@pytest.mark.gpu
def test_argument_errors_write_nothing_on_the_device(ds, B):
    import torch
    L = ds.L
    n = 16
    dev = [torch.zeros(n * 8 + 8, device="cuda:0") for _ in range(4)]
    dp = lambda t, k=0: C.c_void_p(t.data_ptr() + k)
    good = dict(rgba=dp(dev[0]), hits=dp(dev[1]), prims=dp(dev[2]), out=dp(dev[3]), scale=None, p=None, w=4, h=4)

    def call(**kw):
        a = dict(good, **kw)
        rc = L.gpuart_despeckle_run(ds.h, a["rgba"], a["hits"], a["prims"], C.c_uint32(0), C.c_uint32(a["w"]), C.c_uint32(a["h"]), a["p"], a["out"], a["scale"])
        return rc, L.gpuart_despeckle_last_error().decode()

    for kw, msg in ((dict(rgba=dp(dev[0], 4)), "misaligned"), (dict(out=dp(dev[0], 16)), "overlaps"), (dict(scale=dp(dev[3], 4)), "scale overlaps"),
                    (dict(w=65537), "bad size"), (dict(p=C.byref(B.despeckle_params(dict(k=0.0)))), "k must"), (dict(hits=None), "NULL")):
        rc, said = call(**kw)
        assert rc == ERR_ARG and msg in said, (kw, rc, said)
    torch.cuda.synchronize()
    assert all((d == 0).all() for d in dev)
    assert call()[0] == 0    # all-zero records are type 0: surface pixels with zero radiance, nothing to clamp
    ds.finish()
    assert ds.summary() == dict(surface=16, clamped=0, too_few=4) and (dev[3] == 0).all()   # (a corner has three neighbours of min_count 4)
