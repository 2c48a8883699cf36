"""A fast history that overrides the long one where the lighting changed (include/gpuart_antilag.h, libgpuart_antilag.so): the library's
boundary and record, the restatement's (tests/antilag_ref.py) properties and its ledger over the planted cases, the statistic under no
change and what the mix is worth on the oracle's tracks (tests/antilag_tracks.py), the kernel against the restatement bit for bit,
Renderer::SetHistoryAntiLag / ReadGuidedPreview against the chain of restatements, and what they leave alone."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import antilag_ref as A
from tests import antilag_tracks as K
from tests import denoise_ref as D
from tests import moments_ref as M
from tests import refine_ref as R
from tests import temporal_ref as T
from tests.test_denoise import synthetic_gbuffer
from tests.test_moments import LUM_FLOOR, Shadow
from tests.test_temporal import SPHERE, TRACK, cam_dict
from tests.util import assert_same_bits, exported, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
FLOOR = 20                  # every ledger entry over the planted cases (as tests/test_filter_edges.py)
OTHER_LIBS = ("denoise", "temporal", "converge", "refine", "adaptive", "moments", "display")
ENTRY_POINTS = ["gpuart_antilag_" + n for n in ("create", "defaults", "destroy", "finish", "last_error", "mix", "mix_host")]
P_X = dict(fast_history=2.0, min_batches=2.5, min_votes=2.0, clip=1.5, z_lo=0.5, z_hi=2.0)   # a non-default setting
# tools/antilag_quality.py (profiles/antilag.txt, section 1), with the defaults and window 32: per scene and lighting-change track the
# ratio with / without of the guided preview's surface RMSE at the last view (R), and per scene the share of voting pixels with
# alpha > 0 over the 24 views of the static track B.
CPU_RATIO = {("box", "diffuse_fixed"): 0.9995, ("box", "diffuse_moving"): 0.9992, ("box", "emissive"): 0.9288,
             ("scene_p", "diffuse_fixed"): 0.9977, ("scene_p", "diffuse_moving"): 0.9967, ("scene_p", "emissive"): 0.9966}
CPU_FIRED = {"box": 0.00873, "scene_p": 0.01745}


def _declared(name):
    return sorted(set(re.findall(r"\b(gpuart_%s_[a-z_0-9]+)\s*\(" % name, open(os.path.join(ROOT, "include", "gpuart_%s.h" % name)).read())))


# ---- CPU: the library's boundary and its record ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_antilag_library_exports_exactly_its_header(lib):
    assert _declared("antilag") == ENTRY_POINTS
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_antilag.so")
    assert exported(path) == ENTRY_POINTS
    # images alone: the HIP runtime, and neither the renderer's back end nor another image library
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart" not in dyn and "libamdhip64" in dyn, dyn
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    capi = open(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h")).read()
    for n in ("gpuart_renderer_set_history_antilag", "gpuart_renderer_set_user_sphere_pos"):
        assert n in host and re.search(r"\b%s\s*\(" % n, capi), n
    # the other libraries export what their headers declare, as before, and nothing of this one
    for other in OTHER_LIBS:
        names = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % other))
        assert names == _declared(other), other
    assert not [n for n in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so")) if "antilag" in n or "al_mix" in n]


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_antilag_keeps_its_own_last_error(lib):
    libs = {n: C.CDLL(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % n)) for n in ("antilag", "moments", "temporal")}
    for n in libs:
        getattr(libs[n], "gpuart_%s_last_error" % n).restype = C.c_char_p
    last = lambda n: getattr(libs[n], "gpuart_%s_last_error" % n)()
    before = {n: last(n) for n in libs}
    assert libs["antilag"].gpuart_antilag_finish(None) == ERR_ARG and last("antilag") == b"antilag: handle is NULL"
    assert last("moments") == before["moments"] and last("temporal") == before["temporal"]
    assert libs["moments"].gpuart_moments_finish(None) == ERR_ARG and last("antilag") == b"antilag: handle is NULL"


def test_params_record_matches_the_header(tmp_path):
    from gpuart_amd import binding as B
    fields = ("fast_history", "min_batches", "min_votes", "clip", "z_lo", "z_hi")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_antilag.h"\n#define P gpuart_antilag_params\n'
                   'int main(void) { printf("%%zu %s\\n", sizeof(P), %s); return 0; }\n'
                   % (" ".join(["%zu"] * len(fields)), ", ".join("offsetof(P, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    P = B.AntiLagParams
    assert got == [C.sizeof(P)] + [getattr(P, f).offset for f in fields] == [24, 0, 4, 8, 12, 16, 20]
    assert B.ANTILAG_DEFAULTS == A.DEFAULTS and tuple(A.DEFAULTS) == fields
    with pytest.raises(ValueError):
        B.antilag_params(dict(z_lo=2, sigma=1))
    # the defaults the header's text and its function's comment state are the restatement's, and the library's
    hdr = open(os.path.join(ROOT, "include", "gpuart_antilag.h")).read()
    stated = ", ".join("%s %g" % (f, A.DEFAULTS[f]) for f in fields)
    assert hdr.count(stated) == 2, stated
    L = C.CDLL(os.path.join(ROOT, "gpuart_amd", "lib_test", "libgpuart_antilag.so"))
    p = P()
    assert L.gpuart_antilag_defaults(C.byref(p)) == 0 and L.gpuart_antilag_defaults(None) == ERR_ARG
    assert {f: getattr(p, f) for f in fields} == A.DEFAULTS


# ---- CPU: the planted cases and the ledger -----------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 2), (33, 7), (160, 120)] + [(w, h) for w in (15, 16, 17) for h in (15, 16, 17)] + [(w, h) for w in (63, 64, 65) for h in (3, 4, 5)]


def plant(seed, w, h, scale=1.0, params=None, flags=0, same_len=False):
    """A made-up tile -> a case dict. Slow lengths 1..40 with fractions, q 1 or 1/2 (so some B are short), fast lengths capped at 2, 4
    or 8 (a fifth of the pixels keep the slow length), moments around the slow blend's luminance, and a fast blend that is the slow one
    plus noise of the statistic's own standard deviation, with a firefly of ten of them at one pixel in a hundred. In the first rows
    of a tile of 15 columns or more, patches of surface pixels: 12 columns whose variance is exactly 0 and whose fast blend is brighter
    (S2 == 0 with S1 != 0), then (24 columns or more) 12 columns with B == min_batches exactly, lifted by 3.5 standard deviations (clipped, alpha 1), then (33 or more)
    9 columns lifted by one (alpha between 0 and 1). The last twenty rows of a tile of 100 rows or more keep the slow length. same_len: fast_len is slow_len everywhere."""
    rng = np.random.default_rng(seed)
    ap = dict(A.DEFAULTS, **(params or {}))
    words, prims = synthetic_gbuffer(rng, h, w)
    slow = (rng.uniform(0.2, 2, (h, w, 4)) * scale).astype(F)
    sl = (rng.integers(1, 41, (h, w)) + rng.choice([0.0, 0.0, 0.25, 0.5], (h, w))).astype(F)
    q = rng.choice([1.0, 1.0, 1.0, 0.5], (h, w)).astype(F)
    fl = np.minimum(sl, F(rng.choice([2.0, 4.0, 8.0]))).astype(F)
    keep = rng.random((h, w)) < 0.2
    fl[keep] = sl[keep]
    m1 = (D.lum(slow) * rng.uniform(0.8, 1.2, (h, w))).astype(F)
    m2 = (m1 * m1 * rng.uniform(1.05, 1.5, (h, w))).astype(F)
    lift = np.zeros((h, w), F)        # in standard deviations
    gain = np.ones((h, w), F)
    rows = slice(0, min(h, 12))

    def patch(cols, length, fast_length):
        words[rows, cols, 7] = np.int32(1).view(F)
        prims[rows, cols] = 5
        sl[rows, cols], fl[rows, cols], q[rows, cols] = length, fast_length, 1
        return rows, cols

    if w >= 15:
        p = patch(slice(0, 12), 20, 4)
        m2[p] = m1[p] * m1[p]
        gain[p] = 1.25
    if w >= 24:
        lift[patch(slice(12, 24), ap["min_batches"], 2)] = 3.5    # B == min_batches exactly: these vote
    if w >= 33:
        lift[patch(slice(24, 33), 30, 4)] = 1.0
    if h >= 100:
        fl[h - 20:] = sl[h - 20:]     # twenty rows without a voter: windows with few votes or none
    if same_len:
        fl = sl.copy()
    m = np.stack([m1, m2, q, slow[..., 3]], -1).astype(F)
    with np.errstate(all="ignore"):
        _, _, var = A.statistic(slow, sl, slow, fl, m, np.ones((h, w), bool), ap["min_batches"], ap["clip"])
    sd = np.sqrt(np.where(var > 0, var, 0)).astype(F)
    noise = rng.normal(size=(h, w)) + lift + np.where(rng.random((h, w)) < 0.01, 10.0, 0.0)
    fast = slow * gain[..., None]
    fast[..., :3] += (sd * noise)[..., None].astype(F)
    fast[..., 3] = rng.uniform(0, 1, (h, w))
    fast = fast.astype(F)
    out, out_len, alpha, led = A.mix(slow, sl, fast, fl, m, words, prims, flags, want_ledger=True, **ap)
    return dict(name="%d x %d, seed %d, scale %g, %s, flags %d" % (w, h, seed, scale, params, flags), slow=slow, sl=sl, fast=fast, fl=fl, m=m,
                words=words, prims=prims, flags=flags, params=params, out=out, out_len=out_len, alpha=alpha, ledger=led)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [plant(900 + i, w, h, params=P_X if i % 2 else None, flags=D.SPECULAR if i % 3 == 0 else 0) for i, (w, h) in enumerate(SIZES)]
    cs.append(plant(990, 33, 7, scale=2.0 ** -100))    # tiny radiances: var is a denormal or underflows to 0
    cs.append(plant(991, 65, 5, scale=2.0 ** -100, params=P_X))
    return cs


def total_ledger(cs):
    return {k: sum(c["ledger"][k] for c in cs) for k in A.LEDGER_KEYS}


def args_of(c):
    return c["slow"], c["sl"], c["fast"], c["fl"], c["m"], c["words"], c["prims"], c["flags"]


def test_cases_take_every_branch():
    cs = cases()
    assert [c["slow"].shape[1::-1] for c in cs[:len(SIZES)]] == SIZES
    led = total_ledger(cs)
    print(led)
    assert set(led) == set(A.LEDGER_KEYS) and all(v >= FLOOR for v in led.values()), led
    for c in cs:
        surf, _ = D.surface(c["words"], c["prims"], c["flags"])
        assert (c["alpha"][~surf] == 0).all() and (c["alpha"] >= 0).all() and (c["alpha"] <= 1).all(), c["name"]
        # alpha == 0: slow and its len, bit for bit; the alpha channel is slow's everywhere
        keep = c["alpha"] == 0
        assert same_bits(c["out"][keep], c["slow"][keep]) and same_bits(c["out_len"][keep], c["sl"][keep]), c["name"]
        assert same_bits(c["out"][..., 3], c["slow"][..., 3]), c["name"]
        moved = c["alpha"] == 1
        assert np.abs(c["out"][moved][:, :3] - c["fast"][moved][:, :3]).max(initial=0) <= 1e-5 * max(1.0, float(np.abs(c["fast"]).max()))
    # B == min_batches votes: a restatement with ">" in place of ">=" differs
    c = cs[2]
    mb = F(dict(A.DEFAULTS, **(c["params"] or {}))["min_batches"])
    B = c["sl"] * c["m"][..., 2]
    assert ((B == mb) & (c["fl"] < c["sl"])).sum() >= 4
    nudged = A.mix(*args_of(c), **dict(A.DEFAULTS, **(c["params"] or {}), min_batches=np.nextafter(mb, F(99))))
    assert not same_bits(nudged[2], c["alpha"])


def test_equal_lengths_leave_the_slow_history_alone():
    """fast_len == slow_len everywhere: nobody votes, whatever the fast blend holds."""
    for i, (w, h) in enumerate(((33, 7), (65, 5), (160, 120))):
        c = plant(950 + i, w, h, same_len=True, params=P_X if i else None)
        assert c["ledger"]["no_vote_same_len"] > 0 and c["ledger"]["alpha_zero"] + c["ledger"]["not_surface"] == w * h, c["ledger"]
        assert same_bits(c["out"], c["slow"]) and same_bits(c["out_len"], c["sl"]) and (c["alpha"] == 0).all()
        assert not same_bits(c["fast"][..., :3], c["slow"][..., :3])


@pytest.mark.parametrize("n", [-10, 7])
def test_alpha_does_not_depend_on_the_exposure(n):
    """Every radiance times 2^n (the moments' m2 times 2^2n): r scales by 2^n and var by 2^2n exactly, so Z and alpha keep their bits."""
    k = F(2.0 ** n)
    for c in cases()[2:6]:
        m = c["m"] * np.array([k, k * k, 1, 1], F)
        out, out_len, alpha = A.mix(c["slow"] * k, c["sl"], c["fast"] * k, c["fl"], m, c["words"], c["prims"], c["flags"], **dict(A.DEFAULTS, **(c["params"] or {})))
        assert_same_bits(alpha, c["alpha"], c["name"])
        assert_same_bits(out_len, c["out_len"], c["name"])
        assert_same_bits(out[..., :3], c["out"][..., :3] * k, c["name"])
    assert all((c["alpha"] > 0).any() for c in cases()[2:6]) and any((c["alpha"] == 0).any() for c in cases()[2:6])


def test_a_planted_step_is_followed_and_only_there():
    """33 x 33 surface pixels, slow len 32, fast len 4, a small measured variance, fast == slow except for a 9 x 9 patch lifted by many
    standard deviations. Every lifted r is clipped to clip*sd, so a pixel whose window holds k patch pixels among 49 voters has
    Z = k*clip/7: 16*3/7 = 6.86 at the patch's corners (their window holds 4 x 4 of it), more inside. With z_hi 6 alpha is 1 on the
    whole patch; four pixels away the window holds none of it, S1 is 0 and alpha is 0."""
    h = w = 33
    words = np.zeros((h, w, 8), F)
    words[..., 0], words[..., 6] = 2.0, 1.0
    prims = np.zeros((h, w), np.int32)
    slow = np.full((h, w, 4), 0.5, F)
    sl, fl = np.full((h, w), 32, F), np.full((h, w), 4, F)
    m = np.stack([np.full((h, w), 0.5, F), np.full((h, w), 0.25 + 1e-4, F), np.ones((h, w), F), slow[..., 3]], -1)
    fast = slow.copy()
    patch = np.zeros((h, w), bool)
    patch[12:21, 12:21] = True
    fast[patch, :3] += F(0.1)
    out, out_len, alpha = A.mix(slow, sl, fast, fl, m, words, prims, 0, **dict(A.DEFAULTS, clip=3.0, min_votes=8.0, z_lo=2.0, z_hi=6.0))
    assert (alpha[patch] == 1).all()
    far = np.ones((h, w), bool)
    far[9:24, 9:24] = False      # four pixels and more from the patch
    assert far.sum() > 500 and (alpha[far] == 0).all()
    assert np.abs(out[patch][:, :3] - fast[patch][:, :3]).max() < 1e-6 and same_bits(out[far], slow[far])
    assert (out_len[patch] == 4).all() and (out_len[far] == 32).all()


# ---- CPU: the oracle's tracks --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blends(name, track, fast_history=None):
    """(views, the slow chains, the fast chain with the defaults' window) of one oracle track."""
    views = K.track_views(name, track)
    return views, K.slow_chains(views), K.fast_chain(views, A.DEFAULTS["fast_history"] if fast_history is None else fast_history)


def ratio_at(name, track, i):
    views, slow, fast = blends(name, track)
    ref, mask = K.reference(name, track, i), K.surface_mask(views[i])
    return K.rmse(K.preview(views[i], slow[i], fast[i]), ref, mask) / K.rmse(K.preview(views[i], slow[i]), ref, mask)


@pytest.mark.parametrize("name", K.SCENES)
def test_the_statistic_under_no_change(name):
    """The 24 views of the static track B: the share of voting pixels with alpha > 0 at the defaults is at most the share
    tools/antilag_quality.py measured (profiles/antilag.txt, section 1; CPU_FIRED) and a margin of one half of it."""
    views, slow, fast = blends(name, "B")
    votes = fired = 0
    for v, s, f in zip(views, slow, fast):
        _, _, alpha = A.mix(s[0], s[1], f[0], f[1], s[2], v[1], v[2], v[4], **A.DEFAULTS)
        vt, _, _ = A.statistic(s[0], s[1], f[0], f[1], s[2], K.surface_mask(v), A.DEFAULTS["min_batches"], A.DEFAULTS["clip"])
        votes += int(vt.sum())
        fired += int((vt & (alpha > 0)).sum())
    share = fired / votes
    print("%s: %d of %d voting pixels have alpha > 0: %.5f; the tool's %.5f, the bound %.5f" % (name, fired, votes, share, CPU_FIRED[name], 1.5 * CPU_FIRED[name]))
    assert votes > 100000
    assert share <= 1.5 * CPU_FIRED[name], share


@pytest.mark.parametrize("track", sorted(K.CHANGE))
@pytest.mark.parametrize("name", K.SCENES)
def test_the_fast_history_helps_where_the_lighting_changes(name, track):
    """At the last view of each lighting-change track the ratio with / without of the guided preview's surface RMSE against 256 paths
    is at most R + (1 - R)/4, R the ratio tools/antilag_quality.py recorded (CPU_RATIO; tests/test_moments.py's margin)."""
    R_ = CPU_RATIO[(name, track)]
    ratio = ratio_at(name, track, K.N_CHANGE - 1)
    print("%s, %s: with / without %.4f, the tool's %.4f, the bound %.4f" % (name, track, ratio, R_, R_ + (1 - R_) / 4))
    assert ratio <= R_ + (1 - R_) / 4, ratio


@pytest.mark.parametrize("track", sorted(K.STATIC))
@pytest.mark.parametrize("name", K.SCENES)
def test_the_fast_history_costs_nothing_where_the_lighting_is_static(name, track):
    """On the static tracks the ratio is at most 1.02 at every view."""
    ratios = [ratio_at(name, track, i) for i in range(len(K.STATIC[track][0]))]
    print("%s, track %s: with / without per view: %s" % (name, track, " ".join("%.4f" % r for r in ratios)))
    assert max(ratios) <= 1.02, ratios


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def al(B):
    h = B.AntiLag(0)
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
    with binding.phase("tests/test_antilag.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)


def check_mix(al, slow, sl, fast, fl, m, words, prims, flags, params, exp, what):
    """gpuart_antilag_mix_host, and gpuart_antilag_mix on torch tensors into separate buffers and in place, against exp = (out, out_len,
    alpha); the inputs stay as they were."""
    words = np.ascontiguousarray(words).view(F).reshape(slow.shape[:2] + (8,))
    host_in = [a.copy() for a in (slow, sl, fast, fl, m)]
    for got, e, n in zip(al.mix(slow, sl, fast, fl, m, words, prims, flags, params=params), exp, ("out", "out_len", "alpha")):
        assert_same_bits(got, e, "%s, host: %s" % (what, n))
    o, ol = slow.copy(), sl.copy()
    got = al.mix(o, ol, fast, fl, m, words, prims, flags, params=params, out=o, out_len=ol, want_alpha=False)
    assert got[0] is o and got[1] is ol and got[2] is None
    assert_same_bits(o, exp[0], what + ", host in place: out")
    assert_same_bits(ol, exp[1], what + ", host in place: out_len")
    for a, b in zip((slow, sl, fast, fl, m), host_in):
        assert_same_bits(a, b, what + ", host: an input")
    d = [to_device(a) for a in (slow, sl, fast, fl, m, words, prims)]
    for got, e, n in zip(al.mix(*d, flags, params=params), exp, ("out", "out_len", "alpha")):
        assert_same_bits(got.cpu().numpy(), e, "%s, device: %s" % (what, n))
    for a, b in zip(d[:5], (slow, sl, fast, fl, m)):
        assert_same_bits(a.cpu().numpy(), b, what + ", device: an input")
    got = al.mix(*d, flags, params=params, out=d[0], out_len=d[1])
    assert got[0] is d[0] and got[1] is d[1]
    for g, e, n in zip(got, exp, ("out", "out_len", "alpha")):
        assert_same_bits(g.cpu().numpy(), e, "%s, device in place: %s" % (what, n))


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(len(SIZES) + 2))
def test_kernel_equals_the_restatement_on_planted_tiles(al, i):
    cs = cases()
    assert len(cs) == len(SIZES) + 2
    led = total_ledger(cs)
    assert all(v >= FLOOR for v in led.values()), led
    c = cs[i]
    check_mix(al, *args_of(c), c["params"], (c["out"], c["out_len"], c["alpha"]), c["name"])


@pytest.mark.gpu
def test_kernel_equals_the_restatement_on_a_lighting_change_track(al):
    """The box with the diffuse sphere that moves every view (tests/antilag_tracks.py, the oracle's frames): the three chains through
    tests/temporal_ref.py, then mix at every view through both entry points, with the defaults and with another setting."""
    views, slow, fast = blends("box", "diffuse_fixed")
    fast_x = K.fast_chain(views, P_X["fast_history"])
    led = dict.fromkeys(A.LEDGER_KEYS, 0)
    for i, (v, s) in enumerate(zip(views, slow)):
        for params, f in ((None, fast[i]), (P_X, fast_x[i])):
            *exp, l = A.mix(s[0], s[1], f[0], f[1], s[2], v[1], v[2], v[4], want_ledger=True, **dict(A.DEFAULTS, **(params or {})))
            for k in led:
                led[k] += l[k]
            check_mix(al, s[0], s[1], f[0], f[1], s[2], v[1], v[2], v[4], params, exp, "view %d, %s" % (i, params))
    assert led["alpha_one"] > 100 and led["alpha_mid"] > 100 and led["alpha_zero"] > 10000 and led["not_surface"] > 100 and led["clipped"] > 100, led


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65536, 1), (1, 65536)])
def test_the_largest_sides(al, w, h):
    """One row and one column of the largest size: 1024 blocks across, 16384 up; every window is cut by the tile's edge."""
    rng = np.random.default_rng(w)
    words = np.zeros((h, w, 8), F)
    words[..., 7] = np.where(rng.random((h, w)) < 0.1, -1, 1).astype(np.int32).view(F)
    prims = np.zeros((h, w), np.int32)
    slow = rng.uniform(0.2, 2, (h, w, 4)).astype(F)
    fast = (slow * rng.choice([1.0, 1.0, 1.3], (h, w, 1))).astype(F)
    sl = rng.integers(1, 41, (h, w)).astype(F)
    fl = np.minimum(sl, F(4))
    m1 = D.lum(slow)
    m = np.stack([m1, m1 * m1 * F(1.01), np.ones((h, w), F), slow[..., 3]], -1).astype(F)
    p = dict(min_votes=3.0, z_lo=0.5, z_hi=2.0)
    *exp, led = A.mix(slow, sl, fast, fl, m, words, prims, 0, want_ledger=True, **dict(A.DEFAULTS, **p))
    assert min(led[k] for k in ("alpha_zero", "alpha_mid", "alpha_one", "few_votes", "not_surface", "win_outside")) > 100, led
    for got, e, n in zip(al.mix(slow, sl, fast, fl, m, words, prims, 0, params=p), exp, ("out", "out_len", "alpha")):
        assert_same_bits(got, e, n)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_one_handle_grows_and_shrinks(B, entry):
    """1 x 1, then 65 x 5 (every buffer allocated again behind the first call's work), then 1 x 1 in buffers larger than it needs; the
    device calls in place, so that the handle's copy grows and shrinks with them."""
    to = to_device if entry == "device" else (lambda a: a.copy())
    back = (lambda a: a.cpu().numpy()) if entry == "device" else (lambda a: a)
    handle = B.AntiLag(0)
    try:
        for i, (w, h) in enumerate([(1, 1), (65, 5), (1, 1)]):
            c = plant(970 + i, w, h, params=P_X)
            d = [to(a) for a in args_of(c)[:7]]
            got = handle.mix(*d, c["flags"], params=P_X, out=d[0], out_len=d[1])
            for g, e, n in zip(got, (c["out"], c["out_len"], c["alpha"]), ("out", "out_len", "alpha")):
                assert_same_bits(back(g), e, "%s, call %d (%d x %d): %s" % (entry, i, w, h, n))
    finally:
        handle.close()


@pytest.mark.gpu
def test_argument_errors(al, B):
    """Every ERR_ARG case returns the error with its message and writes nothing."""
    import torch
    L = al.L
    h, w = 4, 4
    n = h * w
    mk4 = lambda: np.ones((n + 1, 4), F)
    slow, fast, m, out = mk4(), mk4(), mk4(), np.full((n + 1, 4), 7.0, F)
    sl, fl, ol, alpha = np.ones(n + 2, F), np.ones(n + 2, F), np.full(n + 2, 7.0, F), np.full(n + 2, 7.0, F)
    hits = np.zeros((n + 1, 8), F)
    prims = np.zeros(n + 2, np.int32)
    ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
    par = lambda **kw: C.byref(B.AntiLagParams(**dict(A.DEFAULTS, **kw)))
    good = dict(slow=ptr(slow), sl=ptr(sl), fast=ptr(fast), fl=ptr(fl), m=ptr(m), hits=ptr(hits), prims=ptr(prims), w=w, h=h, p=None, out=ptr(out),
                ol=ptr(ol), alpha=ptr(alpha))

    def call(fn, handle=None, **kw):
        a = dict(good, **kw)
        return getattr(L, fn)(handle if handle is not None else al.h, a["slow"], a["sl"], a["fast"], a["fl"], a["m"], a["hits"], a["prims"], C.c_uint32(0),
                              C.c_uint32(a["w"]), C.c_uint32(a["h"]), a["p"], a["out"], a["ol"], a["alpha"])

    def expect(fn, cases_, base=None):
        for kw, msg in cases_:
            rc = call(fn, **dict(base or {}, **kw))
            assert rc == ERR_ARG and msg in L.gpuart_antilag_last_error().decode(), (kw, msg, rc, L.gpuart_antilag_last_error())

    nan, inf = float("nan"), float("inf")
    before = [a.copy() for a in (slow, sl, fast, fl, m, hits, prims)]
    expect("gpuart_antilag_mix_host",
           [(dict(**{k: None}), "NULL") for k in ("slow", "sl", "fast", "fl", "m", "hits", "prims", "out", "ol")] +
           [(dict(slow=ptr(slow, 2)), "misaligned"), (dict(fast=ptr(fast, 1)), "misaligned"), (dict(m=ptr(m, 2)), "misaligned"),
            (dict(hits=ptr(hits, 2)), "misaligned"), (dict(sl=ptr(sl, 2)), "misaligned"), (dict(fl=ptr(fl, 1)), "misaligned"),
            (dict(prims=ptr(prims, 2)), "misaligned"), (dict(out=ptr(out, 2)), "misaligned"), (dict(ol=ptr(ol, 2)), "misaligned"),
            (dict(alpha=ptr(alpha, 2)), "misaligned"), (dict(w=0), "bad size"), (dict(h=0), "bad size"), (dict(w=65537), "bad size"),
            (dict(h=65537), "bad size"),
            (dict(p=par(fast_history=-1.0)), "fast_history"), (dict(p=par(fast_history=nan)), "fast_history"), (dict(p=par(fast_history=inf)), "fast_history"),
            (dict(p=par(min_batches=1.0)), "min_batches"), (dict(p=par(min_batches=nan)), "min_batches"), (dict(p=par(min_batches=inf)), "min_batches"),
            (dict(p=par(min_votes=0.5)), "min_votes"), (dict(p=par(min_votes=nan)), "min_votes"), (dict(p=par(min_votes=inf)), "min_votes"),
            (dict(p=par(clip=0.0)), "clip"), (dict(p=par(clip=nan)), "clip"), (dict(p=par(clip=inf)), "clip"),
            (dict(p=par(z_lo=-1.0)), "z_lo"), (dict(p=par(z_lo=nan)), "z_lo"), (dict(p=par(z_lo=inf)), "z_lo"),
            (dict(p=par(z_lo=2.0, z_hi=2.0)), "z_hi"), (dict(p=par(z_hi=nan)), "z_hi"), (dict(p=par(z_hi=inf)), "z_hi"),
            (dict(out=ptr(slow, 16)), "overlaps an input"), (dict(out=ptr(fast)), "overlaps an input"), (dict(out=ptr(m, 16)), "overlaps an input"),
            (dict(out=ptr(hits, 32)), "overlaps an input"), (dict(out=ptr(sl)), "overlaps an input"), (dict(out=ptr(prims, 4)), "overlaps an input"),
            (dict(ol=ptr(sl, 4)), "overlaps an input"), (dict(ol=ptr(fl)), "overlaps an input"), (dict(ol=ptr(slow)), "overlaps an input"),
            (dict(ol=ptr(prims)), "overlaps an input"), (dict(alpha=ptr(sl)), "overlaps an input"), (dict(alpha=ptr(fl, 4)), "overlaps an input"),
            (dict(alpha=ptr(slow, 16)), "overlaps an input"), (dict(alpha=ptr(hits)), "overlaps an input"),
            (dict(alpha=ptr(ol, 4)), "another output"), (dict(ol=ptr(out, 16)), "another output"), (dict(alpha=ptr(out)), "another output"),
            (dict(out=ptr(slow), alpha=ptr(slow, 16)), "overlaps")])   # (in place, alpha inside slow: an input and an output)
    dev = [torch.zeros(n * 8 + 8, device="cuda:0") for _ in range(10)]
    dp = lambda t, k=0: C.c_void_p(t.data_ptr() + k)
    dgood = dict(slow=dp(dev[0]), sl=dp(dev[1]), fast=dp(dev[2]), fl=dp(dev[3]), m=dp(dev[4]), hits=dp(dev[5]), prims=dp(dev[6]), out=dp(dev[7]),
                 ol=dp(dev[8]), alpha=dp(dev[9]))
    expect("gpuart_antilag_mix",
           [(dict(slow=dp(dev[0], 4)), "misaligned"), (dict(fast=dp(dev[2], 8)), "misaligned"), (dict(m=dp(dev[4], 4)), "misaligned"),
            (dict(hits=dp(dev[5], 8)), "misaligned"), (dict(out=dp(dev[7], 4)), "misaligned"), (dict(sl=dp(dev[1], 2)), "misaligned"),
            (dict(alpha=dp(dev[9], 1)), "misaligned"), (dict(out=dp(dev[0], 32)), "overlaps an input"), (dict(ol=dp(dev[1], 8)), "overlaps an input"),
            (dict(alpha=dp(dev[8], 4)), "another output"), (dict(w=0), "bad size"), (dict(p=par(clip=-1.0)), "clip"), (dict(slow=None), "NULL")], dgood)
    assert call("gpuart_antilag_mix_host", handle=C.c_void_p(None)) == ERR_ARG and "handle" in L.gpuart_antilag_last_error().decode()
    assert L.gpuart_antilag_finish(None) == ERR_ARG and L.gpuart_antilag_defaults(None) == ERR_ARG and L.gpuart_antilag_create(C.c_int(0), None) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ol == 7.0).all() and (alpha == 7.0).all() and all((d == 0).all() for d in dev)
    for a, b in zip((slow, sl, fast, fl, m, hits, prims), before):
        assert (a == b).all()
    # ... and the good calls write their tile and nothing beyond it (all-zero records are type 0: surface pixels); alpha may be NULL
    assert call("gpuart_antilag_mix_host") == 0 and same_bits(out[:n], slow[:n]) and (out[n] == 7.0).all() and (ol[:n] == 1).all() and (ol[n:] == 7.0).all()
    assert (alpha[:n] == 0).all() and (alpha[n:] == 7.0).all()
    alpha[:] = 7.0
    assert call("gpuart_antilag_mix_host", alpha=None) == 0 and (alpha == 7.0).all()
    assert call("gpuart_antilag_mix_host", out=ptr(slow), ol=ptr(sl)) == 0    # the in-place pair
    # the Renderer: parameters out of range change nothing
    r = B.Renderer(16, 8, cam_dict(TRACK[0]))
    try:
        for bad in (dict(min_batches=1.0), dict(z_lo=3.0, z_hi=3.0), dict(fast_history=-1.0), dict(clip=0.0), dict(min_votes=0.0), dict(z_lo=float("nan"))):
            with pytest.raises(ValueError):
                r.set_history_antilag(True, bad)
        with pytest.raises(ValueError):
            r.set_history_antilag(True, dict(z_lo=2, sigma=1))
        r.set_temporal_history(True)
        assert r.read_guided_preview(LUM_FLOOR) is None   # (set_history_variance is still off: anti-lag alone has no effect)
    finally:
        r.close()


# ---- GPU: the Renderer ---------------------------------------------------------------------------------------------------------------
class Shadow3(Shadow):
    """tests/test_moments.py's Shadow with the third history: the restatements' side of a Renderer with all three switches on."""

    def __init__(self, B, r, temporal=None, moments=None, antilag=None):
        super().__init__(B, r, temporal, moments)
        self.ap = dict(A.DEFAULTS, **(antilag or {}))
        self.hf = None
        self.fired = 0

    def _fast(self, tp):
        return dict(tp, max_history=min(self.ap["fast_history"], tp["max_history"]))

    def commit(self, cam, spp):
        rgba, hits, prims, v, _ = self._inputs(cam)
        _, _, self.hx = T.accumulate(self.hx, rgba, spp, hits, prims, v, **self.tp)
        _, _, self.hm = T.accumulate(self.hm, M.pack(rgba, spp), spp, hits, prims, v, **self.tp)
        _, _, self.hf = T.accumulate(self.hf, rgba, spp, hits, prims, v, **self._fast(self.tp))

    def drop(self):
        self.hx = self.hm = self.hf = None

    def preview(self, cam, spp, refine=None, temporal=None, want_len=False):
        rgba, hits, prims, v, flags = self._inputs(cam)
        tp = dict(self.tp, **(temporal or {}))
        x, ln, _ = T.accumulate(self.hx, rgba, spp, hits, prims, v, **tp)
        m, _, _ = T.accumulate(self.hm, M.pack(rgba, spp), spp, hits, prims, v, **tp)
        f, fl, _ = T.accumulate(self.hf, rgba, spp, hits, prims, v, **self._fast(tp))
        x, ln, alpha = A.mix(x, ln, f, fl, m, hits, prims, flags, **self.ap)
        self.fired = int((alpha > 0).sum())
        e = M.error(x, ln, m, hits, prims, LUM_FLOOR, flags, **self.mp)
        out = R.refine(x, hits, prims, e, LUM_FLOOR, flags, **dict(R.DEFAULTS, **(refine or {})))
        return (out, ln) if want_len else out


VIEWS = 10
P_TRACK = dict(fast_history=2.0, min_batches=3.0, min_votes=4.0, clip=3.0, z_lo=1.0, z_hi=3.0)   # ten views are short: B reaches 8 only at the end
P_LEAVE = dict(P_TRACK, min_batches=2.0, z_lo=0.25, z_hi=1.0)   # three views of twelve paths: B is 3


def moving_sphere(i):
    return K.sphere_at(i)[:3]


def run_track(B, antilag, guided_at=range(VIEWS), shadow=False):
    """The box at 160 x 120, one path per view, window 32, a diffuse user sphere that moves before every view and a camera that moves
    before every second one -> read_guided_preview per view (and, with shadow, the chain of restatements' frames and its counts of
    pixels with alpha > 0). antilag: None (the switch off) or the parameters."""
    cams = [cam_dict((0.10 + 0.02 * (i // 2), -3.05, 1.0)) for i in range(VIEWS)]
    tparams = dict(max_history=K.WINDOW)
    r = B.Renderer(K.W, K.H, cams[0])
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(moving_sphere(0), 0.25)
        r.set_temporal_history(True, tparams)
        r.set_history_variance(True)
        if antilag is not None:
            r.set_history_antilag(True, antilag)
        sh = Shadow3(B, r, tparams, antilag=antilag) if shadow else None
        r.restart_path_tracing(1, 1)
        got, exp, fired = [], [], []
        for i in range(VIEWS):
            if i:
                if sh:
                    sh.commit(cams[i - 1], 1)
                if i % 2 == 0:
                    r.set_camera(cams[i])          # commits the view; the move below finds no path rendered and commits nothing
                r.set_user_sphere_pos(moving_sphere(i))
            assert r.path_tracing_pass() == 1
            if i in guided_at:
                got.append(r.read_guided_preview(LUM_FLOOR))
                if sh:
                    exp.append(sh.preview(cams[i], 1))
                    fired.append(sh.fired)
        return got, exp, fired
    finally:
        r.close()


@pytest.mark.gpu
def test_read_guided_preview_equals_the_chain_of_restatements(B):
    """Ten views of the moving diffuse sphere on the box: read_guided_preview with anti-lag on equals temporal (slow), moments, temporal
    (fast), mix, error and refine of the restatements over the renderer's own accumulators and G-buffers, bit for bit, at every view;
    the mix moves pixels from the fourth view on. A fast_history at or above the window gives exactly the bits of the switch off."""
    got, exp, fired = run_track(B, P_TRACK, shadow=True)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert_same_bits(g, e, "view %d" % i)
    assert fired[0] == 0 and min(fired[4:]) > 50, fired
    off, _, _ = run_track(B, None)
    assert not same_bits(got[-1], off[-1])
    for fh in (K.WINDOW, 2 * K.WINDOW):
        same, _, _ = run_track(B, dict(P_TRACK, fast_history=fh))
        for i, (g, e) in enumerate(zip(same, off)):
            assert_same_bits(g, e, "fast_history %g, view %d" % (fh, i))


@pytest.mark.gpu
def test_the_switch_and_the_history(B):
    """Toggling the switch drops the history: a history the third handle has not seen, or one it saw while the others went on, is never
    blended; the next preview is the chain's without history (len = s everywhere), and the commits that follow build all three again.
    Other parameters, the window of the fast history included, reach the mix without a toggle and keep the history. Without
    set_history_variance the switch has no effect."""
    W, H = 96, 64
    cams = [cam_dict(p) for p in TRACK]
    r = B.Renderer(W, H, cams[0])
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(SPHERE[:3], SPHERE[3])
        r.set_temporal_history(True)
        r.set_history_variance(True)
        r.restart_path_tracing(1, 2)

        def view(cam):
            r.set_camera(cam)
            r.path_tracing_pass(); r.path_tracing_pass()

        r.path_tracing_pass(); r.path_tracing_pass()
        view(cams[1])                                            # commits the radiance and the moments
        two = Shadow(B, r)
        assert not same_bits(r.read_preview(), r.read_denoised())
        r.set_history_antilag(True, P_TRACK)                     # drops that history
        assert_same_bits(r.read_preview(), r.read_denoised(), "the switch dropped the history")
        sh = Shadow3(B, r, antilag=P_TRACK)
        exp, ln = sh.preview(cams[1], 2, want_len=True)
        assert ln.max() == 2
        assert_same_bits(r.read_guided_preview(LUM_FLOOR), exp, "after switching on: no history")
        for k in (2, 3, 0, 1):
            sh.commit(cams[(k - 1) % 4], 2)
            view(cams[k])
        exp, ln = sh.preview(cams[1], 2, want_len=True)
        assert sh.fired > 0 and ln.max() > 4
        got = r.read_guided_preview(LUM_FLOOR)
        assert_same_bits(got, exp, "all three histories committed")
        two.hx, two.hm = sh.hx, sh.hm
        assert not same_bits(got, two.preview(cams[1], 2))       # (the third history matters)
        other = dict(P_TRACK, fast_history=3.0, z_lo=0.25)
        r.set_history_antilag(True, other)                       # (no toggle: the histories stay)
        sh.ap = dict(A.DEFAULTS, **other)
        assert_same_bits(r.read_guided_preview(LUM_FLOOR), sh.preview(cams[1], 2), "other parameters, same histories")
        r.set_history_antilag(False)                             # drops all three
        assert_same_bits(r.read_preview(), r.read_denoised(), "switching off dropped the history")
        two.drop()
        assert_same_bits(r.read_guided_preview(LUM_FLOOR), two.preview(cams[1], 2), "off: today's sequence without history")
        two.commit(cams[1], 2)
        view(cams[2])
        assert_same_bits(r.read_guided_preview(LUM_FLOOR), two.preview(cams[2], 2), "off: today's sequence")
        r.set_history_variance(False)
        r.set_history_antilag(True)                              # without the variance: no effect but the drop
        assert r.read_guided_preview(LUM_FLOOR) is None
        assert_same_bits(r.read_preview(), r.read_denoised(), "switching on dropped the history")
        view(cams[3])
        assert not same_bits(r.read_preview(), r.read_denoised())
    finally:
        r.close()


P_SEAM = dict(P_TRACK, fast_history=3.0)
FAILING_COMMIT = r"""
import ctypes, os, sys
shim = ctypes.CDLL(sys.argv[1], mode=ctypes.RTLD_GLOBAL)      # before anything loads libgpuart.so: its calls of accumulate bind here
from gpuart_amd import binding as B
from tests.test_antilag import LUM_FLOOR, P_SEAM, SPHERE, TRACK, Shadow3, cam_dict
from tests.util import assert_same_bits, same_bits, scene
n = int(sys.argv[2])
cams = [cam_dict(p) for p in TRACK]
r = B.Renderer(96, 64, cams[0])
r.set_primitives(scene("box"))
r.set_user_sphere(SPHERE[:3], SPHERE[3])
r.set_temporal_history(True, dict(max_history=32.0))
r.set_history_variance(True)
r.set_history_antilag(True, P_SEAM)
r.restart_path_tracing(1, 2)
sh = Shadow3(B, r, dict(max_history=32.0), antilag=P_SEAM)

def view(cam):
    r.set_camera(cam)
    r.path_tracing_pass(); r.path_tracing_pass()

def three_views(what):
    for k in (1, 2, 3):
        sh.commit(cams[k - 1], 2)
        view(cams[k])
    exp, ln = sh.preview(cams[3], 2, want_len=True)
    assert sh.fired > 0 and ln.max() > 4, (what, sh.fired, float(ln.max()))
    assert_same_bits(r.read_guided_preview(LUM_FLOOR), exp, what)
    assert not same_bits(r.read_preview(), r.read_denoised()), what

r.path_tracing_pass(); r.path_tracing_pass()
three_views("three commits to all three histories")
assert shim.temporal_fail_failed() == 0 and shim.temporal_fail_passed_on() >= 9       # (the Renderer's calls do come through here)
shim.temporal_fail_after(n)          # of the commit that follows (radiance, moments, fast) the n-th fails
view(cams[0])
assert shim.temporal_fail_failed() == 1
sh.drop()                            # all three: none keeps a history the others have lost
assert_same_bits(r.read_preview(), r.read_denoised(), "a failed commit leaves no history")
exp, ln = sh.preview(cams[0], 2, want_len=True)
assert ln.max() == 2
assert_same_bits(r.read_guided_preview(LUM_FLOOR), exp, "after the failed commit: the chain without history")
three_views("the three histories grow again together")    # (a fast history that had survived would be longer than the chain's here)
assert shim.temporal_fail_failed() == 1
r.close()
print("failing commit %d: OK" % n)
"""


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 2])
def test_a_failed_commit_drops_all_three_histories(tmp_path, n):
    """Renderer::CommitTemporalView with the three switches on, in a child process in which tests/stubs/temporal_fail.c stands between
    libgpuart.so and libgpuart_temporal.so (the product has no hook: the stand-in is loaded with RTLD_GLOBAL before libgpuart.so, so the
    Renderer's gpuart_temporal_accumulate binds to it): after three good commits the n-th accumulate of the next commit fails, 3 = the
    fast history's, 2 = the moments'. Then read_preview is read_denoised, the guided preview is the chain of restatements without
    history (len = s everywhere), and after three more commits it is the chain's that dropped all three there, bit for bit, with
    pixels the mix moved: a handle that had kept its history would blend views the chain has forgotten."""
    import sys
    from gpuart_amd import binding
    so = str(tmp_path / "libtemporal_fail.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-O1", "-o", so, os.path.join(ROOT, "tests", "stubs", "temporal_fail.c"), "-ldl"], check=True)
    env = dict(os.environ, GPUART_TEMPORAL_REAL=os.path.join(binding.LIBDIR, "libgpuart_temporal.so"), GPUART_LIBDIR=binding.LIBDIR)
    res = subprocess.run([sys.executable, "-c", FAILING_COMMIT, so, str(n)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and ("failing commit %d: OK" % n) in res.stdout, (res.returncode, res.stdout[-2000:], res.stderr[-4000:])
    assert "committing" in res.stderr     # (the Renderer said which commit failed)


@pytest.mark.gpu
def test_antilag_leaves_everything_else_alone(B):
    """With the three switches on and guided reads among the passes, against a run with anti-lag off: the accumulator, the counters,
    the number of timed launches, RenderUntil's summaries and error map, read_denoised (its cached G-buffer), read_preview, read_refined
    and the 8-bit frames of the other sources are the same (tests/test_moments.py's
    test_guided_reads_and_the_switch_leave_everything_else_alone, one switch further)."""
    W, H = 96, 64
    cams = [cam_dict(p) for p in TRACK]

    def run(antilag):
        r = B.Renderer(W, H, cams[0])
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
            r.set_temporal_history(True)
            r.set_history_variance(True)
            if antilag:
                r.set_history_antilag(True, P_LEAVE)
            r.backend.set_mode(4)
            res = []
            for i, cam in enumerate(cams[:3]):
                if i:
                    r.set_camera(cam)
                r.restart_path_tracing(1, 12)
                for k in range(4):
                    r.path_tracing_pass()
                    if k in (0, 3):   # (a read between passes ends a planned run: both runs read at the same points)
                        assert r.read_guided_preview(LUM_FLOOR) is not None
                res += [r.read_radiance(False), r.read_preview(), r.read_denoised(), r.read_display("preview", dict(auto_exposure=1))]
            converged, s1 = r.render_until(1e30, 0.0, 4, LUM_FLOOR)
            assert converged and s1["total"] == 8 and s1["batches"] == 2
            assert r.read_guided_preview(LUM_FLOOR) is not None and r.read_display("guided_preview") is not None
            res += [r.read_refined(LUM_FLOOR), r.read_error_map(LUM_FLOOR)]
            converged, s2 = r.render_until(0.0, 0.0, 4, LUM_FLOOR)
            assert not converged and s2["total"] == 12 and s2["batches"] == 3
            res += [r.read_radiance(False), r.read_refined(LUM_FLOOR), r.read_error_map(LUM_FLOOR), r.read_preview(), r.read_denoised(),
                    r.read_display("denoised", dict(auto_exposure=1))]
            return res, (r.backend.counters().as_dict(), r.backend.kernel_time(0)[1], s1, s2), r.read_guided_preview(LUM_FLOOR)
        finally:
            r.close()

    (a, sa, ga), (b, sb, gb) = run(False), run(True)
    assert sa == sb, (sa, sb)
    assert len(a) == len(b)
    for k, (p, q) in enumerate(zip(a, b)):
        assert_same_bits(q, p, "result %d" % k)
    assert not same_bits(ga, gb)   # (and the guided preview itself does follow the third history)


@pytest.mark.gpu
@pytest.mark.parametrize("name_of_track", ["diffuse_fixed", "emissive"])
def test_the_gpu_reproduces_the_cpu_ratio(B, name_of_track):
    """The box with the camera fixed and a user sphere that moves every view, diffuse and emissive (tests/antilag_tracks.py, 16 views,
    seed 1234, window 32, the defaults): at the last view, against one pass of 256 paths of seed 2, read_guided_preview's surface RMSE
    with anti-lag over the one without is at most R + (1 - R)/4, R the CPU's ratio (CPU_RATIO). The GPU's frames equal the oracle's
    and the kernels their restatements, so the GPU reproduces the CPU's ratio, here to the four decimals it is recorded with; read_display follows by itself."""
    xs, spheres, em, flags = K.CHANGE[name_of_track]
    cam = K.cam_of(xs[0])
    r = B.Renderer(K.W, K.H, cam)
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(spheres[-1][:3], spheres[-1][3], emittance=em)
        r.set_seed(2)
        r.restart_path_tracing(256, 256)
        assert r.path_tracing_pass() == 256
        ref = r.read_radiance(True)
        y, x = np.divmod(np.arange(K.W * K.H), K.W)
        hits, prims = r.pick(np.stack([x, y], 1), want_prims=True)
        mask = ((hits["type"] >= 0) & ~((prims == -2) & bool(flags))).reshape(K.H, K.W)

        def track(antilag):
            r.set_seed(1234)
            r.set_user_sphere(spheres[0][:3], spheres[0][3], emittance=em)
            r.set_temporal_history(True, dict(max_history=K.WINDOW))
            r.set_history_variance(True)
            r.set_history_antilag(antilag)
            r.restart_path_tracing(1, 1)
            for i in range(len(xs)):
                if i:
                    r.set_user_sphere_pos(spheres[i][:3])
                assert r.path_tracing_pass() == 1
            out = r.read_guided_preview(LUM_FLOOR), r.read_display("guided_preview")
            r.set_temporal_history(False)
            return out

        (without, d0), (with_, d1) = track(False), track(True)
        ratio = K.rmse(with_, ref, mask) / K.rmse(without, ref, mask)
        R_ = CPU_RATIO[("box", name_of_track)]
        print("box, %s: with / without %.6f on the GPU, %.4f on the CPU, the bound %.4f" % (name_of_track, ratio, R_, R_ + (1 - R_) / 4))
        assert ratio <= R_ + (1 - R_) / 4, ratio
        assert abs(ratio - R_) <= 1e-4, (ratio, R_)    # the same arithmetic on the same frames; R is recorded to four decimals
        assert d0 is not None and d1 is not None and (d0 != d1).any()
    finally:
        r.close()
