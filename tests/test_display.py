"""The display stage (include/gpuart_display.h, libgpuart_display.so): the library's boundary, the sRGB table, the restatement
(tests/display_ref.py) against gpuart_cli --ppm's formula, against the correctly rounded sRGB code and against the properties the
exposure and the dither are built for, the parameter checks; on the GPU the kernels against the restatement bit for bit — codes,
histogram and gain — Renderer::ReadDisplay against the restatement of every Read*, what it leaves alone, and gpuart_cli --display."""
import ctypes as C
import functools
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import display_ref as R
from tests.test_temporal import SPHERE, TRACK, cam_dict
from tests.util import default_camera, exported, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
ORIGIN = (3, 5)   # non-zero and odd
ALL = dict(auto_exposure=1, curve=R.REINHARD, transfer=R.SRGB, dither=1, gain=1.5)   # every stage at once
IMAGE_LIBS = ("denoise", "temporal", "converge", "refine", "adaptive", "moments", "display")


@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


def assert_same_bytes(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == np.uint8 and got.shape == exp.shape, (what, got.dtype, got.shape, exp.shape)
    bad = (got != exp).any(-1)
    assert not bad.any(), "%s: %d of %d pixels differ; first %d: got %s expected %s" % (
        what, int(bad.sum()), bad.size, int(np.argmax(bad)), got[bad][0], exp[bad][0])


def assert_state(got, exp, what):
    assert got["histogram"] == exp["histogram"], (what, [(b, g, e) for b, (g, e) in enumerate(zip(got["histogram"], exp["histogram"])) if g != e])
    assert (got["counted"], got["skipped"], got["valid"]) == (exp["counted"], exp["skipped"], exp["valid"]), (what, got["counted"], got["skipped"], got["valid"])
    assert F(got["gain"]).view(np.uint32) == F(exp["gain"]).view(np.uint32), (what, got["gain"], exp["gain"])


def seeded(rng, h, w, lo=1e-6, hi=1e4):
    """Radiance log-uniform over lo..hi, every channel of its own."""
    img = np.exp(rng.uniform(np.log(lo), np.log(hi), (h, w, 4))).astype(np.float32)
    img[..., 3] = rng.random((h, w), np.float32)
    return img


# ---- CPU: the library's boundary -----------------------------------------------------------------------------------------------
def _declared():
    return sorted(set(re.findall(r"\b(gpuart_display_[a-z_0-9]+)\s*\(", open(os.path.join(ROOT, "include", "gpuart_display.h")).read())))


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_display_library_exports_exactly_its_header(lib):
    names = _declared()
    assert len(names) == 10, names
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_display.so")
    assert exported(path) == names
    # images alone: the HIP runtime, and neither the renderer's back end nor another image library
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart" not in dyn and "libamdhip64" in dyn, dyn
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    capi = open(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h")).read()
    assert "gpuart_renderer_read_display" in host and re.search(r"\bgpuart_renderer_read_display\s*\(", capi)
    for other in ("hip",) + IMAGE_LIBS[:-1]:
        assert not [n for n in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % other)) if "display" in n], other


def test_params_record_is_the_headers(B, tmp_path):
    """binding.DisplayParams and DisplayState against what a C compiler makes of the header; the library's defaults are the binding's
    and the restatement's."""
    fields = [f for f, _ in B.DisplayParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_display.h"\nint main(void) { printf("%%zu %%zu %s\\n", '
                   'sizeof(gpuart_display_params), sizeof(gpuart_display_state), %s); return 0; }\n'
                   % (" ".join(["%zu"] * len(fields)), ", ".join("offsetof(gpuart_display_params, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(B.DisplayParams), C.sizeof(B.DisplayState)] + [getattr(B.DisplayParams, f).offset for f in fields]
    p = B.DisplayParams()
    assert B.display_lib().gpuart_display_defaults(C.byref(p)) == 0
    assert {f: getattr(p, f) for f in fields} == {f: (F(v) if isinstance(v, float) else v) for f, v in B.DISPLAY_DEFAULTS.items()}
    assert B.DISPLAY_DEFAULTS == R.DEFAULTS


# ---- CPU: the table and the restatement ----------------------------------------------------------------------------------------
def test_srgb_table_is_the_restatements(B):
    E, ref = B.srgb_table(), R.srgb_table()
    assert E.dtype == np.float32 and same_bits(E, ref)
    assert (np.diff(E) > 0).all() and E[0] == 0 and E[255] == 1
    # (the table's own definition: the nearest fp32 to the float64 inverse, which inverts the forward function)
    fwd = np.where(ref.astype(np.float64) <= 0.0031308, 12.92 * ref.astype(np.float64), 1.055 * ref.astype(np.float64) ** (1 / 2.4) - 0.055)
    assert np.abs(fwd * 255 - np.arange(256)).max() < 1e-4


def _image(values):
    """values as the red channel of a one-row image."""
    img = np.zeros((1, len(values), 4), np.float32)
    img[0, :, 0] = values
    return img


def test_defaults_are_the_clis_bytes():
    """With the defaults the restatement is std::lround(clamp(v)*255.0f) of gpuart_cli --ppm, on 2 M seeded values and at the half-way
    cases."""
    rng = np.random.default_rng(20)
    half = F(0.5 / 255)
    halves = [F((k + 0.5) / 255) for k in range(255)]
    v = np.concatenate([rng.random(1_000_000, np.float32) * F(1.25) - F(0.125), np.exp(rng.uniform(np.log(1e-6), np.log(2.0), 1_000_000)).astype(np.float32),
                        np.array([half, np.nextafter(half, F(0)), np.nextafter(half, F(1)), 0, -0.0, 1, np.nextafter(F(1), F(0)), 1.5, 1e30, -1, -1e-30,
                                  np.nan, np.inf, -np.inf], np.float32),
                        np.array(halves, np.float32), np.nextafter(np.array(halves, np.float32), F(0)), np.nextafter(np.array(halves, np.float32), F(1))])
    got = R.encode(_image(v))[0, :, 0]
    assert (got == R.cli_bytes(v)).all()
    k, frac = R.parts(np.clip(np.nan_to_num(v, nan=0.0), 0, 1).astype(np.float32))
    assert int((frac == F(0.5)).sum()) >= 10   # (exact half-way cases are among them)


def test_srgb_code_against_the_correctly_rounded_one():
    """On a seeded sample, uniform and log-uniform over 1e-5..1, the table's code is at most one from the correctly rounded float64 code,
    and differs for at most 0.5 % (measured with this definition: 0.12 %)."""
    rng = np.random.default_rng(21)
    y = np.concatenate([rng.random(500_000, np.float32), np.exp(rng.uniform(np.log(1e-5), 0.0, 500_000)).astype(np.float32)])
    y = np.minimum(y, F(1))
    got = R.encode(_image(y), transfer=R.SRGB)[0, :, 0].astype(np.int64)
    y64 = y.astype(np.float64)
    true = np.floor(255.0 * np.where(y64 <= 0.0031308, 12.92 * y64, 1.055 * y64 ** (1 / 2.4) - 0.055) + 0.5).astype(np.int64)
    d = np.abs(got - true)
    share = float((d != 0).mean())
    print("sRGB: %.4f %% of %d codes differ from the correctly rounded one, by at most %d" % (100 * share, y.size, d.max()))
    assert d.max() <= 1 and share <= 0.005


@pytest.mark.parametrize("transfer", [R.LINEAR, R.SRGB])
def test_dither_keeps_the_mean(transfer):
    """A constant patch, 64 values of frac: the mean code over an 8x8 cell is k + frac within 1/64, at any origin."""
    assert sorted(R.B8.ravel()) == list(range(64))
    qx, qy = np.meshgrid(np.arange(8), np.arange(8))
    q = qx ^ qy   # the matrix is the bits of x ^ y and of y, interleaved and reversed: what the kernel computes
    assert (R.B8 == ((q & 1) << 5 | (qy & 1) << 4 | (q & 2) << 2 | (qy & 2) << 1 | (q & 4) >> 1 | (qy & 4) >> 2)).all()
    E = R.srgb_table()
    for j in range(64):
        kk = 3 + 3 * j
        y = F(E[kk] + (E[kk + 1] - E[kk]) * F(j / 64)) if transfer else F((kk + j / 64) / 255)
        k, frac = R.parts(y, transfer)
        assert kk - 1 <= k <= kk
        img = np.full((8, 8, 4), y, np.float32)
        for origin in ((0, 0), ORIGIN):
            mean = R.encode(img, transfer=transfer, dither=1, origin=origin)[..., :3].astype(np.float64).mean()
            assert abs(mean - (int(k) + float(frac))) <= 1 / 64, (j, origin, mean, k, frac)


# ---- CPU: the exposure -----------------------------------------------------------------------------------------------------------
def test_exposure_scales_exactly_with_powers_of_two():
    """Scaling every radiance by 2^n moves every pixel by 4n bins. With Nw a power of two (2048 pixels, lo_share 0.5, hi_share 0:
    Nw = 1024) S/Nw, m and f are exact, so the target is scaled by exactly 2^-n; no clamp acts."""
    img = seeded(np.random.default_rng(22), 32, 64, 1e-3, 1e2)
    h0, skipped = R.histogram(img)
    assert skipped == 0 and sum(h0) == 2048 and R.window(h0, 0.5, 0.0)[2] == 1024
    t0 = R.target_gain(h0, 0.18, 0.5, 0.0)
    for n in range(-3, 4):
        h, _ = R.histogram(img * F(2.0 ** n))
        assert h == ([0] * 256 + h0 + [0] * 256)[256 - 4 * n:512 - 4 * n]
        t = R.target_gain(h, 0.18, 0.5, 0.0)
        assert t == t0 * 2.0 ** -n and 2.0 ** -16 < t < 2.0 ** 16, (n, t, t0)


def test_exposure_window_cuts_inside_bins():
    """lo_share and hi_share that start and end the window inside a bin, against the numbers worked out by hand."""
    img = np.zeros((1, 20, 4), np.float32)
    img[0, :10, :3] = F(1.1 * 2.0 ** -7)    # bin 100: 2^-7 .. 2^-6.75
    img[0, 10:, :3] = F(1.1 * 2.0 ** -2)    # bin 120
    h, skipped = R.histogram(img)
    assert skipped == 0 and h[100] == 10 and h[120] == 10 and sum(h) == 20
    t, S, Nw = R.window(h, 0.25, 0.25)
    assert (t[100], t[120], S, Nw) == (5, 5, 5 * 201 + 5 * 241, 10)
    # m = 2210/10/8 - 32 = -4.375: i = -5, f = 0.625
    assert R.target_gain(h, 0.18, 0.25, 0.25) == float(F(0.18)) / (1.625 * 2.0 ** -5)
    t, S, Nw = R.window(h, 0.5, 0.0)
    assert (t[100], t[120], Nw) == (0, 10, 10)
    t, S, Nw = R.window(h, 0.0, 0.75)
    assert (t[100], t[120], Nw) == (5, 0, 5)
    # the clamps
    assert R.target_gain(h, 0.18, 0.25, 0.25, min_gain=100.0) == 100.0 and R.target_gain(h, 0.18, 0.25, 0.25, max_gain=0.5) == 0.5


def test_exposure_state_over_calls():
    """Nothing counted leaves the word alone; the first counted frame takes its target whole; adapt below 1 moves a part of the way;
    reset forgets."""
    rng = np.random.default_rng(23)
    frames = [seeded(rng, 8, 8, 1e-2, 1e1) * F(s) for s in (1.0, 8.0, 0.25)]
    targets = [R.target_gain(R.histogram(f)[0]) for f in frames]
    d = R.Display()
    black = np.zeros((4, 4, 4), np.float32)
    black[0, 0, 0], black[0, 1, 1], black[1, 1, 2] = np.nan, -1.0, np.inf
    out = d.run(black, auto_exposure=1, adapt=0.25)
    s = d.state()
    assert (s["counted"], s["skipped"], s["gain"], s["valid"]) == (0, 16, 1.0, 0) and (out[..., :3] == np.where(np.isinf(black[..., :3]), 255, 0)).all()
    g = None
    for f, t in zip(frames, targets):
        d.run(f, auto_exposure=1, adapt=0.25)
        g = F(t) if g is None else F(float(g) + (t - float(g)) * 0.25)
        assert d.state()["gain"] == g and d.state()["valid"] == 1
    assert not F(targets[2]) == g   # (the gain lags its target)
    d.run(black, auto_exposure=1, adapt=0.25)
    assert d.state()["gain"] == g and d.state()["valid"] == 1 and d.state()["counted"] == 0
    d.reset()
    assert d.state()["gain"] == 1 and d.state()["valid"] == 0
    d.run(frames[0], auto_exposure=1, adapt=0.25)
    assert d.state()["gain"] == F(targets[0])
    # without auto_exposure the word is neither used nor changed
    assert (d.run(frames[1], gain=2.0) == R.encode(frames[1], 2.0)).all() and d.state()["gain"] == F(targets[0])


BAD_PARAMS = [("gain", 0.0), ("gain", -1.0), ("gain", np.inf), ("gain", np.nan), ("auto_exposure", 2), ("key", 0.0), ("key", np.nan),
              ("lo_share", -1e-6), ("hi_share", -1e-6), ("lo_share", np.nan), ("hi_share", 0.5), ("adapt", 0.0), ("adapt", float(np.nextafter(F(1), F(2)))),
              ("adapt", np.nan), ("min_gain", 0.0), ("min_gain", np.inf), ("max_gain", float(np.nextafter(F(2.0 ** -16), F(0)))), ("max_gain", np.inf),
              ("curve", 3), ("white", 0.0), ("white", np.inf), ("transfer", 2), ("dither", 2)]


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_parameter_checks(B, field, value):
    """Each field just outside its range: the argument error, a message that begins "display:" and names the field. The parameters are
    checked before the handle, so no device is needed; the same call with the defaults gets as far as the handle."""
    L = B.display_lib()
    rgba, out = np.ones((2, 2, 4), np.float32), np.full((2, 2, 4), 7, np.uint8)
    p = B.display_params({field: value})
    for fn in (L.gpuart_display_run, L.gpuart_display_run_host):
        args = [None, rgba.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(2), C.c_uint32(2), C.c_uint32(0), C.c_uint32(0)]
        assert fn(*args, C.byref(p)) == ERR_ARG
        msg = L.gpuart_display_last_error().decode()
        assert msg.startswith("display: ") and field in msg, msg
        assert fn(*args, C.byref(B.display_params({}))) == ERR_ARG and L.gpuart_display_last_error() == b"display: handle is NULL"
        assert fn(*args, None) == ERR_ARG and L.gpuart_display_last_error() == b"display: handle is NULL"
    assert (out == 7).all()
    assert L.gpuart_display_defaults(None) == ERR_ARG and L.gpuart_display_srgb_table(None) == ERR_ARG
    for fn in (L.gpuart_display_reset, L.gpuart_display_finish):
        assert fn(None) == ERR_ARG and L.gpuart_display_last_error() == b"display: handle is NULL"


# ---- GPU: the kernels against the restatement --------------------------------------------------------------------------------------
def _torch_first():
    import torch
    torch.cuda.init()


@pytest.fixture(scope="module")
def torch_first_in_module():
    _torch_first()


@pytest.fixture(autouse=True)
def torch_first(request):
    """torch brings a HIP runtime of its own beside the one the libraries link. Run by itself, this file would otherwise give the device
    to the libraries' runtime first, and torch then finds no GPU: every GPU test lets torch find it first (in the whole suite an
    earlier file has done so)."""
    if request.node.get_closest_marker("gpu") is not None:
        _torch_first()


@pytest.fixture(scope="module")
def handles(B, torch_first_in_module):
    hs = {"host": B.Display(0), "device": B.Display(0)}
    yield hs
    for h in hs.values():
        h.close()


def run_entry(handle, entry, img, params, origin=ORIGIN):
    if entry == "device":
        return handle.run(to_device(img), params, origin).cpu().numpy()
    return handle.run(img, params, origin)


SIZES = [(1, 1), (63, 3), (64, 4), (65, 5), (257, 9), (65536, 1), (1, 65536)]
# past the histogram's capped grid (256 blocks of 1024 threads, a stride of 262 144 pixels): the cap alone, the 4-way unrolled body for
# some threads only (the others take three tail turns), for every thread once with a tail turn for some or for all, and twice;
# test_sizes_reach_the_histograms_loops has the counts
BIG_SIZES = [(513, 512), (887, 887), (1049, 1000), (1283, 1025), (1537, 1537)]
UNCOUNTABLE = (np.nan, np.inf, -1.0, 0.0)


def uncountable_pixels(n, stride=262144):
    """The flat indices at which a frame of n pixels (past one stride) gets a pixel the histogram skips: eight in the first 1024, eight
    around every multiple of the stride and eight in the last 1024, so that both of the histogram's loops meet them at both ends of
    the grid."""
    idx = [0, 1, 2, 3, 511, 1020, 1022, 1023]
    for m in range(stride, n, stride):
        idx += list(range(m - 4, m + 4))
    idx += [n - 1024, n - 1023, n - 1022, n - 1021, n - 4, n - 3, n - 2, n - 1]
    assert len(set(idx)) == len(idx) and 0 <= min(idx) and max(idx) == n - 1
    return np.array(idx)


def plant_uncountable(img):
    """NaN, +inf, -1 and 0 in turn, in all three channels, at uncountable_pixels -> how many were planted."""
    rgb = img[..., :3].reshape(-1, 3)   # (a view)
    idx = uncountable_pixels(rgb.shape[0])
    rgb[idx] = np.array(UNCOUNTABLE, np.float32)[np.arange(idx.size) % 4][:, None]
    return idx.size


@functools.lru_cache(maxsize=None)
def sized_case(w, h):
    img = seeded(np.random.default_rng(100 + w + h), h, w)
    planted = plant_uncountable(img) if (w, h) in BIG_SIZES else 0
    d = R.Display()
    out = d.run(img, ORIGIN, **ALL)
    assert d.state()["skipped"] == planted and d.state()["counted"] == w * h - planted
    return img, out, d.state()


@functools.lru_cache(maxsize=None)
def flat_case():
    """1283 x 1025 of 0.3: every wave of the unrolled body falls into one bin."""
    img = np.full((1025, 1283, 4), 0.3, np.float32)
    d = R.Display()
    out = d.run(img, ORIGIN, **ALL)
    assert max(d.state()["histogram"]) == 1283 * 1025
    return img, out, d.state()


def hist_constants():
    """(HIST_THREADS, HIST_UNROLL, the default DP_HIST_MAX_BLOCKS) as gpuart_amd/csrc/display/display.hip has them."""
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "display", "display.hip")).read()
    out = []
    for pattern in (r"\bHIST_THREADS\s*=\s*(\d+)", r"\bHIST_UNROLL\s*=\s*(\d+)", r"#define\s+DP_HIST_MAX_BLOCKS\s+(\d+)"):
        found = re.findall(pattern, src)
        assert len(found) == 1, (pattern, found)
        out.append(int(found[0]))
    return tuple(out)


def hist_walk(n, t, threads, unroll, max_blocks):
    """k_dp_histogram's two loops for thread t of the grid over n pixels -> (blocks wanted, blocks launched, unrolled passes, tail turns)."""
    want = (n + threads - 1) // threads
    grid = min(want, max_blocks)
    stride = grid * threads
    i, passes, tail = t, 0, 0
    while i + (unroll - 1) * stride < n:
        i, passes = i + unroll * stride, passes + 1
    while i < n:
        i, tail = i + stride, tail + 1
    return want, grid, passes, tail


def test_sizes_reach_the_histograms_loops():
    """(CPU) what test_sizes' shapes are for, computed from the constants of display.hip: a grid below the cap, a capped grid without
    an unrolled pass, exactly one unrolled pass, two, no tail turn and three or more; the figures of each of BIG_SIZES; and the planted
    pixels lie in the first and the last block's share of both loops."""
    threads, unroll, max_blocks = hist_constants()
    walk = {}
    for w, h in SIZES + BIG_SIZES:
        n = w * h
        grid = min((n + threads - 1) // threads, max_blocks)
        walk[w, h] = [hist_walk(n, t, threads, unroll, max_blocks) for t in (0, grid * threads - 1)]
    print(walk)
    every = [v for pair in walk.values() for v in pair]
    assert any(want <= max_blocks for want, _, _, _ in every)
    assert any(want > max_blocks and passes == 0 for want, _, passes, _ in every)
    assert any(passes == 1 for _, _, passes, _ in every) and any(passes >= 2 for _, _, passes, _ in every)
    assert any(tail == 0 for _, _, _, tail in every) and any(tail >= 3 for _, _, _, tail in every)
    assert all(want <= max_blocks and passes == 0 for (w, h) in SIZES for want, _, passes, _ in walk[w, h])   # (the gap this closes)
    assert walk[513, 512] == [(257, 256, 0, 2), (257, 256, 0, 1)]
    assert walk[887, 887] == [(769, 256, 1, 0), (769, 256, 0, 3)]
    assert walk[1049, 1000] == [(1025, 256, 1, 1), (1025, 256, 1, 0)]
    assert walk[1283, 1025] == [(1285, 256, 1, 2), (1285, 256, 1, 1)]
    assert walk[1537, 1537] == [(2308, 256, 2, 2), (2308, 256, 2, 1)]
    # 337 threads of 887 x 887 take the unrolled body (five waves and 17 lanes of a sixth) and the others three tail turns, 424 threads
    # of 1049 x 1000 a tail turn after it, the first 512 of 513 x 512 a second tail turn
    assert sum(hist_walk(887 * 887, t, threads, unroll, max_blocks)[2] for t in range(0, 1024)) == 337
    assert sum(hist_walk(1049000, t, threads, unroll, max_blocks)[3] for t in range(0, 1024)) == 424
    assert sum(hist_walk(513 * 512, t, threads, unroll, max_blocks)[3] == 2 for t in range(0, 1024)) == 512
    # the planted pixels: in every frame past three strides some are met by the unrolled body and some by the tail
    stride = max_blocks * threads
    for w, h in BIG_SIZES[1:]:
        assert w * h > 3 * stride
        n = w * h
        idx = uncountable_pixels(n, stride)
        passes = np.array([hist_walk(n, int(p % stride), threads, unroll, max_blocks)[2] for p in idx])
        in_body = idx // stride < passes * unroll
        assert in_body.sum() >= 8 and (~in_body).sum() >= 8, (w, h)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("w,h", SIZES + BIG_SIZES)
def test_sizes(handles, entry, w, h):
    """Below, at and above the encode's four pixels per thread and 1024 per block and the histogram's block, a width that is no multiple
    of four, and the longest row and column: every stage on, at an odd origin. BIG_SIZES: past the histogram's capped grid, through its
    unrolled body and round its tail more than once, with pixels it skips planted at both ends of every stride."""
    img, exp, state = sized_case(w, h)
    handles[entry].reset()
    assert_same_bytes(run_entry(handles[entry], entry, img, ALL), exp, "%d x %d, %s" % (w, h, entry))
    assert_state(handles[entry].state(), state, "%d x %d, %s" % (w, h, entry))


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_a_flat_frame_through_the_unrolled_body(handles, entry):
    """1283 x 1025 of 0.3: in the unrolled body every lane of every wave counts into one bin, so each wave adds its count through one
    lane; the bin ends with 1 315 075 counts, a block's LDS word with about 5 000."""
    img, exp, state = flat_case()
    handles[entry].reset()
    assert_same_bytes(run_entry(handles[entry], entry, img, ALL), exp, "flat, %s" % entry)
    assert_state(handles[entry].state(), state, "flat, %s" % entry)


def exact_values(transfer, dither):
    """[(y, B)]: values y in [0, 1] whose frac is exactly a threshold — 0.5 without dither (B = -1), (B + 0.5)/64 with — searched among
    the floats around where each code step's should be."""
    E, ks = R.srgb_table(), np.arange(1, 254)
    Bs = np.arange(64) if dither else np.array([-1])
    ts = (Bs.astype(np.float32) + F(0.5)) / F(64) if dither else np.array([0.5], np.float32)
    K, T = np.meshgrid(ks, ts, indexing="ij")
    y0 = (E[K] + (E[K + 1] - E[K]) * T).astype(np.float32) if transfer else ((K + T.astype(np.float64)) / 255).astype(np.float32)
    out = []
    for y in (y0, np.nextafter(y0, F(0)), np.nextafter(y0, F(2))):
        k, frac = R.parts(y, transfer)
        hit = (k == K) & (frac == T)
        out += [(F(v), int(b)) for v, b in zip(y[hit], np.broadcast_to(Bs[None, :], K.shape)[hit])]
    return out


@functools.lru_cache(maxsize=None)
def planted_frame():
    """65 x 5: seeded radiance over 1e-6..1e4 and, planted among it, NaN, +-inf, negatives, denormals, 1e30, every E[k] with its two fp32
    neighbours, and for each transfer, with and without dither, values whose frac is its threshold exactly (for the clamp curve at
    gain 1). Every fifth pixel is kept for the seeded radiance and the threshold cases: those pixels lie in every row and in every
    column of the dither matrix. -> (the frame, the number of exact values planted per (transfer, dither))."""
    w, h = 65, 5
    img = seeded(np.random.default_rng(24), h, w)
    rgb = img[..., :3].reshape(-1, 3)
    E = R.srgb_table()
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e-45, 1e-39, 1e30, 65504.0, 1.0], np.float32)
    values = np.concatenate([E, np.nextafter(E, F(-1)), np.nextafter(E, F(2)), special])
    others = [p for p in range(w * h) if p % 5]
    slots = np.array([(p, c) for p in others for c in range(3)])[:values.size]
    rgb[slots[:, 0], slots[:, 1]] = values
    free = [p for p in range(w * h) if p % 5 == 0][::2]   # (every other one keeps its seeded radiance)
    bayer = R.B8[(ORIGIN[1] + np.arange(w * h) // w) & 7, (ORIGIN[0] + np.arange(w * h) % w) & 7]
    counts = {}
    for transfer, dither in itertools.product((R.LINEAR, R.SRGB), (0, 1)):
        counts[transfer, dither] = 0
        for y, b in exact_values(transfer, dither):
            fit = [p for p in free if not dither or bayer[p] == b]
            if fit:
                free.remove(fit[0])
                rgb[fit[0], counts[transfer, dither] % 3] = y
                counts[transfer, dither] += 1
            if counts[transfer, dither] == 3:
                break
    img[..., :3] = rgb.reshape(h, w, 3)
    return img, counts


def test_planted_frame_holds_its_cases():
    """(CPU) the threshold cases were found, and are hit exactly, for every transfer with and without dither."""
    img, counts = planted_frame()
    assert all(n >= 1 for n in counts.values()), counts
    y = np.where(img[..., :3] > 0, img[..., :3], 0).clip(0, 1).astype(np.float32)
    for (transfer, dither), n in counts.items():
        _, frac = R.parts(y, transfer)
        t = R.threshold(5, 65, dither, ORIGIN)
        assert int((frac == (t[..., None] if dither else t)).sum()) >= n, (transfer, dither)
    E = R.srgb_table()
    assert np.isin(E, img).all() and np.isnan(img).any() and np.isinf(img).any() and (img < 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_every_curve_transfer_and_dither(handles, entry):
    img, _ = planted_frame()
    for curve, transfer, dither in itertools.product((R.CLAMP, R.REINHARD, R.ACES), (R.LINEAR, R.SRGB), (0, 1)):
        for extra in ({}, dict(gain=0.37, white=1.5)):
            p = dict(curve=curve, transfer=transfer, dither=dither, **extra)
            exp = R.encode(img, p.get("gain", 1.0), curve, p.get("white", 4.0), transfer, dither, ORIGIN)
            assert_same_bytes(run_entry(handles[entry], entry, img, p), exp, "%s, %s" % (p, entry))
    # the defaults, given as no record at all, are gpuart_cli --ppm's bytes
    assert (run_entry(handles[entry], entry, img, None)[..., :3] == R.cli_bytes(img[..., :3])).all()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_auto_exposure(handles, entry):
    """One bin for every pixel (the atomics' worst case), nothing to count, three calls that lag their targets and a reset, and a bin
    count past 65536 (65537 is prime: 32769 x 2 is the nearest frame)."""
    hd, d = handles[entry], R.Display()
    hd.reset()
    rng = np.random.default_rng(25)
    flat = np.full((5, 65, 4), 0.3, np.float32)
    black = np.zeros((5, 65, 4), np.float32)
    black[2, 3, :3] = (np.nan, -2.0, np.inf)
    frames = [seeded(rng, 5, 65, 1e-2, 1e1) * F(s) for s in (1.0, 8.0, 0.25)]
    big = np.full((2, 32769, 4), 2.5, np.float32)
    P = dict(auto_exposure=1, adapt=0.25, curve=R.ACES, transfer=R.SRGB)
    for name, img, p in [("black", black, P), ("one bin", flat, P), ("black again", black, P)] + [("adapt %d" % i, f, P) for i, f in enumerate(frames)] + \
                       [("other shares", frames[0], dict(P, lo_share=0.1, hi_share=0.3, key=0.5)), ("clamped", frames[1], dict(P, adapt=1.0, min_gain=3.0, max_gain=3.5)),
                        ("fixed gain only", frames[2], dict(gain=2.0)), ("reset", None, None), ("after reset", frames[1], P), ("65538 in a bin", big, P)]:
        if img is None:
            hd.reset()
            d.reset()
        else:
            assert_same_bytes(run_entry(hd, entry, img, p), d.run(img, ORIGIN, **p), "%s, %s" % (name, entry))
        assert_state(hd.state(), d.state(), "%s, %s" % (name, entry))
    assert max(d.state()["histogram"]) == 65538


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
def test_one_handle_grows_and_shrinks(B, entry):
    """1 x 1 -> 65 x 5 -> 1 x 1 through one handle (the pattern of tests/test_image_libs.py): the staging is allocated again behind the
    first call's work, then larger than needed; the adapted gain is carried across the sizes."""
    hd, d = B.Display(0), R.Display()
    try:
        rng = np.random.default_rng(26)
        for i, (w, h) in enumerate([(1, 1), (65, 5), (1, 1)]):
            img = seeded(rng, h, w, 1e-2, 1e1)
            p = dict(ALL, adapt=0.5)
            assert_same_bytes(run_entry(hd, entry, img, p), d.run(img, ORIGIN, **p), "call %d, %s" % (i, entry))
            assert_state(hd.state(), d.state(), "call %d, %s" % (i, entry))
    finally:
        hd.close()


@pytest.mark.gpu
def test_argument_errors(B, handles):
    """NULL, misaligned and overlapping pointers and sizes out of range: the argument error, a message, nothing written."""
    import torch
    hd, L = handles["device"], B.display_lib()
    rgba = torch.ones((4 * 4 + 1) * 4, device="cuda:0")
    out = torch.full((4 * 4 * 4 + 32,), 7, dtype=torch.uint8, device="cuda:0")
    run = lambda r, o, w=4, h=4: L.gpuart_display_run(hd.h, C.c_void_p(r), C.c_void_p(o), C.c_uint32(w), C.c_uint32(h), C.c_uint32(0), C.c_uint32(0), None)
    for r, o, w, h, msg in [(0, out.data_ptr(), 4, 4, "NULL"), (rgba.data_ptr(), 0, 4, 4, "NULL"), (rgba.data_ptr() + 4, out.data_ptr(), 4, 4, "misaligned"),
                            (rgba.data_ptr(), out.data_ptr() + 4, 4, 4, "misaligned"), (rgba.data_ptr(), out.data_ptr(), 0, 4, "bad size"),
                            (rgba.data_ptr(), out.data_ptr(), 4, 65537, "bad size"), (rgba.data_ptr(), rgba.data_ptr() + 16 * 12, 4, 4, "overlaps"),
                            (rgba.data_ptr(), rgba.data_ptr(), 4, 4, "overlaps")]:
        assert run(r, o, w, h) == ERR_ARG
        assert L.gpuart_display_last_error().decode().startswith("display: ") and msg in L.gpuart_display_last_error().decode()
    hd.finish()
    assert (out == 7).all() and (rgba == 1).all()
    assert L.gpuart_display_read_state(hd.h, None) == ERR_ARG
    assert run(rgba.data_ptr(), out.data_ptr()) == 0   # (and the call they all fail is a good one)
    hd.finish()
    assert (out[:64].view(4, 4, 4).cpu().numpy() == 255).all() and (out[64:] == 7).all()


# ---- GPU: Renderer::ReadDisplay -----------------------------------------------------------------------------------------------------
P_R = dict(curve="reinhard", transfer="srgb", dither=1, gain=1.5)
P_R_REF = dict(G=1.5, curve=R.REINHARD, transfer=R.SRGB, dither=1)


def new_renderer(B, cam, em=20.0):
    r = B.Renderer(64, 48, cam)
    r.set_primitives(scene("box"))
    r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=em)
    return r


@pytest.mark.gpu
def test_read_display_is_the_restatement_of_every_read(B):
    """On the box at 64 x 48 (an emissive user sphere: radiance far above 1), read_display(source) = the restatement applied to what the
    matching read_* returns, with the defaults (gpuart_cli --ppm's bytes) and with every stage on; None exactly where that read fails."""
    cams = [cam_dict(p) for p in TRACK]

    def check(r, source, floats, origin=(0, 0)):
        assert floats is not None, source
        assert_same_bytes(r.read_display(source), R.encode(floats), source + ", defaults")
        assert (r.read_display(source)[..., :3] == R.cli_bytes(floats[..., :3])).all()
        assert_same_bytes(r.read_display(source, P_R), R.encode(floats, origin=origin, **P_R_REF), source + ", every stage")

    r = new_renderer(B, cams[0])
    try:
        r.set_temporal_history(True)
        r.render_direct()
        check(r, "direct", r.read_direct())
        r.restart_path_tracing(1, 3)
        for _ in range(3):
            r.path_tracing_pass()
        assert r.read_radiance(True).max() > 1.5
        check(r, "radiance", r.read_radiance(True))
        check(r, "denoised", r.read_denoised())
        check(r, "preview", r.read_preview())   # (no history yet: the denoised frame)
        assert r.read_guided_preview() is None and r.read_display("guided_preview") is None   # the variance is off
        assert r.read_refined() is None and r.read_display("refined") is None                 # no estimate
        r.set_history_variance(True)
        for _ in range(3):
            r.path_tracing_pass()
        r.set_camera(cams[1])                    # commits the view
        assert r.read_guided_preview() is None and r.read_display("guided_preview") is None   # before the view's first path
        for _ in range(2):
            r.path_tracing_pass()
        assert not same_bits(r.read_preview(), r.read_denoised())
        check(r, "preview", r.read_preview())
        check(r, "guided_preview", r.read_guided_preview())
        assert_same_bytes(r.read_display("guided_preview", P_R, lum_floor=0.05), R.encode(r.read_guided_preview(0.05), **P_R_REF), "guided, other floor")
        r.set_tile(10, 6, 40, 30)               # the dither's origin is the tile's
        r.path_tracing_pass()
        check(r, "radiance", r.read_radiance(True), (10, 6))
        check(r, "denoised", r.read_denoised(), (10, 6))
        with pytest.raises(ValueError):
            r.read_display("radiance", dict(bloom=1))
        assert r.read_display("radiance", dict(white=0.0)) is None   # out of range
    finally:
        r.close()
    r = new_renderer(B, cams[0])
    try:
        r.restart_path_tracing(1, 4)
        converged, summary = r.render_until(0.0, batch_paths=2)
        assert not converged and summary["batches"] == 2
        check(r, "refined", r.read_refined())
        assert_same_bytes(r.read_display("refined", P_R, lum_floor=0.05), R.encode(r.read_refined(0.05), **P_R_REF), "refined, other floor")
    finally:
        r.close()


@pytest.mark.gpu
def test_read_display_adapts_across_views_and_forgets_with_the_history(B):
    """The adapted gain lives in the Renderer: a camera move keeps it, a setter that drops the temporal history resets it."""
    cams = [cam_dict(p) for p in TRACK]
    P = dict(auto_exposure=1, adapt=0.5, curve=R.ACES, transfer=R.SRGB)
    r, d = new_renderer(B, cams[0]), R.Display()
    try:
        r.restart_path_tracing(1, 2)

        def step(what):
            r.path_tracing_pass()
            assert_same_bytes(r.read_display("radiance", P), d.run(r.read_radiance(True), **P), what)

        step("first view")
        step("one more pass")
        r.set_camera(cams[3])
        step("after a camera move")
        assert d.valid and d.g != F(R.target_gain(d.h))   # (it was adapting)
        r.set_sun(2.0, 0.5)
        d.reset()
        step("after the Sun moved")
        assert d.g == F(R.target_gain(d.h))
    finally:
        r.close()


@pytest.mark.gpu
def test_read_display_leaves_rendering_alone(B):
    """A run with read_display calls of every source between the passes and a run without leave the same accumulator, the same counters,
    the same estimate and the same previews (after the pattern of the denoiser's side-effect test)."""
    cams = [cam_dict(p) for p in TRACK]

    def run(with_reads):
        r = new_renderer(B, cams[0])
        try:
            r.set_temporal_history(True)
            r.set_history_variance(True)
            r.backend.set_mode(4)
            r.render_direct()
            r.restart_path_tracing(1, 100)
            out = []
            for i in range(2):
                if i:
                    r.set_camera(cams[1])
                converged, summary = r.render_until(0.0, max_above_share=1.0, batch_paths=2)
                assert converged and summary["batches"] == 2
                if with_reads:
                    for source in B.DISPLAY_SOURCES:
                        assert r.read_display(source, dict(P_R, auto_exposure=1)) is not None, source
                r.path_tracing_pass()
                out += [r.read_radiance(False), r.read_preview(), r.read_guided_preview(), r.read_refined(), r.read_error_map(), summary]
            return out, r.backend.counters().as_dict()
        finally:
            r.close()

    out0, cnt0 = run(False)
    out1, cnt1 = run(True)
    assert cnt0 == cnt1
    for a, b in zip(out0, out1):
        assert a == b if isinstance(a, dict) else same_bits(a, b)


@pytest.mark.gpu
def test_cli_display(B, tmp_path):
    """gpuart_cli --display a.ppm --ppm b.ppm writes two byte-equal files; with --srgb --tonemap reinhard the file is the restatement of
    the --pfm frame; the line gains its key only with --display; the refusals."""
    W, H = 64, 48
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", str(W), "--height", str(H), "--spp", "4", "--per-pass", "1", "--user-sphere", "-0.4,0,0.2,0.25,20"]
    a, b, c, pfm = (str(tmp_path / n) for n in ("a.ppm", "b.ppm", "c.ppm", "c.pfm"))
    out = subprocess.run(base + ["--display", a, "--ppm", b], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["display"] == dict(tonemap="clamp", transfer="linear", gain=1, auto_exposure=False, dither=False)
    head = b"P6\n%d %d\n255\n" % (W, H)
    assert open(a, "rb").read() == open(b, "rb").read() and open(a, "rb").read().startswith(head)
    for extra in ([], ["--denoise"]):
        out = subprocess.run(base + extra + ["--display", c, "--pfm", pfm, "--srgb", "--tonemap", "reinhard", "--white", "2", "--exposure-ev", "-1", "--dither"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        raw = open(pfm, "rb").read()
        fhead = b"PF\n%d %d\n-1.0\n" % (W, H)
        rgb = np.frombuffer(raw[len(fhead):], np.float32).reshape(H, W, 3)
        exp = R.encode(np.concatenate([rgb, np.zeros((H, W, 1), np.float32)], 2), 0.5, R.REINHARD, 2.0, R.SRGB, 1)
        got = np.frombuffer(open(c, "rb").read()[len(head):], np.uint8).reshape(H, W, 3)
        assert (got == exp[::-1, :, :3]).all(), extra   # (top-down)
        assert rgb.max() > 1.5
    out = subprocess.run(base + ["--ppm", b], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "display" not in json.loads(out.stdout.strip().splitlines()[-1])
    for extra, msg in ((["--srgb"], "give --display"), (["--tonemap", "aces"], "give --display"), (["--display", a, "--gpus", "2"], "--gpus 1"),
                       (["--display", a, "--tonemap", "filmic"], "usage")):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and msg in out.stderr and not out.stdout, (extra, out.returncode, out.stdout, out.stderr)
