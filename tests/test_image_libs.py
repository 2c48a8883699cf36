"""What libgpuart_denoise.so, libgpuart_temporal.so, libgpuart_converge.so and libgpuart_refine.so share (gpuart_amd/csrc/image/image_lib.h): every library
keeps a last error of its own, and one handle of each that grows and shrinks — its buffers allocated again behind work on its stream,
its staging offsets moved — still computes its restatement's bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from tests import converge_ref
from tests import denoise_ref
from tests import filter_cases as FC
from tests import refine_ref
from tests import temporal_ref
from tests.util import assert_same_bits, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("denoise", "temporal", "converge", "refine")
ERR_ARG = -1


# ---- CPU --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_each_library_keeps_its_own_last_error(lib):
    """gpuart_<name>_finish(NULL) fails before any HIP call: that library's last error then carries its own prefix, and the other
    libraries' strings are as they were."""
    libs = {n: C.CDLL(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % n)) for n in NAMES}
    for n in NAMES:
        getattr(libs[n], "gpuart_%s_last_error" % n).restype = C.c_char_p
    last = lambda n: getattr(libs[n], "gpuart_%s_last_error" % n)()
    seen = {n: last(n) for n in NAMES}
    for n in NAMES:
        assert getattr(libs[n], "gpuart_%s_finish" % n)(None) == ERR_ARG
        assert last(n) == ("%s: handle is NULL" % n).encode()
        seen[n] = last(n)
        assert {m: last(m) for m in NAMES} == seen, n
    assert len(set(seen.values())) == len(NAMES)


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
# One above the 64 x 4 row block in both directions between two single pixels: the second call allocates every buffer again behind the
# first call's work, the third runs in buffers larger than it needs, and each size puts the staged planes at other offsets. The single
# pixel is a tile in the middle of the 65 x 5 frame, and the camera moves by a fraction of a pixel, so that each view finds the history
# of the other size.
FRAME = temporal_ref.full_frame(65, 5)
PIXEL = (65, 5, 32, 2, 1, 1, 1, 1)
GEOMS = [PIXEL, FRAME, PIXEL]
POSITIONS = [FC.POS_0, (0.02, 0.0, 0.01), FC.POS_0]
BATCHES = (4, 3)   # paths of the convergence estimate's two updates per size


@functools.lru_cache(maxsize=None)
def views():
    """One view per size (tests/filter_cases.py `step`, seed 4242), and per view what each restatement makes of it: the denoised image;
    the blend and lengths of a chain that commits every view; the states after two updates of an estimator reset at every size, and
    its measure; the variance-guided filter of the view with that measure's error map."""
    rng = np.random.default_rng(4242)
    out, hist = [], None
    for geom, pos in zip(GEOMS, POSITIONS):
        rgba, spp, words, prims, view = FC.step(rng, pos, geom, 2, mix=geom is FRAME)   # (the single pixel is a surface pixel)
        v = dict(w=geom[4], h=geom[5], rgba=rgba, spp=spp, words=words, prims=prims, view=view)
        v["denoised"] = denoise_ref.denoise(rgba, words, prims, 0)
        v["blend"], v["len"], hist = temporal_ref.accumulate(hist, rgba, spp, words, prims, view)
        est = converge_ref.Estimator()
        v["accums"] = [rgba * np.float32(BATCHES[0]), rgba * np.float32(BATCHES[0]) + FC.radiance(rng, view["geom"]) * np.float32(BATCHES[1])]
        v["totals"] = [BATCHES[0], BATCHES[0] + BATCHES[1]]
        v["states"] = [est.update(a, t).copy() for a, t in zip(v["accums"], v["totals"])]
        v["summary"], v["error"] = est.measure(0.05, 1.0 / 256)
        v["refined"] = refine_ref.refine(rgba, words, prims, v["error"], 1.0 / 256)
        out.append(v)
    assert all((v["len"] > v["spp"]).any() for v in out[1:])   # (each found the history of the other size)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("name", NAMES)
def test_one_handle_grows_and_shrinks(name, entry):
    import torch

    from gpuart_amd import binding as B
    from tests.test_converge import assert_summary
    from tests.test_filter_edges import binding_view
    to = to_device if entry == "device" else (lambda a: a)
    back = (lambda a: a.cpu().numpy()) if entry == "device" else (lambda a: a)
    handle = {"denoise": B.Denoiser, "temporal": B.Temporal, "converge": B.Converge, "refine": B.Refine}[name](0)
    try:
        for i, v in enumerate(views()):
            what = "%s, %s, call %d (%d x %d)" % (name, entry, i, v["w"], v["h"])
            if name == "denoise":
                assert_same_bits(back(handle.run(to(v["rgba"]), to(v["words"]), to(v["prims"]))), v["denoised"], what)
            elif name == "refine":
                assert_same_bits(back(handle.run(to(v["rgba"]), to(v["words"]), to(v["prims"]), to(v["error"]), 1.0 / 256)), v["refined"], what)
            elif name == "temporal":
                out, ln = handle.accumulate(to(v["rgba"]), v["spp"], to(v["words"]), to(v["prims"]), binding_view(B, v["view"]), commit=True)
                assert_same_bits(back(out), v["blend"], what)
                assert_same_bits(back(ln), v["len"], what + ", length")
            else:
                handle.reset()   # (the state's size is fixed until a reset)
                for k in range(2):
                    handle.update(to(v["accums"][k]), v["totals"][k])
                    assert_same_bits(handle.state(), v["states"][k], "%s: state after update %d" % (what, k))
                emap = torch.full((v["h"], v["w"]), 7.0, device="cuda:0") if entry == "device" else True
                summary, e = handle.measure(0.05, 1.0 / 256, error_map=emap)
                assert_summary(summary, v["summary"], what)
                assert_same_bits(back(e), v["error"], what + ": error map")
    finally:
        handle.close()
