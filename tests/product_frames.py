#!/usr/bin/env python3
"""The child process of tests/test_product_library.py: runs on the PRODUCT library pair (the caller passes GPUART_LIBDIR=gpuart_amd/lib),
through the C++ Renderer only — no test hook — and says at the end that the product pair, and nothing of lib_test, was mapped.

    python3 tests/product_frames.py fixture cfg1|cfg2|cfg3|cfg4
        BASELINE cfg1-cfg4 through the Renderer against the reference's own renders (tests/golden): the Renderer's setup (Params,
        camera basis, RandSeed draws) first, then direct lighting and path tracing in modes 0, 3 and 5. Prints "<cfg> OK".
    python3 tests/product_frames.py bench -- <bench.py arguments>
        bench.py as it is, in this process (its own command line), then the library check; the caller compares the dumped frame."""
import os
import runpy
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

# BASELINE.json's configurations as the fixtures hold them (tests/golden/make_golden.py gen_scene_p / gen_fullsize): scene, camera,
# depth; cfg1 is stored as whole frames, the others as per-row checksums of the float bit patterns
FIXTURES = {
    "cfg1": ("frames_scene_p_seg4", "scene_p", "DEFAULT_CAMERA"),
    "cfg2": ("fullsize_scene_p_1080p", "scene_p", "DEFAULT_CAMERA"),
    "cfg3": ("fullsize_scene_d_1080p", "scene_d", "BENCH_CAMERA"),
    "cfg4": ("fullsize_scene_d_4k", "scene_d", "BENCH_CAMERA"),
}
RMSE_TOL = 1e-4


def check_product_mapped():
    maps = open("/proc/self/maps").read()
    for lib in ("/gpuart_amd/lib/libgpuart_hip.so", "/gpuart_amd/lib/libgpuart.so"):
        assert lib in maps, "%s is not mapped: this process did not run the product library" % lib
    assert "lib_test" not in maps, "a library under lib_test is mapped"
    print("product library mapped", flush=True)


def params_diff(a, b):
    """The fields of two gpuart_params that differ, for the failure message."""
    out = []
    for name, _ in type(a)._fields_:
        x, y = getattr(a, name), getattr(b, name)
        x, y = (list(x), list(y)) if hasattr(x, "__len__") else (x, y)
        if x != y:
            out.append("%s: %r vs %r" % (name, x, y))
    return out


def run_fixture(cfg):
    import ctypes as C

    from gpuart_amd import binding as B
    from gpuart_amd import synth_scenes as S
    from oracle import oracle as O
    from tests.util import assert_bits, golden, rmse_per_channel, row_checksums

    name, sc, camsel = FIXTURES[cfg]
    g = golden(name)
    W, H, segs, npass = int(g["W"]), int(g["H"]), int(g["max_segments"]), int(g["npasses"])
    whole = cfg == "cfg1"
    cam = dict(getattr(S, camsel))
    cam["dir"] = S.camera_dir(cam)

    # ---- setup: the Renderer's must equal the fixture's, or the comparison below would test the wrong thing ----
    basis = B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
    assert basis.view(np.uint32).tolist() == np.asarray(g["cam"], np.float32).view(np.uint32).tolist(), \
        "setup: the host library's camera basis %s != the fixture's %s" % (basis, g["cam"])
    seeds = O.randseeds(npass)  # mt19937(5489): the Renderer's default generator (renderer.h RndGen)
    assert np.array_equal(seeds.view(np.uint32), np.asarray(g["seeds"][:npass], np.float32).view(np.uint32)), \
        "setup: the fixture's RandSeeds are not the first draws of mt19937(5489)"
    r = B.Renderer(W, H, cam, device=0)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_primitives(B.make_prims(S.scene_p() if sc == "scene_p" else S.scene_d()))
    r.set_max_path_segments(segs)
    assert r.is_ok(), "Renderer not OK"
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    cb = g["cam"]
    exp_p = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(cb[12]), cb[0:3], segs, 0.01)
    got_p = r.params()
    assert C.string_at(C.addressof(got_p), C.sizeof(got_p)) == C.string_at(C.addressof(exp_p), C.sizeof(exp_p)), \
        "setup: Renderer params differ from the fixture's: %s" % params_diff(got_p, exp_p)

    def check(got, key, what):
        if whole:
            ref = np.asarray(g[key], np.float32)
            rm = rmse_per_channel(got[..., :3], ref)
            assert (rm < RMSE_TOL).all(), "%s %s: RMSE %s exceeds %g" % (cfg, what, rm, RMSE_TOL)
            assert_bits(got[..., :3].reshape(-1, 3), ref.reshape(-1, 3), "%s %s (pixels)" % (cfg, what))
        else:
            bad = (row_checksums(got) != g[key]).any(1)
            assert not bad.any(), "%s %s: %d of %d rows differ from the reference's row checksums (first: %d)" % (
                cfg, what, int(bad.sum()), H, int(np.argmax(bad)))

    def acc_key(k):  # the fixture's accumulator after pass k + 1
        return ("pt_pass1" if k == 0 else "pt_acc") if whole else "pt_acc%d" % (k + 1)

    r.render_direct()
    check(r.read_direct(), "direct", "direct lighting")
    be = r.backend
    # mode 0 (the product's default) on the Renderer's own, never re-seeded generator: the fixture's pass count as one restart, read
    # after the last pass only, so the planner groups the passes as a caller's run is grouped
    r.restart_path_tracing(1, npass)
    assert [r.path_tracing_pass() for _ in range(npass)] == list(range(1, npass + 1))
    check(r.read_radiance(False), acc_key(npass - 1), "mode 0, %d passes" % npass)
    for mode in (3, 5):  # 3: the launch pipeline (k_trace / k_shade); 5: the persistent run kernel (k_run); read after every pass
        r.set_seed(5489)
        be.set_mode(mode)
        r.restart_path_tracing(1, npass)
        for k in range(npass):
            assert r.path_tracing_pass() == k + 1
            check(r.read_radiance(False), acc_key(k), "mode %d, pass %d" % (mode, k + 1))
    be.set_mode(0)
    info = be.scene_info()
    r.close()
    check_product_mapped()
    print("%s OK: %s, %dx%d, depth %d, %d nodes / %d primitives: direct lighting and %d passes in modes 0, 3, 5 equal the reference"
          % (cfg, name, W, H, segs, info["nodes"], info["prims"], npass), flush=True)


def run_bench(args):
    bench = os.path.join(ROOT, "bench.py")
    sys.argv = [bench] + args
    try:
        runpy.run_path(bench, run_name="__main__")
    except SystemExit as e:
        if e.code not in (None, 0):
            raise
    check_product_mapped()


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "fixture" and sys.argv[2] in FIXTURES:
        run_fixture(sys.argv[2])
    elif len(sys.argv) >= 3 and sys.argv[1:3] == ["bench", "--"]:
        run_bench(sys.argv[3:])
    else:
        sys.exit(__doc__)


if __name__ == "__main__":
    main()
