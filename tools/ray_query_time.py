#!/usr/bin/env python3
"""Rates of the batched ray queries (gpuart_hip_trace_rays / _pick, k_ray_query) against the test build's one-thread-per-ray hook
(gpuart_hip_test_traverse, k_test_traverse) and against a direct-lighting frame, on cfg3's scene (Scene D) and camera at 1920x1080.

   python3 tools/ray_query_time.py [--repeats R] [--rays LOG2]

Workloads: (a) the frame's camera rays, through pick (pixels in, rays made in-kernel) and through trace_rays (rays in);
(b) 2^LOG2 incoherent rays: origins at primary hit points, uniform directions; (c) (b) in occlusion mode, tmax = the distance to a
random primary hit point. Methods are run alternately in one process (R repeats each after a warm-up). Each timing is a pair of
HIP events on torch's stream around a call that ends in a synchronise: the host-memory paths include their copies, the torch
path (rays already on the GPU) does not. Loads the test build (gpuart_amd/lib_test) for the hook; both libraries hold the same
product kernels."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPUART_LIBDIR", os.path.join(ROOT, "gpuart_amd", "lib_test"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def rays8(rs, rd, tmax=np.inf):
    r = np.zeros((len(rs), 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7] = rs[:, :3], tmax, rd[:, :3]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rays", type=int, default=22, help="log2 of the incoherent batch")
    a = ap.parse_args()
    W, H = 1920, 1080
    cam = dict(S.BENCH_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    basis = np.zeros(13, np.float32)
    B.host_lib().gpuart_camera_basis(B._f3(cam["pos"]), B._f3(cam["dir"]), B._f3(cam["up"]), C.c_float(cam["fov_y"]),
                                     C.c_float(cam["screen_dist"]), C.c_uint(W), C.c_uint(H), B._p(basis))
    quads, _ = B.compile_bvh(S.scene_d())
    be = B.Backend(0)
    be.resize(W, H)
    be.upload_bvh(quads)
    be.set_camera(basis)
    us = S.USER_SPHERE
    print("# libraries: %s" % B.LIBDIR)
    print("# scene D: %d nodes, %d primitives; frame %dx%d; user sphere %s" % (be.scene_info()["nodes"], be.scene_info()["prims"], W, H, us))

    # direct-lighting params of the same frame (the bench's: Sun on, user sphere as above, not emissive)
    sun = np.zeros(3, np.float32)
    B.host_lib().gpuart_sun_direction(C.c_float(S.SUN_AZIMUTH), C.c_float(S.SUN_ALTITUDE), B._p(sun))
    P = B.Params()
    P.sunDirAlt[:] = [float(sun[0]), float(sun[1]), float(sun[2]), float(S.SUN_ALTITUDE)]
    P.sunEnabled = 1
    P.userSphere[:] = [float(v) for v in us]
    P.pixelSize = float(basis[12])
    P.cameraPos[:] = [float(v) for v in basis[0:3]]
    P.maxSegments, P.minWeight = 5, 0.01

    # (a) camera rays
    y, x = np.divmod(np.arange(W * H), W)
    xy = np.stack([x, y], 1).astype(np.uint32)
    rs, rd = be.test_cam_rays()
    rs, rd = rs.reshape(-1, 4), rd.reshape(-1, 4)
    cam_rays = rays8(rs, rd)
    cam_rays_t = torch.from_numpy(cam_rays).to("cuda:0")
    prim = be.pick(xy, user_sphere=us)
    # (b) incoherent: origins at primary hit points, uniform directions; (c) tmax = distance to a random primary hit point
    rng = np.random.default_rng(11)
    n = 1 << a.rays
    pts = prim["p"][prim["pos"] > 0]
    o = pts[rng.integers(0, len(pts), n)]
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    q = pts[rng.integers(0, len(pts), n)]
    inc = rays8(o, d)
    occ = rays8(o, d, np.linalg.norm(q - o, axis=1).astype(np.float32))
    inc_t, occ_t = torch.from_numpy(inc).to("cuda:0"), torch.from_numpy(occ).to("cuda:0")
    hits_t = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
    cam_hits_t = torch.empty((W * H, 8), dtype=torch.float32, device="cuda:0")
    o4, d4 = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    o4[:, :3], d4[:, :3] = o, d
    cs4, cd4 = np.ascontiguousarray(rs), np.ascontiguousarray(rd)

    def direct():
        be.render_direct(P)
        be.finish()

    workloads = [
        ("(a) camera rays 1920x1080", W * H, [
            ("pick (host xy)", lambda: be.pick(xy, user_sphere=us)),
            ("trace_rays (host)", lambda: be.trace_rays(cam_rays, user_sphere=us)),
            ("trace_rays (torch)", lambda: be.trace_rays(cam_rays_t, user_sphere=us, out=cam_hits_t)),
            ("hook k_test_traverse (host)", lambda: be.test_traverse(cs4, cd4, us)),
            ("render_direct (frame)", direct),
        ]),
        ("(b) 2^%d incoherent rays" % a.rays, n, [
            ("trace_rays (host)", lambda: be.trace_rays(inc, user_sphere=us)),
            ("trace_rays (torch)", lambda: be.trace_rays(inc_t, user_sphere=us, out=hits_t)),
            ("hook k_test_traverse (host)", lambda: be.test_traverse(o4, d4, us)),
        ]),
        ("(c) 2^%d occlusion rays, tmax = distance to a random point" % a.rays, n, [
            ("trace_rays occlusion (host)", lambda: be.trace_rays(occ, occlusion=True, user_sphere=us)),
            ("trace_rays occlusion (torch)", lambda: be.trace_rays(occ_t, occlusion=True, user_sphere=us, out=hits_t)),
            ("trace_rays closest hit, same rays (torch)", lambda: be.trace_rays(occ_t, user_sphere=us, out=hits_t)),
        ]),
    ]
    # the answers first: the new kernel must agree with the hook on (a) and (b) (the timings below would mean nothing otherwise)
    h = be.trace_rays(cam_rays, user_sphere=us)
    o0, o1 = be.test_traverse(cs4, cd4, us)
    assert (h["pos"].view(np.uint32) == o0[:, 0].view(np.uint32)).all(), "camera rays: trace_rays differs from the hook"
    h = be.trace_rays(inc[:1 << 18], user_sphere=us)
    o0, o1 = be.test_traverse(o4[:1 << 18], d4[:1 << 18], us)
    assert (h["pos"].view(np.uint32) == o0[:, 0].view(np.uint32)).all(), "incoherent rays: trace_rays differs from the hook"
    hc = be.trace_rays(occ, occlusion=True, user_sphere=us)
    print("# (c): %.1f %% of the rays occluded" % (100.0 * (hc["pos"] > 0).mean()))

    for title, count, methods in workloads:
        for _, fn in methods:  # warm-up
            fn()
        ms = {name: [] for name, _ in methods}
        for _ in range(a.repeats):
            for name, fn in methods:
                ms[name].append(timed(fn))
        print("%s: %d rays, %d repeats each, alternating" % (title, count, a.repeats))
        for name, _ in methods:
            v = np.array(ms[name])
            print("  %-42s median %8.3f ms  (min %8.3f, max %8.3f, spread %4.1f %%)  %8.1f Mrays/s" % (
                name, np.median(v), v.min(), v.max(), 100.0 * (v.max() - v.min()) / np.median(v), count / np.median(v) / 1e3))
    be.close()


if __name__ == "__main__":
    main()
