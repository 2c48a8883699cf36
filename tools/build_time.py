#!/usr/bin/env python3
"""What rebuilding the tree on the device costs and what the rebuilt tree is worth (include/gpuart_build.h), on one GPU, beside the
SetPrimitives of the same primitives in the same process:

    python3 tools/build_time.py [--repeats R] [--passes K]
    python3 tools/build_time.py --drift

per scene — scene_d (cfg3's, 100 k triangles) and big (dragon871k = scene_d(660, 660)) —

  time     SetPrimitives (GetLastSetPrimitivesMs); Backend.rebuild(out = a device tensor), call to return, first call (it allocates the
           spare arrays and the scratch) and best of R, with the device time of its steps from HIP events on the handle's stream (keys,
           sort, permute, hierarchy, number, emit, level launches + root); Renderer::RebuildTree call to return with the share that is
           the host tree (RebuildMorton from the device's order)
  quality  ms per path-tracing pass at 1920x1080 (K passes in one sequence, best of 3), box steps per ray (the device counters of two
           passes in mode 1) and tree_cost() on the reference-built tree and on the rebuilt one
  drift    (--drift, a run of its own) scene_d with every primitive translated to another primitive's place (a seeded shuffle) and
           refitted: the same three figures after the refit alone and after refit + rebuild, at 240x135 and from single passes — a ray
           through the shuffled mesh meets most of its boxes, and a full-size pass on the refitted tree would take minutes

profiles/build.txt keeps the output."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

W, H = 1920, 1080
QUADS = {S.SPHERE: (0,), S.DISC: (0,), S.TRIANGLE: (0, 4, 8)}    # where a payload holds points (the scenes timed here have no cones)


def tree_payloads(q):
    """Per device ordinal (the leaves' primitives in address order) the type and the 16 floats of its data quads."""
    bits, types, data, a, n = q.view(np.uint32), [], [], 0, len(q)
    while a < n:
        flags = int(bits[a + 2, 0])
        a += 3
        if flags & 0x80000000:
            for _ in range(flags & 0x1fffffff):
                t = int(bits[a, 0])
                d = np.zeros(16, np.float32)
                d[:4 * (t + 1)] = q[a + 1:a + 2 + t].reshape(-1)
                types.append(t); data.append(d)
                a += 2 + t
    return np.array(types), np.stack(data)


def quality(r, passes, rounds=3):
    """(ms per pass, box steps per ray, tree cost) of the renderer's scene as it is."""
    be = r.backend
    be.set_mode(1); be.counters(reset=True)
    r.restart_path_tracing(1, 2); r.path_tracing_pass(); r.path_tracing_pass(); r.finish()
    cnt = be.counters(reset=True)
    be.set_mode(0)
    best = 1e9
    for _ in range(rounds):
        r.restart_path_tracing(1, passes)
        t = time.perf_counter()
        for _ in range(passes):
            r.path_tracing_pass()
        r.finish()
        best = min(best, (time.perf_counter() - t) / passes)
    return best * 1e3, cnt.box_steps / max(1, cnt.rays), be.tree_cost()


def say_quality(label, q):
    print("  %-34s %8.3f ms per pass   %7.2f box steps per ray   tree cost %10.2f" % ((label,) + q))


def drift():
    import torch
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    descs = S.scene_d()
    n = len(descs)
    arr = B.make_prims(descs)
    r = B.Renderer(240, 135, cam)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_max_path_segments(8)
    r.set_primitives(arr); r.finish()
    be = r.backend
    q, _ = B.compile_bvh(arr)
    types, data = tree_payloads(q)
    centre = data[:, 0:3].astype(np.float64)
    tri = types == S.TRIANGLE
    centre[tri] = (data[tri, 0:3].astype(np.float64) + data[tri, 4:7] + data[tri, 8:11]) / 3
    to = np.random.default_rng(77).permutation(n)
    delta = (centre[to] - centre).astype(np.float32)
    pay = data.copy()
    for t_, cols in QUADS.items():
        for c in cols:
            pay[types == t_, c:c + 3] += delta[types == t_]
    print("drift: scene_d (%d primitives) at 240x135, every primitive translated to another primitive's place" % n)
    say_quality("as built by SetPrimitives", quality(r, 1, 1))
    be.refit(torch.arange(n, dtype=torch.int32, device="cuda:0"), torch.from_numpy(pay).to("cuda:0"))
    say_quality("refit only", quality(r, 1, 1))
    be.rebuild(out=True)
    say_quality("refit + rebuild", quality(r, 1, 1))
    r.set_primitives(arr); r.finish()
    be.rebuild(out=True)
    say_quality("rebuilt without the drift", quality(r, 1, 1))
    be.close()   # (the build and refit handles; the context is the renderer's)
    r.close()


def main():
    import torch
    if "--drift" in sys.argv:
        return drift()
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    passes = int(sys.argv[sys.argv.index("--passes") + 1]) if "--passes" in sys.argv else 32
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        descs = make()
        n = len(descs)
        arr = B.make_prims(descs)
        r = B.Renderer(W, H, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_max_path_segments(8)
        lib = None
        for _ in range(3):
            r.set_primitives(arr); r.finish()
            lib = min(lib or r.last_setprims_ms(), r.last_setprims_ms())
        be = r.backend
        info = be.scene_info()
        print("%s: %d primitives, reference-built tree of depth %d" % (which, n, info["max_depth"]))
        print("  SetPrimitives: %.1f ms in the library (build %.1f + compile %.1f + re-layout and upload %.1f)" % tuple(lib))
        ref = quality(r, passes)
        # the device build alone
        out = torch.empty((n,), dtype=torch.int32, device="cuda:0")
        t = time.perf_counter(); be.rebuild(out=out); first = (time.perf_counter() - t) * 1e3
        wall, steps = 1e9, None
        for _ in range(repeats):
            t = time.perf_counter(); be.rebuild(out=out); dt = (time.perf_counter() - t) * 1e3
            res = be.last_rebuild
            if dt < wall:
                wall, steps = dt, res["step_ms"]
        print("  Backend.rebuild (device tensor out): first call %.3f ms, then %.3f ms call to return; tree of depth %d, %d level launches"
              % (first, wall, res["max_depth"], res["levels"]))
        print("    device time of its steps, %.3f ms in all: %s" % (sum(steps.values()), "  ".join("%s %.3f" % kv for kv in steps.items())))
        built = quality(r, passes)
        say_quality("reference-built tree", ref)
        say_quality("rebuilt (Morton) tree", built)
        print("    the rebuilt tree walks %.2f x the box steps and takes %.2f x the time per pass" % (built[1] / ref[1], built[0] / ref[0]))
        # through the Renderer, host tree included
        total, host = 1e9, 0.0
        for _ in range(repeats):
            r.set_primitives(arr); r.finish()
            t = time.perf_counter(); ok = r.rebuild_tree(); dt = (time.perf_counter() - t) * 1e3
            if ok is None:
                sys.exit("rebuild_tree refused")
            if dt < total:
                total, host = dt, r.last_rebuild_ms()[1]
        print("  Renderer::RebuildTree: %.1f ms call to return, of which the host tree %.1f ms (%.0f %%)" % (total, host, 100 * host / total))
        be.close()   # (the build handle; the context is the renderer's)
        r.close()


if __name__ == "__main__":
    main()
