#!/usr/bin/env python3
"""What the clustered rebuild (include/gpuart_ploc.h) costs and what its tree is worth beside the Morton rebuild (include/gpuart_build.h)
and the SetPrimitives of the same primitives, on one GPU, in one process:

    python3 tools/ploc_time.py [--repeats R]

per scene — scene_d (cfg3's, 100 k triangles) and big (dragon871k = scene_d(660, 660)) —

  build    Backend.rebuild(mode, out = a device tensor) call to return: the first call on the SetPrimitives tree (it allocates the spare
           arrays and the scratch) and the median and range of R more, with the device time of the steps of the median call from HIP
           events on the handle's stream; for the clustered build the iteration count and the share of the iteration loop, whose events
           span its per-iteration read-backs; Renderer::RebuildTree call to return with the share that is the host tree, both modes
  quality  for three trees on the same box in the same session — SetPrimitives', the Morton rebuild's (the baseline) and the clustered
           rebuild's —: tree_cost(), box steps per ray (the device counters of two passes in mode 1, tools/build_time.py `quality`) and ms
           per path-tracing pass at 1920x1080 for sequences of K = 20 and K = 64 passes (after one warm-up sequence: median and range of 5)

profiles/ploc.txt keeps the output."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

W, H = 1920, 1080
KS = (20, 64)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def quality(r, label, rounds=5):
    be = r.backend
    be.set_mode(1); be.counters(reset=True)
    r.restart_path_tracing(1, 2); r.path_tracing_pass(); r.path_tracing_pass(); r.finish()
    cnt = be.counters(reset=True)
    be.set_mode(0)
    out = {"steps": cnt.box_steps / max(1, cnt.rays), "cost": be.tree_cost()}
    for k in KS:
        ms = []
        for i in range(rounds + 1):   # the first sequence warms up
            r.restart_path_tracing(1, k)
            t = time.perf_counter()
            for _ in range(k):
                r.path_tracing_pass()
            r.finish()
            if i:
                ms.append((time.perf_counter() - t) / k * 1e3)
        out[k] = ms
    print("  %-22s tree cost %9.2f   %7.2f box steps per ray   ms per pass, K = 20: %s   K = 64: %s"
          % (label, out["cost"], out["steps"], spread(out[20]), spread(out[64])))
    return out


def timed_rebuilds(r, arr, mode, repeats):
    import torch
    be = r.backend
    r.set_primitives(arr); r.finish()
    n = be.scene_device().n_prims
    out = torch.empty((n,), dtype=torch.int32, device="cuda:0")
    t = time.perf_counter(); be.rebuild(out=out, mode=mode); first = (time.perf_counter() - t) * 1e3
    first_report = dict(be.last_rebuild)
    calls = []
    for _ in range(repeats):
        t = time.perf_counter(); be.rebuild(out=out, mode=mode); calls.append(((time.perf_counter() - t) * 1e3, be.last_rebuild))
    calls.sort(key=lambda c: c[0])
    wall, res = calls[len(calls) // 2]
    steps = res["step_ms"]
    print("  Backend.rebuild(mode=%r): first call %.3f ms, then %s ms call to return" % (mode, first, spread([c[0] for c in calls])))
    print("    the median call: %d records, depth %d; device time of its steps %.3f ms: %s"
          % (res["n_recs"], res["max_depth"], sum(steps.values()), "  ".join("%s %.3f" % kv for kv in steps.items())))
    if mode == "clustered":
        print("    %d iterations (%d on the SetPrimitives tree's order); the iteration loop with its read-backs is %.0f %% of the device time, "
              "%.3f ms per iteration, and %.0f %% of the call" % (res["iterations"], first_report["iterations"], 100 * steps["iterations"] / sum(steps.values()),
                                                                steps["iterations"] / max(1, res["iterations"]), 100 * steps["iterations"] / wall))
    # the tree that is measured is the rebuild of the SetPrimitives tree
    r.set_primitives(arr); r.finish()
    be.rebuild(out=out, mode=mode)


def timed_renderer(r, arr, mode, repeats):
    total = []
    for _ in range(repeats):
        r.set_primitives(arr); r.finish()
        t = time.perf_counter(); ok = r.rebuild_tree(mode); dt = (time.perf_counter() - t) * 1e3
        if ok is None:
            sys.exit("rebuild_tree refused")
        total.append((dt, r.last_rebuild_ms()[1]))
    total.sort()
    dt, host = total[len(total) // 2]
    print("  Renderer::RebuildTree(%s): %s ms call to return (each after a SetPrimitives: the spare arrays are allocated anew), of which the host tree %.1f ms (%.0f %%)"
          % (mode, spread([t[0] for t in total]), host, 100 * host / dt))


def main():
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 7
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        descs = make()
        arr = B.make_prims(descs)
        r = B.Renderer(W, H, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_max_path_segments(8)
        r.set_primitives(arr); r.finish()
        print("%s: %d primitives; SetPrimitives %.1f ms in the library" % (which, len(descs), r.last_setprims_ms()[0]))
        q = {"set": quality(r, "SetPrimitives")}
        for mode in ("morton", "clustered"):
            timed_rebuilds(r, arr, mode, repeats)
            q[mode] = quality(r, "%s rebuild" % mode)
        for mode in ("morton", "clustered"):
            timed_renderer(r, arr, mode, repeats)
        for k in KS:
            m, c, s = (statistics.median(q[x][k]) for x in ("morton", "clustered", "set"))
            print("  K = %d: the clustered tree takes %.2f x the Morton tree's time per pass and %.2f x the SetPrimitives tree's" % (k, c / m, c / s))
        print("  box steps per ray: clustered %.2f x Morton, %.2f x SetPrimitives" % (q["clustered"]["steps"] / q["morton"]["steps"], q["clustered"]["steps"] / q["set"]["steps"]))
        r.backend.close()   # (the build handles; the context is the renderer's)
        r.close()


if __name__ == "__main__":
    main()
