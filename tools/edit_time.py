#!/usr/bin/env python3
"""What an edit of the uploaded scene (include/gpuart_edit.h) costs beside the SetPrimitives of a list of the same size, on one GPU, in
one process:

    python3 tools/edit_time.py [--repeats R]

per scene — scene_d (cfg3's, 100 k triangles) and big (dragon871k = scene_d(660, 660)) — and per share, 1 % and 50 %: that share of
the primitives removed (every k-th device ordinal) and as many triangles added, through Backend.edit with three device tensors, each
edit on a fresh SetPrimitives of the scene, in both build modes:

  call     Backend.edit call to return: the first (it allocates the staging arrays, the spare set and the scratch) and the median and
           range of R more, each on a fresh SetPrimitives — the call then also moves the upload's primitive boxes to the device and
           allocates and zeroes the spare set, as the first rebuild after an upload does —, and of R edits in a row, which reuse both
  steps    of the median call: the edit's device steps (validate and flags, scan, move = compact and append, reduce) and the build's,
           from HIP events on the handles' streams
  move     the edit's streaming step moves 72 bytes in and 72 bytes out per primitive; beside it a device-to-device copy of the same
           byte count (72 x n_new), timed in this run with events. A yardstick, not a pass mark
  set      Renderer.set_primitives (last_setprims_ms) in the same run of a list of the same size and make: the same added triangles, and
           as many primitives removed by the caller's index (which primitives go does not change what the host build and the upload cost)

profiles/edit.txt keeps the output."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

W, H = 1920, 1080


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


def triangles(n, seed):
    """n small triangles inside the scene's box: (descs, payload n x 16)."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.5, 0.5, (n, 3)).astype(np.float32)
    v = np.concatenate([c, c + rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32), c + rng.uniform(-0.01, 0.01, (n, 3)).astype(np.float32)], 1)
    payload = np.zeros((n, 16), np.float32)
    payload[:, 0:3], payload[:, 4:7], payload[:, 8:11] = v[:, 0:3], v[:, 3:6], v[:, 6:9]
    return [(S.TRIANGLE, [float(x) for x in row]) for row in v], payload


def copy_ms(nbytes, rounds=9):
    import torch
    a = torch.empty((nbytes,), dtype=torch.uint8, device="cuda:0")
    b = torch.empty_like(a)
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); b.copy_(a); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms[1:])


def main():
    import torch
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        descs = make()
        arr = B.make_prims(descs)
        r = B.Renderer(W, H, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(arr); r.finish()
        be = r.backend
        n = int(be.scene_device().n_prims)
        print("%s: %d primitives; SetPrimitives %.1f ms in the library" % (which, n, r.last_setprims_ms()[0]))
        for share in (0.01, 0.5):
            k = max(1, int(round(share * n)))
            remove = np.arange(0, n, n // k, dtype=np.int32)[:k]
            add_descs, payload = triangles(k, 7)
            rem_d = torch.from_numpy(remove).to("cuda:0")
            typ_d = torch.full((k,), int(S.TRIANGLE), dtype=torch.int32, device="cuda:0")
            pay_d = torch.from_numpy(payload).to("cuda:0")
            print("  %g %% removed and added (%d each):" % (100 * share, k))
            for mode in ("morton", "clustered"):
                calls = []
                for i in range(repeats + 1):
                    r.set_primitives(arr); r.finish()
                    t = time.perf_counter(); be.edit(rem_d, typ_d, pay_d, mode=mode); dt = (time.perf_counter() - t) * 1e3
                    calls.append((dt, be.last_edit))
                again = []   # edits in a row: the spare set (the former scene arrays) and the prim boxes on the device are reused
                for _ in range(repeats):
                    t = time.perf_counter(); be.edit(rem_d, typ_d, pay_d, mode=mode); again.append((time.perf_counter() - t) * 1e3)
                first, calls = calls[0][0], sorted(calls[1:], key=lambda c: c[0])
                wall, le = calls[len(calls) // 2]
                es, bs = le["step_ms"], le["rebuild"]["step_ms"]
                print("    Backend.edit(mode=%r): first call %.3f ms, then %s ms call to return, each on a fresh SetPrimitives (the call moves the upload's "
                      "primitive boxes to the device and allocates and zeroes the spare set); %s ms for edits in a row" % (mode, first, spread([c[0] for c in calls]), spread(again)))
                print("      the median call: edit %.3f ms on the device (%s), build %.3f ms (%s)"
                      % (sum(es.values()), "  ".join("%s %.3f" % kv for kv in es.items()), sum(bs.values()), "  ".join("%s %.3f" % kv for kv in bs.items())))
                if mode == "morton":
                    print("      move: %.3f ms for %d primitives; a device-to-device copy of the same %d bytes: %.3f ms"
                          % (es["move"], le["n_prims"], 72 * le["n_prims"], copy_ms(72 * le["n_prims"])))
            gone = set(remove.tolist())
            edited = B.make_prims([d for i, d in enumerate(descs) if i not in gone] + add_descs)
            ms = []
            for _ in range(max(3, repeats // 2)):
                r.set_primitives(edited); r.finish()
                ms.append(r.last_setprims_ms()[0])
            print("    SetPrimitives of a list of the same size (%d primitives): %s ms in the library" % (len(edited), spread(ms)))
        be.close()   # (the edit and build handles; the context is the renderer's)
        r.close()


if __name__ == "__main__":
    main()
