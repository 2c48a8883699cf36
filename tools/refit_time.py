#!/usr/bin/env python3
"""What moving primitives costs (include/gpuart_refit.h), call to return, on one GPU, beside a SetPrimitives of the same moved primitives
in the same process:

    python3 tools/refit_time.py [scene_d|big] [--repeats R]

  UpdatePrimitives   Renderer::UpdatePrimitives through the C API (the host tree's verdict and refit, scene_device, the device sequence from
                     host memory, scene_refitted, the restart of the accumulation), descriptions made beforehand
  Backend.refit      the device-pointer entry: ordinals and payload already in device tensors (scene_device, the device sequence, scene_refitted)
  SetPrimitives      GetLastSetPrimitivesMs of a SetPrimitives of the moved scene: whole call = build + compile + re-layout and upload

for 1 primitive, 1 % and all of them. The tree's record levels are the launches of the level kernel per refit. The level kernels' summed
time comes from a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -- python3 tools/refit_time.py scene_d --profile

which only refits (all primitives, --repeats times) and prints how many refits the kernel statistics cover. profiles/refit.txt keeps the output.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

DELTA = np.float32([0.01, -0.02, 0.015])
POINTS = {S.SPHERE: (0,), S.DISC: (0,), S.TRIANGLE: (0, 3, 6)}   # where a description holds points (the scenes timed here have no cones)
QUADS = {S.SPHERE: (0,), S.DISC: (0,), S.TRIANGLE: (0, 4, 8)}    # ... and a payload


def moved_desc(d):
    t, f = d
    f = np.asarray(f, np.float32).copy()
    for a in POINTS[t]:
        f[a:a + 3] += DELTA
    return (t, [float(v) for v in f])


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


def best(f, repeats):
    out = 1e9
    for _ in range(repeats):
        t = time.perf_counter(); f(); out = min(out, time.perf_counter() - t)
    return out * 1e3


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    which = args[0] if args else "scene_d"
    repeats = int(sys.argv[sys.argv.index("--repeats") + 1]) if "--repeats" in sys.argv else 5
    descs = {"scene_d": S.scene_d, "big": lambda: S.scene_d(660, 660)}[which]()
    n = len(descs)
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    q, depth = B.compile_bvh(B.make_prims(descs))
    types, data = tree_payloads(q)
    pay = data.copy()
    for t, cols in QUADS.items():
        for c in cols:
            pay[types == t, c:c + 3] += DELTA
    r = B.Renderer(64, 64, cam)
    r.set_primitives(B.make_prims(descs))
    be = r.backend
    ordinals = torch.arange(n, dtype=torch.int32, device="cuda:0")
    payload = torch.from_numpy(pay).to("cuda:0")
    info = be.refit(ordinals[:0], payload[:0])   # binds; nothing moves
    if "--profile" in sys.argv:
        for _ in range(repeats):
            be.refit(ordinals, payload)
        print("%s: %d refits of all %d primitives + 1 of none, %d level launches each (tree depth %d)" % (which, repeats, n, info["levels"], depth))
        r.close()
        return
    print("%s: %d primitives, tree depth %d, %d record levels = level launches per refit" % (which, n, depth, info["levels"]))
    rng = np.random.default_rng(1)
    for label, k in (("1 primitive", 1), ("1 %", max(1, n // 100)), ("all", n)):
        sel = np.sort(rng.choice(n, k, replace=False))
        arr = B.make_prims([moved_desc(descs[i]) for i in sel])
        t_update = best(lambda: r.update_primitives(sel, arr) or sys.exit("update_primitives refused"), repeats)
        o, p = ordinals[torch.from_numpy(sel).to("cuda:0")].contiguous(), payload[torch.from_numpy(sel).to("cuda:0")].contiguous()
        t_refit = best(lambda: be.refit(o, p), repeats)
        print("  %-12s (%7d): UpdatePrimitives %8.3f ms   Backend.refit (device pointers) %8.3f ms" % (label, k, t_update, t_refit))
    allmoved = B.make_prims([moved_desc(d) for d in descs])
    lib, whole = None, 1e9
    for _ in range(3):
        t = time.perf_counter(); r.set_primitives(allmoved); r.finish(); whole = min(whole, time.perf_counter() - t)
        lib = min(lib or r.last_setprims_ms(), r.last_setprims_ms())
    print("  SetPrimitives of the moved scene: %.1f ms in the library (build %.1f + compile %.1f + re-layout and upload %.1f); %.1f ms call to return "
          "through the C API, which like UpdatePrimitives' figures includes making one object per description" % (tuple(lib) + (whole * 1e3,)))
    r.close()


if __name__ == "__main__":
    main()
