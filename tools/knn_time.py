#!/usr/bin/env python3
"""What the k nearest (include/gpuart_nearest.h, "k nearest") cost on one GPU. One scene per process, each under a time limit of its own,
the second only if the first ended well:

    timeout -k 10 600 python3 tools/knn_time.py --scene scene_d --out profiles/knn.txt && \\
    timeout -k 10 900 python3 tools/knn_time.py --scene big --out profiles/knn.txt --append

per scene — scene_d (cfg3's, 100 k triangles) or big (dragon871k = scene_d(660, 660)) — N = 2^20 queries of three kinds, from a seed, all
with r = +inf:

  surface  points within 1e-3 of the surface: the hit points of Backend.gbuffer's camera rays, each displaced by up to 1e-3 in a uniform direction
  box      points uniform in the root box
  far      points on the sphere of three root extents about the root box's centre

and per kind k = 1, 8 and 32. Per point (scene, kind, k):

  knn      the walk in ms from HIP events (gpuart_nearest_knn_step_ms): 2 warm-up rounds, then R rounds (default 7), alternating with
  closest  closest_points (gpuart_nearest_run) on the same points in the same rounds — the baseline: median and range of both, Mqueries/s,
           and the ratio of the medians. At k = 1 the two outputs are compared bit for bit first
  spread   the k-nearest walk against itself: a second handle of the same library in the same rounds, the ratio of the two medians
  parent   gpuart_amd/lib_ab/libgpuart_nearest_parent.so, if it is there — the library of another commit, copied there by hand —, in the same
           rounds: shipped / parent time beside the spread, half the range of the parent's rounds, and its records compared with the shipped ones
  route    what a caller did before, on the first N / 4 queries, 1 warm-up round and 3 rounds: `within` at the radius whose mean list is k
           items long (bisection on the count over the first 2^16 queries; 2^12 of the far points, whose lists grow to the whole scene
           within the bracket), count + scan + fill from HIP events, then the items copied to the host and sorted there by (query, d2,
           ordinal) with NumPy, call to return. The lists of that route hold k items in the mean, not k each: it answers another
           question, at a guessed radius, and is the nearest thing to compare with

Nothing here is a pass/fail threshold."""
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

OUT = []
KS = (1, 8, 32)


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


PARENT = os.path.join(ROOT, "gpuart_amd", "lib_ab", "libgpuart_nearest_parent.so")


class Handle:
    """A gpuart_nearest of the shipped library, or of the library at `path`."""

    def __init__(self, path=None):
        self.L = C.CDLL(path) if path else B.nearest_lib()
        self.L.gpuart_nearest_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self.chk(self.L.gpuart_nearest_create(C.c_int(0), C.byref(self.h)))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.gpuart_nearest_last_error().decode())

    def bind(self, scene):
        self.chk(self.L.gpuart_nearest_bind(self.h, C.byref(scene)))

    def knn(self, scene, points, k, hits):
        """-> the walk's ms."""
        self.chk(self.L.gpuart_nearest_knn_run(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), C.c_size_t(k), None,
                                               C.c_void_p(hits.data_ptr())))
        self.chk(self.L.gpuart_nearest_finish(self.h))
        ms = (C.c_double * 1)()
        self.chk(self.L.gpuart_nearest_knn_step_ms(self.h, ms))
        return ms[0]

    def nearest(self, scene, points, hits):
        """-> the walk's ms."""
        self.chk(self.L.gpuart_nearest_run(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None, C.c_void_p(hits.data_ptr())))
        self.chk(self.L.gpuart_nearest_finish(self.h))
        ms = (C.c_double * 2)()
        self.chk(self.L.gpuart_nearest_step_ms(self.h, ms))
        return ms[1]

    def count(self, scene, points, offsets):
        """-> the total; one above the cap is a value like any other (the bisection starts far above its target)."""
        total = C.c_uint64(0)
        self.chk(self.L.gpuart_nearest_within_count(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None,
                                                    C.c_void_p(offsets.data_ptr())))
        rc = self.L.gpuart_nearest_within_total(self.h, C.byref(total))
        if total.value <= 0x7fffffff:
            self.chk(rc)
        return total.value

    def within_ms(self):
        ms = (C.c_double * 3)()
        self.chk(self.L.gpuart_nearest_within_step_ms(self.h, ms))
        return sum(ms)

    def last_blocks(self):
        blocks = C.c_uint32()
        self.chk(self.L.gpuart_nearest_last_launch(self.h, C.byref(blocks), None))
        return blocks.value

    def close(self):
        self.L.gpuart_nearest_destroy(self.h)


def workloads(be, scene, n, side):
    """name -> (n, 3) device tensor of points."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, device="cuda:0", generator=g)
    lo = torch.tensor(scene.root_min[:], device="cuda:0")
    hi = torch.tensor(scene.root_max[:], device="cuda:0")
    hits = torch.empty((side, side, 8), dtype=torch.float32, device="cuda:0")
    prims = torch.empty((side, side), dtype=torch.int32, device="cuda:0")
    be.gbuffer(out=hits, prims_out=prims)
    hits = hits.reshape(-1, 8)
    on = hits[hits[:, 7].view(torch.int32) >= 0][:, 1:4]
    on = on[torch.randint(0, on.shape[0], (n,), device="cuda:0", generator=g)]
    d = torch.randn(n, 3, device="cuda:0", generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    f = torch.randn(n, 3, device="cuda:0", generator=g)
    f = f / f.norm(dim=1, keepdim=True)
    return {"surface": on + d * rnd(n, 1) * 1e-3, "box": lo + rnd(n, 3) * (hi - lo), "far": (lo + hi) / 2 + f * 3 * (hi - lo).max()}


def with_radius(p, r):
    import torch
    return torch.cat([p, torch.full((p.shape[0], 1), float(r), device=p.device)], 1).contiguous()


def radius_for(h, scene, p, target, extent):
    """The radius at which the mean list of the queries p is about `target` items long: 24 bisection steps on the count, below four root
    extents (the far points are three away)."""
    import torch
    offsets = torch.zeros(p.shape[0] + 1, dtype=torch.int32, device=p.device)
    lo, hi = 0.0, 4 * extent
    for _ in range(24):
        mid = (lo + hi) / 2
        if h.count(scene, with_radius(p, mid), offsets) / p.shape[0] < target:
            lo = mid
        else:
            hi = mid
    return hi


def main():
    import numpy as np
    import torch
    arg = lambda name, default, kind=int: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats, n, out_path, which = arg("--repeats", 7), arg("--queries", 1 << 20), arg("--out", "", str), arg("--scene", "scene_d", str)
    make = {"scene_d": S.scene_d, "big": lambda: S.scene_d(660, 660)}[which]
    side = int(round(n ** 0.5))
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    first, again = Handle(), Handle()
    parent = Handle(PARENT) if os.path.exists(PARENT) else None
    say("k nearest on %s; %d queries per kind, r = +inf, median (range) of %d rounds after 2 warm-up rounds; times in ms" % (torch.cuda.get_device_name(0), n, repeats))
    r = B.Renderer(side, side, cam)
    r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
    r.set_primitives(B.make_prims(make())); r.finish()
    be = r.backend
    scene = be.scene_device()
    extent = max(b - a for a, b in zip(scene.root_min[:], scene.root_max[:]))
    say("%s: %d primitives, %d records, depth %d, root extent %.4g" % (which, scene.n_prims, scene.n_recs, scene.max_depth, extent))
    first.bind(scene); again.bind(scene)
    if parent:
        parent.bind(scene)
    for kind, p in workloads(be, scene, n, side).items():
        points = with_radius(p, float("inf"))
        one = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
        for k in KS:
            hits = torch.empty((n, k, 8), dtype=torch.float32, device="cuda:0")
            ms = {"knn": [], "again": [], "closest": [], "parent": []}
            theirs = torch.empty_like(hits) if parent else None
            for round_ in range(repeats + 2):
                for name, t in (("knn", first.knn(scene, points, k, hits)), ("closest", first.nearest(scene, points, one)), ("again", again.knn(scene, points, k, hits))) + (
                        (("parent", parent.knn(scene, points, k, theirs)),) if parent else ()):
                    if round_ >= 2:
                        ms[name].append(t)
            blocks = again.last_blocks()
            med = {name: statistics.median(v) for name, v in ms.items() if v}
            same = ""
            if parent:
                same = "; knn / parent time %.3f (half the range of the parent's rounds: %.1f %%), records %s" % (
                    med["knn"] / med["parent"], 50 * (max(ms["parent"]) - min(ms["parent"])) / med["parent"],
                    "bit-identical" if torch.equal(hits.view(torch.int32), theirs.view(torch.int32)) else "DIFFER")
            if k == 1:
                same += "; k = 1 against closest_points: " + ("bit-identical" if torch.equal(hits.view(torch.int32).reshape(n, 8), one.view(torch.int32)) else "DIFFER")
            found = float((hits[:, :, 5].view(torch.int32) != -1).sum()) / n
            say("  %-8s k = %-2d  knn %s = %.1f Mq/s on %d workgroups | closest_points %s = %.1f Mq/s | knn / closest time %.2f | same build twice %+.1f %% | %.2f found per query%s"
                % (kind, k, spread(ms["knn"]), n / med["knn"] / 1e3, blocks, spread(ms["closest"]), n / med["closest"] / 1e3, med["knn"] / med["closest"],
                   100 * (med["again"] / med["knn"] - 1), found, same))
            # the route through the neighbour lists
            m = n // 4
            radius = radius_for(first, scene, p[:1 << (12 if kind == "far" else 16)], k, extent)
            listed = with_radius(p[:m], radius)
            dev, wall, total = [], [], 0
            for round_ in range(4):
                torch.cuda.synchronize()
                t = time.perf_counter()
                offsets, items = be.within(listed, max_items=0x7fffffff)
                dev_ms = be._nearest_handle(scene)
                out = (C.c_double * 3)()
                B.nearest_lib().gpuart_nearest_within_step_ms(dev_ms, out)
                rows = items.cpu().numpy()
                lengths = np.diff(offsets.cpu().numpy().astype(np.int64))
                order = np.lexsort((rows[:, 5].view(np.uint32), rows[:, 4], np.repeat(np.arange(m), lengths)))
                rows = rows[order]
                took = (time.perf_counter() - t) * 1e3
                total = len(rows)
                if round_ >= 1:
                    dev.append(sum(out)); wall.append(took)
            say("            within at r = %.6g (%.3g of the extent, %.2f items per query) + host sort, %d queries: count + scan + fill %s, with the copy and the sort, call to return %s"
                " = %.2f Mq/s | per query knn takes 1 / %.1f of the device passes' time and 1 / %.0f of the whole route's"
                % (radius, radius / extent, total / m, m, spread(dev), spread(wall), m / statistics.median(wall) / 1e3, statistics.median(dev) * (n / m) / med["knn"],
                   statistics.median(wall) * (n / m) / med["knn"]))
            del hits, theirs, rows, items, offsets
    be.close()
    r.close()
    say("NOT MEASURED: mixed-type scenes at this size (both scenes are triangles only); a register-resident list for k <= 4; a k per query; user "
        "spheres; host-memory (staged) calls; a sorted insertion list in place of the heap")
    first.close(); again.close()
    if parent:
        parent.close()
    if out_path:
        with open(out_path, "a" if "--append" in sys.argv else "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
