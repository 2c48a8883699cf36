#!/usr/bin/env python3
"""What neighbour lists (include/gpuart_nearest.h, "Neighbour lists") cost on one GPU, in one process:

    make -C gpuart_amd/csrc nearest-variants      # the plain form of the kernels and the counting builds, into gpuart_amd/lib_ab/
    python3 tools/within_time.py [--repeats R] [--queries N] [--out profiles/within.txt]

per scene — scene_d (cfg3's, 100 k triangles) and big (dragon871k = scene_d(660, 660)) — N = 2^20 queries of two kinds, from a seed:

  surface  points within 1e-3 of the surface: the hit points of Backend.gbuffer's camera rays, each displaced by up to 1e-3 in a uniform direction
  box      points uniform in the root box

and per kind three radii, found by bisection on the count pass over the first 2^16 queries so that the mean list is about 1, 8 and 64 items
long. Per point (scene, kind, radius):

  passes   count, scan and fill in ms from HIP events (gpuart_nearest_within_step_ms): 2 warm-up rounds, then R rounds, the shipped
           (persistent-lane) form and the plain form alternating; median and range. Mqueries/s over count + scan + fill, Mitems/s over the
           fill, and the fill's 32 bytes per item over its time against the HBM peak (8.0 TB/s: MI355X_MICROARCH.md) — the bytes the result
           needs, not what the walk reads. Offsets and items of both forms are compared bit for bit first
  spread   the shipped form against itself: a second handle of the same library, alternating, the ratio of the two medians
  parent   gpuart_amd/lib_ab/libgpuart_nearest_parent.so, if it is there — the library of another commit, copied there by hand —, in the same
           rounds: shipped / parent time per pass beside the spread, and half the range of the parent's rounds, the other noise the run shows
  steps    box steps and primitive tests per query and pass, from the counting builds (-DNEAREST_COUNT), not from the timed ones
  beside   closest_points (gpuart_nearest_run) on the same points with the same r and with r = +inf, HIP events; Backend.within on device
           tensors, call to return

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

AB = os.path.join(ROOT, "gpuart_amd", "lib_ab")
HBM_PEAK = 8.0e12
OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def spread(v):
    return "%.3f (%.3f .. %.3f)" % (statistics.median(v), min(v), max(v))


class Handle:
    """A gpuart_nearest of the library at `path`."""

    def __init__(self, path):
        self.L = C.CDLL(path)
        self.L.gpuart_nearest_last_error.restype = C.c_char_p
        self.h = C.c_void_p()
        self.chk(self.L.gpuart_nearest_create(C.c_int(0), C.byref(self.h)))

    def chk(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.gpuart_nearest_last_error().decode())

    def bind(self, scene):
        self.chk(self.L.gpuart_nearest_bind(self.h, C.byref(scene)))

    def count(self, scene, points, offsets, searching=False):
        """-> the total. searching: a total above the cap is a value like any other (the bisection starts far above its target)."""
        total = C.c_uint64(0)
        self.chk(self.L.gpuart_nearest_within_count(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None,
                                                    C.c_void_p(offsets.data_ptr())))
        rc = self.L.gpuart_nearest_within_total(self.h, C.byref(total))
        if not (searching and total.value > 0x7fffffff):
            self.chk(rc)
        return total.value

    def fill(self, scene, points, offsets, items):
        self.chk(self.L.gpuart_nearest_within_fill(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None,
                                                   C.c_void_p(offsets.data_ptr()), C.c_void_p(items.data_ptr()), C.c_size_t(items.shape[0])))
        self.chk(self.L.gpuart_nearest_finish(self.h))

    def step_ms(self):
        ms = (C.c_double * 3)()
        self.chk(self.L.gpuart_nearest_within_step_ms(self.h, ms))
        return tuple(ms)

    def counts(self):
        out = (C.c_uint64 * 2)()
        self.chk(self.L.gpuart_nearest_within_counts(self.h, out))
        return int(out[0]), int(out[1])

    def nearest(self, scene, points, hits):
        """-> the walk's ms."""
        self.chk(self.L.gpuart_nearest_run(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None, C.c_void_p(hits.data_ptr())))
        self.chk(self.L.gpuart_nearest_finish(self.h))
        ms = (C.c_double * 2)()
        self.chk(self.L.gpuart_nearest_step_ms(self.h, ms))
        return ms[1]

    def close(self):
        self.L.gpuart_nearest_destroy(self.h)


def variant(name):
    path = os.path.join(AB, "libgpuart_nearest_%s.so" % name)
    return Handle(path) if os.path.exists(path) else None


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
    return {"surface": on + d / d.norm(dim=1, keepdim=True) * rnd(n, 1) * 1e-3, "box": lo + rnd(n, 3) * (hi - lo)}


def with_radius(p, r):
    import torch
    return torch.cat([p, torch.full((p.shape[0], 1), float(r), device=p.device)], 1).contiguous()


def radius_for(h, scene, p, target, extent):
    """The radius at which the mean list of the queries p is about `target` items long: 20 bisection steps on the count, below a sixteenth
    of the root extent."""
    import torch
    offsets = torch.zeros(p.shape[0] + 1, dtype=torch.int32, device=p.device)
    lo, hi = 0.0, extent / 16
    for _ in range(20):
        mid = (lo + hi) / 2
        if h.count(scene, with_radius(p, mid), offsets, searching=True) / p.shape[0] < target:
            lo = mid
        else:
            hi = mid
    return hi


def main():
    import torch
    arg = lambda name, default, kind=int: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats, n, out_path = arg("--repeats", 7), arg("--queries", 1 << 20), arg("--out", "", str)
    side = int(round(n ** 0.5))
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    shipped_path = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    shipped, again = Handle(shipped_path), Handle(shipped_path)
    plain, count, plain_count, parent = variant("plain"), variant("count"), variant("plain_count"), variant("parent")
    if not (plain and count and plain_count):
        say("the variants are not built (make -C gpuart_amd/csrc nearest-variants): the plain form and the step counts are NOT MEASURED")
    say("neighbour lists on %s; %d queries per kind, median (range) of %d rounds after 2 warm-up rounds; times in ms" % (torch.cuda.get_device_name(0), n, repeats))
    verdict = []
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        r = B.Renderer(side, side, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(B.make_prims(make())); r.finish()
        be = r.backend
        scene = be.scene_device()
        extent = max(b - a for a, b in zip(scene.root_min[:], scene.root_max[:]))
        say("%s: %d primitives, %d records, depth %d, root extent %.4g" % (which, scene.n_prims, scene.n_recs, scene.max_depth, extent))
        forms = [("persistent", shipped), ("again", again)] + ([("plain", plain)] if plain else []) + ([("parent", parent)] if parent else [])
        for _, h in forms:
            h.bind(scene)
        for c in (count, plain_count):
            if c:
                c.bind(scene)
        for kind, p in workloads(be, scene, n, side).items():
            for target in (1, 8, 64):
                radius = radius_for(shipped, scene, p[:1 << 16], target, extent)
                points = with_radius(p, radius)
                offsets = {name: torch.zeros(n + 1, dtype=torch.int32, device="cuda:0") for name, _ in forms}
                total = shipped.count(scene, points, offsets["persistent"])
                items = {name: torch.empty((total, 8), dtype=torch.float32, device="cuda:0") for name, _ in forms}
                ms = {name: ([], [], []) for name, _ in forms}
                for round_ in range(repeats + 2):
                    for name, h in forms:
                        assert h.count(scene, points, offsets[name]) == total
                        h.fill(scene, points, offsets[name], items[name])
                        if round_ >= 2:
                            for k, t in enumerate(h.step_ms()):
                                ms[name][k].append(t)
                same = all(torch.equal(offsets["persistent"], offsets[name]) and torch.equal(items["persistent"].view(torch.int32), items[name].view(torch.int32))
                           for name, _ in forms)
                say("  %-8s r = %.6g (%.3g of the extent): %d items, %.2f per query; offsets and items of all forms %s"
                    % (kind, radius, radius / extent, total, total / n, "bit-identical" if same else "DIFFER"))
                med = {}
                for name, _ in forms:
                    c, s, f = (statistics.median(v) for v in ms[name])
                    med[name] = (c, s, f)
                    say("            %-10s count %s  scan %s  fill %s  | %.1f Mq/s over the three, fill %.1f Mitems/s = %.2f %% of the HBM peak for its 32 B per item"
                        % (name, spread(ms[name][0]), spread(ms[name][1]), spread(ms[name][2]), n / (c + s + f) / 1e3, total / f / 1e3, 100 * total * 32 / (f * 1e-3) / HBM_PEAK))
                noise = [abs(med["again"][k] / med["persistent"][k] - 1) for k in (0, 2)]
                line = "            same build twice: count %+.1f %%, fill %+.1f %%" % tuple(100 * (med["again"][k] / med["persistent"][k] - 1) for k in (0, 2))
                if plain:
                    ratio = [med["plain"][k] / med["persistent"][k] for k in (0, 2)]
                    line += "; plain / persistent time: count %.3f, fill %.3f" % tuple(ratio)
                    verdict.append(all(ratio[k] < 1 - noise[k] for k in (0, 1)))
                if parent:
                    line += "; persistent / parent time: count %.3f, fill %.3f (half the range of the parent's rounds: count %.1f %%, fill %.1f %%)" % (
                        tuple(med["persistent"][k] / med["parent"][k] for k in (0, 2))
                        + tuple(50 * (max(ms["parent"][k]) - min(ms["parent"][k])) / med["parent"][k] for k in (0, 2)))
                say(line)
                for name, c in (("persistent", count), ("plain", plain_count)):
                    if c:
                        c.counts()
                        c.count(scene, points, offsets["again"])
                        cb, ct = c.counts()
                        c.fill(scene, points, offsets["again"], items["again"])
                        fb, ft = c.counts()
                        say("            %s, counting build: count pass %.1f box steps and %.1f primitive tests per query, fill pass %.1f and %.1f"
                            % (name, cb / n, ct / n, fb / n, ft / n))
                hits = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
                inf = with_radius(p, float("inf"))
                near = {"the same r": [], "r = +inf": []}
                for round_ in range(repeats + 2):
                    for label, q in (("the same r", points), ("r = +inf", inf)):
                        t = shipped.nearest(scene, q, hits)
                        if round_ >= 2:
                            near[label].append(t)
                wall = []
                for round_ in range(repeats + 2):
                    torch.cuda.synchronize()
                    t = time.perf_counter(); be.within(points); wall.append((time.perf_counter() - t) * 1e3)
                say("            closest_points on the same points: %s with the same r, %s with r = +inf; Backend.within on device tensors, call to return: %s"
                    % (spread(near["the same r"]), spread(near["r = +inf"]), spread(wall[2:])))
                del items, offsets, hits
        be.close()
        r.close()
    if verdict:
        say("the plain form is faster than the persistent one by more than the same-build spread, in both passes, at %d of %d points" % (sum(verdict), len(verdict)))
    say("NOT MEASURED: mixed-type scenes at this size (both scenes are triangles only); a one-pass variant with a fixed number of slots per query; "
        "user spheres; host-memory (staged) calls")
    for h in (shipped, again, plain, count, plain_count, parent):
        if h:
            h.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
