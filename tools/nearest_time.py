#!/usr/bin/env python3
"""What closest-point queries (include/gpuart_nearest.h) cost on one GPU, in one process:

    make -C gpuart_amd/csrc nearest-variants      # the plain form of k_nearest and the counting builds, into gpuart_amd/lib_ab/
    python3 tools/nearest_time.py [--repeats R] [--queries N]

per scene — scene_d (cfg3's, 100 k triangles) and big (dragon871k = scene_d(660, 660)) — N = 2^20 queries with r = +inf of three kinds:

  surface  points within 1e-3 of the surface: the hit points of Backend.gbuffer's camera rays, each displaced by up to 1e-3 per axis
  box      points uniform in the root box
  far      points at three root extents from the root box's centre, in uniform directions

and per kind:

  rate     Mqueries/s of the shipped library (persistent lanes) and of the plain form (one thread per query, grid stride), from HIP events
           around the launch (gpuart_nearest_step_ms): 2 warm-up launches each, then R launches of each, alternating; median and range.
           All forms' records are compared bit for bit first: faster and different is not faster
  spread   the shipped form against itself: a second handle of the same library in the same rounds, the ratio of the two medians
  parent   gpuart_amd/lib_ab/libgpuart_nearest_parent.so, if it is there — the library of another commit, copied there by hand —, in the same
           rounds: shipped / parent time beside the spread, and half the range of the parent's rounds, the other noise the run shows
  steps    box steps (records read) and primitive tests per query, from the counting builds (-DNEAREST_COUNT), not from the timed ones
  rays     Backend.trace_rays closest-hit on as many incoherent rays (origins uniform in the root box, uniform directions), call to return
           on device tensors, in the same run: the yardstick

and per scene the nesting check of gpuart_nearest_bind (HIP events) beside a Backend.refit of 1 % of the primitives (call to return).
profiles/nearest.txt keeps the output."""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

AB = os.path.join(ROOT, "gpuart_amd", "lib_ab")


def spread(v):
    return "%.1f (%.1f .. %.1f)" % (statistics.median(v), min(v), max(v))


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

    def run(self, scene, points, hits):
        self.chk(self.L.gpuart_nearest_run(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None, C.c_void_p(hits.data_ptr())))
        self.chk(self.L.gpuart_nearest_finish(self.h))

    def step_ms(self):
        ms = (C.c_double * 2)()
        self.chk(self.L.gpuart_nearest_step_ms(self.h, ms))
        return ms[0], ms[1]

    def counts(self):
        out = (C.c_uint64 * 2)()
        self.chk(self.L.gpuart_nearest_counts(self.h, out))
        return int(out[0]), int(out[1])

    def close(self):
        self.L.gpuart_nearest_destroy(self.h)


def variant(name):
    path = os.path.join(AB, "libgpuart_nearest_%s.so" % name)
    return Handle(path) if os.path.exists(path) else None


def workloads(be, scene, n, side):
    """name -> (n, 4) device tensor."""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(5)
    rnd = lambda *shape: torch.rand(*shape, device="cuda:0", generator=g)
    lo = torch.tensor(scene.root_min[:], device="cuda:0")
    hi = torch.tensor(scene.root_max[:], device="cuda:0")
    inf = torch.full((n, 1), float("inf"), device="cuda:0")
    hits = torch.empty((side, side, 8), dtype=torch.float32, device="cuda:0")
    prims = torch.empty((side, side), dtype=torch.int32, device="cuda:0")
    be.gbuffer(out=hits, prims_out=prims)
    hits = hits.reshape(-1, 8)
    on = hits[hits[:, 7].view(torch.int32) >= 0][:, 1:4]
    on = on[torch.randint(0, on.shape[0], (n,), device="cuda:0", generator=g)]
    d = torch.randn(n, 3, device="cuda:0", generator=g)
    d = d / d.norm(dim=1, keepdim=True)
    return {
        "surface": torch.cat([on + (rnd(n, 3) * 2 - 1) * 1e-3, inf], 1).contiguous(),
        "box": torch.cat([lo + rnd(n, 3) * (hi - lo), inf], 1).contiguous(),
        "far": torch.cat([(lo + hi) / 2 + 3 * (hi - lo) * d, inf], 1).contiguous(),
    }, on.shape[0]


def main():
    import torch
    arg = lambda name, default: int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats, n = arg("--repeats", 7), arg("--queries", 1 << 20)
    side = int(round(n ** 0.5))
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    shipped_path = os.path.join(B.LIBDIR, "libgpuart_nearest.so")
    shipped, again = Handle(shipped_path), Handle(shipped_path)
    plain, count, plain_count, parent = variant("plain"), variant("count"), variant("plain_count"), variant("parent")
    if not (plain and count and plain_count):
        print("the variants are not built (make -C gpuart_amd/csrc nearest-variants): the plain form and the step counts are NOT MEASURED")
    hip = C.CDLL("libamdhip64.so")
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        r = B.Renderer(side, side, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(B.make_prims(make())); r.finish()
        be = r.backend
        scene = be.scene_device()
        print("%s: %d primitives, %d records, depth %d" % (which, scene.n_prims, scene.n_recs, scene.max_depth))
        sets, surface_pixels = workloads(be, scene, n, side)
        print("  %d queries per kind; the surface points come from %d hit pixels of a %d x %d frame" % (n, surface_pixels, side, side))
        forms = [("persistent", shipped), ("again", again)] + ([("plain", plain)] if plain else []) + ([("parent", parent)] if parent else [])
        checks = []
        for _, h in forms:
            for _ in range(3):
                h.bind(scene)
                checks.append(h.step_ms()[0])
        for c in (count, plain_count):
            if c:
                c.bind(scene)
        for kind, points in sets.items():
            out = {name: torch.empty((n, 8), dtype=torch.float32, device="cuda:0") for name, _ in forms}
            ms = {name: [] for name, _ in forms}
            for name, h in forms:
                for _ in range(2):
                    h.run(scene, points, out[name])
            same = all(torch.equal(out["persistent"].view(torch.int32), o.view(torch.int32)) for o in out.values())
            hit_share = float((out["persistent"][:, 5].view(torch.int32) >= 0).float().mean())
            for _ in range(repeats):
                for name, h in forms:
                    h.run(scene, points, out[name])
                    ms[name].append(h.step_ms()[1])
            med = {name: statistics.median(ms[name]) for name, _ in forms}
            line = "  %-8s" % kind + "".join("  %s %s Mq/s" % (name, spread([n / t / 1e3 for t in ms[name]])) for name, _ in forms)
            line += "  same build twice %+.1f %%" % (100 * (med["again"] / med["persistent"] - 1))
            if plain:
                line += "; persistent/plain time %.3f" % (med["persistent"] / med["plain"])
            if parent:
                line += "; persistent/parent time %.3f (half the range of the parent's rounds: %.1f %%)" % (
                    med["persistent"] / med["parent"], 50 * (max(ms["parent"]) - min(ms["parent"])) / med["parent"])
            print(line + "; records of all forms %s  (%.0f %% answered)" % ("bit-identical" if same else "DIFFER", 100 * hit_share))
            for name, c in (("persistent", count), ("plain", plain_count)):
                if c:
                    c.counts()
                    c.run(scene, points, out["persistent"])
                    boxes, tests = c.counts()
                    print("            %s, counting build: %.1f box steps and %.1f primitive tests per query" % (name, boxes / n, tests / n))
            # the yardstick: as many incoherent rays
            lo, hi = points.new_tensor(scene.root_min[:]), points.new_tensor(scene.root_max[:])
            if kind == "box":
                g = torch.Generator(device="cuda:0").manual_seed(9)
                d = torch.randn(n, 3, device="cuda:0", generator=g)
                rays = torch.cat([points[:, :3], torch.full((n, 1), float("inf"), device="cuda:0"), d / d.norm(dim=1, keepdim=True),
                                  torch.zeros((n, 1), device="cuda:0")], 1).contiguous()
                rhits = torch.empty((n, 8), dtype=torch.float32, device="cuda:0")
                tr = []
                for i in range(repeats + 2):
                    t = time.perf_counter(); be.trace_rays(rays, out=rhits); tr.append((time.perf_counter() - t) * 1e3)
                print("            trace_rays, closest hit, %d incoherent rays from the same points: %s Mrays/s call to return" % (n, spread([n / t / 1e3 for t in tr[2:]])))
        # the nesting check beside a refit of 1 % of the primitives (all triangles here: the payload is rebuilt from the device records)
        prims = np.zeros((scene.n_prims, 12), np.float32)
        assert hip.hipMemcpy(prims.ctypes.data_as(C.c_void_p), C.c_void_p(scene.prims), C.c_size_t(prims.nbytes), C.c_int(2)) == 0
        ordinals = np.arange(0, scene.n_prims, 100, dtype=np.int32)
        ordinals = ordinals[(prims.view(np.uint32)[ordinals, 3] & 3) == 2]
        payload = np.zeros((len(ordinals), 16), np.float32)
        p = prims[ordinals]
        payload[:, 0:3], payload[:, 4:7], payload[:, 8:11] = p[:, 0:3], p[:, 0:3] + p[:, 4:7], p[:, 0:3] + p[:, 8:11]
        od, pd = torch.from_numpy(ordinals).to("cuda:0"), torch.from_numpy(payload).to("cuda:0")
        rf = []
        for _ in range(repeats + 1):
            t = time.perf_counter(); be.refit(od, pd); rf.append((time.perf_counter() - t) * 1e3)
        print("  nesting check of bind: %s us on the device (HIP events, %d launches); Backend.refit of %d primitives: %s us call to return"
              % (spread([1e3 * c for c in checks]), len(checks), len(ordinals), spread([1e3 * t for t in rf[1:]])))
        be.close()
        r.close()
    for h in (shipped, again, plain, count, plain_count, parent):
        if h:
            h.close()


if __name__ == "__main__":
    main()
