#!/usr/bin/env python3
"""What box-overlap queries and overlapping-pair lists (include/gpuart_nearest.h, "Box overlap") cost on one GPU, in one process:

    make -C gpuart_amd/csrc nearest-variants      # the plain form of the kernels and the counting builds, into gpuart_amd/lib_ab/
    python3 tools/overlap_time.py [--repeats R] [--queries N] [--out profiles/overlap.txt]

per scene — scene_d (cfg3's, 100 352 triangles) and big (dragon871k = scene_d(660, 660)):

  pairs    gpuart_nearest_pairs_count / _fill over the scene's own boxes at margin 0 and at the margins, found by bisection on the count,
           whose mean list is about 8 and about 64 items long: count, scan and fill in ms from HIP events (gpuart_nearest_overlap_step_ms),
           1 warm-up round, then R rounds (default 7), median and range; Mprimitives/s and Gitems/s over count + scan + fill
  boxes    N = 2^20 box queries — cubes centred uniformly in the root box — of three sizes, found by bisection so that the mean list is about
           1, 8 and 64 items long, the same way
  plain    the persistent-lane form against the NEAREST_PLAIN build, alternating in the same rounds; offsets and items compared first
  spread   the shipped form against itself: a second handle of the same library, alternating, the ratio of the two medians
  parent   gpuart_amd/lib_ab/libgpuart_nearest_parent.so, if it is there — the library of another commit, copied there by hand —, in the same
           rounds: shipped / parent time per pass beside the spread, and half the range of the parent's rounds, the other noise the run shows
  steps    box steps and box tests per query and pass, from the counting build (-DNEAREST_COUNT), not from the timed ones
  within   gpuart_nearest_within_count / _fill on the boxes' centres at the radius of the same mean list length: the only existing route
           to the same candidates, in the same run

One run; nothing here is a pass/fail threshold."""
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
from gpuart_amd import binding as B  # noqa: E402
from gpuart_amd import synth_scenes as S  # noqa: E402

AB = os.path.join(ROOT, "gpuart_amd", "lib_ab")
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

    def total(self, searching):
        total = C.c_uint64(0)
        rc = self.L.gpuart_nearest_overlap_total(self.h, C.byref(total))
        if not (searching and total.value > 0x7fffffff):
            self.chk(rc)
        return total.value

    def pairs_count(self, scene, margin, offsets, searching=False):
        self.chk(self.L.gpuart_nearest_pairs_count(self.h, C.byref(scene), C.c_float(margin), C.c_void_p(offsets.data_ptr())))
        return self.total(searching)

    def pairs_fill(self, scene, margin, offsets, items):
        self.chk(self.L.gpuart_nearest_pairs_fill(self.h, C.byref(scene), C.c_float(margin), C.c_void_p(offsets.data_ptr()), C.c_void_p(items.data_ptr()),
                                                  C.c_size_t(items.shape[0])))
        self.chk(self.L.gpuart_nearest_finish(self.h))

    def count(self, scene, boxes, offsets, searching=False):
        self.chk(self.L.gpuart_nearest_overlap_count(self.h, C.byref(scene), C.c_void_p(boxes.data_ptr()), C.c_size_t(boxes.shape[0]), C.c_float(0), None,
                                                     C.c_void_p(offsets.data_ptr())))
        return self.total(searching)

    def fill(self, scene, boxes, offsets, items):
        self.chk(self.L.gpuart_nearest_overlap_fill(self.h, C.byref(scene), C.c_void_p(boxes.data_ptr()), C.c_size_t(boxes.shape[0]), C.c_float(0), None,
                                                    C.c_void_p(offsets.data_ptr()), C.c_void_p(items.data_ptr()), C.c_size_t(items.shape[0])))
        self.chk(self.L.gpuart_nearest_finish(self.h))

    def step_ms(self):
        ms = (C.c_double * 3)()
        self.chk(self.L.gpuart_nearest_overlap_step_ms(self.h, ms))
        return tuple(ms)

    def counts(self):
        out = (C.c_uint64 * 2)()
        self.chk(self.L.gpuart_nearest_overlap_counts(self.h, out))
        return int(out[0]), int(out[1])

    def within_count(self, scene, points, offsets, searching=False):
        self.chk(self.L.gpuart_nearest_within_count(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None,
                                                    C.c_void_p(offsets.data_ptr())))
        total = C.c_uint64(0)
        rc = self.L.gpuart_nearest_within_total(self.h, C.byref(total))
        if not (searching and total.value > 0x7fffffff):
            self.chk(rc)
        return total.value

    def within_fill(self, scene, points, offsets, items):
        self.chk(self.L.gpuart_nearest_within_fill(self.h, C.byref(scene), C.c_void_p(points.data_ptr()), C.c_size_t(points.shape[0]), None,
                                                   C.c_void_p(offsets.data_ptr()), C.c_void_p(items.data_ptr()), C.c_size_t(items.shape[0])))
        self.chk(self.L.gpuart_nearest_finish(self.h))

    def within_ms(self):
        ms = (C.c_double * 3)()
        self.chk(self.L.gpuart_nearest_within_step_ms(self.h, ms))
        return tuple(ms)

    def close(self):
        self.L.gpuart_nearest_destroy(self.h)


def variant(name):
    path = os.path.join(AB, "libgpuart_nearest_%s.so" % name)
    return Handle(path) if os.path.exists(path) else None


def bisect(mean_of, target, hi, steps=18):
    """The parameter in (0, hi] at which mean_of(parameter) is about `target`."""
    lo = 0.0
    for _ in range(steps):
        mid = (lo + hi) / 2
        if mean_of(mid) < target:
            lo = mid
        else:
            hi = mid
    return hi


def timed(forms, rounds, run, read):
    """name -> three lists of ms (count, scan, fill) over `rounds` rounds after one warm-up round, the forms alternating."""
    ms = {name: ([], [], []) for name, _ in forms}
    for round_ in range(rounds + 1):
        for name, h in forms:
            run(name, h)
            if round_ >= 1:
                for k, t in enumerate(read(h)):
                    ms[name][k].append(t)
    return ms


def report(label, ms, n, total, unit):
    for name, v in ms.items():
        c, s, f = (statistics.median(x) for x in v)
        say("            %-10s count %s  scan %s  fill %s  | %.1f M%s/s and %.3f Gitems/s over the three" % (name, spread(v[0]), spread(v[1]), spread(v[2]),
                                                                                                          n / (c + s + f) / 1e3, unit, total / (c + s + f) / 1e6))
    med = lambda name, k: statistics.median(ms[name][k])
    if "plain" in ms:
        say("            plain / persistent time: count %.3f, fill %.3f" % (med("plain", 0) / med("persistent", 0), med("plain", 2) / med("persistent", 2)))
    if "again" in ms:
        line = "            same build twice: count %+.1f %%, fill %+.1f %%" % tuple(100 * (med("again", k) / med("persistent", k) - 1) for k in (0, 2))
        if "parent" in ms:
            line += "; persistent / parent time: count %.3f, fill %.3f (half the range of the parent's rounds: count %.1f %%, fill %.1f %%)" % (
                tuple(med("persistent", k) / med("parent", k) for k in (0, 2))
                + tuple(50 * (max(ms["parent"][k]) - min(ms["parent"][k])) / med("parent", k) for k in (0, 2)))
        say(line)


def main():
    import torch
    arg = lambda name, default, kind=int: kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default
    repeats, n, out_path = arg("--repeats", 7), arg("--queries", 1 << 20), arg("--out", "", str)
    cam = dict(S.BENCH_CAMERA); cam["dir"] = S.camera_dir(cam)
    shipped, again = (Handle(os.path.join(B.LIBDIR, "libgpuart_nearest.so")) for _ in range(2))
    plain, counting, parent = variant("plain"), variant("count"), variant("parent")
    if not (plain and counting):
        say("the variants are not built (make -C gpuart_amd/csrc nearest-variants): the plain form and the step counts are NOT MEASURED")
    say("box overlap on %s; median (range) of %d rounds after 1 warm-up round, one run; times in ms" % (torch.cuda.get_device_name(0), repeats))
    forms = [("persistent", shipped), ("again", again)] + ([("plain", plain)] if plain else []) + ([("parent", parent)] if parent else [])
    for which, make in (("scene_d", S.scene_d), ("big", lambda: S.scene_d(660, 660))):
        r = B.Renderer(64, 64, cam)
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0, 0.0)
        r.set_primitives(B.make_prims(make())); r.finish()
        be = r.backend
        scene = be.scene_device()
        P = int(scene.n_prims)
        extent = max(b - a for a, b in zip(scene.root_min[:], scene.root_max[:]))
        say("%s: %d primitives, %d records, depth %d, root extent %.4g" % (which, P, scene.n_recs, scene.max_depth, extent))
        for h in (shipped, again, plain, counting, parent):
            if h:
                h.bind(scene)
        # ---- pairs
        off = {name: torch.zeros(P + 1, dtype=torch.int32, device="cuda:0") for name, _ in forms}
        mean = lambda m: shipped.pairs_count(scene, m, off["persistent"], searching=True) / P
        margins = [("margin 0", 0.0)] + [("mean list about %d" % t, bisect(mean, t, extent / 8)) for t in (8, 64)]
        for label, margin in margins:
            total = shipped.pairs_count(scene, margin, off["persistent"])
            items = {name: torch.empty((total,), dtype=torch.int32, device="cuda:0") for name, _ in forms}

            def run(name, h):
                assert h.pairs_count(scene, margin, off[name]) == total
                h.pairs_fill(scene, margin, off[name], items[name])

            ms = timed(forms, repeats, run, lambda h: h.step_ms())
            same = all(torch.equal(off["persistent"], off[name]) and torch.equal(items["persistent"], items[name]) for name, _ in forms)
            say("  pairs, %s: margin %.6g (%.3g of the extent): %d pairs, %.2f per primitive; offsets and items of all forms %s"
                % (label, margin, margin / extent, total, total / P, "identical" if same else "DIFFER"))
            report(label, ms, P, total, "primitives")
            if counting:
                counting.counts()
                counting.pairs_count(scene, margin, off["persistent"])
                cb, ct = counting.counts()
                say("            counting build: count pass %.1f box steps and %.1f box tests per primitive" % (cb / P, ct / P))
            del items
        # ---- box queries, and within beside them
        g = torch.Generator(device="cuda:0").manual_seed(5)
        lo = torch.tensor(scene.root_min[:], device="cuda:0")
        hi = torch.tensor(scene.root_max[:], device="cuda:0")
        centre = lo + torch.rand(n, 3, device="cuda:0", generator=g) * (hi - lo)
        cubes = lambda half: torch.cat([centre - half, centre + half], 1).contiguous()
        balls = lambda radius: torch.cat([centre, torch.full((n, 1), float(radius), device="cuda:0")], 1).contiguous()
        off = {name: torch.zeros(n + 1, dtype=torch.int32, device="cuda:0") for name, _ in forms}
        sample = 1 << 16
        soff = torch.zeros(sample + 1, dtype=torch.int32, device="cuda:0")
        for target in (1, 8, 64):
            half = bisect(lambda x: shipped.count(scene, cubes(x)[:sample].contiguous(), soff, searching=True) / sample, target, extent / 8)
            boxes = cubes(half)
            total = shipped.count(scene, boxes, off["persistent"])
            items = {name: torch.empty((total,), dtype=torch.int32, device="cuda:0") for name, _ in forms}

            def run(name, h):
                assert h.count(scene, boxes, off[name]) == total
                h.fill(scene, boxes, off[name], items[name])

            ms = timed(forms, repeats, run, lambda h: h.step_ms())
            same = all(torch.equal(off["persistent"], off[name]) and torch.equal(items["persistent"], items[name]) for name, _ in forms)
            say("  boxes, mean list about %d: half edge %.6g (%.3g of the extent): %d items, %.2f per query; offsets and items of all forms %s"
                % (target, half, half / extent, total, total / n, "identical" if same else "DIFFER"))
            report("boxes", ms, n, total, "queries")
            if counting:
                counting.counts()
                counting.count(scene, boxes, off["persistent"])
                cb, ct = counting.counts()
                say("            counting build: count pass %.1f box steps and %.1f box tests per query" % (cb / n, ct / n))
            del items
            radius = bisect(lambda x: shipped.within_count(scene, balls(x)[:sample].contiguous(), soff, searching=True) / sample, target, extent / 8)
            points = balls(radius)
            wtotal = shipped.within_count(scene, points, off["persistent"])
            hits = torch.empty((wtotal, 8), dtype=torch.float32, device="cuda:0")

            def wrun(name, h):
                assert h.within_count(scene, points, off["persistent"]) == wtotal
                h.within_fill(scene, points, off["persistent"], hits)

            wms = timed([("within", shipped)], repeats, wrun, lambda h: h.within_ms())
            say("            within on the centres, r = %.6g: %d items, %.2f per query" % (radius, wtotal, wtotal / n))
            report("within", wms, n, wtotal, "queries")
            del hits
        be.close()
        r.close()
    say("NOT MEASURED: skipping subtrees by ordinal range in the pairs (every pair's walk is done from both sides and the half with j <= i is discarded: "
        "the records hold no per-record maximum ordinal); mixed-type scenes at this size; user spheres; the host-memory (staged) calls; a margin per query")
    for h in (shipped, again, plain, counting, parent):
        if h:
            h.close()
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
