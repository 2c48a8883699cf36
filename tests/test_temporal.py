"""Temporal accumulation by reprojection (include/gpuart_temporal.h, libgpuart_temporal.so): the library's boundary and records, the
properties of its NumPy restatement (tests/temporal_ref.py) on G-buffers the oracle makes on the CPU, the kernel against the restatement
bit for bit, Renderer::SetTemporalHistory / ReadPreview, what the history is worth on a camera track, and the argument checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import denoise_ref as R
from tests import temporal_ref as T
from tests.util import assert_same_bits, exported, same_bits, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
SPHERE = (-0.4, 0.0, 0.2, 0.25)     # a user sphere in view of the default camera
SPHERE_2 = (0.3, -0.2, 0.3, 0.3)    # ... moved
P_A = dict(max_history=2.0, plane_tol=0.05, normal_min=0.5)   # two non-default settings
P_B = dict(max_history=32.0, plane_tol=0.005, normal_min=0.95)
TRACK = [(0.1, -3.05, 1.0), (0.25, -3.05, 1.0), (0.4, -3.05, 1.0), (0.4, -2.6, 1.0)]   # sideways, then a dolly
# (history + spatial filter) / (spatial filter alone), surface RMSE at the last view of the eight-view track, computed on the CPU by
# tools/temporal_quality.py with the oracle and the two restatements (profiles/temporal.txt); the bound is that ratio plus a quarter
# of its distance to 1.
CPU_RATIO = {"box": 0.8615, "scene_p": 0.6607}
RATIO_BOUND = {"box": 0.8961, "scene_p": 0.7455}


def cam_dict(pos):
    cam = dict(S.DEFAULT_CAMERA, pos=tuple(pos))
    cam["dir"] = S.camera_dir(cam)
    return cam


# ---- CPU: the boundary and the records --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_temporal_library_exports_exactly_its_header(lib):
    hdr = open(os.path.join(ROOT, "include", "gpuart_temporal.h")).read()
    names = sorted(set(re.findall(r"\b(gpuart_temporal_[a-z_0-9]+)\s*\(", hdr)))
    assert len(names) == 8, names
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_temporal.so")
    assert exported(path) == names
    # images alone: it links neither the renderer's back end nor the spatial filter
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart_hip.so" not in dyn and "libgpuart_denoise.so" not in dyn and "libamdhip64" in dyn, dyn
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    assert "gpuart_renderer_set_temporal_history" in host and "gpuart_renderer_read_preview" in host
    capi = open(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h")).read()
    for n in ("gpuart_renderer_set_temporal_history", "gpuart_renderer_read_preview"):
        assert re.search(r"\b%s\s*\(" % n, capi)
    # the other two device libraries gained nothing
    assert not [n for n in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so")) if "temporal" in n]
    assert not [n for n in exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_denoise.so")) if "temporal" in n]


def test_records_match_the_header(tmp_path):
    from gpuart_amd import binding as B
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_temporal.h"\n'
                   '#define V gpuart_temporal_view\n#define P gpuart_temporal_params\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(V), offsetof(V, pos), offsetof(V, bottomLeft), '
                   'offsetof(V, deltaHorz), offsetof(V, deltaVert), offsetof(V, geom), offsetof(V, userSphere), offsetof(V, userSphereFlags), '
                   'sizeof(P), offsetof(P, max_history), offsetof(P, plane_tol), offsetof(P, normal_min)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    V, P = B.TemporalView, B.TemporalParams
    assert got == [C.sizeof(V), V.pos.offset, V.bottomLeft.offset, V.deltaHorz.offset, V.deltaVert.offset, V.geom.offset, V.userSphere.offset,
                   V.userSphereFlags.offset, C.sizeof(P), P.max_history.offset, P.plane_tol.offset, P.normal_min.offset]
    assert got == [100, 0, 12, 24, 36, 48, 80, 96, 12, 0, 4, 8]
    assert B.TEMPORAL_DEFAULTS == T.DEFAULTS
    with pytest.raises(ValueError):
        B.temporal_params(dict(max_history=2, sigma=1))
    # the defaults the header's text and its functions' comments state are the restatement's
    hdr = open(os.path.join(ROOT, "include", "gpuart_temporal.h")).read()
    stated = "max_history %g, plane_tol %g, normal_min %g" % (T.DEFAULTS["max_history"], T.DEFAULTS["plane_tol"], T.DEFAULTS["normal_min"])
    assert hdr.count(stated) == 2, stated


# ---- CPU: properties of the restatement on the oracle's G-buffers -----------------------------------------------------------------
W0, H0 = 160, 120
_CPU = {}


def oracle():
    from oracle import oracle as O
    return O


def cpu_tree(name):
    if ("tree", name) not in _CPU:
        _CPU[("tree", name)] = oracle().build_bvh(scene(name))[0]
    return _CPU[("tree", name)]


def cpu_camera(pos, W=W0, H=H0):
    cam = cam_dict(pos)
    return oracle().camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def cpu_gbuffer(name, pos, user_sphere=None):
    """(words (H, W, 8), ordinals (H, W), the view's 13 camera floats) of the oracle's camera rays: what gpuart_hip_gbuffer writes, with
    ordinal -2 on the user sphere and 0 elsewhere."""
    key = (name, tuple(pos), user_sphere)
    if key not in _CPU:
        O = oracle()
        c = cpu_camera(pos)
        rs, rd = O.cam_rays(c, W0, H0)
        rs, rd = rs.reshape(-1, 4), rd.reshape(-1, 4)
        o0, o1 = O.traverse(cpu_tree(name), rs, rd, user_sphere)
        prims = np.zeros(W0 * H0, np.int32)
        if user_sphere is not None:
            b0, _ = O.traverse(cpu_tree(name), rs, rd, None)
            prims[(o0.view(np.uint32) != b0.view(np.uint32)).any(1)] = -2
        words = np.concatenate([o0, o1], 1).astype(np.float32)
        words[:, 7] = np.floor(o1[:, 3]).astype(np.int32).view(np.float32)
        _CPU[key] = (words.reshape(H0, W0, 8), prims.reshape(H0, W0), c)
    return _CPU[key]


def radiance(seed, h=H0, w=W0):
    return np.random.default_rng(seed).uniform(0, 2, (h, w, 4)).astype(np.float32)


@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_restatement_without_history_and_on_the_same_view(name):
    """No history: the output is the input bit for bit and the length is spp on surface pixels, 0 elsewhere. The same view twice: EVERY
    surface pixel finds history, its length is min(spp1, max_history) + spp2 to a few ulps, and every surface pixel's own hit point
    projects to within 0.01 pixel of the pixel itself — which pins step 3 to the oracle's camera rays, independently of the kernel."""
    words, prims, c = cpu_gbuffer(name, TRACK[0])
    v = T.view(c, T.full_frame(W0, H0))
    surf = words[..., 7].view(np.int32) >= 0
    assert surf.sum() > 5000 and (~surf).sum() > 100
    a, b = radiance(1), radiance(2)
    out, ln, hist = T.accumulate(None, a, 3, words, prims, v)
    assert same_bits(out, a)
    assert (ln[surf] == 3).all() and (ln[~surf] == 0).all()
    for spp1, spp2, mh in ((3, 2, 4.0), (7, 1, 4.0), (1, 1, 32.0)):
        _, _, hist = T.accumulate(None, a, spp1, words, prims, v)
        out, ln, _, (fx, fy) = T.accumulate(hist, b, spp2, words, prims, v, max_history=mh, want_coords=True)
        want = np.float32(min(spp1, mh) + spp2)
        assert (ln[surf] > spp2).all(), "%d surface pixels found no history" % int((ln[surf] <= spp2).sum())
        assert np.abs(ln[surf] - want).max() <= 4 * np.spacing(want), np.abs(ln[surf] - want).max()
        assert (ln[~surf] == 0).all() and same_bits(out[~surf], b[~surf]) and same_bits(out[..., 3], b[..., 3])
        yy, xx = np.mgrid[0:H0, 0:W0]
        ex, ey = np.abs(fx - xx)[surf].max(), np.abs(fy - yy)[surf].max()
        print("%s: a view's own hit points land within %.2e, %.2e pixel of their pixels" % (name, ex, ey))
        assert ex <= 0.01 and ey <= 0.01, (ex, ey)
        # where nothing moved the blend is the running mean, up to what the neighbouring taps' weights (ex, ey) bring in of colours in 0..2
        if spp1 <= mh:
            mean = (spp1 * a[..., :3].astype(np.float64) + spp2 * b[..., :3]) / (spp1 + spp2)
            assert np.abs(out[..., :3] - mean)[surf].max() < 2 * 2 * (ex + ey) + 1e-5


def test_restatement_passes_through_what_is_not_a_surface():
    """Sky pixels always, and emissive or mirror user-sphere pixels, come out bit for bit as they went in with length 0, whatever the
    history holds, for every flag combination; alpha everywhere. A diffuse or fuzzy user sphere that did not move takes history, one
    that moved neither takes nor gives any."""
    w0, p0, c0 = cpu_gbuffer("box", TRACK[0], SPHERE)
    w1, p1, c1 = cpu_gbuffer("box", TRACK[1], SPHERE)
    w2, p2, _ = cpu_gbuffer("box", TRACK[1], SPHERE_2)
    assert (p0 == -2).sum() > 50 and (p1 == -2).sum() > 50 and (p2 == -2).sum() > 50
    a, b = radiance(3), radiance(4)
    sky = w1[..., 7].view(np.int32) < 0
    g = T.full_frame(W0, H0)
    for f0 in (0, 1, 2, 3, 4):
        for f1 in (0, 1, 2, 3, 4, 7):
            _, _, hist = T.accumulate(None, a, 2, w0, p0, T.view(c0, g, SPHERE, f0))
            out, ln, _ = T.accumulate(hist, b, 1, w1, p1, T.view(c1, g, SPHERE, f1))
            still = sky | ((p1 == -2) & bool(f1 & 3))
            assert same_bits(out[still], b[still]) and (ln[still] == 0).all() and same_bits(out[..., 3], b[..., 3]), (f0, f1)
            assert (ln[~still] >= 1).all()
            on_sphere = ln[p1 == -2]
            if (f0 & 3) or (f1 & 3):     # not a surface in one of the two views: the sphere's pixels have no history
                assert (on_sphere <= 1).all(), (f0, f1)
            else:
                assert (on_sphere > 1).mean() > 0.8, (f0, f1)
            assert (ln[~still & (p1 != -2)] > 1).mean() > 0.9
    # the sphere moved between the views
    _, ln0, hist = T.accumulate(None, a, 2, w0, p0, T.view(c0, g, SPHERE, 0))
    out, ln, _ = T.accumulate(hist, b, 1, w2, p2, T.view(c1, g, SPHERE_2, 0))
    assert (ln[p2 == -2] == 1).all() and same_bits(out[p2 == -2], b[p2 == -2])
    # ... and no pixel took history from a pixel of the old sphere: with the old sphere's history pixels made unmistakable, nothing changes
    marked = dict(hist, col=hist["col"].copy())
    marked["col"][p0 == -2] = 1e6
    out_m, ln_m, _ = T.accumulate(marked, b, 1, w2, p2, T.view(c1, g, SPHERE_2, 0))
    assert same_bits(out_m, out) and same_bits(ln_m, ln)
    # a sphere that stayed gives history to itself only
    out_s, _, _ = T.accumulate(marked, b, 1, w1, p1, T.view(c1, g, SPHERE, 0))
    assert (out_s[p1 == -2][:, 0] > 1e4).mean() > 0.8 and not (out_s[p1 != -2][:, 0] > 1e4).any()


def erode(m, r):
    out = m.copy()
    h, w = m.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            s = np.zeros_like(m)     # (the image border counts as not hidden)
            y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            s[y0:y1, x0:x1] = m[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            out &= s
    return out


@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_restatement_rejects_history_where_the_old_view_saw_something_else(name):
    """History at the default camera, current view from x = 0.5. A surface pixel was hidden before if the oracle's closest hit from the
    old camera towards its hit point is nearer than 0.99 of the distance, or the point projects outside the old frame or behind the old
    camera. Every pixel of that mask eroded by 2 (a bilinear tap beside an occluder's edge may rightly see the same surface) has found
    no history, with the defaults: no exceptions, and the mask is not trivial."""
    O = oracle()
    w0, p0, c0 = cpu_gbuffer(name, TRACK[0])
    w1, p1, c1 = cpu_gbuffer(name, (0.5, -3.05, 1.0))
    g = T.full_frame(W0, H0)
    _, _, hist = T.accumulate(None, radiance(5), 4, w0, p0, T.view(c0, g))
    out, ln, _, (fx, fy) = T.accumulate(hist, radiance(6), 1, w1, p1, T.view(c1, g), want_coords=True, **T.DEFAULTS)
    surf = w1[..., 7].view(np.int32) >= 0
    P = w1[..., 1:4].astype(np.float32)
    d = P - c0[0:3]
    dist = np.sqrt((d.astype(np.float64) ** 2).sum(2))
    rd = np.concatenate([(d / dist[..., None]).reshape(-1, 3), np.zeros((W0 * H0, 1))], 1).astype(np.float32)
    rs = np.broadcast_to(np.concatenate([c0[0:3], [0]]).astype(np.float32), (W0 * H0, 4)).copy()
    t = O.traverse(cpu_tree(name), rs, rd, None)[0][:, 0].reshape(H0, W0)
    _, _, k, _, _ = T.backproject(P, T.view(c0, g))
    outside = (fx < -0.5) | (fx > W0 - 0.5) | (fy < -0.5) | (fy > H0 - 0.5) | ~(k > 0)
    hidden = surf & (((t > 0) & (t < 0.99 * dist)) | outside)
    core = erode(hidden, 2)
    wrong = core & (ln != 1)
    print("%s: hidden before %d pixels, eroded by 2: %d, of which found history: %d; surface pixels with history %.3f"
          % (name, int(hidden.sum()), int(core.sum()), int(wrong.sum()), float((ln[surf] > 1).mean())))
    assert core.sum() >= 200, int(core.sum())
    assert not wrong.any(), int(wrong.sum())
    assert (ln[surf] > 1).mean() > 0.5    # ... and not by rejecting everything


# ---- GPU --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    return oracle()


@pytest.fixture(scope="module")
def be(B):
    b = B.Backend(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def tp(B):
    handles = [B.Temporal(0), B.Temporal(0)]   # one fed through the host entry point, one through the device entry point
    yield handles
    for t in handles:
        t.close()


def gpu_camera(O, pos, W, H):
    cam = cam_dict(pos)
    return O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)


def gpu_view_data(be, B, O, pos, W, H, passes, us, em, flags, seed):
    """The normalised accumulator of `passes` one-path passes from `pos`, the tile's G-buffer, and the view in both forms."""
    c = gpu_camera(O, pos, W, H)
    be.set_camera(c)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P0 = O.make_params(sun, S.SUN_ALTITUDE, True, us or (0, 0, 0, 0), em, flags, float(c[12]), c[0:3], 5, 0.01)
    P = B.Params()
    C.memmove(C.byref(P), C.byref(P0), C.sizeof(P))
    be.pt_reset()
    for s in O.randseeds(passes, seed=seed):
        be.pt_pass(P, s, 1)
    rgba = be.read(1, divide_by=float(passes))
    hits, prims = be.gbuffer(user_sphere=us)
    g = be.get_share()
    return rgba, hits, prims, B.temporal_view(c, g, us, flags), T.view(c, g, us or (0, 0, 0, 0), flags)


def run_chain(tp, data, params, what, preview_at=2, ledger=None, alias_at=None):
    """Commits the views of `data` one after the other through both entry points and holds every blend and length to the restatement; before
    view `preview_at` a call without commit, which must equal the restatement too and leave what follows unchanged. The views may differ
    in geometry: each call takes its sizes from its own arrays and the history keeps the geometry it was committed with. `ledger`: a
    dict that the restatement's branch counts of every call are added to; at view `alias_at` the device call's out_rgba is its rgba."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    kw = dict(T.DEFAULTS, **(params or {}))
    for h in tp:
        h.reset()
    hist = None
    found = 0
    for i, (rgba, spp, hits, prims, view, ref_view) in enumerate(data):
        words = hits.view(np.float32).reshape(rgba.shape[:2] + (8,))
        commits = [False, True] if i == preview_at else [True]
        for commit in commits:
            exp, exp_len, new, led = T.accumulate(hist, rgba, spp, words, prims, ref_view, want_ledger=True, **kw)
            if ledger is not None:
                for k, v in led.items():
                    ledger[k] = ledger.get(k, 0) + v
            tag = "%s, view %d, commit %d" % (what, i, commit)
            out, ln = tp[0].accumulate(rgba, spp, hits, prims, view, params=params, commit=commit)
            assert_same_bits(out, exp, tag + ", host")
            assert_same_bits(ln, exp_len, tag + ", host, length")
            d_rgba = t(rgba)
            dout = d_rgba if i == alias_at else torch.full(rgba.shape, 7.0, device="cuda:0")
            res, dln = tp[1].accumulate(d_rgba, spp, t(words), t(prims), view, params=params, commit=commit, out=dout)
            assert res is dout
            assert_same_bits(dout.cpu().numpy(), exp, tag + ", torch")
            assert_same_bits(dln.cpu().numpy(), exp_len, tag + ", torch, length")
        hist = new
        if i:
            found += int((exp_len > spp).sum())
    return found


CONFIGS = [("box", SPHERE, 0.0, 0, None), ("box", SPHERE, 3.0, R.EM_NONZERO, None), ("box", SPHERE, 0.0, R.SPECULAR, None),
           ("box", SPHERE, 0.0, 0, SPHERE_2), ("scene_p", SPHERE, 0.0, 0, None), ("scene_d", None, 0.0, 0, None)]
GEOMS = [(160, 120, "full"), (37, 23, "full"), (3, 2, "full"), (1, 1, "full"), (160, 120, "tile"), (160, 120, "share")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,us,em,flags,moved", CONFIGS)
def test_kernel_equals_the_restatement(be, tp, B, O, name, us, em, flags, moved):
    """Chains of four committed views (a sideways track, then a dolly) on the box with a diffuse, an emissive, a mirror and a moved user
    sphere, scene P and scene D; full frames of four sizes, a rectangular tile and share 1 of 3; rendered radiance with the defaults and
    seeded random radiance with two other settings; through the host and the device entry points."""
    from tests.test_denoise import tree
    rng = np.random.default_rng(99)
    be.upload_bvh(tree(O, name))
    total = 0
    for W, H, geom in GEOMS:
        be.resize(W, H)
        if geom == "tile":
            be.set_tile(21, 13, 37, 23)
        elif geom == "share":
            be.set_share(B.share_of_rank(W, H, 1, 3))
        data = []
        for i, pos in enumerate(TRACK):
            sphere = moved if (moved and i >= 2) else us
            rgba, hits, prims, view, ref_view = gpu_view_data(be, B, O, pos, W, H, (1, 2, 1, 3)[i], sphere, em, flags, 50 + i)
            data.append((rgba, (1, 2, 1, 3)[i], hits, prims, view, ref_view))
        what = "%s %dx%d %s flags %d" % (name, W, H, geom, flags)
        found = run_chain(tp, data, None, what + " rendered")
        for k, p in enumerate((P_A, P_B)):
            noise = [(rng.uniform(0, 2, d[0].shape).astype(np.float32), 2 + k) + d[2:] for d in data]
            run_chain(tp, noise, p, what + " random %s" % (p,), preview_at=1 + k)
        if W * H > 1000:
            assert found > 0.5 * data[0][0].shape[0] * data[0][0].shape[1], (what, found)   # of three views' pixels: the chain is not trivial
            if us and geom == "full":
                assert all((d[3] == -2).any() for d in data), what   # the user sphere is in view
        total += found
    assert total > 0


@pytest.mark.gpu
def test_kernel_at_1080p(be, tp, B, O):
    from tests.test_denoise import tree
    W, H = 1920, 1080
    be.upload_bvh(tree(O, "scene_p"))
    be.resize(W, H)
    data = []
    for i, pos in enumerate(TRACK[:2]):
        rgba, hits, prims, view, ref_view = gpu_view_data(be, B, O, pos, W, H, 1, SPHERE, 0.0, 0, 70 + i)
        data.append((rgba, 1, hits, prims, view, ref_view))
    found = run_chain(tp, data, None, "scene_p 1920x1080", preview_at=-1)
    assert found > 0.3 * W * H


def renderer_view(B, r, cam, us, flags):
    c = B.camera_basis(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], r.W, r.H)
    return T.view(c, r.backend.get_share(), us, flags)


def tile_xy(r):
    g = r.backend.get_share()
    ly, lx = np.divmod(np.arange(g.tw * g.th), g.tw)
    return np.stack([g.x0 + lx, g.y0 + (ly // g.band_rows) * g.band_stride + ly % g.band_rows], 1)


class Shadow:
    """The restatement's side of a Renderer with history on: commit() before every call that leaves a view, preview() for read_preview."""

    def __init__(self, B, r, us, flags, params=None):
        self.B, self.r, self.us, self.flags = B, r, us, flags
        self.kw = dict(T.DEFAULTS, **(params or {}))
        self.hist = None

    def _inputs(self, cam):
        r = self.r
        _, _, tw, th = r.tile
        hits, prims = r.pick(tile_xy(r), want_prims=True)
        return r.read_radiance(True), hits, prims.reshape(th, tw), renderer_view(self.B, r, cam, self.us, self.flags)

    def commit(self, cam, spp):
        rgba, hits, prims, v = self._inputs(cam)
        _, _, self.hist = T.accumulate(self.hist, rgba, spp, hits, prims, v, **self.kw)

    def preview(self, cam, spp, denoise=None, temporal=None):
        rgba, hits, prims, v = self._inputs(cam)
        out, _, _ = T.accumulate(self.hist, rgba, spp, hits, prims, v, **dict(self.kw, **(temporal or {})))
        return R.denoise(out, hits, prims, self.flags, **dict(R.DEFAULTS, **(denoise or {})))


@pytest.mark.gpu
def test_read_preview_carries_history_and_leaves_rendering_alone(B):
    """With history on, read_preview after each set_camera + passes equals the restatement chain built from read_radiance, pick of every
    tile pixel and the cameras, followed by the denoiser's restatement, bit for bit; a run with previews and a run without leave the same
    accumulator and the same counters; with history off, and before the first commit, read_preview is read_denoised."""
    W, H = 96, 64
    us, em = SPHERE, 0.0
    cams = [cam_dict(p) for p in TRACK]
    DN = dict(iterations=3, lum_k=1.5, normal_pow2=2, depth_sigma=0.2)

    def run(with_previews, history=True):
        r = B.Renderer(W, H, cams[0])
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(us[:3], us[3], emittance=em)
            if history:
                r.set_temporal_history(True)
            sh = Shadow(B, r, us, 0)
            r.backend.set_mode(4)
            r.restart_path_tracing(1, 3)
            accs = []
            for i, cam in enumerate(cams):
                if i:
                    if with_previews and history:
                        sh.commit(cams[i - 1], 3)
                    r.set_camera(cam)
                for k in range(3):
                    r.path_tracing_pass()
                    if with_previews and k in (0, 2):
                        got = r.read_preview()
                        if not history or i == 0:
                            assert_same_bits(got, r.read_denoised(), "no history: view %d after %d passes" % (i, k + 1))
                        else:
                            assert_same_bits(got, sh.preview(cam, k + 1), "view %d after %d passes" % (i, k + 1))
                            assert not same_bits(got, r.read_denoised())
                        if history and i == 2 and k == 2:
                            assert_same_bits(r.read_preview(DN, P_A), sh.preview(cam, 3, DN, P_A), "other parameters")
                accs.append(r.read_radiance(False))
            return accs, r.backend.counters().as_dict()
        finally:
            r.close()

    acc0, cnt0 = run(False)
    acc1, cnt1 = run(True)
    acc2, cnt2 = run(True, history=False)
    assert cnt0 == cnt1 == cnt2
    for a, b, c in zip(acc0, acc1, acc2):
        assert same_bits(a, b) and same_bits(a, c)


@pytest.mark.gpu
def test_setters_that_change_the_light_drop_the_history(B, tmp_path):
    """Everything that restarts the accumulation, other than a camera move, drops the history: the next read_preview is read_denoised
    until a view has been committed again. restart_path_tracing keeps it; switching history off drops it."""
    W, H = 64, 48
    cams = [cam_dict(p) for p in TRACK]
    ck = str(tmp_path / "ck.bin")
    r = B.Renderer(W, H, cams[0])
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(SPHERE[:3], SPHERE[3])
        r.set_temporal_history(True, P_A)
        r.restart_path_tracing(1, 2)

        def passes(n=2):
            for _ in range(n):
                r.path_tracing_pass()

        def with_history():
            """Two views committed... one: the renderer now holds a history and shows it."""
            r.set_camera(cams[0]); passes()
            r.set_camera(cams[1]); passes()
            assert not same_bits(r.read_preview(), r.read_denoised())

        droppers = [("set_primitives", lambda: r.set_primitives(scene("box"))),
                    ("set_sun", lambda: r.set_sun(float(S.SUN_AZIMUTH), 0.6)),
                    ("set_user_sphere (emittance, flags)", lambda: r.set_user_sphere(SPHERE[:3], SPHERE[3], fuzzy=True)),
                    ("set_max_path_segments", lambda: r.set_max_path_segments(4)),
                    ("set_min_weight", lambda: r.set_min_weight(0.02)),
                    ("set_seed", lambda: r.set_seed(9)),
                    ("set_nearest_first", lambda: r.set_nearest_first(0xffffffff)),
                    ("update_viewport", lambda: r.update_viewport(W, H)),
                    ("set_tile", lambda: r.set_tile(0, 0, W, H)),
                    ("set_interleaved_tile", lambda: r.set_interleaved_tile(0, 0, W, H, H, H)),
                    ("load_checkpoint", lambda: r.load_checkpoint(ck)),
                    ("set_temporal_history(False)", lambda: (r.set_temporal_history(False), r.set_temporal_history(True, P_A)))]
        for what, drop in droppers:
            with_history()
            if what == "load_checkpoint":
                assert r.save_checkpoint(ck)
            drop()
            passes()
            assert_same_bits(r.read_preview(), r.read_denoised(), what)
        with_history()
        r.restart_path_tracing(1, 2)
        passes()
        assert not same_bits(r.read_preview(), r.read_denoised())
        with pytest.raises(ValueError):
            r.set_temporal_history(True, dict(normal_min=2.0))
        # history off: read_preview is read_denoised throughout, camera moves included
        r.set_temporal_history(False)
        for cam in cams[:3]:
            r.set_camera(cam); passes()
            assert_same_bits(r.read_preview(), r.read_denoised(), "history off")
    finally:
        r.close()


def surface_rmse(img, ref, mask):
    d = img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)
    return float(np.sqrt((d[mask] ** 2).mean()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["box", "scene_p"])
def test_history_helps_the_preview(B, name):
    """Eight views, camera x = 0.10, 0.15 ... 0.45, one path each from one seed sequence, 160 x 120, the Sun on, no user sphere; the
    reference is 512 paths at the last view from another seed. The surface-pixel RMSE of read_preview at the last view over that of
    read_denoised there must be below the bound the CPU run of tools/temporal_quality.py gives (its ratio plus a quarter of its
    distance to 1), and in any case below 1. The frames equal the oracle's and both filters their restatements, so the GPU ratio
    reproduces the CPU's (measured: 0.8615 / 0.6607 on both). The reference is rendered exactly as the CPU run renders it, 512 passes
    of one path: at 512 paths its own noise still moves the box's ratio, whose two errors are small (0.021 against 0.024) — rendered as
    8 passes of 64 paths from the same seed it is 0.9102 on the CPU and on the GPU alike (scene P: 0.6658), above the box's bound
    and below 1 (profiles/temporal.txt)."""
    W, H = 160, 120
    xs = [0.10 + 0.05 * i for i in range(8)]
    cams = [cam_dict((x, -3.05, 1.0)) for x in xs]
    r = B.Renderer(W, H, cams[-1])
    try:
        r.set_primitives(scene(name))
        r.set_user_sphere(S.USER_SPHERE[:3], 0.0)
        r.set_seed(2)
        r.restart_path_tracing(1, 512)     # 512 passes of one path, as the CPU run renders it: the ratio depends on the reference's own noise
        while r.path_tracing_pass() < 512:
            pass
        ref = r.read_radiance(True)
        y, x = np.divmod(np.arange(W * H), W)
        mask = (r.pick(np.stack([x, y], 1))["type"] >= 0).reshape(H, W)
        r.set_seed(1234)
        r.set_temporal_history(True)
        r.restart_path_tracing(1, 1)
        for cam in cams:
            r.set_camera(cam)
            assert r.path_tracing_pass() == 1
        with_history, spatial = r.read_preview(), r.read_denoised()
        ratio = surface_rmse(with_history, ref, mask) / surface_rmse(spatial, ref, mask)
        print("%s: (history + spatial) / spatial surface RMSE at the last view: %.4f on the GPU, %.4f on the CPU, bound %.4f"
              % (name, ratio, CPU_RATIO[name], RATIO_BOUND[name]))
        assert ratio < 1 and ratio <= RATIO_BOUND[name], ratio
    finally:
        r.close()


@pytest.mark.gpu
def test_argument_errors(tp, B):
    """Every ERR_ARG case returns the error with its message and writes nothing."""
    import torch
    L = tp[0].L
    h, w = 4, 4
    rgba = np.ones((h * w + 1, 4), np.float32)
    hits = np.zeros((h * w + 1, 8), np.float32)
    prims = np.zeros(h * w + 2, np.int32)
    out = np.full((h * w + 1, 4), 7.0, np.float32)
    ln = np.full(h * w + 2, 7.0, np.float32)
    ptr = lambda a, k=0: C.c_void_p(a.ctypes.data + k)
    cam = np.array([0, -3, 1, -1, -2, 0, 2, 0, 0, 0, 0, 2], np.float32)
    view = lambda **kw: B.temporal_view(cam, tuple(dict(dict(W=w, H=h, x0=0, y0=0, tw=w, th=h, band_rows=h, band_stride=h), **kw).values()))
    good = dict(rgba=ptr(rgba), spp=1, hits=ptr(hits), prims=ptr(prims), w=w, h=h, view=C.byref(view()), p=None, out=ptr(out), ln=ptr(ln))
    par = lambda **kw: C.byref(B.TemporalParams(**dict(T.DEFAULTS, **kw)))

    def call(fn, handle=None, **kw):
        a = dict(good, **kw)
        return getattr(L, fn)(handle if handle is not None else tp[0].h, a["rgba"], C.c_uint32(a["spp"]), a["hits"], a["prims"], C.c_uint32(a["w"]),
                              C.c_uint32(a["h"]), a["view"], a["p"], C.c_int(1), a["out"], a["ln"])

    H_ = "gpuart_temporal_accumulate_host"
    cases = [(H_, dict(rgba=None), "NULL"), (H_, dict(hits=None), "NULL"), (H_, dict(prims=None), "NULL"), (H_, dict(out=None), "NULL"),
             (H_, dict(view=None), "NULL"), (H_, dict(rgba=ptr(rgba, 2)), "misaligned"), (H_, dict(prims=ptr(prims, 1)), "misaligned"),
             (H_, dict(ln=ptr(ln, 2)), "misaligned"), (H_, dict(w=0), "bad size"), (H_, dict(h=0), "bad size"), (H_, dict(w=65537), "bad size"),
             (H_, dict(spp=0), "spp"), (H_, dict(view=C.byref(view(tw=w + 1))), "geom"), (H_, dict(view=C.byref(view(th=h - 1))), "geom"),
             (H_, dict(view=C.byref(view(W=w - 1))), "geom"), (H_, dict(view=C.byref(view(H=h - 1))), "geom"), (H_, dict(view=C.byref(view(x0=1))), "geom"),
             (H_, dict(view=C.byref(view(y0=1))), "geom"), (H_, dict(view=C.byref(view(band_rows=0))), "geom"),
             (H_, dict(view=C.byref(view(band_rows=2, band_stride=1))), "geom"), (H_, dict(view=C.byref(view(W=0))), "geom"),
             (H_, dict(view=C.byref(view(H=65537))), "geom"),
             (H_, dict(p=par(max_history=-1.0)), "max_history"), (H_, dict(p=par(max_history=float("inf"))), "max_history"),
             (H_, dict(p=par(plane_tol=float("nan"))), "plane_tol"), (H_, dict(p=par(plane_tol=-0.1)), "plane_tol"),
             (H_, dict(p=par(normal_min=1.5)), "normal_min"), (H_, dict(p=par(normal_min=float("nan"))), "normal_min")]
    dev = [torch.zeros(h * w * 8 + 8, device="cuda:0") for _ in range(3)]
    dp = lambda t, k=0: C.c_void_p(t.data_ptr() + k)
    dgood = dict(rgba=dp(dev[0]), hits=dp(dev[1]), prims=dp(dev[2]), out=dp(dev[0]), ln=dp(dev[2], 256))
    D_ = "gpuart_temporal_accumulate"
    cases += [(D_, dict(dgood, rgba=dp(dev[0], 4)), "misaligned"), (D_, dict(dgood, hits=dp(dev[1], 8)), "misaligned"),
              (D_, dict(dgood, out=dp(dev[0], 4)), "misaligned"), (D_, dict(dgood, prims=dp(dev[2], 2)), "misaligned"),
              (D_, dict(dgood, ln=dp(dev[2], 2)), "misaligned"), (D_, dict(dgood, spp=0), "spp"), (D_, dict(dgood, w=0), "bad size"),
              (D_, dict(dgood, p=par(normal_min=-2.0)), "normal_min"), (D_, dict(dgood, view=C.byref(view(tw=1))), "geom")]
    tp[0].reset()
    for fn, kw, msg in cases:
        rc = call(fn, **kw)
        assert rc == ERR_ARG and msg in L.gpuart_temporal_last_error().decode(), (fn, kw, msg, rc, L.gpuart_temporal_last_error())
    assert call(H_, handle=C.c_void_p(None)) == ERR_ARG and "handle" in L.gpuart_temporal_last_error().decode()
    assert L.gpuart_temporal_finish(None) == ERR_ARG and L.gpuart_temporal_reset(None) == ERR_ARG
    assert L.gpuart_temporal_defaults(None) == ERR_ARG and L.gpuart_temporal_create(C.c_int(0), None) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (ln == 7.0).all() and all((d == 0).all() for d in dev)
    # ... and none of them committed anything: the first good call finds no history
    assert call(H_, ln=None) == 0
    assert same_bits(out[:h * w], rgba[:h * w]) and (out[h * w] == 7.0).all() and (ln == 7.0).all()
    assert call(H_) == 0 and (ln[:h * w] >= 1).all() and (ln[h * w:] == 7.0).all()   # (all-zero records are type 0: surface pixels)
    # the Renderer: no scene
    r = B.Renderer(16, 8, cam_dict(TRACK[0]))
    try:
        r.set_temporal_history(True)
        with pytest.raises(B.HipError):
            r.read_preview()
        with pytest.raises(ValueError):
            r.read_preview(temporal=dict(max_history=2, sigma=1))
    finally:
        r.close()
