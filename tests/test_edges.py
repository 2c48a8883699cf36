"""Geometric edges resolved from a sub-pixel G-buffer (include/gpuart_edges.h, libgpuart_edges.so; gpuart_hip_trace_subpixel of
include/gpuart_hip.h): the libraries' boundaries and the parameter record, the restatement's (tests/edges_ref.py) ledger over planted
tiles and what the resolve is worth on the oracle's protocol (tests/edges_protocol.py), the sub-pixel rays against the oracle and the
kernels against the restatement bit for bit, Renderer::SetEdgeResolve against the chain of restatements, and what it leaves alone."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from gpuart_amd import synth_scenes as S
from tests import denoise_ref as D
from tests import display_ref as DR
from tests import edges_protocol as P
from tests import edges_ref as E
from tests.util import assert_same_bits, exported, same_bits, scene, to_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
F = np.float32
ENTRY_POINTS = ["gpuart_edges_" + n for n in ("create", "defaults", "destroy", "finish", "last_error", "mark", "offsets", "resolve")]
NEW_HOST = ["gpuart_renderer_get_edge_resolve", "gpuart_renderer_set_edge_resolve"]
OTHER_LIBS = ("denoise", "temporal", "converge", "refine", "adaptive", "moments", "display", "antilag")
P_X = dict(n_sub=3, normal_min=0.5, plane_tol=0.1)   # a non-default setting
# tools/edges_quality.py (profiles/edges.txt, section A.3), the defaults: the resolved / denoised surface RMSE against the oracle's
# 1024-path reference at 1 and 16 paths
CPU_RATIO = {("box", 1): 0.6924, ("box", 16): 0.5845, ("scene_p", 1): 0.8288, ("scene_p", 16): 0.8094}


def _declared(name):
    return sorted(set(re.findall(r"\b(gpuart_%s_[a-z_0-9]+)\s*\(" % name, open(os.path.join(ROOT, "include", "gpuart_%s.h" % name)).read())))


# ---- CPU: the libraries' boundaries and the record ------------------------------------------------------------------------------
@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_libraries_export_the_new_entry_points(lib):
    assert _declared("edges") == ENTRY_POINTS
    path = os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_edges.so")
    assert exported(path) == ENTRY_POINTS
    # images alone: the HIP runtime, and neither the renderer's back end nor another image library
    dyn = subprocess.run(["readelf", "-d", path], capture_output=True, text=True, check=True).stdout
    assert "libgpuart" not in dyn and "libamdhip64" in dyn, dyn
    hip = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_hip.so"))
    assert "gpuart_hip_trace_subpixel" in hip and not [n for n in hip if "edges" in n]
    assert re.search(r"\bgpuart_hip_trace_subpixel\s*\(", open(os.path.join(ROOT, "include", "gpuart_hip.h")).read())
    host = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart.so"))
    capi = open(os.path.join(ROOT, "gpuart_amd", "csrc", "host", "capi.h")).read()
    for n in NEW_HOST:
        assert n in host and re.search(r"\b%s\s*\(" % n, capi), n
    for other in OTHER_LIBS:
        names = exported(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % other))
        assert names == _declared(other), other


@pytest.mark.parametrize("lib", ["lib", "lib_test"])
def test_edges_keeps_its_own_last_error(lib):
    libs = {n: C.CDLL(os.path.join(ROOT, "gpuart_amd", lib, "libgpuart_%s.so" % n)) for n in ("edges", "denoise")}
    for n in libs:
        getattr(libs[n], "gpuart_%s_last_error" % n).restype = C.c_char_p
    last = lambda n: getattr(libs[n], "gpuart_%s_last_error" % n)()
    before = last("denoise")
    assert libs["edges"].gpuart_edges_finish(None) == ERR_ARG and last("edges") == b"edges: handle is NULL"
    assert last("denoise") == before


def test_params_record_offsets_and_defaults_match_the_header(tmp_path):
    from gpuart_amd import binding as B
    fields = ("n_sub", "normal_min", "plane_tol")
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_edges.h"\n#define P gpuart_edges_params\n'
                   'int main(void) { printf("%%zu %s %%u %%u\\n", sizeof(P), %s, GPUART_EDGES_MAX_SUB, GPUART_HIP_MAX_SUBPIXEL);\n'
                   'for (int n = 0; n <= 16; n++) printf("%%d ", GPUART_EDGES_ROTATION[n]); for (int k = 0; k < 4; k++) printf("%%d ", GPUART_EDGES_RGSS[k]);\n'
                   'return 0; }\n' % (" ".join(["%zu"] * len(fields)), ", ".join("offsetof(P, %s)" % f for f in fields)))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Pm = B.EdgesParams
    assert got[:4] == [C.sizeof(Pm)] + [getattr(Pm, f).offset for f in fields] == [12, 0, 4, 8]
    assert got[4:6] == [E.MAX_SUB, E.MAX_SUB] == [B.EDGES_MAX_SUB] * 2
    assert tuple(got[6:23]) == E.ROTATION and tuple(got[23:]) == E.RGSS
    assert B.EDGES_DEFAULTS == E.DEFAULTS and tuple(E.DEFAULTS) == fields
    with pytest.raises(ValueError):
        B.edges_params(dict(n_sub=2, sigma=1))
    hdr = open(os.path.join(ROOT, "include", "gpuart_edges.h")).read()
    stated = ", ".join("%s %g" % (f, E.DEFAULTS[f]) for f in fields)
    assert hdr.count(stated) == 2, stated
    L = C.CDLL(os.path.join(ROOT, "gpuart_amd", "lib_test", "libgpuart_edges.so"))
    p = Pm()
    assert L.gpuart_edges_defaults(C.byref(p)) == 0 and L.gpuart_edges_defaults(None) == ERR_ARG
    assert {f: getattr(p, f) for f in fields} == pytest.approx(E.DEFAULTS) and p.normal_min == F(E.DEFAULTS["normal_min"])
    # the offsets: the library's are the restatement's, bit for bit; one sample per row and per column of the n x n grid
    uv = np.zeros((16, 2), F)
    assert L.gpuart_edges_offsets(0, uv.ctypes.data_as(C.c_void_p)) == ERR_ARG and L.gpuart_edges_offsets(17, uv.ctypes.data_as(C.c_void_p)) == ERR_ARG
    assert L.gpuart_edges_offsets(4, None) == ERR_ARG
    for n in range(1, 17):
        assert_same_bits(B.Edges.offsets(n), E.offsets(n), "offsets of n_sub %d" % n)
        o = E.offsets(n)
        for axis in (0, 1):
            assert sorted(np.floor(o[:, axis] * n).astype(int)) == list(range(n)), (n, axis)
        assert (o >= 0).all() and (o < 1).all()


# ---- CPU: planted tiles and the ledger ------------------------------------------------------------------------------------------
NORMALS = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0.6, 0.8, 0]], F)
TANGENTS = np.array([[[1, 0, 0], [0, 1, 0]], [[1, 0, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1]], [[-0.8, 0.6, 0], [0, 0, 1]]], F)
# a region: ("sky",), ("sphere",) or ("surface", type, normal index, offset along the normal)
REGIONS = [("sky",), ("sphere",)] + [("surface", t, n, off) for t, n, off in
                                     ((0, 0, 0.0), (1, 0, 0.0), (2, 1, 0.0), (3, 1, 0.0), (2, 0, 0.0), (2, 0, 0.7), (0, 2, 0.0), (2, 3, 0.0), (2, 2, 0.3))]
SIZES = [(1, 1), (7, 1), (67, 5), (160, 120)]   # (w, h)


def region_records(reg, seed):
    """(words (h, w, 8), ordinals (h, w)) of a map of REGIONS indices: a surface pixel lies on its region's plane."""
    h, w = reg.shape
    rs = np.random.RandomState(seed)
    words = np.zeros((h, w, 8), F)
    prims = np.full((h, w), -1, np.int32)
    y, x = np.mgrid[0:h, 0:w].astype(F)
    for i, r in enumerate(REGIONS):
        m = reg == i
        if r[0] == "sky":
            words[m, 0] = -1
            words[m, 7] = np.int32(-1).view(F)
            continue
        t, n, off = (0, 3, 1.5) if r[0] == "sphere" else r[1:]
        p = NORMALS[n] * F(off) + TANGENTS[n][0] * (x * F(0.01))[..., None] + TANGENTS[n][1] * (y * F(0.01))[..., None]
        words[m, 0] = F(2.0 + 0.1 * i)
        words[m, 1:4] = p[m]
        words[m, 4:7] = NORMALS[n]
        words[m, 7] = np.int32(t).view(F)
        prims[m] = -2 if r[0] == "sphere" else rs.randint(0, 50, int(m.sum()))
    return words, prims


def planted(seed, w, h, n_sub, flags, kind="mixed", params=None):
    """A tile whose resolve takes every branch: a G-buffer of REGIONS (blocks on the left, single pixels on the right; "none": one
    region, "all": a checkerboard of two), a random frame, and for every listed pixel sub-samples that copy the centre record of one
    of the nine candidates, or a record nothing matches, or the sky."""
    rs = np.random.RandomState(seed)
    pr = dict(dict(E.DEFAULTS, **(params or {})), n_sub=n_sub)
    if kind == "none":
        reg = np.full((h, w), 4)
    elif kind == "all":
        y, x = np.mgrid[0:h, 0:w]
        reg = np.where((x + y) & 1, 2, 5)
    else:
        blocks = rs.randint(0, len(REGIONS), ((h + 2) // 3, (w + 4) // 5))
        reg = np.repeat(np.repeat(blocks, 3, 0), 5, 1)[:h, :w]
        noisy = np.arange(w)[None, :] >= (2 * w) // 3
        reg = np.where(noisy, rs.randint(0, len(REGIONS), (h, w)), reg)
    words, prims = region_records(reg, seed + 1)
    filtered = (rs.rand(h, w, 4) * 2 + 0.01).astype(F)
    lst = E.mark(words, prims, flags, pr["normal_min"], pr["plane_tol"])
    n = lst.size
    sw, sp = np.zeros((n_sub, n, 8), F), np.full((n_sub, n), -1, np.int32)
    junk = np.array([3.0, 50, 50, 50, 0, -1, 0, 0], F)
    junk[7] = np.int32(3).view(F)
    sky = np.array([-1, 0, 0, 0, 0, 0, 0, 0], F)
    sky[7] = np.int32(-1).view(F)
    y, x = lst.astype(np.int64) // w, lst.astype(np.int64) % w
    for k in range(n_sub):
        c = rs.randint(0, 11, n)
        for ci, (dy, dx) in enumerate(E.CANDIDATES):
            qy, qx = y + dy, x + dx
            ok = (c == ci) & (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            sw[k, ok], sp[k, ok] = words[qy[ok], qx[ok]], prims[qy[ok], qx[ok]]
            out = (c == ci) & ~ok
            sw[k, out], sp[k, out] = junk, 7
        sw[k, c == 9], sp[k, c == 9] = junk, 7
        sw[k, c == 10] = sky
    return dict(name="%s %dx%d n_sub %d flags %d" % (kind, w, h, n_sub, flags), words=words, prims=prims, flags=flags, filtered=filtered, lst=lst,
                sw=sw, sp=sp, params=pr)


def expected(c):
    return E.resolve(c["filtered"], c["words"], c["prims"], c["lst"], c["sw"], c["sp"], c["flags"], want_ledger=True, **c["params"])


def resolve_cases():
    """Sizes x n_sub 1 / 8 / 16 x every user-sphere flag, the all-edge and the no-edge tile, and a non-default setting."""
    cs = [planted(10 + i, w, h, n_sub, flags) for i, ((w, h), n_sub, flags) in enumerate(zip(SIZES, (8, 1, 16, 8), (1, 2, 4, 3)))]
    cs += [planted(20, 67, 5, 8, 0), planted(21, 33, 9, 8, 1, "all"), planted(22, 33, 9, 8, 1, "none"), planted(23, 67, 5, 3, 1, params=P_X),
           planted(24, 1, 7, 8, 1)]
    return cs


def test_cases_take_every_branch():
    """The restatement's ledger over the planted tiles: the pixel's own match, each of the 8 neighbours, no match, and the sky, sphere
    and surface classes; unlisted pixels are the input bit for bit; the all-edge tile lists every pixel, the no-edge tile none."""
    total = dict.fromkeys(E.LEDGER_KEYS, 0)
    for c in resolve_cases():
        out, led = expected(c)
        for k, v in led.items():
            total[k] += v
        h, w = c["prims"].shape
        listed = np.zeros(h * w, bool)
        listed[c["lst"]] = True
        assert same_bits(out.reshape(-1, 4)[~listed], c["filtered"].reshape(-1, 4)[~listed]), c["name"]
        assert same_bits(out[..., 3], c["filtered"][..., 3])
        assert sum(led["cand_%d" % i] for i in range(9)) + led["unmatched"] == led["sky"] + led["sphere"] + led["surface"] == c["lst"].size * c["params"]["n_sub"]
        if c["name"].startswith("all"):
            assert c["lst"].size == h * w
        if c["name"].startswith("none"):
            assert c["lst"].size == 0 and same_bits(out, c["filtered"])
        assert (np.diff(c["lst"].astype(np.int64)) > 0).all()
    assert all(v >= 20 for v in total.values()), total


WAVE = 64   # one ballot word per wave of k_ed_flag


def scan_block():
    """SCAN_BLOCK of gpuart_amd/csrc/edges/edges.hip: the ballot words k_ed_scan takes per pass of its loop."""
    src = open(os.path.join(ROOT, "gpuart_amd", "csrc", "edges", "edges.hip")).read()
    found = re.findall(r"\bSCAN_BLOCK\s*=\s*(\d+)", src)
    assert len(found) == 1, found
    return int(found[0])


@functools.lru_cache(maxsize=None)
def chunk_cases():
    """Tiles whose ballot words fill more than one pass of k_ed_scan's loop, or one pass exactly: 1031 x 130 (2095 words in three
    chunks, 14 pixels in the last word, a partial last block of k_ed_flag), 1025 x 64 (1025 words: a second chunk of one word), the two
    limit shapes (1024 words), and the all-edge and the no-edge tile at 1025 x 65 (1041 words, the last one partial)."""
    return [planted(70, 1031, 130, 1, 1), planted(72, 1025, 64, 1, 2), planted(73, 65536, 1, 1, 1), planted(74, 1, 65536, 1, 4),
            planted(75, 1025, 65, 1, 1, "all"), planted(76, 1025, 65, 1, 1, "none")]


def chunk_counts(c, block):
    """(ballot words, listed pixels per chunk of `block` words) of a case."""
    words = (c["prims"].size + WAVE - 1) // WAVE
    chunks = (words + block - 1) // block
    return words, np.bincount(c["lst"].astype(np.int64) // WAVE // block, minlength=chunks)


def test_chunk_cases_reach_the_scans_carry():
    """(CPU) what the multi-chunk cases are for, computed from their expected lists, SCAN_BLOCK as edges.hip has it and the wave width:
    three chunks and more, every chunk of the mixed multi-chunk tiles with a listed pixel (a lost carry moves its prefix), a chunk of
    exactly one word, a partial last word; and the figures of the 1031 x 130 tile."""
    block = scan_block()
    assert block % WAVE == 0
    stats = {c["name"]: chunk_counts(c, block) for c in chunk_cases()}
    print(stats)
    assert max(len(per) for _, per in stats.values()) >= 3
    multi = [(name, per) for name, (_, per) in stats.items() if name.startswith("mixed") and len(per) > 1]
    assert len(multi) >= 2 and all((per >= 1).all() for _, per in multi), multi
    assert any(words % block == 1 for words, _ in stats.values())
    assert any(c["prims"].size % WAVE for c in chunk_cases())
    assert any(words == block for words, _ in stats.values())             # one full chunk exactly: the limit shapes
    first = chunk_cases()[0]
    assert first["prims"].shape == (130, 1031) and stats[first["name"]][0] == 2095 and first["prims"].size % WAVE == 14
    assert first["lst"].size == 111604 and list(stats[first["name"]][1]) == [54462, 54606, 2536]
    every, none = chunk_cases()[4], chunk_cases()[5]
    assert (every["lst"] == np.arange(1025 * 65)).all() and none["lst"].size == 0 and len(stats[every["name"]][1]) == 2
    # the long list of the resolve: past 65 536 entries, so with n_sub 2 the sub-sample index k * n + i passes 2^17
    assert long_list_case()["lst"].size > 65536 and 2 * long_list_case()["lst"].size > 2 ** 17


@functools.lru_cache(maxsize=None)
def long_list_case():
    return planted(71, 1031, 130, 2, 1)


def test_match_follows_the_classes_and_the_thresholds():
    """match() on records built by hand: the class rule with every user-sphere flag, the type, the normal and the plane."""
    def rec(t, prim, n=(0, 0, 1), p=(0, 0, 0), pos=2.0):
        w = np.array([pos, *p, *n, 0], F)
        w[7] = np.int32(t).view(F)
        return w[None], np.array([prim], np.int32)
    m = lambda a, b, flags=0, nm=0.9, pt=0.02: bool(E.match(E.records(*a, flags), E.records(*b, flags), nm, pt)[0])
    sky, us, s0 = rec(-1, -1), rec(0, -2), rec(0, 5)
    assert m(sky, sky) and not m(sky, s0) and not m(s0, sky)
    for flags in (0, 4):
        assert m(us, us, flags) and not m(us, s0, flags) and not m(s0, us, flags)     # a diffuse user sphere: a surface of its own
    for flags in (1, 2, 3):
        assert m(us, us, flags) and not m(us, s0, flags) and E.records(*us, flags)["cls"][0] == E.SPHERE
    assert m(s0, rec(0, 9)) and not m(s0, rec(1, 5))
    assert not m(s0, rec(0, 5, n=(0, 0.6, 0.8))) and m(s0, rec(0, 5, n=(0, 0.6, 0.8)), nm=0.75)
    assert m(rec(0, 5, p=(3, 3, 0.04)), s0) and not m(rec(0, 5, p=(3, 3, 0.0401)), s0) and not m(rec(0, 5, p=(0, 0, -0.05)), s0)
    assert m(rec(0, 5, p=(0, 0, 1e-9)), rec(0, 5, pos=0.0)) and not m(rec(0, 5, p=(0, 0, 1e-7)), rec(0, 5, pos=0.0))   # max(pos, 1e-6)


# ---- CPU: the protocol -------------------------------------------------------------------------------------------------------------
def test_the_protocol_rays_are_the_path_tracers_first_segments():
    """tests/edges_protocol.py `subpixel_rays` (NumPy float32) against the oracle's own first segments for the draws of a seed."""
    O = P.K.oracle()
    c = P.camera()
    seeds = O.randseeds(3, seed=77)
    x, y = np.zeros((3, 4), F), np.zeros((3, 4), F)
    x[:, 0], y[:, 0] = seeds[:, 0], seeds[:, 1]
    uv = np.stack([O.random(x)[:, 0], O.random(y)[:, 0]], 1)
    rs, rd = P.subpixel_rays(c, uv)
    Pm = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    for k in range(3):
        es, ed = O.first_segment_rays(c, P.W, P.H, Pm, seeds[k])
        # (the jitter is ~1e-3 of a ray that starts ~3 from the origin: a few ulp of the start are 1e-3 of the offset)
        np.testing.assert_allclose(rs[k][..., :3], es[..., :3], rtol=0, atol=1e-6)
        np.testing.assert_allclose(rd[k][..., :3], ed[..., :3], rtol=0, atol=1e-6)


@pytest.mark.parametrize("paths", [1, 16])
@pytest.mark.parametrize("name", P.SCENES)
def test_resolving_the_edges_helps_the_denoised_frame(name, paths):
    """The protocol of tests/edges_protocol.py with the shipped defaults: the surface RMSE of the resolved frame over that of the
    denoised frame, both against the oracle's 1024-path reference, is at most r + (1 - r)/4, r the ratio tools/edges_quality.py
    printed (CPU_RATIO)."""
    surf, ref = P.surface_mask(name), P.reference(name)
    den = P.denoised(name, paths)
    out, led = P.resolved(name, den, E.offsets(E.DEFAULTS["n_sub"]), want_ledger=True)
    got = P.rmse(out, ref, surf) / P.rmse(den, ref, surf)
    r = CPU_RATIO[(name, paths)]
    print("%s, %d paths: resolved / denoised = %.4f (recorded %.4f, bound %.4f); %s" % (name, paths, got, r, r + (1 - r) / 4, led))
    assert got <= r + (1 - r) / 4, (got, r)
    assert led["listed"] > 1000 and led["cand_0"] > led["listed"] and led["sky"] > 0 and led["surface"] > 0


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def B():
    from gpuart_amd import binding
    return binding


@pytest.fixture(scope="module")
def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def ed(B):
    h = B.Edges(0)
    yield h
    h.close()


@pytest.fixture(autouse=True)
def bounded(request):
    """Every GPU test of this file runs as one phase of the library's watchdog (gpuart_hip_phase_begin): a test that hangs ends the
    process after two minutes instead of waiting for ever. A device that no longer answers after a test ends the session: nothing more
    is started on it."""
    if request.node.get_closest_marker("gpu") is None:
        yield
        return
    import torch
    from gpuart_amd import binding
    was = binding.phase_log(False)
    with binding.phase("tests/test_edges.py::" + request.node.name, 120000):
        yield
    binding.phase_log(was)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("the device failed after %s: %s" % (request.node.name, e), 3)


W0, H0 = 160, 120
TILES = {"full": None, "tile": (13, 31, 67, 5), "interleaved": (0, 8, 160, 24, 8, 32)}
SPHERE = (-0.4, 0.0, 0.2, 0.25)


def frame_rows(tile_name):
    """(x0, tw, the frame row of every local row) of a tile of TILES."""
    t = TILES[tile_name]
    if t is None:
        return 0, W0, np.arange(H0)
    if len(t) == 4:
        return t[0], t[2], t[1] + np.arange(t[3])
    x0, y0, tw, th, band, stride = t
    ly = np.arange(th)
    return x0, tw, y0 + (ly // band) * stride + ly % band


def make_backend(B, O, name, tile_name):
    cam = dict(S.DEFAULT_CAMERA, pos=(0.35, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W0, H0)
    tree, _ = O.build_bvh(S.scene_d(12, 12) if name == "triangles" else scene(name))
    be = B.Backend(0)
    be.resize(W0, H0); be.upload_bvh(tree); be.set_camera(c)
    t = TILES[tile_name]
    if t is not None:
        (be.set_tile if len(t) == 4 else be.set_tile_interleaved)(*t)
    return be, tree, c


def oracle_subpixel(O, be, tree, c, tile_name, pixels, seeds, us):
    """(words (n_sub, n, 8), user-sphere mask, uv) of the first segments of the listed local pixels for the draws of `seeds`."""
    x0, tw, rows = frame_rows(tile_name)
    Pm = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
    px = np.asarray(pixels, np.int64)
    fy, fx = rows[px // tw], x0 + px % tw
    words, ush = [], []
    for s in seeds:
        rs, rd = O.first_segment_rays(c, W0, H0, Pm, s)
        o0, o1 = O.traverse(tree, rs[fy, fx].reshape(-1, 4), rd[fy, fx].reshape(-1, 4), us)
        w = np.concatenate([o0, o1], 1).astype(F)
        t = o1[:, 3]
        w[:, 7] = np.floor(t).astype(np.int32).view(F)
        words.append(w)
        ush.append(t == 0.5)
    x, y = np.zeros((len(seeds), 4), F), np.zeros((len(seeds), 4), F)
    x[:, 0], y[:, 0] = seeds[:, 0], seeds[:, 1]
    uv = np.stack([O.random(x)[:, 0], O.random(y)[:, 0]], 1).astype(F)
    return np.stack(words).reshape(len(seeds), -1, 8), np.stack(ush).reshape(len(seeds), -1), uv


def pixel_lists(tw, th, seed, more):
    """The lists of the issue: n = 0, 1, 63, 65, and one that is unordered and has repeats (and holds the pixels `more`)."""
    rs = np.random.RandomState(seed)
    n = tw * th
    mixed = np.concatenate([rs.randint(0, n, 150), [n - 1, 0, n - 1, 0], more])
    rs.shuffle(mixed)
    return [np.zeros(0, np.int64), np.array([n - 1]), np.sort(rs.choice(n, 63, replace=False)), np.sort(rs.choice(n, 65, replace=False)), mixed]


@pytest.mark.gpu
@pytest.mark.parametrize("tile_name", sorted(TILES))
@pytest.mark.parametrize("name", ["box", "scene_p", "triangles"])
def test_trace_subpixel_equals_the_oracles_first_segments(B, O, name, tile_name):
    """gpuart_hip_trace_subpixel with u = O.random(seed.x), v = O.random(seed.y) equals O.traverse(O.first_segment_rays(seed)) bit for
    bit, with and without the user sphere, for n_sub 1 and 3 and every list; the ordinals are those gpuart_hip_trace_rays gives the
    same rays."""
    import torch
    be, tree, c = make_backend(B, O, name, tile_name)
    try:
        _, tw, rows = frame_rows(tile_name)
        on_sphere = np.flatnonzero(be.gbuffer(user_sphere=SPHERE)[1].reshape(-1) == -2)[::3]
        assert on_sphere.size or tile_name == "tile"
        for li, px in enumerate(pixel_lists(tw, len(rows), 5, on_sphere)):
            for n_sub, us in ((1, None), (3, SPHERE)) if li % 2 else ((3, None), (1, SPHERE)):
                seeds = O.randseeds(n_sub, seed=31 + li)
                what = "%s, %s, list %d, n_sub %d, sphere %s" % (name, tile_name, li, n_sub, us)
                d_px = to_device(px.astype(np.int32))
                if len(px) == 0:
                    hits, prims = be.trace_subpixel(d_px, E.offsets(n_sub), float(c[12]), user_sphere=us)
                    assert tuple(hits.shape) == (n_sub, 0, 8) and tuple(prims.shape) == (n_sub, 0), what
                    continue
                exp, ush, uv = oracle_subpixel(O, be, tree, c, tile_name, px, seeds, us)
                hits, prims = be.trace_subpixel(d_px, uv, float(c[12]), user_sphere=us)
                assert tuple(hits.shape) == (n_sub, len(px), 8) and tuple(prims.shape) == (n_sub, len(px))
                got, gp = hits.cpu().numpy(), prims.cpu().numpy()
                assert_same_bits(got.reshape(-1, 8), exp.reshape(-1, 8), what)
                miss = exp[..., 7].view(np.int32) < 0
                assert ((gp == -2) == ush).all() and ((gp == -1) == miss).all() and (gp[~miss & ~ush] >= 0).all(), what
                if us is not None and li == 4 and on_sphere.size:
                    assert ush.any(), what
                # the ordinals: the same rays through gpuart_hip_trace_rays
                x0, _, _ = frame_rows(tile_name)
                Pm = O.make_params(O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE), S.SUN_ALTITUDE, True, (0, 0, 0, 0), 0.0, 0, float(c[12]), c[0:3], 5, 0.01)
                rs, rd = O.first_segment_rays(c, W0, H0, Pm, seeds[0])
                fy, fx = rows[px // tw], x0 + px % tw
                rays = np.zeros((len(px), 8), F)
                rays[:, 0:3], rays[:, 3], rays[:, 4:7] = rs[fy, fx][:, :3], np.inf, rd[fy, fx][:, :3]
                _, rp = be.trace_rays(rays, user_sphere=us, want_prims=True)
                assert (gp[0] == rp).all(), what
                assert torch.equal(d_px.cpu(), torch.from_numpy(px.astype(np.int32)))
    finally:
        be.close()


@pytest.mark.gpu
def test_trace_subpixel_changes_nothing_else_and_checks_its_arguments(B, O):
    """The call leaves the accumulator, the counters and the timed launches alone, and its argument errors write nothing."""
    import torch
    be, tree, c = make_backend(B, O, "box", "tile")
    try:
        L, ctx = be.L, be.ctx
        n = 67 * 5
        px = to_device(np.arange(n, dtype=np.int32))
        uv = np.array([[0.25, 0.75], [0.5, 0.5]], F)
        ps = float(c[12])
        sentinel = torch.full((2, n, 8), 7.0, device="cuda:0")
        sp = torch.full((2, n), 7, dtype=torch.int32, device="cuda:0")
        fp = lambda a: a.ctypes.data_as(C.c_void_p)
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)

        def call(pixels=None, count=n, uvp=None, n_sub=2, pixel_size=ps, hits=None, prims=None):
            return L.gpuart_hip_trace_subpixel(ctx, pixels if pixels is not None else dp(px), C.c_size_t(count), uvp if uvp is not None else fp(uv),
                                               C.c_uint32(n_sub), C.c_float(pixel_size), None, hits if hits is not None else dp(sentinel),
                                               prims if prims is not None else dp(sp))
        assert call(n_sub=0) == ERR_ARG and call(n_sub=17) == ERR_ARG
        assert call(uvp=C.c_void_p(0)) == ERR_ARG
        assert call(uvp=fp(np.array([[0.25, 1.0], [0.5, 0.5]], F))) == ERR_ARG and call(uvp=fp(np.array([[-0.1, 0.0], [0.5, 0.5]], F))) == ERR_ARG
        assert call(uvp=fp(np.array([[np.nan, 0.0], [0.5, 0.5]], F))) == ERR_ARG
        assert call(pixel_size=-1.0) == ERR_ARG and call(pixel_size=float("inf")) == ERR_ARG
        assert call(pixels=C.c_void_p(0)) == ERR_ARG and call(hits=C.c_void_p(0)) == ERR_ARG
        assert call(pixels=dp(px, 2)) == ERR_ARG and call(hits=dp(sentinel, 8)) == ERR_ARG and call(prims=dp(sp, 2)) == ERR_ARG
        assert call(count=2 ** 31 - 1) == ERR_ARG and b"GPUART_HIP_MAX_RAYS" in L.gpuart_hip_last_error()
        assert L.gpuart_hip_trace_subpixel(None, dp(px), C.c_size_t(n), fp(uv), C.c_uint32(2), C.c_float(ps), None, dp(sentinel), dp(sp)) == ERR_ARG
        for bad in (n, n + 5, 2 ** 31, 2 ** 32 - 1):
            lst = np.arange(n, dtype=np.uint32)
            lst[n // 2] = bad
            d_lst = to_device(lst.view(np.int32))
            assert call(pixels=dp(d_lst)) == ERR_ARG and b"outside the 67 x 5 tile" in L.gpuart_hip_last_error(), bad
        be.finish()
        assert (sentinel == 7.0).all() and (sp == 7).all()        # nothing was written
        assert call(count=0, pixels=C.c_void_p(0), hits=C.c_void_p(0), prims=C.c_void_p(0)) == 0     # n = 0 does nothing
        assert call(prims=C.c_void_p(0)) == 0                       # prims is optional
        be.finish()
        assert not (sentinel == 7.0).any() and (sp == 7).all()
        # a context without a scene, a frame or a camera
        b2 = B.Backend(0)
        try:
            args = (dp(px), C.c_size_t(n), fp(uv), C.c_uint32(2), C.c_float(ps), None, dp(sentinel), dp(sp))
            assert L.gpuart_hip_trace_subpixel(b2.ctx, *args) == ERR_ARG
            b2.upload_bvh(tree)
            assert L.gpuart_hip_trace_subpixel(b2.ctx, *args) == ERR_ARG
            b2.resize(W0, H0)
            assert L.gpuart_hip_trace_subpixel(b2.ctx, *args) == ERR_ARG and b"camera" in L.gpuart_hip_last_error()
        finally:
            b2.close()
        # passes, counters and timings
        from tests.test_gen_walk import params, sun_params
        Pm = params(B, sun_params(O, c, 5))
        be.set_mode(4)
        be.pt_reset()
        seeds = O.randseeds(2)
        be.pt_pass(Pm, seeds[0], 1)
        be.finish()
        before = (be.read(1).copy(), be.counters().as_dict(), be.kernel_time(0))
        be.pt_pass(Pm, seeds[1], 1)            # collected, not flushed by the query
        be.launched()
        assert call() == 0
        ran = be.launched(reset=False)    # the query kernel alone: its generation pass, then the walk
        assert ran and all("k_ray_query" in k for k in ran), ran
        be2, _, _ = make_backend(B, O, "box", "tile")
        try:
            be2.set_mode(4)
            be2.pt_reset()
            for s in seeds:               # (the same two runs, without the query between them)
                be2.pt_pass(Pm, s, 1)
                be2.finish()
            assert_same_bits(be.read(1), be2.read(1), "the accumulator after a query between two passes")
            assert be.counters().as_dict() == be2.counters().as_dict() and be.kernel_time(0)[1] == be2.kernel_time(0)[1]
        finally:
            be2.close()
        assert before[1]["rays"] < be.counters().as_dict()["rays"]
    finally:
        be.close()


def check_mark(ed, words, prims, flags, params, what):
    exp = E.mark(words, prims, flags, **{k: v for k, v in dict(E.DEFAULTS, **(params or {})).items() if k != "n_sub"})
    got = ed.mark(to_device(words), to_device(prims), flags, params)
    got = got.cpu().numpy().view(np.uint32)
    assert got.shape == exp.shape and (got == exp).all(), "%s: %d listed, %d expected" % (what, got.size, exp.size)
    return exp


@pytest.mark.gpu
def test_mark_equals_the_restatement(B, O, ed):
    """The list and its count on 1x1, 7x1, 1x7, 67x5 and 160x120 planted tiles with every user-sphere flag, the all-edge and the no-edge
    tile, a non-default setting, and the G-buffers of the box's full frame and of an interleaved share's rows."""
    for c in resolve_cases():
        lst = check_mark(ed, c["words"], c["prims"], c["flags"], {k: v for k, v in c["params"].items()}, c["name"])
        assert (lst == c["lst"]).all()
    for flags in (0, 1, 2, 4):
        c = planted(40 + flags, 67, 5, 1, flags)
        check_mark(ed, c["words"], c["prims"], flags, None, "flags %d" % flags)
    counts = {}
    for tile_name in ("full", "interleaved"):
        be, _, _ = make_backend(B, O, "box", tile_name)
        try:
            hits, prims = be.gbuffer(user_sphere=SPHERE)
            words = np.ascontiguousarray(hits).view(F).reshape(prims.shape + (8,))
            for flags in (0, 1):
                counts[(tile_name, flags)] = check_mark(ed, words, prims, flags, None, "%s, flags %d" % (tile_name, flags)).size
        finally:
            be.close()
    assert all(v > 100 for v in counts.values()), counts


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(6))
def test_mark_across_scan_chunks(B, ed, i):
    """The list and its count where k_ed_scan's loop goes round more than once, or fills one pass exactly (chunk_cases): the carry
    between chunks, s_wave used again, the partial last chunk. The no-edge tile carries a count of 0 through two chunks and writes
    nothing to the list."""
    import torch
    assert len(chunk_cases()) == 6
    c = chunk_cases()[i]
    lst = check_mark(ed, c["words"], c["prims"], c["flags"], dict(c["params"]), c["name"])
    assert (lst == c["lst"]).all()
    if c["name"].startswith("none"):
        h, w = c["prims"].shape
        words, prims = to_device(c["words"]), to_device(c["prims"])
        big = torch.full((h * w + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
        torch.cuda.synchronize()
        assert ed.L.gpuart_edges_mark(ed.h, dp(words), dp(prims), c["flags"], w, h, C.byref(B.EdgesParams(**c["params"])), dp(big), dp(big, 4 * h * w)) == 0
        ed.finish()
        assert int(big[h * w].item()) == 0 and (big[:h * w] == 0x5A5A5A5A).all()


@pytest.mark.gpu
def test_mark_through_one_handle_shrinks_and_grows_across_chunks(B):
    """One handle: 1031 x 130 (three chunks), then 7 x 1 (one word), then 1031 x 130 of another seed. The ballots and prefixes the
    large frames left past the small frame's word, and the small frame's in front of the second large one, do not show."""
    h = B.Edges(0)
    try:
        for c in (chunk_cases()[0], planted(77, 7, 1, 1, 1), planted(78, 1031, 130, 1, 1)):
            lst = check_mark(h, c["words"], c["prims"], c["flags"], dict(c["params"]), c["name"])
            assert (lst == c["lst"]).all()
    finally:
        h.close()


def check_resolve(ed, c):
    """ed.resolve of a planted case against `expected`: bit for bit, the unlisted pixels the input's bits, the input untouched."""
    exp, _ = expected(c)
    d = [to_device(a) for a in (c["filtered"], c["words"], c["prims"], c["lst"].view(np.int32), c["sw"], c["sp"])]
    got = ed.resolve(*d, c["flags"], c["params"]).cpu().numpy()
    assert_same_bits(got, exp, c["name"])
    assert_same_bits(d[0].cpu().numpy(), c["filtered"], c["name"] + ": the input")
    h, w = c["prims"].shape
    listed = np.zeros(h * w, bool)
    listed[c["lst"]] = True
    assert same_bits(got.reshape(-1, 4)[~listed], c["filtered"].reshape(-1, 4)[~listed])
    assert not same_bits(got, c["filtered"])


@pytest.mark.gpu
def test_resolve_with_a_long_list(ed):
    """1031 x 130 with n_sub 2: 111 456 listed pixels in 436 blocks, the second sub-sample's records from index 111 456 on."""
    c = long_list_case()
    assert c["lst"].size > 65536
    check_resolve(ed, c)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(65536, 1), (1, 65536)])
def test_resolve_at_the_limit_shapes(ed, w, h):
    """The longest row and the longest column, n_sub 1: every candidate outside the tile lies on one axis."""
    c = chunk_cases()[2 if h == 1 else 3]
    assert c["prims"].shape == (h, w) and c["params"]["n_sub"] == 1
    check_resolve(ed, c)


@pytest.mark.gpu
@pytest.mark.parametrize("i", range(9))
def test_resolve_equals_the_restatement_on_planted_tiles(ed, i):
    """n_sub 1, 8, 16 and 3, every flag: bit for bit, the unlisted pixels the input's bits, the inputs untouched."""
    assert len(resolve_cases()) == 9
    c = resolve_cases()[i]
    exp, _ = expected(c)
    d = [to_device(a) for a in (c["filtered"], c["words"], c["prims"], c["lst"].view(np.int32), c["sw"], c["sp"])]
    got = ed.resolve(*d, c["flags"], c["params"])
    assert_same_bits(got.cpu().numpy(), exp, c["name"])
    assert_same_bits(d[0].cpu().numpy(), c["filtered"], c["name"] + ": the input")
    h, w = c["prims"].shape
    listed = np.zeros(h * w, bool)
    listed[c["lst"]] = True
    assert same_bits(got.cpu().numpy().reshape(-1, 4)[~listed], c["filtered"].reshape(-1, 4)[~listed])


@pytest.mark.gpu
def test_resolve_takes_any_list(ed):
    """A list that is unordered and has repeats, and one with an index outside the tile (skipped)."""
    c = planted(50, 67, 5, 8, 1)
    rs = np.random.RandomState(3)
    pick = rs.randint(0, c["lst"].size, 200)
    lst, sw, sp = c["lst"][pick], np.ascontiguousarray(c["sw"][:, pick]), np.ascontiguousarray(c["sp"][:, pick])
    exp = E.resolve(c["filtered"], c["words"], c["prims"], lst, sw, sp, c["flags"], **c["params"])
    d = [to_device(a) for a in (c["filtered"], c["words"], c["prims"], lst.view(np.int32), sw, sp)]
    assert_same_bits(ed.resolve(*d, c["flags"], c["params"]).cpu().numpy(), exp, "repeats")
    far = lst.copy()
    far[:5] = [67 * 5, 67 * 5 + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 - 2]
    keep = np.arange(5, lst.size)
    exp = E.resolve(c["filtered"], c["words"], c["prims"], lst[keep], sw[:, keep], sp[:, keep], c["flags"], **c["params"])
    d[3] = to_device(far.view(np.int32))
    assert_same_bits(ed.resolve(*d, c["flags"], c["params"]).cpu().numpy(), exp, "indices outside the tile")


@pytest.mark.gpu
def test_edges_argument_errors(B, ed):
    import torch
    c = planted(60, 33, 9, 2, 1)
    w, h, n = 33, 9, c["lst"].size
    f, words, prims, lst, sw, sp = [to_device(a) for a in (c["filtered"], c["words"], c["prims"], c["lst"].view(np.int32), c["sw"], c["sp"])]
    out = torch.full((h, w, 4), 7.0, device="cuda:0")
    big = torch.full((h * w + 8,), 7, dtype=torch.int32, device="cuda:0")
    L = ed.L
    dp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    pr = lambda **kw: C.byref(B.EdgesParams(**dict(c["params"], **kw)))

    def mark(hits=None, pr_=None, w_=w, h_=h, lst_=None, count=None, prims_=None):
        return L.gpuart_edges_mark(ed.h, hits if hits is not None else dp(words), prims_ if prims_ is not None else dp(prims), 1, w_, h_,
                                   pr_, lst_ if lst_ is not None else dp(big), count if count is not None else dp(big, 4 * h * w))

    def resolve(f_=None, out_=None, pr_=None, lst_=None, n_=n, sw_=None, sp_=None, w_=w, h_=h):
        return L.gpuart_edges_resolve(ed.h, f_ if f_ is not None else dp(f), dp(words), dp(prims), 1, w_, h_, lst_ if lst_ is not None else dp(lst),
                                      C.c_size_t(n_), sw_ if sw_ is not None else dp(sw), sp_ if sp_ is not None else dp(sp),
                                      pr_ if pr_ is not None else pr(), out_ if out_ is not None else dp(out))
    null = C.c_void_p(0)
    assert L.gpuart_edges_mark(None, dp(words), dp(prims), 1, w, h, None, dp(big), dp(big)) == ERR_ARG
    assert mark(hits=null) == ERR_ARG and mark(prims_=null) == ERR_ARG and mark(lst_=null) == ERR_ARG and mark(count=null) == ERR_ARG
    assert mark(hits=dp(words, 4)) == ERR_ARG and mark(lst_=dp(big, 2)) == ERR_ARG and mark(count=dp(big, 1)) == ERR_ARG
    assert mark(w_=0) == ERR_ARG and mark(h_=65537) == ERR_ARG
    for bad in (dict(n_sub=0), dict(n_sub=17), dict(normal_min=1.5), dict(normal_min=float("nan")), dict(plane_tol=-1.0), dict(plane_tol=float("inf"))):
        assert mark(pr_=pr(**bad)) == ERR_ARG and resolve(pr_=pr(**bad)) == ERR_ARG, bad
        with pytest.raises(ValueError):
            r = B.Renderer(16, 8, dict(S.DEFAULT_CAMERA, dir=S.camera_dir(S.DEFAULT_CAMERA)))
            try:
                r.set_edge_resolve(True, dict(c["params"], **bad))
            finally:
                r.close()
    assert resolve(f_=null) == ERR_ARG and resolve(out_=null) == ERR_ARG and resolve(lst_=null) == ERR_ARG and resolve(sw_=null) == ERR_ARG
    assert resolve(sp_=null) == ERR_ARG and resolve(f_=dp(f, 4)) == ERR_ARG and resolve(sw_=dp(sw, 8)) == ERR_ARG and resolve(sp_=dp(sp, 2)) == ERR_ARG
    assert resolve(out_=dp(f)) == ERR_ARG and b"overlaps" in L.gpuart_edges_last_error()
    assert resolve(n_=2 ** 31 - 1) == ERR_ARG and resolve(w_=0) == ERR_ARG
    ed.finish()
    assert (out == 7.0).all() and (big == 7).all()
    assert resolve(n_=0, lst_=null, sw_=null, sp_=null) == 0    # n = 0 copies the frame
    ed.finish()
    assert torch.equal(out, f)
    assert mark(pr_=None) == 0                                   # NULL: the defaults
    ed.finish()
    assert int(big[h * w].item()) == E.mark(c["words"], c["prims"], 1).size


# ---- GPU: the Renderer -------------------------------------------------------------------------------------------------------------
def chain(B, r, filtered, params=None):
    """mark, the sub-pixel rays and resolve of the restatements over the renderer's own G-buffer and its back end's sub-pixel records."""
    pr = dict(E.DEFAULTS, **(params or {}))
    gp = r.params()
    us, flags = tuple(gp.userSphere), gp.userSphereFlags
    hits, prims = r.backend.gbuffer(user_sphere=us)
    words = np.ascontiguousarray(hits).view(F).reshape(prims.shape + (8,))
    lst = E.mark(words, prims, flags, pr["normal_min"], pr["plane_tol"])
    sh, sp = r.backend.trace_subpixel(to_device(lst.view(np.int32)), E.offsets(pr["n_sub"]), gp.pixelSize, user_sphere=us)
    return E.resolve(filtered, words, prims, lst, sh.cpu().numpy(), sp.cpu().numpy(), flags, **pr), lst.size


def cam_at(x):
    cam = dict(S.DEFAULT_CAMERA, pos=(x, -3.05, 1.0))
    cam["dir"] = S.camera_dir(cam)
    return cam


@pytest.mark.gpu
@pytest.mark.parametrize("tile", [None, (8, 16, 67, 37)])
def test_read_denoised_equals_the_chain_of_restatements(B, tile):
    """With the switch on, read_denoised is denoise, mark and resolve of the restatements over the renderer's own accumulator, G-buffer
    and sub-pixel records, bit for bit, and read_display of it the display restatement of that; other parameters reach all three
    steps; SetCamera, SetUserSpherePos, SetTile and SetPrimitives drop the cached list and records."""
    r = B.Renderer(96, 64, cam_at(0.35))
    try:
        r.set_primitives(scene("box"))
        r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
        if tile:
            assert r.set_tile(*tile)
        r.restart_path_tracing(1, 4)
        for _ in range(2):
            r.path_tracing_pass()

        def check(what, params=None):
            gp = r.params()
            hits, prims = r.backend.gbuffer(user_sphere=tuple(gp.userSphere))
            den = D.denoise(r.read_radiance(True), hits, prims, gp.userSphereFlags, **D.DEFAULTS)
            exp, n = chain(B, r, den, params)
            got = r.read_denoised()
            assert_same_bits(got, exp, what)
            assert n > 50 and not same_bits(got, den), what
            assert (r.read_display("denoised") == DR.encode(exp)).all(), what
            assert_same_bits(r.read_denoised(), exp, what + ", cached")
            return got

        plain = r.read_denoised()
        r.set_edge_resolve(True)
        assert r.get_edge_resolve()
        first = check("the defaults")
        assert not same_bits(first, plain)
        r.set_edge_resolve(True, P_X)
        check("other parameters", P_X)
        r.set_edge_resolve(True)
        r.set_camera(cam_at(0.45))
        for _ in range(2):
            r.path_tracing_pass()
        check("after SetCamera")
        r.set_user_sphere_pos((-0.2, 0.1, 0.3))
        r.path_tracing_pass()
        check("after SetUserSpherePos")
        r.set_user_sphere(( -0.2, 0.1, 0.3), SPHERE[3], emittance=0.0)     # the flags change the classes, not the G-buffer
        r.path_tracing_pass()
        check("after the user sphere's flags changed")
        assert r.set_tile(4, 4, 70, 33)
        r.path_tracing_pass()
        check("after SetTile")
        r.set_primitives(scene("scene_p"))
        r.restart_path_tracing(1, 4)
        r.path_tracing_pass()
        check("after SetPrimitives")
        r.set_edge_resolve(False)
        assert not r.get_edge_resolve()
        gp = r.params()
        hits, prims = r.backend.gbuffer(user_sphere=tuple(gp.userSphere))
        assert_same_bits(r.read_denoised(), D.denoise(r.read_radiance(True), hits, prims, gp.userSphereFlags, **D.DEFAULTS), "switched off")
    finally:
        r.close()


@pytest.mark.gpu
def test_the_switch_leaves_everything_else_alone(B):
    """A run with the switch never touched, one with on -> off before anything is read, and one with the switch on and resolved reads
    among the passes: the accumulator, the counters, the timed launches, RenderUntil's summaries and error map are the same in all
    three; every filtered read of the first two is the same, and every filtered read of the third is the chain's resolve of the
    first's."""
    from tests.test_moments import LUM_FLOOR
    from tests.test_temporal import TRACK, cam_dict
    cams = [cam_dict(p) for p in TRACK]

    def run(mode):
        r = B.Renderer(96, 64, cams[0])
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
            r.set_temporal_history(True)
            r.set_history_variance(True)
            if mode == "on_off":
                r.set_edge_resolve(True)
                r.set_edge_resolve(False)
            if mode == "on":
                r.set_edge_resolve(True)
            r.backend.set_mode(4)
            raw, filtered, resolved = [], [], []
            for i, cam in enumerate(cams[:2]):
                if i:
                    r.set_camera(cam)
                r.restart_path_tracing(1, 12)
                for k in range(4):
                    r.path_tracing_pass()
                    if k in (0, 3):
                        assert r.read_denoised() is not None
                raw += [r.read_radiance(False)]
                filtered += [r.read_preview(), r.read_denoised(), r.read_guided_preview(LUM_FLOOR)]
                if mode == "off":
                    resolved += [chain(B, r, f)[0] for f in filtered[-3:]]
            converged, s1 = r.render_until(1e30, 0.0, 4, LUM_FLOOR)
            assert converged and s1["batches"] == 2
            raw += [r.read_radiance(False), r.read_error_map(LUM_FLOOR), r.read_display("radiance")]
            filtered += [r.read_refined(LUM_FLOOR)]
            if mode == "off":
                resolved += [chain(B, r, filtered[-1])[0]]
            filtered += [r.read_display("refined", None, LUM_FLOOR), r.read_display("preview")]
            return raw, filtered, resolved, (r.backend.counters().as_dict(), r.backend.kernel_time(0)[1], s1)
        finally:
            r.close()

    off, on_off, on = run("off"), run("on_off"), run("on")
    assert off[3] == on_off[3] == on[3], (off[3], on_off[3], on[3])
    for k, (a, b, c) in enumerate(zip(off[0], on_off[0], on[0])):
        assert (a == b).all() and (a == c).all(), "raw result %d" % k
    for k, (a, b) in enumerate(zip(off[1], on_off[1])):
        assert (a.view(np.uint8) == b.view(np.uint8)).all(), "filtered result %d after on -> off" % k
    for k, (e, g) in enumerate(zip(off[2], on[1])):
        assert_same_bits(g, e, "resolved read %d" % k)
        assert not same_bits(g, off[1][k])
    assert (on[1][-2] == DR.encode(off[2][-1])).all() and not (on[1][-1] == off[1][-1]).all()


@pytest.mark.gpu
def test_edge_resolve_over_antilag_past_one_scan_chunk(B):
    """320 x 240 (76 800 pixels: 1200 ballot words, two chunks of k_ed_scan) on the box with the emissive user sphere, the history, its
    variance and anti-lag on (tests/test_antilag.py's P_LEAVE, which lets two views of four paths vote), two views of 4 passes of 1
    path with the sphere moved between them by set_user_sphere_pos, so that the history is kept. A run with the switch off and one
    with it on: every filtered read of the second is the chain's resolve of the first's, bit for bit, and not the unresolved frame;
    read_display of the guided preview is the display restatement of the resolved frame; the accumulator, the counters and the error
    map are the same; the restatement's list has entries on both sides of pixel 65 536; and the mix did move the guided preview."""
    from tests.test_antilag import P_LEAVE
    from tests.test_moments import LUM_FLOOR
    W, H = 320, 240
    # closer than the tracks' cameras and looking down: the back wall's upper rim lies in the frame's top rows (from the tracks' cameras
    # everything above row 123 is sky, and the list ends at pixel 39 620)
    cam = dict(S.DEFAULT_CAMERA, pos=(0.1, -1.2, 0.6), target=(0.0, 0.0, 0.2))
    cam["dir"] = S.camera_dir(cam)

    def run(mode):
        r = B.Renderer(W, H, cam)
        try:
            r.set_primitives(scene("box"))
            r.set_user_sphere(SPHERE[:3], SPHERE[3], emittance=2.0)
            r.set_temporal_history(True)
            r.set_history_variance(True)
            r.set_history_antilag(mode != "no_antilag", P_LEAVE)
            r.set_edge_resolve(mode == "on")
            r.backend.set_mode(4)
            raw, filtered, resolved, lists = [], [], [], []
            r.restart_path_tracing(1, 12)
            for i in range(2):
                if i:
                    r.set_user_sphere_pos((-0.2, 0.1, 0.3))
                for _ in range(4):
                    r.path_tracing_pass()
                filtered += [r.read_guided_preview(LUM_FLOOR), r.read_preview(), r.read_denoised()]
                if mode == "no_antilag":
                    continue
                raw += [r.read_radiance(False)]
                if mode == "off":
                    resolved += [chain(B, r, f)[0] for f in filtered[-3:]]
                    gp = r.params()
                    hits, prims = r.backend.gbuffer(user_sphere=tuple(gp.userSphere))
                    lists += [E.mark(np.ascontiguousarray(hits).view(F).reshape(prims.shape + (8,)), prims, gp.userSphereFlags)]
            if mode == "no_antilag":
                return filtered
            shown = r.read_display("guided_preview", None, LUM_FLOOR)
            converged, s1 = r.render_until(1e30, 0.0, 4, LUM_FLOOR)
            assert converged and s1["batches"] == 2
            raw += [r.read_radiance(False), r.read_error_map(LUM_FLOOR)]
            return raw, filtered, resolved, (r.backend.counters().as_dict(), s1), shown, lists
        finally:
            r.close()

    off, on = run("off"), run("on")
    assert off[3] == on[3], (off[3], on[3])
    assert len(off[0]) == len(on[0]) == 4 and off[0][-1] is not None
    for k, (a, b) in enumerate(zip(off[0], on[0])):
        assert_same_bits(b, a, "raw result %d" % k)
    assert len(off[2]) == len(on[1]) == 6
    for k, (e, g) in enumerate(zip(off[2], on[1])):
        assert_same_bits(g, e, "resolved read %d" % k)
        assert not same_bits(g, off[1][k])
    assert (on[4] == DR.encode(off[2][3])).all() and not (on[4] == off[4]).all()
    for lst in off[5]:
        assert (lst < 65536).sum() > 100 and (lst >= 65536).sum() > 100, lst.size
    plain = run("no_antilag")
    assert not same_bits(plain[3], off[1][3])     # the second view's guided preview follows the fast history


@pytest.mark.gpu
def test_gpuart_cli_edge_resolve(tmp_path):
    """gpuart_cli --denoise --edge-resolve writes another frame than --denoise alone; --edge-resolve alone is a usage error."""
    exe = os.path.join(ROOT, "gpuart_amd", "bin", "gpuart_cli")
    base = [exe, "--scene", "box", "--width", "96", "--height", "64", "--spp", "2", "--per-pass", "1", "--denoise"]
    outs = []
    for extra in ([], ["--edge-resolve"]):
        pfm = str(tmp_path / ("f%d.pfm" % len(extra)))
        subprocess.run(base + extra + ["--pfm", pfm], check=True, capture_output=True, timeout=120)
        outs.append(open(pfm, "rb").read())
    assert len(outs[0]) == len(outs[1]) and outs[0] != outs[1]
    bad = subprocess.run([exe, "--scene", "box", "--width", "96", "--height", "64", "--edge-resolve"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "--edge-resolve" in bad.stderr
