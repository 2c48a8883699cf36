"""Shared helpers for the parity tests: golden loading, scene lookup, bit-exact comparison."""
import os
import subprocess

import numpy as np

from gpuart_amd import synth_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def pad4(a, w=0.0):
    a = np.asarray(a, np.float32)
    if a.shape[-1] == 4:
        return a
    return np.concatenate([a, np.full(a.shape[:-1] + (4 - a.shape[-1],), w, np.float32)], -1)


SCENES = {
    "box": S.box_scene,
    "scene_p": S.scene_p,
    "scene_d": S.scene_d,
    "cluster": S.cluster_scene,
    "tree": S.tree_scene,
    "dragon871k": lambda: S.scene_d(660, 660),
    "scene_pc": lambda: S.scene_p(seed=3, nspheres=96, ndiscs=24, ncones=64),
    "lattice": S.lattice_scene,                               # coplanar / coincident primitives: the visiting order decides (round 4)
    "lattice_big": lambda: S.lattice_scene(seed=5, n=3000),   # ... on a tree large enough for the nearest-first kernels by default
}


def scene(name):
    return SCENES[name]()


def bit_mismatch(got, ref):
    """Number of rows whose float32 bit patterns differ (+0/-0 and NaN/NaN count as equal)."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    eq = (got.view(np.uint32) == ref.view(np.uint32)) | ((got == 0) & (ref == 0)) | (np.isnan(got) & np.isnan(ref))
    return int((~eq.reshape(eq.shape[0], -1).all(1)).sum()) if eq.ndim > 1 else int((~eq).sum())


def assert_bits(got, ref, what=""):
    n = bit_mismatch(got, ref)
    assert n == 0, "%s: %d of %d rows differ bitwise" % (what, n, np.asarray(ref).shape[0])


def same_bits(a, b):
    """Strictly bit for bit, unlike bit_mismatch: the image libraries' kernels against their restatements."""
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def assert_same_bits(got, exp, what):
    got, exp = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(exp, np.float32)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if got.ndim == 2:
        got, exp = got[..., None], exp[..., None]
    bad = (got.view(np.uint32) != exp.view(np.uint32)).reshape(-1, got.shape[-1]).any(1)
    assert not bad.any(), "%s: %d of %d pixels differ; first %d: got %s expected %s" % (
        what, int(bad.sum()), bad.size, int(np.argmax(bad)), got.reshape(-1, got.shape[-1])[bad][0], exp.reshape(-1, exp.shape[-1])[bad][0])


def exported(path):
    """The names a shared library defines and exports, sorted."""
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def default_camera():
    """The default camera of the synthetic scenes, with its direction."""
    cam = dict(S.DEFAULT_CAMERA)
    cam["dir"] = S.camera_dir(cam)
    return cam


def to_device(a):
    """A NumPy array as a contiguous torch tensor on GPU 0."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def filter_params_layout(tmp_path, name):
    """[sizeof, the four fields' offsets, GPUART_<NAME>_MAX_ITERATIONS] of gpuart_<name>_params as a C compiler lays include/gpuart_<name>.h out."""
    rec = "gpuart_%s_params" % name
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpuart_%s.h"\n'
                   'int main(void) { printf("%%zu %%zu %%zu %%zu %%zu %%u\\n", sizeof(%s), %s, GPUART_%s_MAX_ITERATIONS); return 0; }\n'
                   % (name, rec, ", ".join("offsetof(%s, %s)" % (rec, f) for f in ("iterations", "lum_k", "normal_pow2", "depth_sigma")), name.upper()))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(os.path.dirname(GOLDEN), os.pardir, "include"), "-o", str(exe), str(src)], check=True)
    return [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]


def rmse_per_channel(got, ref):
    d = np.asarray(got, np.float64)[..., :3] - np.asarray(ref, np.float64)[..., :3]
    return np.sqrt(np.nanmean(d * d, axis=tuple(range(d.ndim - 1))))


def frame_golden_params(O, g):
    """orc Params for a frames_*.npz fixture (defaults = reference defaults)."""
    cam = g["cam"]
    us = g["user_sphere"] if "user_sphere" in g else np.array(S.USER_SPHERE, np.float32)
    em = float(g["user_sphere_em"]) if "user_sphere_em" in g else 0.0
    fl = int(g["user_sphere_flags"]) if "user_sphere_flags" in g else 0
    ms = int(g["max_segments"]) if "max_segments" in g else 5
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    return lambda sun_on=True: O.make_params(sun, S.SUN_ALTITUDE, sun_on, us, em, fl, float(cam[12]), cam[0:3], ms, 0.01)


def fuzz_case_setup(O, seed):
    """(case, tree, camera, params, seeds) of random case `seed` (gpuart_amd.synth_scenes.random_case), as
    tests/golden/make_golden.py `fuzz` and tests/fuzz_parity.py set it up."""
    case = S.random_case(seed)
    cd = case["cam"]
    cam = O.camera(cd["pos"], cd["dir"], cd["up"], cd["fov_y"], cd["screen_dist"], case["W"], case["H"])
    tree, _ = O.build_bvh(case["prims"])
    sun = O.sun_direction(case["sun_az"], case["sun_alt"])
    P = O.make_params(sun, case["sun_alt"], case["sun_on"], case["user_sphere"], case["us_em"], case["us_flags"], float(cam[12]),
                      cam[0:3], case["max_segments"], 0.01)
    return case, tree, cam, P, O.randseeds(case["passes"], seed=5489 + seed)


def row_checksums(img):
    """Per row and channel: sum of the float32 bit patterns (uint64), as tests/golden/make_golden.py `fullsize` stores them."""
    return np.ascontiguousarray(img[..., :3], np.float32).view(np.uint32).astype(np.uint64).sum(axis=1)
