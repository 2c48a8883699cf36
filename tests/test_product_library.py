"""The product library (gpuart_amd/lib: what bench.py, smoke(), gpuart_cli and every caller of the C++ Renderer load) held to the reference.

The rest of the suite runs on gpuart_amd/lib_test, the product's sources compiled with -DGPUART_HIP_TEST_HOOKS (tests/conftest.py).
Two kinds of evidence tie that to the product:
  * CPU: both builds carry the same device code. Every product kernel has the same instructions and the same per-kernel metadata
    (registers, spills, LDS, scratch, kernarg layout) in the test build, the test build adds only k_test_* kernels, the product has
    none, and the two host libraries have the same code and constant data. A flag, Makefile or #ifdef that reached a kernel of one
    build only would fail here, naming the kernels.
  * GPU: the product pair itself, in fresh child processes (tests/product_frames.py), renders the BASELINE configurations and the
    frame bench.py times, compared with the reference's own renders and with the oracle, bit for bit.
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.util import assert_bits, rmse_per_channel

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRODUCT_DIR = os.path.join(ROOT, "gpuart_amd", "lib")
LLVM = "/opt/rocm/llvm/bin"
GFX950 = "hipv4-amdgcn-amd-amdhsa--gfx950"
RMSE_TOL = 1e-4  # north_star: per-channel RMSE < 1e-4 vs the reference render (the bit comparison below is the stronger check)


# ---- CPU: the two builds run the same kernels ---------------------------------------------------------------------------------


def _tool(name):
    return os.path.join(LLVM, name)


def _code_object(lib, d):
    """The gfx950 code object embedded in a HIP shared library (its .hip_fatbin bundle), written to d; returns its path."""
    tag = os.path.basename(os.path.dirname(lib))
    fatbin = os.path.join(d, tag + ".hip_fatbin")
    co = os.path.join(d, tag + ".gfx950.co")
    subprocess.run([_tool("llvm-objcopy"), "--dump-section=.hip_fatbin=" + fatbin, lib, os.path.join(d, tag + ".stripped")], check=True)
    subprocess.run([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=" + GFX950, "--input=" + fatbin, "--output=" + co],
                   check=True)
    return co


def _functions(co):
    """{symbol: [instruction, ...]} of a code object's disassembly: comments (encodings, branch-target names) and the `...` padding
    marker dropped; branch targets are relative immediates, so a function's text does not depend on where it sits."""
    out = subprocess.run([_tool("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                         text=True).stdout
    funcs, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^<(.+)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins or ins == "...":
            continue
        cur.append(" ".join(ins.split()))
    return funcs


def _kernel_metadata(co):
    """{kernel name: its amdhsa.kernels entry as text lines} of a code object's AMDGPU metadata note; each entry is cut out by itself
    (the list's last entry is followed by the top-level amdhsa.target / amdhsa.version keys, which belong to no kernel)."""
    out = subprocess.run([_tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")) + 1
    blocks, cur = [], None
    for l in lines[start:]:
        if not l.startswith(" "):  # the next top-level key (or the document end) closes the list
            break
        if l.startswith("  - "):
            cur = []
            blocks.append(cur)
        if cur is not None:
            cur.append(l.rstrip())
    kernels = {}
    for b in blocks:
        name = next(l.split(":", 1)[1].strip() for l in b if re.match(r"^\s+\.name:", l))
        assert name not in kernels, "kernel %s listed twice" % name
        kernels[name] = b
    return kernels


def _demangled(names):
    """Short readable kernel names for a failure message ("k_run<true, false, 31>"; the mangled ones if no demangler is there)."""
    import shutil
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True).stdout.splitlines()
    if len(out) != len(names):
        return list(names)
    return [o.replace("(anonymous namespace)::", "").replace("void ", "", 1).split("(")[0] for o in out]


def _section(lib, name, d):
    path = os.path.join(d, "%s%s" % (os.path.basename(os.path.dirname(lib)), name))
    subprocess.run([_tool("llvm-objcopy"), "--dump-section=%s=%s" % (name, path), lib, os.path.join(d, "x.stripped")], check=True)
    with open(path, "rb") as f:
        return f.read()


def test_product_and_test_builds_run_the_same_kernels(tmp_path):
    """The device code of the product library equals that of the library the suite loads (gpuart_amd/lib_test unless GPUART_LIBDIR says
    otherwise), kernel by kernel: same instructions, same metadata. The test build's extra kernels are exactly its k_test_* kernels,
    and the product carries none. The host libraries (libgpuart.so) are built from the same sources with the same flags: same code
    and constant data. This is what makes the hook-based GPU tests evidence about the product."""
    from gpuart_amd import binding as B
    product_hip, product_host = os.path.join(PRODUCT_DIR, "libgpuart_hip.so"), os.path.join(PRODUCT_DIR, "libgpuart.so")
    tested_hip, tested_host = B.HIP_LIB, B.HOST_LIB
    for f in (product_hip, product_host, tested_hip, tested_host):
        assert os.path.exists(f), "%s not built: run __graft_entry__.build()" % f
    dp, dt = tmp_path / "product", tmp_path / "tested"
    dp.mkdir()
    dt.mkdir()
    co_p, co_t = _code_object(product_hip, str(dp)), _code_object(tested_hip, str(dt))

    fp, ft = _functions(co_p), _functions(co_t)
    mp, mt = _kernel_metadata(co_p), _kernel_metadata(co_t)
    assert len(mp) >= 30 and len(fp) >= len(mp), "too few kernels found in %s: %s" % (product_hip, sorted(mp))
    assert all(fp.values()), "a function without instructions: the disassembly was not split as expected"

    in_product = [n for n in list(fp) + list(mp) if "k_test_" in n]
    assert not in_product, "the product library carries test kernels: %s" % sorted(set(in_product))
    missing = sorted(set(fp) - set(ft)) + sorted(set(mp) - set(mt))
    assert not missing, "product kernels absent from the tested build %s: %s" % (tested_hip, missing)
    extra = sorted(n for n in (set(ft) - set(fp)) | (set(mt) - set(mp)) if "k_test_" not in n)
    assert not extra, "the tested build has kernels beyond its k_test_* ones: %s" % extra

    code_differs = sorted(n for n in fp if fp[n] != ft[n])
    meta_differs = sorted(n for n in mp if mp[n] != mt[n])
    assert not code_differs and not meta_differs, (
        "%d of %d product kernels differ in their instructions, %d of %d in their metadata (registers, spills, LDS, scratch, kernargs) "
        "between %s and %s:\n  instructions: %s\n  metadata: %s"
        % (len(code_differs), len(fp), len(meta_differs), len(mp), product_hip, tested_hip, _demangled(code_differs), _demangled(meta_differs)))

    for sec in (".text", ".rodata", ".data.rel.ro"):
        a, b = _section(product_host, sec, str(dp)), _section(tested_host, sec, str(dt))
        assert a == b, "%s of %s and %s differ (%d vs %d bytes)" % (sec, product_host, tested_host, len(a), len(b))


@pytest.mark.parametrize("name", ["refit", "build", "ploc", "edit"])
def test_the_tree_libraries_the_suite_loads_are_copies_of_the_products(name):
    """The four tree libraries have no hooks: gpuart_amd/lib_test holds copies of the gpuart_amd/lib ones (csrc/Makefile), byte for byte."""
    import filecmp
    lib = "libgpuart_%s.so" % name
    product, tested = os.path.join(PRODUCT_DIR, lib), os.path.join(ROOT, "gpuart_amd", "lib_test", lib)
    assert os.path.exists(product) and os.path.exists(tested), "%s not built: run __graft_entry__.build()" % lib
    assert filecmp.cmp(product, tested, shallow=False), "%s and %s differ" % (product, tested)


# ---- CPU: the compile-time knobs and the three diagnostic builds --------------------------------------------------------------------

CSRC = os.path.join(ROOT, "gpuart_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DIAGNOSTIC_BUILDS = ("GD_STEP_STATS", "GD_QUICK_CHECK", "GD_RUN_TIMELINE")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")
@pytest.mark.parametrize("name", DIAGNOSTIC_BUILDS)
def test_a_diagnostic_build_still_compiles(name):
    """No test builds the diagnostic libraries (csrc/hip/diag.h; tools/README.md), so each must at least pass the compiler's front end,
    host and device side, with the Makefile's own flags and the test hooks: what a diagnostic site names must still exist."""
    flags = subprocess.run(["make", "-s", "-C", CSRC, "--eval", "print-hipflags: ; @echo $(HIPFLAGS)", "print-hipflags"], check=True,
                           capture_output=True, text=True).stdout.split()
    assert "--offload-arch=gfx950" in flags, "HIPFLAGS of csrc/Makefile not read: %s" % flags
    r = subprocess.run([HIPCC] + flags + ["-DGPUART_HIP_TEST_HOOKS", "-D" + name, "-fsyntax-only", "hip/gpuart_hip.hip"], cwd=CSRC,
                       capture_output=True, text=True)
    assert r.returncode == 0, "-D%s no longer compiles:\n%s" % (name, r.stderr[-4000:])


def test_the_knob_table_lists_what_the_sources_let_a_build_set():
    """tools/README.md's table of compile-time knobs and diagnostic builds against the device sources: every `#ifndef NAME` that is
    followed by `#define NAME` (a default a build may override) and every `#ifdef GD_*` (a diagnostic build), no more and no fewer. A
    switch added for an experiment shows up here until it is listed or gone."""
    import glob
    found = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "hip", "*.h"))) + [os.path.join(CSRC, "display", "display.hip")]:
        with open(path) as f:
            text = f.read()
        found |= set(re.findall(r"^[ \t]*#[ \t]*ifndef[ \t]+(\w+)[^\n]*\n[ \t]*#[ \t]*define[ \t]+\1\b", text, re.M))
        found |= set(re.findall(r"^[ \t]*#[ \t]*ifdef[ \t]+(GD_\w+)", text, re.M))
        found |= set(re.findall(r"\bdefined[ \t]*\(?[ \t]*(GD_\w+)", text))
    with open(os.path.join(ROOT, "tools", "README.md")) as f:
        doc = f.read()
    section = doc.split("## Compile-time knobs and diagnostic builds", 1)
    assert len(section) == 2, "tools/README.md has no section 'Compile-time knobs and diagnostic builds'"
    listed = re.findall(r"^\| `(\w+)` \|", section[1].split("\n## ", 1)[0], re.M)
    assert len(listed) == len(set(listed)), "listed twice: %s" % sorted(n for n in set(listed) if listed.count(n) > 1)
    assert set(DIAGNOSTIC_BUILDS) <= found, "diagnostic builds the sources no longer know: %s" % sorted(set(DIAGNOSTIC_BUILDS) - found)
    assert found == set(listed), "in the sources, not in the table: %s; in the table, not in the sources: %s" % (
        sorted(found - set(listed)), sorted(set(listed) - found))


# ---- GPU: the product pair against the reference, in fresh child processes --------------------------------------------------------


def _child_env():
    """The product pair, named explicitly (binding.py honours GPUART_LIBDIR; conftest's setdefault does not override it)."""
    return dict(os.environ, GPUART_LIBDIR=PRODUCT_DIR)


def _run_child(args, what, timeout):
    """One child on the product library. No retry: a failed or timed-out child ends the test with what it printed."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "product_frames.py")] + args
    try:
        p = subprocess.run(cmd, cwd=ROOT, env=_child_env(), capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail("%s: no result within %d s\nstdout: %s\nstderr: %s" % (what, timeout, out[-2000:], err[-3000:]))
    assert p.returncode == 0, "%s: child exited %d\nstdout: %s\nstderr: %s" % (what, p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert "product library mapped" in p.stdout, (what, p.stdout[-2000:])
    return p.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", ["cfg1", "cfg2", "cfg3", "cfg4"])
def test_product_renderer_equals_the_reference_renders(cfg):
    """BASELINE cfg1-cfg4 through the product's C++ Renderer, against the reference's own renders on llvmpipe (the fixtures
    test_frames_vs_reference_goldens and test_full_size_frame_vs_reference_checksums hold the test build to): the Renderer's setup
    first (Params, camera basis, RandSeed draws), then direct lighting and path tracing in modes 0 (the planner's grouping: one run
    of the fixture's passes), 3 (launch pipeline) and 5 (persistent run kernel)."""
    out = _run_child(["fixture", cfg], "product Renderer, " + cfg, timeout=180)
    assert "%s OK" % cfg in out, out[-2000:]


def _bench_frame(workload, tmp_path, timeout):
    """bench.py's plain run (the driver's command + --dump-outputs) on the product library; returns (result line, frame)."""
    d = str(tmp_path / ("bench_" + workload))
    args = ["--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", d]
    if workload != "cfg3":
        args += ["--workload", workload]
    out = _run_child(["bench", "--"] + args, "bench.py " + " ".join(args), timeout=timeout)
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "expected exactly one JSON line, got %d:\n%s" % (len(lines), out[-2000:])
    res = json.loads(lines[0])
    assert res["n_gpus"] == 1 and res["steps"] == 20, res
    assert res["config"]["workload"].startswith(workload + ":"), res["config"]["workload"]
    frame = np.load(os.path.join(d, "frame.npy"))
    assert frame.shape == (1080, 1920, 4) and frame.dtype == np.float32, (frame.shape, frame.dtype)
    return res, frame


def _oracle_setup(workload):
    """(oracle module, tree, camera basis, Params) for bench.py's workload: the scene as bench.py:make_renderer builds it."""
    from gpuart_amd import synth_scenes as S
    from oracle import oracle as O
    cam = dict({"cfg3": S.BENCH_CAMERA, "cfg2": S.DEFAULT_CAMERA, "cluster": S.CLUSTER_NEAR_CAMERA, "tree": S.TREE_NEAR_CAMERA}[workload])
    cam["dir"] = S.camera_dir(cam)
    if workload in ("cfg3", "cfg2"):
        descs = S.scene_d() if workload == "cfg3" else S.scene_p()
    else:
        lines = S.cluster_dat_lines() if workload == "cluster" else S.tree_dat_lines()
        descs = S.dat_descs(lines, **(S.CLUSTER_LOAD if workload == "cluster" else S.TREE_LOAD)) + [S.FLOOR_DISC_CT]
    segs = {"cfg3": 8, "cfg2": 4, "cluster": 5, "tree": 5}[workload]
    tree, _ = O.build_bvh(descs)
    c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], 1920, 1080)
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], segs, 0.01)
    return O, tree, c, P


def _oracle_threads():
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        n = 16
    return max(1, min(16, n))


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["cfg3", "cfg2"])
def test_the_frame_bench_times_equals_the_oracle(workload, tmp_path):
    """The frame behind the headline number: `bench.py --gpus 1 --steps 20 --warmup 5` (+ --dump-outputs) on the product library, its
    normalised frame after the 20 timed passes (seeded by set_seed(5489)) against the oracle accumulating the same 20 RandSeeds over
    the whole 1080p frame and dividing by 20 (pt_normalize), bit for bit. At 20 passes of 1080p the planner runs the launch
    pipeline: the timed kernels, at the timed shape, in the shipped binary."""
    _, frame = _bench_frame(workload, tmp_path, timeout=300)
    O, tree, c, P = _oracle_setup(workload)
    exp = np.zeros((1080, 1920, 4), np.float32)
    for sd in O.randseeds(20):
        O.pt_pass(tree, c, 1920, 1080, P, sd, 1, exp, nthreads=_oracle_threads())
    exp = exp / np.float32(20)
    r = rmse_per_channel(frame, exp)
    assert (r < RMSE_TOL).all(), "%s: RMSE %s exceeds %g" % (workload, r, RMSE_TOL)
    assert_bits(frame[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "bench.py %s frame (pixels)" % workload)


@pytest.mark.gpu
@pytest.mark.parametrize("workload", ["tree", "cluster"])
def test_the_frame_bench_times_on_the_loader_scenes(workload, tmp_path):
    """As above for bench.py's two loader workloads (InitTree / InitCluster on the seeded stand-ins, depth 5, near cameras): three 64x8
    windows of the frame, placed as test_cfg4_and_cfg5_at_their_stated_depth places them, against the oracle, bit for bit."""
    _, frame = _bench_frame(workload, tmp_path, timeout=300)
    O, tree, c, P = _oracle_setup(workload)
    seeds = O.randseeds(20)
    W, H = 1920, 1080
    for fx, fy in ((0.5, 0.5), (0.3, 0.12), (0.7, 0.62)):
        y0, x0 = int(fy * H) // 8 * 8, int(fx * W) // 8 * 8
        exp = np.zeros((8, 64, 4), np.float32)
        for sd in seeds:
            O.pt_pass(tree, c, W, H, P, sd, 1, exp, tile=(x0, y0, 64, 8), nthreads=_oracle_threads())
        exp = exp / np.float32(20)
        got = frame[y0:y0 + 8, x0:x0 + 64]
        assert_bits(got[..., :3].reshape(-1, 3), exp[..., :3].reshape(-1, 3), "bench.py %s window at (%d, %d)" % (workload, x0, y0))
