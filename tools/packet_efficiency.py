#!/usr/bin/env python3
"""Packet efficiency on the CPU (the gate of the packet walk, device_scene.h trav_packet): how many lanes of a 64-query packet take part in
its steps, for the queries k_trace walks as packets, grouped as k_trace sees them.
    python3 tools/packet_efficiency.py [--size 480x270] [--block-order row|z] [--shadow-pool SLOTS] [workload ...]
                                                                             (cfg3 cfg2 tree dragon871k; default: all four)

A packet visits the union of the nodes its queries enter, in the tree's one depth-first order; a query is active at the nodes it enters
itself. Per chunk of 64 consecutive queue entries this prints the packet's node steps (interior + leaf), the mean active lanes per step and
the per-lane visits the per-lane walk makes. Queues:
  * camera rays in k_gen's slot order — 8x8 pixel blocks in row-major block order, pixel-major inside a block, the passes of a run
    interleaved — at 3 passes per run (K = 20) and at 8 (K = 64);
  * the Sun-shadow queries of segment 0 in k_shade's order (the camera rays that hit something, in queue order; a shadow ray leaves the hit
    point towards the Sun), chunks from the start of the shadow part;
  * the Sun-shadow queries a walking k_gen walks itself (GPUART_HIP_GEN_SHADE = 2), at both run lengths: per camera packet, the lanes whose
    hit faces the Sun (face-forwarded normal) — the packet holds only those —, and with --shadow-pool SLOTS the same lanes pooled in slot
    order within groups of SLOTS path slots and cut into packets of 64 (GPUART_HIP_SHADOW_POOL, GPUART_HIP_POOL_CHUNK).
--block-order z: pixel w of an 8x8 block by bit de-interleave (GPUART_HIP_BLOCK_ORDER = 1; kernels_pipeline.h block_pixel) instead of row-major.
Each line ends with the packet steps of the whole run, the figure the orders and pools are compared by.
An ESTIMATE, not the kernel's walk: the box test is the slab test, a closest-hit query prunes with its FINAL closest hit (the oracle's
answer: the real walk, which only learns it on the way, enters at least these nodes) and a shadow query walks the whole tree (the real one
stops at its first hit). The GPU's own count is the GD_STEP_STATS build (tools/step_stats.py)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))
from gpuart_amd import synth_scenes as S  # noqa: E402
from oracle import oracle as O  # noqa: E402

def scene_of(w):
    if w == "cfg2":
        return S.scene_p(), S.DEFAULT_CAMERA, 4
    if w == "tree":
        return S.tree_scene(), S.TREE_NEAR_CAMERA, 5
    if w == "dragon871k":
        return S.scene_d(660, 660), S.BENCH_CAMERA, 8
    return S.scene_d(), S.BENCH_CAMERA, 8


def walk(tree, ro, rd, limit, pkt=None):
    """Union walk of every query at once, node by node. ro, rd: (n, 3); limit: (n,) the pruning bound (entry > limit: not entered).
    Returns (steps, visits) per chunk of 64 queries: nodes the chunk's packet visits, and the nodes its queries enter (summed).
    pkt: (n,) the packet of every query where packets are not 64 consecutive queries."""
    n = ro.shape[0]
    if pkt is None:
        pkt = np.arange(n) >> 6
    nchunks = int(pkt.max()) + 1 if n else 0
    steps = np.zeros(nchunks, np.int64)
    visits = np.zeros(nchunks, np.int64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rdiv = (1.0 / rd).astype(np.float32)
    info = tree.view(np.uint32)
    leaf_bit = np.uint32(1 << 31)  # BVH_LEAF (oracle/restate: the info word's top bit)
    stack = [(0, np.arange(n))]
    while stack:
        node, idx = stack.pop()
        bmin, bmax = tree[node, :3], tree[node + 1, :3]
        o, d = ro[idx], rdiv[idx]
        with np.errstate(invalid="ignore", over="ignore"):
            t1, t2 = (bmin - o) * d, (bmax - o) * d
            tmin = np.nanmax(np.minimum(t1, t2), axis=1)
            tmax = np.nanmin(np.maximum(t1, t2), axis=1)
        inside = np.all((o >= bmin) & (o <= bmax), axis=1)
        entry = np.where(inside, -1.0, tmin)
        ok = (inside | ((tmax >= np.maximum(tmin, 0)) & (tmin >= 0))) & ~(entry > limit[idx])
        idx = idx[ok]
        if idx.size == 0:
            continue
        ch = pkt[idx]
        visits += np.bincount(ch, minlength=nchunks)
        steps[np.unique(ch)] += 1
        flags = info[node + 2, 0]
        if flags & leaf_bit:
            continue
        lo, hi = int(info[node + 2, 1]), int(info[node + 2, 2])
        stack.append((hi, idx))  # (the lower child is walked first; the order does not change the counts)
        stack.append((lo, idx))
    return steps, visits


def report(what, steps, visits, valid):
    keep = valid > 0
    s, v = steps[keep], visits[keep]
    lanes = v / np.maximum(s, 1)
    print("  %-34s chunks %7d  packet steps/chunk %7.1f  per-lane visits/chunk %8.1f  active lanes/step: mean %5.1f  (weighted %5.1f)  "
          "p10 %5.1f  p50 %5.1f  steps of the run %9d" % (what, keep.sum(), s.mean(), v.mean(), lanes.mean(), v.sum() / max(1, s.sum()),
                                                         np.percentile(lanes, 10), np.percentile(lanes, 50), s.sum()), flush=True)
    return v.sum() / max(1, s.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="480x270")
    ap.add_argument("--block-order", choices=["row", "z"], default="row")
    ap.add_argument("--shadow-pool", type=int, default=0, metavar="SLOTS")
    ap.add_argument("workloads", nargs="*", default=["cfg3", "cfg2", "tree", "dragon871k"])
    a = ap.parse_args()
    W, H = (int(x) for x in a.size.split("x"))
    sun = O.sun_direction(S.SUN_AZIMUTH, S.SUN_ALTITUDE)
    for w in a.workloads:
        descs, cam0, segs = scene_of(w)
        tree, depth = O.build_bvh(descs)
        cam = dict(cam0); cam["dir"] = S.camera_dir(cam)
        c = O.camera(cam["pos"], cam["dir"], cam["up"], cam["fov_y"], cam["screen_dist"], W, H)
        P = O.make_params(sun, S.SUN_ALTITUDE, True, S.USER_SPHERE, 0.0, 0, float(c[12]), c[0:3], segs, 0.01)
        print("%s: %d x %d, %d tree quads, depth %d" % (w, W, H, tree.shape[0], depth), flush=True)
        # k_gen's slot order: block-major (row-major blocks), pixel p of a block = (p & 7, p >> 3) or its Z-order, passes interleaved per pixel
        bx, by = (W + 7) // 8, (H + 7) // 8
        blk = np.arange(bx * by)
        p = np.arange(64)
        if a.block_order == "z":
            px_, py_ = (p & 1) | ((p >> 1) & 2) | ((p >> 2) & 4), ((p >> 1) & 1) | ((p >> 2) & 2) | ((p >> 3) & 4)
        else:
            px_, py_ = p & 7, p >> 3
        lx = ((blk[:, None] % bx) * 8 + px_[None, :]).ravel()
        ly = ((blk[:, None] // bx) * 8 + py_[None, :]).ravel()
        for batch in (3, 8):
            seeds = O.randseeds(batch)
            rays = [O.first_segment_rays(c, W, H, P, seeds[k]) for k in range(batch)]
            valid = (lx < W) & (ly < H)
            px, py = np.minimum(lx, W - 1), np.minimum(ly, H - 1)
            ro = np.stack([rays[k][0][py, px, :3] for k in range(batch)], 1).reshape(-1, 3)
            rd = np.stack([rays[k][1][py, px, :3] for k in range(batch)], 1).reshape(-1, 3)
            val = np.repeat(valid, batch)
            ro, rd = ro[val], rd[val]  # (padding slots hold no query; at these sizes they only shift the chunks of the last block row)
            pad = lambda v: np.concatenate([v, np.zeros((v.shape[0], 1), np.float32)], 1)
            o0, o1 = O.traverse(tree, pad(ro), pad(rd))
            t = o0[:, 0]
            limit = np.where(t > 0, t, np.float32(1e19)).astype(np.float32)
            steps, visits = walk(tree, ro, rd, limit)
            valid_ch = np.bincount(np.arange(ro.shape[0]) >> 6)
            report("camera rays, %d passes per run" % batch, steps, visits, valid_ch)
            # k_gen's own shadow packets: the Sun-facing hits of each camera packet (path slots, padding included, 64 at a time)
            nrm = o1[:, :3]
            nrm = np.where((nrm * rd).sum(1, keepdims=True) > 0, -nrm, nrm)
            asks = (t > 0) & ((nrm * sun.astype(np.float32)).sum(1) > 0)
            slot = np.flatnonzero(val)[asks]
            so = o0[asks, 1:4]
            sd = np.broadcast_to(sun.astype(np.float32), so.shape).copy()
            pools = [(64, "own 64 slots")] + ([(a.shadow_pool, "pooled per %d slots" % a.shadow_pool)] if a.shadow_pool else [])
            for slots, name in pools:
                group = slot // slots
                first = np.searchsorted(group, group)  # (slot is ascending) rank of a query within its group
                sub = (np.arange(slot.size) - first) >> 6
                per_group = (np.bincount(group).max() + 63) >> 6 if slot.size else 1
                _, pkt = np.unique(group * per_group + sub, return_inverse=True)
                steps, visits = walk(tree, so, sd, np.full(so.shape[0], np.float32(1e19)), pkt)
                report("k_gen shadow, %d passes, %s" % (batch, name), steps, visits, np.bincount(pkt))
            if batch == 3:
                hit = t > 0
                so = o0[hit, 1:4]
                sd = np.broadcast_to(sun.astype(np.float32), so.shape).copy()
                steps, visits = walk(tree, so, sd, np.full(so.shape[0], np.float32(1e19)))
                report("Sun-shadow rays of segment 0", steps, visits, np.bincount(np.arange(so.shape[0]) >> 6))


if __name__ == "__main__":
    main()
