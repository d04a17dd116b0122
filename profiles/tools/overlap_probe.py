#!/usr/bin/env python3
"""What an overlap query (p3d_overlap_box_device) costs on the 100k-triangle scene (scenes/make_tri100k.py) with a tree built on
the device:
  - a voxelisation: 2^21 cells of a 128^3 grid over the scene's bounds (the cells in x-fastest order from the grid's origin),
    at k = 0, the count alone: the occupancy of every cell;
  - 2^20 random boxes whose diagonal is 1 % and 5 % of the scene's, at k = 0, 4 and 16;
each without a filter and with a skip range (1000 objects round a random one: a body that leaves itself out).  In the same run,
round by round, the workaround the query replaces: nearest_k_device at the boxes' CENTRES with the half diagonal as limit, same
k (k = 1 for the count alone).  That answers a different, LOOSER question - the circumscribed ball, not the box, and never more
than 16 objects - so its time is a yardstick for the traversal, not a like-for-like comparison.
Before any time is taken the BVH's answers are compared with the brute force's (P3D_ACCEL_NONE) on a subset for bits, with and
without the range, with and without P3D_OVERLAP_SOLID.

    python profiles/tools/overlap_probe.py [--out profiles/scene_update/overlap.json] [--boxes 1048576] [--cells 2097152]
                                           [--repeats 10] [--warmup 2] [--subset 8192]

Timing: a pair of events around the call on the current stream (GPU time of what the call enqueues); the forms are timed in
alternation, round by round, so that a drift of the machine falls on all of them.  Reported: median, min, max in ms."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402

KS = (0, 4, 16)
SIZES = {"1_percent": 0.01, "5_percent": 0.05}
GRID = 128
RANGE = 1000


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def timed_in_turn(calls, repeats, warmup):
    """name -> GPU times of the calls, each round running every call once"""
    gpu_ms = {name: [] for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + repeats):
        for name, call in calls.items():
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                gpu_ms[name].append(e0.elapsed_time(e1))
    return {name: dict(gpu_ms=spread(gpu_ms[name])) for name in calls}


def probe(path, n, cells, repeats, warmup, subset):
    hs = p3d.HostScene(path)
    arrays = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    n_objs = int(arrays["n_prims"])
    lo, hi = arrays["prim_bmin"].min(0).astype(np.float64), arrays["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    out = dict(boxes=n, cells=cells, grid=GRID, n_objects=n_objs, bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag,
               subset=subset, skip_range_length=RANGE)

    # the inputs: the voxels, and the random boxes of both sizes (a cube with that diagonal, stretched per axis by 0.5 .. 1.5)
    step = (hi - lo) / GRID
    cell = np.arange(cells)
    ijk = np.stack([cell % GRID, (cell // GRID) % GRID, cell // (GRID * GRID)], 1)
    sets = {"voxels": (up(lo + ijk * step), up(lo + (ijk + 1) * step))}
    for label, share in SIZES.items():
        half = 0.5 * share * diag / np.sqrt(3.0) * rng.uniform(0.5, 1.5, (n, 3))
        centre = rng.uniform(lo, hi, (n, 3))
        sets[label] = (up(centre - half), up(centre + half))
    first = rng.integers(0, n_objs, max(n, cells))
    d_range = torch.from_numpy(np.stack([first - RANGE // 2, np.full(len(first), RANGE)], 1).astype(np.int32)).cuda()

    # the answers first: the tree against the brute force on a subset, for bits
    equal = {}
    for label, (d_lo, d_hi) in sets.items():
        for ranged in (False, True):
            for solid in (False, True):
                got = {}
                for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
                    res = p3d.overlap_box_device(dev, accel, d_lo[:subset], d_hi[:subset], 16, skip_range=d_range[:subset] if ranged else None, solid=solid)
                    got[accel] = {name: v.cpu().numpy().tobytes() for name, v in res.items()}
                equal["bvh_equals_none_k16_%s%s%s" % (label, "_range" if ranged else "", "_solid" if solid else "")] = got[p3d.ACCEL_NONE] == got[p3d.ACCEL_BVH]
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    for label, (d_lo, d_hi) in sets.items():
        m = len(d_lo)
        d_centre = ((d_lo + d_hi) * 0.5).contiguous()
        d_radius = (torch.linalg.norm(d_hi - d_lo, dim=1) * 0.5).contiguous()
        calls = {}
        for k in (0,) if label == "voxels" else KS:
            outs = {"total": torch.empty(m, **i32)}
            if k:
                outs["object"] = torch.empty((m, k), **i32)
            kk = max(k, 1)
            ball = {"count": torch.empty(m, **i32), "object": torch.empty((m, kk), **i32), "dist": torch.empty((m, kk), **f32)}
            calls["overlap_k%d" % k] = lambda k=k, outs=outs: p3d.overlap_box_device(dev, p3d.ACCEL_BVH, d_lo, d_hi, k, out=outs)
            calls["overlap_k%d_range" % k] = lambda k=k, outs=outs: p3d.overlap_box_device(dev, p3d.ACCEL_BVH, d_lo, d_hi, k, skip_range=d_range[:m], out=outs)
            calls["ball_nearest_k_device_k%d" % kk] = lambda kk=kk, ball=ball: dev.nearest_k_device(p3d.ACCEL_BVH, d_centre, kk, max_dist=d_radius,
                                                                                                   want=("dist",), out=ball)
        for name, res in timed_in_turn(calls, repeats, warmup).items():
            out["bvh_%s_%s" % (name, label)] = res
        total = p3d.overlap_box_device(dev, p3d.ACCEL_BVH, d_lo, d_hi, 0)["total"].cpu().numpy()
        out["total_" + label] = dict(zero=int((total == 0).sum()), over_16=int((total > 16).sum()), mean=float(total.mean()), max=int(total.max()))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update", "overlap.json"))
    ap.add_argument("--boxes", type=int, default=1 << 20)
    ap.add_argument("--cells", type=int, default=1 << 21)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subset", type=int, default=8192)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.boxes, args.cells, args.repeats, args.warmup, args.subset))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
