#!/usr/bin/env python3
"""What the nearest surfaces to a segment (p3d_nearest_segment_k_device) cost on the 100k-triangle scene (scenes/make_tri100k.py)
with a tree built on the device: 2^20 segments whose length is 1 % of the scene's diagonal, at k = 1, 4 and 16, without a limit
and with a limit of 1 % of the diagonal, each without a filter and with an 8-entry skip list (the 8 objects the segment would
find first: the filter changes every answer, as a cloth edge's does).  In the same run, round by round:
  - the yardstick: nearest_k_device, the existing kernel, at the segments' MIDPOINTS, same k and limit;
  - the workaround the query replaces: nearest_k_device at 4 points per segment (4 n points in one call), same k and limit.
On a subset the BVH's answers are compared with the brute force's (P3D_ACCEL_NONE) for bits, with and without the filter - that
is checked before a time is printed.

    python profiles/tools/nearest_segment_probe.py [--out profiles/scene_update/nearest_segment.json] [--segments 1048576]
                                                   [--repeats 10] [--warmup 2] [--subset 8192]

Timing: a pair of events around the call on the current stream (GPU time of what the call enqueues) and a host clock around
call + synchronize; the forms are timed in alternation, round by round, so that a drift of the machine falls on all of them.
Reported: median, min, max in ms."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402

KS = (1, 4, 16)
LABELS = ("no_limit", "limit_1_percent")
SAMPLES = 4


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def timed_in_turn(calls, repeats, warmup):
    """name -> times of the calls, each round running every call once"""
    gpu_ms, wall = {name: [] for name in calls}, {name: [] for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + repeats):
        for name, call in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                wall[name].append((time.perf_counter() - t0) * 1e3)
                gpu_ms[name].append(e0.elapsed_time(e1))
    return {name: dict(gpu_ms=spread(gpu_ms[name]), wall_ms_with_synchronize=spread(wall[name])) for name in calls}


def probe(path, n, repeats, warmup, subset):
    hs = p3d.HostScene(path)
    arrays = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = arrays["prim_bmin"].min(0).astype(np.float64), arrays["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    a = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    b = a + d / np.linalg.norm(d, axis=1)[:, None] * (0.01 * diag)
    d_a, d_b = torch.from_numpy(a.astype(np.float32)).cuda(), torch.from_numpy(b.astype(np.float32)).cuda()
    d_mid = ((d_a + d_b) * 0.5).contiguous()
    steps = torch.linspace(0.0, 1.0, SAMPLES, device="cuda")[None, :, None]
    d_samples = (d_a[:, None, :] + (d_b - d_a)[:, None, :] * steps).reshape(-1, 3).contiguous()
    limits = {"no_limit": (None, None), "limit_1_percent": tuple(torch.full((m,), np.float32(0.01 * diag), dtype=torch.float32, device="cuda")
                                                                 for m in (n, SAMPLES * n))}
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    want = ("dist", "param", "closest")
    outs = {k: {"count": torch.empty(n, **i32), "object": torch.empty((n, k), **i32), "dist": torch.empty((n, k), **f32),
                "param": torch.empty((n, k), **f32), "closest": torch.empty((n, k, 3), **f32)} for k in KS}
    point_outs = {(k, m): {"count": torch.empty(m, **i32), "object": torch.empty((m, k), **i32), "dist": torch.empty((m, k), **f32),
                           "closest": torch.empty((m, k, 3), **f32)} for k in KS for m in (n, SAMPLES * n)}
    out = dict(segments=n, length=0.01 * diag, n_objects=int(arrays["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]),
               diagonal=diag, limit=0.01 * diag, samples_per_segment=SAMPLES, subset=subset)

    # the 8 objects each segment finds first, as its skip list
    p3d.nearest_segment_k_device(dev, p3d.ACCEL_BVH, d_a, d_b, 16, want=want, out=outs[16])
    d_skip = outs[16]["object"][:, :8].contiguous()

    # the answers first: the tree against the brute force on a subset, for bits
    equal = {}
    for label, (lim, _) in limits.items():
        for filtered in (False, True):
            got = {}
            for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
                res = p3d.nearest_segment_k_device(dev, accel, d_a[:subset], d_b[:subset], 16, max_dist=None if lim is None else lim[:subset],
                                                   skip=d_skip[:subset] if filtered else None, want=("dist", "param", "on_segment", "closest", "normal"))
                got[accel] = {name: v.cpu().numpy().tobytes() for name, v in res.items()}
            equal["bvh_equals_none_k16_%s%s" % (label, "_skip8" if filtered else "")] = got[p3d.ACCEL_NONE] == got[p3d.ACCEL_BVH]
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    for label, (lim, lim_samples) in limits.items():
        calls = {}
        for k in KS:
            calls["segment_k%d" % k] = lambda lim=lim, k=k: p3d.nearest_segment_k_device(dev, p3d.ACCEL_BVH, d_a, d_b, k, max_dist=lim, want=want, out=outs[k])
            calls["segment_k%d_skip8" % k] = lambda lim=lim, k=k: p3d.nearest_segment_k_device(dev, p3d.ACCEL_BVH, d_a, d_b, k, max_dist=lim, skip=d_skip,
                                                                                              want=want, out=outs[k])
            calls["midpoint_nearest_k_device_k%d" % k] = lambda lim=lim, k=k: dev.nearest_k_device(p3d.ACCEL_BVH, d_mid, k, max_dist=lim, want=("dist", "closest"),
                                                                                                    out=point_outs[(k, n)])
            calls["sampled_%d_points_nearest_k_device_k%d" % (SAMPLES, k)] = lambda lim=lim_samples, k=k: dev.nearest_k_device(
                p3d.ACCEL_BVH, d_samples, k, max_dist=lim, want=("dist", "closest"), out=point_outs[(k, SAMPLES * n)])
        for name, res in timed_in_turn(calls, repeats, warmup).items():
            out["bvh_%s_%s" % (name, label)] = res
        count = outs[16]["count"].cpu().numpy()
        out["count_k16_skip8_" + label] = dict(zero=int((count == 0).sum()), full=int((count == 16).sum()), mean=float(count.mean()))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update", "nearest_segment.json"))
    ap.add_argument("--segments", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--subset", type=int, default=8192)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.segments, args.repeats, args.warmup, args.subset))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
