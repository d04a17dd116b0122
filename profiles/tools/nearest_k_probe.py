#!/usr/bin/env python3
"""What the k nearest surfaces (p3d_nearest_k_device) cost on the 100k-triangle scene (scenes/make_tri100k.py) with a tree
built on the device, against the nearest-surface query it extends: nearest_device (the yardstick) and nearest_k_device at
k = 1, 4 and 16 through the BVH, each without a limit and with a limit of 1 % of the scene's diagonal; for k = 16 the brute
force (P3D_ACCEL_NONE) as well, whose answers the BVH's must equal in every bit - that is checked before a time is printed.

    python profiles/tools/nearest_k_probe.py [--out profiles/nearest/nearest_k.json] [--points 1048576] [--repeats 20] [--warmup 3]
                                             [--none-repeats 3] [--none-warmup 1]

The points are uniform in the scene's bounding box (nearest_probe.py's, same seed).  The brute force visits 100 000 objects per
point, so it gets fewer repeats.  Timing: a pair of events around the call on the current stream (GPU time of what the call
enqueues) and a host clock around call + synchronize; the forms are timed in alternation, round by round, so that a drift of
the machine falls on all of them.  Reported: median, min, max in ms."""
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


def probe(path, n, repeats, warmup, none_repeats, none_warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    d_p = torch.from_numpy(rng.uniform(lo, hi, (n, 3)).astype(np.float32)).cuda()
    limits = {"no_limit": None, "limit_1_percent": torch.full((n,), np.float32(0.01 * diag), dtype=torch.float32, device="cuda")}
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    one = {"object": torch.empty(n, **i32), "dist": torch.empty(n, **f32), "closest": torch.empty((n, 3), **f32)}
    outs = {k: {"count": torch.empty(n, **i32), "object": torch.empty((n, k), **i32), "dist": torch.empty((n, k), **f32),
                "closest": torch.empty((n, k, 3), **f32)} for k in KS}
    want = ("dist", "closest")
    out = dict(points=n, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag, limit=0.01 * diag)

    def snapshot(tensors):
        return {name: v.cpu().numpy().tobytes() for name, v in tensors.items()}

    # the answers first: the brute force at k = 16 against the BVH at k = 16, k = 1 against nearest_device, prefixes of k = 16
    equal = {}
    for label, lim in limits.items():
        dev.nearest_k_device(p3d.ACCEL_NONE, d_p, 16, max_dist=lim, want=want, out=outs[16])
        brute = snapshot(outs[16])
        dev.nearest_k_device(p3d.ACCEL_BVH, d_p, 16, max_dist=lim, want=want, out=outs[16])
        equal["bvh_equals_none_k16_" + label] = snapshot(outs[16]) == brute
        count16 = outs[16]["count"].cpu().numpy()
        out["count_k16_" + label] = dict(zero=int((count16 == 0).sum()), full=int((count16 == 16).sum()), mean=float(count16.mean()))
        dev.nearest_device(p3d.ACCEL_BVH, d_p, max_dist=lim, want=want, out=one)
        dev.nearest_k_device(p3d.ACCEL_BVH, d_p, 1, max_dist=lim, want=want, out=outs[1])
        equal["k1_equals_nearest_device_" + label] = all(outs[1][name].reshape(one[name].shape).equal(one[name]) for name in one)
        dev.nearest_k_device(p3d.ACCEL_BVH, d_p, 4, max_dist=lim, want=want, out=outs[4])
        keep = torch.arange(4, device="cuda")[None, :] < outs[4]["count"][:, None]
        equal["k4_is_a_prefix_of_k16_" + label] = bool((outs[4]["count"] == outs[16]["count"].clamp(max=4)).all()) and all(
            outs[4][name][keep].equal(outs[16][name][:, :4][keep]) for name in ("object", "dist", "closest"))
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    for label, lim in limits.items():
        calls = {"nearest_device": lambda lim=lim: dev.nearest_device(p3d.ACCEL_BVH, d_p, max_dist=lim, want=want, out=one)}
        for k in KS:
            calls["nearest_k_device_k%d" % k] = lambda lim=lim, k=k: dev.nearest_k_device(p3d.ACCEL_BVH, d_p, k, max_dist=lim, want=want, out=outs[k])
        for name, res in timed_in_turn(calls, repeats, warmup).items():
            out["bvh_%s_%s" % (name, label)] = res
        brute = {"nearest_k_device_k16": lambda lim=lim: dev.nearest_k_device(p3d.ACCEL_NONE, d_p, 16, max_dist=lim, want=want, out=outs[16])}
        for name, res in timed_in_turn(brute, none_repeats, none_warmup).items():
            out["none_%s_%s" % (name, label)] = res
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest", "nearest_k.json"))
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--none-repeats", type=int, default=3)
    ap.add_argument("--none-warmup", type=int, default=1)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, none_repeats=args.none_repeats,
               none_warmup=args.none_warmup, tri100k=probe(tri, args.points, args.repeats, args.warmup, args.none_repeats, args.none_warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
