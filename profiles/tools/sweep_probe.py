#!/usr/bin/env python3
"""What a sphere sweep (p3d_sweep_sphere_device) costs on the 100k-triangle scene (scenes/make_tri100k.py) with a tree built on
the device, against the closest-hit ray query on the same rays: trace_closest_device (the yardstick), the sweep at r = 0 (the
same question, asked of grown boxes and the sweep rule), and the sweep at r = 1 % of the scene's diagonal with a limit of one
diagonal.  All through the BVH.

    python profiles/tools/sweep_probe.py [--out profiles/ray_query/sweep.json] [--rays 1048576] [--repeats 20] [--warmup 3]

The rays start uniformly in the scene's bounding box grown by a quarter and point at uniform points inside it (unit
directions, so t is a length).  Before a time is printed the sweep at r = 0 is compared with the ray query: where both meet
something the object must agree on all but a thousandth of the rays (a ray that starts within 1e-4 of a triangle: the ray
query skips that hit, the sweep has no such threshold; a ray that grazes an edge two triangles share), and t on the same
object to 1e-4 of the diagonal.  Timing: a pair of events around the call on the current stream (GPU time of what the call
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


def probe(path, n, repeats, warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    mid, half, diag = (lo + hi) / 2, (hi - lo) / 2, float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    o = mid + 1.25 * half * rng.uniform(-1, 1, (n, 3))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    d_o, d_d = torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()
    f32, i32 = dict(dtype=torch.float32, device="cuda"), dict(dtype=torch.int32, device="cuda")
    r0, r1 = torch.zeros(n, **f32), torch.full((n,), np.float32(0.01 * diag), **f32)
    limit = torch.full((n,), np.float32(diag), **f32)
    ray = {"hit_id": torch.empty(n, **i32), "t": torch.empty(n, **f32), "hit_point": torch.empty((n, 3), **f32)}
    swept = {"object": torch.empty(n, **i32), "t": torch.empty(n, **f32), "contact": torch.empty((n, 3), **f32)}
    out = dict(rays=n, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag, radius=0.01 * diag, limit=diag)
    calls = {
        "trace_closest_device": lambda: dev.trace_closest_device(p3d.ACCEL_BVH, d_o, d_d, want=("t", "hit_point"), out=ray),
        "sweep_sphere_device_r0": lambda: p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, d_o, d_d, r0, want=("t", "contact"), out=swept),
        "sweep_sphere_device_r1_percent_limited": lambda: p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, d_o, d_d, r1, t_max=limit, want=("t", "contact"), out=swept),
    }
    # the answers first
    calls["trace_closest_device"]()
    calls["sweep_sphere_device_r0"]()
    torch.cuda.synchronize()
    hit, obj = ray["hit_id"].cpu().numpy(), swept["object"].cpu().numpy()
    both = (hit >= 0) & (obj >= 0)
    t_ray, t_sweep = ray["t"].cpu().numpy(), swept["t"].cpu().numpy()
    same, other = both & (hit == obj), both & (hit != obj)
    t_off = float(np.abs(t_ray[same] - t_sweep[same]).max()) if same.any() else 0.0
    # (the ray query takes no hit nearer than 1e-4, the sweep has no such threshold: a ray that starts on a triangle sees the next one)
    out["r0_against_the_ray_query"] = dict(ray_hits=int((hit >= 0).sum()), sweep_hits=int((obj >= 0).sum()), one_only=int(((hit >= 0) != (obj >= 0)).sum()),
                                           other_object=int(other.sum()), other_object_with_sweep_t_under_1e_4=int((other & (t_sweep < 1e-4)).sum()),
                                           other_object_within_1e_4_in_t=int((other & (np.abs(t_ray - t_sweep) <= 1e-4 * diag)).sum()),
                                           largest_t_difference_on_the_same_object=t_off)
    calls["sweep_sphere_device_r1_percent_limited"]()
    torch.cuda.synchronize()
    obj1, t1 = swept["object"].cpu().numpy(), swept["t"].cpu().numpy()
    out["r1_percent_limited"] = dict(met=int((obj1 >= 0).sum()), at_the_start=int(((obj1 >= 0) & (t1 == 0)).sum()))
    agree = out["r0_against_the_ray_query"]
    if agree["one_only"] > n // 1000 or agree["other_object"] > n // 1000 or t_off > 1e-4 * diag or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the sweep at r = 0 and the ray query disagree: no time is reported")
    out.update(timed_in_turn(calls, repeats, warmup))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "sweep.json"))
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, tri100k=probe(tri, args.rays, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
