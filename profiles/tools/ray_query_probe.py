#!/usr/bin/env python3
"""What a batch of ray queries costs on the 100k-triangle scene (scenes/make_tri100k.py), through the BVH built on the device:
the host forms (p3d_trace_closest / p3d_trace_any: two uploads, the null stream, two device waits, the copies back) against
the device forms (p3d_trace_closest_device / p3d_trace_any_device: rays and results in device tensors, one launch on a
stream), and the segment any-hit against a closest hit with the same limit.

    python profiles/tools/ray_query_probe.py [--out profiles/ray_query/ray_query.json] [--res 1024] [--repeats 20] [--warmup 3]

The rays are primary-like: from the scene's eye through the pixels of a res x res image, directions normalised in float32.
The limit of the segment queries is, per ray, the closest hit's t times a factor from {0.5, 0.9, 1.1, 2}, and 3 where nothing
is hit, so about half of the rays that hit something are occluded.
Host forms: a host clock around the call, which waits by itself.  Device forms: a pair of events around the call on the
current stream (GPU time of the kernel and whatever the call enqueues), and a host clock around call + synchronize.
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


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def primary_like(hs, res):
    """(origins, unit directions) float32 (res * res, 3): a pinhole at the scene's eye looking at its `at` point"""
    view = hs.view()
    eye, at, up = (np.asarray(view[k], np.float64) for k in ("from_", "at", "up"))
    angle = view["angle"]
    n = eye - at
    dist = np.linalg.norm(n)
    n /= dist
    u = np.cross(up, n)
    u /= np.linalg.norm(u)
    v = np.cross(n, u)
    half = dist * np.tan(np.radians(float(angle)) / 2)
    px = (np.arange(res) + 0.5) / res * 2 - 1
    x, y = np.meshgrid(px, px)
    d = (x[..., None] * half * u + y[..., None] * half * v - dist * n).reshape(-1, 3).astype(np.float32)
    d /= np.sqrt((d * d).sum(-1, dtype=np.float32), dtype=np.float32)[:, None]
    return np.ascontiguousarray(np.broadcast_to(eye.astype(np.float32), d.shape)), np.ascontiguousarray(d)


def timed_host(call, repeats, warmup):
    wall = []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        call()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return dict(wall_ms=spread(wall))


def timed_device(call, repeats, warmup):
    gpu_ms, wall = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            gpu_ms.append(e0.elapsed_time(e1))
    return dict(gpu_ms=spread(gpu_ms), wall_ms_with_synchronize=spread(wall))


def probe(path, res, repeats, warmup):
    hs = p3d.HostScene(path)
    dev = p3d.DeviceScene(hs, bvh="device")
    o, d = primary_like(hs, res)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    n = len(o)
    accel = p3d.ACCEL_BVH
    out = dict(rays=n, n_objects=int(hs.arrays()["n_prims"]))
    hit, _, t = dev.trace_closest(accel, o, d, want_t=True)
    out["rays_that_hit"] = int((hit >= 0).sum())
    factor = np.random.default_rng(1).choice(np.float32([0.5, 0.9, 1.1, 2.0]), n)
    limit = torch.from_numpy(np.where(hit >= 0, t * factor, np.float32(3)).astype(np.float32)).cuda()
    closest_out = {"hit_id": torch.empty(n, dtype=torch.int32, device="cuda"), "t": torch.empty(n, dtype=torch.float32, device="cuda")}
    any_out = {"occluded": torch.empty(n, dtype=torch.uint8, device="cuda")}
    out["closest_host_form"] = timed_host(lambda: dev.trace_closest(accel, o, d, want_t=True), repeats, warmup)
    out["closest_device_form"] = timed_device(lambda: dev.trace_closest_device(accel, d_o, d_d, out=closest_out), repeats, warmup)
    out["any_host_form"] = timed_host(lambda: dev.trace_any(accel, o, d), repeats, warmup)
    out["any_device_form"] = timed_device(lambda: dev.trace_any_device(accel, d_o, d_d, out=any_out), repeats, warmup)
    out["closest_with_limit"] = timed_device(lambda: dev.trace_closest_device(accel, d_o, d_d, t_max=limit, out=closest_out), repeats, warmup)
    out["segment_any_hit"] = timed_device(lambda: dev.trace_any_device(accel, d_o, d_d, t_max=limit, out=any_out), repeats, warmup)
    # the two answers to "is something in front of the limit" agree wherever the closest hit is the one that decides
    seen = (closest_out["hit_id"] >= 0).cpu().numpy()
    occluded = any_out["occluded"].cpu().numpy().astype(bool)
    out["occluded_rays"] = int(occluded.sum())
    out["segment_differs_from_limited_closest"] = int((seen != occluded).sum())
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "ray_query.json"))
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, res=args.res,
               tri100k=probe(tri, args.res, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
