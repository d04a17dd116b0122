#!/usr/bin/env python3
"""What the radiance along rays in device memory (p3d_trace_radiance_device) costs against the frame kernels: on balls_low at
1024 x 1024, depth 4, and on the 100k-triangle scene (scenes/make_tri100k.py, device-built tree) at 1024 x 1024, depth 4, the
radiance of the camera's own rays (p3d_camera_rays_device) against the P3D_STACK_PER_PIXEL frame of that camera
(p3d_render_tile_device into device buffers, no counters) - the same floats, which is checked in every bit before any time
is taken.  No bar: the query walks the scene from L2 where the frame kernel of a small scene stages it in LDS.

    python profiles/tools/trace_radiance_probe.py [--out profiles/ray_query/trace_radiance.json] [--repeats 20] [--warmup 3]

Timing: a pair of events around the call on the current stream; the forms are timed in alternation, round by round, so that a
drift of the machine falls on all of them.  Reported: median, min, max in ms, and the ratio of the medians."""
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

RES = (1024, 1024)
DEPTH = 4


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def timed_in_turn(calls, repeats, warmup):
    """name -> GPU times of the calls, each round running every call once"""
    ms = {name: [] for name in calls}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(warmup + repeats):
        for name, call in calls.items():
            torch.cuda.synchronize()
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {name: spread(v) for name, v in ms.items()}


def probe(path, bvh, accels, repeats, warmup):
    hs = p3d.HostScene(path)
    hs.set_resolution(*RES)
    dev = p3d.DeviceScene(hs, bvh=bvh, grid=p3d.ACCEL_GRID in accels.values())
    n = RES[0] * RES[1]
    rays = p3d.camera_rays_device(dev)
    f_rgb, f_hit = torch.empty((n, 3), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    q = {"rgb": torch.empty((n, 3), device="cuda"), "hit_id": torch.empty(n, dtype=torch.int32, device="cuda")}
    out = dict(rays=n, depth=DEPTH, n_objects=int(hs.arrays()["n_prims"]))
    for name, accel in accels.items():
        cfg = p3d.whitted_config(accel=accel, max_depth=DEPTH, stack_mode=p3d.STACK_PER_PIXEL, collect_stats=0)
        frame = lambda: dev.render_device(cfg, dev.full_tile(), f_rgb.data_ptr(), f_hit.data_ptr())
        query = lambda: p3d.trace_radiance_device(dev, accel, rays["origin"], rays["direction"], DEPTH, out=q)
        frame()
        query()
        torch.cuda.synchronize()
        same = bool((f_rgb.view(torch.int32) == q["rgb"].view(torch.int32)).all()) and bool((f_hit == q["hit_id"]).all())
        res = dict(bits_equal=same, staged_f4=dev.staged_f4(cfg))
        if same:
            res.update(timed_in_turn({"frame_per_pixel_ms": frame, "trace_radiance_ms": query,
                                      "camera_rays_ms": lambda: p3d.camera_rays_device(dev, out=rays)}, repeats, warmup))
            res["radiance_over_frame"] = res["trace_radiance_ms"]["median"] / res["frame_per_pixel_ms"]["median"]
        out[name] = res
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "trace_radiance.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    every = {"bvh": p3d.ACCEL_BVH, "grid": p3d.ACCEL_GRID, "none": p3d.ACCEL_NONE}
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               balls_low=probe(os.path.join(ROOT, "tests", "golden", "scenes", "balls_low.p3f"), True, every, args.repeats, args.warmup),
               tri100k=probe(tri, "device", {"bvh": p3d.ACCEL_BVH}, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(v["bits_equal"] for s in ("balls_low", "tri100k") for v in res[s].values() if isinstance(v, dict)):
        raise SystemExit("the radiance differs from the frame")


if __name__ == "__main__":
    main()
