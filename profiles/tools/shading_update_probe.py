#!/usr/bin/env python3
"""What changing the lights and materials of a live scene costs (include/p3d_shading.h) against what there was before: a new
scene with the same values.

    python profiles/tools/shading_update_probe.py [--out profiles/scene_update/shading_update.json]

Scene: the 100k-triangle scene with a device-built tree, 20 timed steps after 3 warm-up ones (stream_pose_probe.py's).  A step
recolours every material and moves and dims every light.
1. stream form: p3d_scene_set_shading_device between two events on its stream, the rows in device tensors; a short producer
   keeps the stream busy while the host is inside the call, so that the events bracket GPU work only (`stream_gpu_ms`);
   `stream_call_host_ms` is the host time of the call itself.
2. waiting form: p3d_scene_set_materials + p3d_scene_set_lights from host arrays, wall time with a synchronise either side.
3. new scene: host_set_materials + host_set_lights on the host scene and a fresh DeviceScene(bvh="device") of it, wall time
   likewise; the old scene is destroyed outside the timed part.
There is no threshold: the gain is the removed scene creation."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.abspath(__file__)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(HERE))), help="the checkout whose package is measured")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--triangles", type=int, default=100000)
    return ap.parse_args()


args = parse()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, "scenes"))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import p3d_amd as p3d  # noqa: E402


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return dict(median=xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), min=xs[0], max=xs[-1], n=len(xs))


def values(mats, lights, step):
    """The rows of a step: every diffuse colour and every light's position and colour change; no predicate does"""
    m, l = mats.copy(), lights.copy()
    m[:, 0:3] = 0.5 + 0.4 * np.sin(0.3 * step + np.arange(3, dtype=np.float32))
    l[:, 0:3] += 0.1 * np.float32(np.sin(0.2 * step))
    l[:, 4:7] = 0.6 + 0.3 * np.float32(np.cos(0.25 * step))
    return m.astype(np.float32), l.astype(np.float32)


def main():
    if not torch.cuda.is_available():
        sys.exit("shading_update_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    import make_tri100k
    path = os.path.join(tempfile.mkdtemp(), "tri.p3f")
    make_tri100k.generate(path, n=args.triangles)
    hs = p3d.HostScene(path)
    hs.set_resolution(256, 256)
    a = hs.arrays()
    mats = a["materials"]
    lights = np.zeros((a["n_lights"], 8), np.float32)
    lights[:, 0:3], lights[:, 4:7] = a["lights"][:, 0:3], a["lights"][:, 3:6]
    dev = p3d.DeviceScene(hs, bvh="device")
    steps = [values(mats, lights, k) for k in range(args.warmup + args.steps)]

    side = torch.cuda.Stream()
    ballast = torch.linspace(0, 1, 1 << 24, device="cuda")
    tensors = [(torch.from_numpy(m).cuda(), torch.from_numpy(l).cuda()) for m, l in steps]
    torch.cuda.synchronize()
    gpu_ms, call_ms = [], []
    for d_m, d_l in tensors:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(side):
            for _ in range(8):
                ballast = torch.sin(ballast)
        e0.record(side)
        t0 = time.perf_counter()
        p3d.set_shading_device(dev, d_m, 0, d_l, 0, stream=side)
        call_ms.append(1e3 * (time.perf_counter() - t0))
        e1.record(side)
        side.synchronize()
        gpu_ms.append(e0.elapsed_time(e1))
    assert dev.status() == 0

    waiting = []
    for m, l in steps:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p3d.set_materials(dev, 0, m)
        p3d.set_lights(dev, 0, l)
        torch.cuda.synchronize()
        waiting.append(1e3 * (time.perf_counter() - t0))

    fresh = []
    for m, l in steps:
        dev.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p3d.host_set_materials(hs, 0, m)
        p3d.host_set_lights(hs, 0, l)
        dev = p3d.DeviceScene(hs, bvh="device")
        torch.cuda.synchronize()
        fresh.append(1e3 * (time.perf_counter() - t0))

    w = args.warmup
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=w, triangles=args.triangles, materials=len(mats), lights=len(lights),
                  stream_gpu_ms=spread(gpu_ms[w:]), stream_call_host_ms=spread(call_ms[w:]), waiting_wall_ms=spread(waiting[w:]),
                  new_scene_wall_ms=spread(fresh[w:]))
    print(json.dumps(result), flush=True)
    out = args.out or os.path.join(args.root, "profiles", "scene_update", "shading_update.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
