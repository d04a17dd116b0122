#!/usr/bin/env python3
"""What the path-traced radiance along rays in device memory (p3d_trace_path_device) costs against the path-traced frame: on
scenes/cornell.p3f and tests/golden/scenes/path_balls.p3f at 1024 x 1024, 16 samples, the camera's own sample rays
(p3d_camera_sample_rays_device) traced one sample per call and accumulated, against the frame of that config
(p3d_render_tile_device into device buffers, no counters) - the same floats, which is checked in every bit before any time is
taken.  No bar: the query walks the scene from L2 where the frame kernel of a small scene stages it in LDS, and it runs 16
launches of one sample where the frame runs one of 16.

    python profiles/tools/trace_path_probe.py [--out profiles/ray_query/trace_path.json] [--repeats 10] [--warmup 2]
                                              [--padded build/variants/libp3d_pathpad.so]

--padded: a variant library whose path_query_kernel asks for unused LDS, so that one workgroup fewer fits a CU
(`make -C p3d-raytracer_amd variant NAME=pathpad EXTRA=-DP3D_PATH_QUERY_LDS_PAD=2048`: 8 KB window + 6 KB pending entries +
2 KB = 16 KB, 10 workgroups in 160 KB where 14 KB fit 11).  The query alone (16 samples per call, seeded mode) is then timed
with both libraries, each in a child process of its own, to see whether the LDS or the registers bound this kernel.

Timing: a pair of events around the call on the current stream; the forms are timed in alternation, round by round, so that a
drift of the machine falls on all of them.  Reported: median, min, max in ms, and the ratio of the medians."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import torch  # noqa: E402  (initialised before the library's first HIP call)

import p3d_amd as p3d  # noqa: E402

RES = (1024, 1024)
SPP_SQRT = 4
DEPTH = 20
SCENES = {"cornell": os.path.join(ROOT, "scenes", "cornell.p3f"), "path_balls": os.path.join(ROOT, "tests", "golden", "scenes", "path_balls.p3f")}


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


def open_scene(path):
    hs = p3d.HostScene(path)
    hs.set_resolution(*RES)
    return p3d.DeviceScene(hs, bvh=True), RES[0] * RES[1]


def probe(path, repeats, warmup):
    dev, n = open_scene(path)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=SPP_SQRT, max_depth=DEPTH, seed=0x5EED, collect_stats=0)
    spp = SPP_SQRT * SPP_SQRT
    f_rgb, f_hit = torch.empty((n, 3), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    rays = p3d.camera_sample_rays_device(dev, cfg, 0)
    total, hit = torch.zeros((n, 3), device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")

    def frame():
        dev.render_device(cfg, dev.full_tile(), f_rgb.data_ptr(), f_hit.data_ptr())

    def query():
        total.zero_()
        for s in range(spp):
            p3d.camera_sample_rays_device(dev, cfg, s, out=rays)
            p3d.trace_path_device(dev, p3d.ACCEL_BVH, rays["origin"], rays["direction"], DEPTH, samples=1, sample_begin=s, rng=rays["rng"],
                                  flags=p3d.PATH_ACCUMULATE, want=("hit_id",) if s == 0 else (), out={"rgb": total, "hit_id": hit} if s == 0 else {"rgb": total})

    frame()
    query()
    torch.cuda.synchronize()
    same = bool(((total / spp).view(torch.int32) == f_rgb.view(torch.int32)).all()) and bool((f_hit == hit).all())
    res = dict(rays=n, samples=spp, depth=DEPTH, bits_equal=same, staged_f4=dev.staged_f4(cfg))
    if same:
        res.update(timed_in_turn({"frame_ms": frame, "sample_rays_and_trace_path_ms": query}, repeats, warmup))
        res["query_over_frame"] = res["sample_rays_and_trace_path_ms"]["median"] / res["frame_ms"]["median"]
    res["status_after"] = dev.status()
    dev.close()
    return res


def query_alone(repeats, warmup):
    """In a child process, with the library P3D_LIB names: the query on the pixel-centre rays, 16 samples in one call"""
    out = {}
    for name, path in SCENES.items():
        dev, n = open_scene(path)
        rays = p3d.camera_rays_device(dev)
        q = {"rgb": torch.empty((n, 3), device="cuda"), "hit_id": torch.empty(n, dtype=torch.int32, device="cuda")}
        call = lambda: p3d.trace_path_device(dev, p3d.ACCEL_BVH, rays["origin"], rays["direction"], DEPTH, samples=SPP_SQRT * SPP_SQRT, seed=0x5EED, out=q)
        out[name] = timed_in_turn({"trace_path_ms": call}, repeats, warmup)["trace_path_ms"]
        out[name]["rgb_checksum"] = float(q["rgb"].double().sum())
        dev.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "trace_path.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--padded", default=None, help="a variant library built with -DP3D_PATH_QUERY_LDS_PAD=2048")
    ap.add_argument("--query-alone", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.query_alone:
        return query_alone(args.repeats, args.warmup)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup)
    for name, path in SCENES.items():
        res[name] = probe(path, args.repeats, args.warmup)
    if args.padded:
        alone = {}
        for kind, lib in (("lds_14kb", None), ("lds_16kb", os.path.abspath(args.padded))):
            env = dict(os.environ)
            env.pop("P3D_LIB", None)
            if lib:
                env["P3D_LIB"] = lib
            text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--query-alone", "--repeats", str(args.repeats),
                                            "--warmup", str(args.warmup)], env=env, text=True)
            alone[kind] = json.loads(text.strip().splitlines()[-1])
        res["query_alone_by_lds"] = alone
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))
    if not all(res[s]["bits_equal"] for s in SCENES):
        raise SystemExit("the accumulated samples differ from the frame")


if __name__ == "__main__":
    main()
