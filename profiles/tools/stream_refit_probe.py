#!/usr/bin/env python3
"""What a REFIT costs once it is enqueued on the caller's stream (p3d_scene_refit_device) instead of waited for.

    python profiles/tools/stream_refit_probe.py [--out profiles/scene_update/stream_refit.json] [--parent-root DIR]

Scenes: the 100k-triangle soup (every position moved) and balls_low (every sphere moved), 20 timed steps after 3 warm-up ones.
1. GPU time: the stream form between two events on its stream, against the update_ms of the waiting form
   (update_triangles / update_spheres with UPDATE_REFIT) for the same buffers - from this tree, and, with --parent-root (a
   checkout of the commit before this entry point, with its library built), from the parent's library in two child
   processes of the same run: the difference of the two parent medians is the spread the comparison allows.
   The events bracket GPU work only: a short producer keeps the stream busy while the host is inside the call, so the first
   event is not stamped during the call's host prologue (`stream_gpu_ms`; `stream_gpu_ms_idle_stream` is the same without
   the producer, host prologue included).
   --merge-kernel-stats DIR adds the per-kernel times of a `rocprofv3 --kernel-trace --stats --output-format csv` run of
   `--trace-only` (23 waiting and 23 stream refits of the triangle scene and nothing else), which tell `refit` from
   `refit_kept_depth` and price the memset launch.
2. Wall time per step of the loop "produce positions on the stream, refit, trace_closest_device of 65 536 rays on the stream",
   with the waiting form and with the stream form, one synchronise at the end.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

HERE = os.path.abspath(__file__)
SPHERE, TRIANGLE = 0, 1


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(HERE))), help="the checkout whose package is measured")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=65536)
    ap.add_argument("--triangles", type=int, default=100000)
    ap.add_argument("--waiting-only", action="store_true", help="update_ms of the waiting REFIT alone (what a parent checkout can do)")
    ap.add_argument("--trace-only", action="store_true", help="waiting and stream refits of the triangle scene alone, to run under a kernel trace")
    ap.add_argument("--merge-kernel-stats", default=None, help="directory of that trace's csv output")
    ap.add_argument("--scene-file", default=None, help="the generated triangle scene, if the caller has one")
    return ap.parse_args()


args = parse()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, "scenes"))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import p3d_amd as p3d  # noqa: E402


def spread(xs):
    xs = sorted(float(x) for x in xs)
    return dict(median=xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), min=xs[0], max=xs[-1], n=len(xs))


class Case:
    """A scene without a grid, its movable objects as one device buffer, and two poses of it to alternate between"""

    def __init__(self, path):
        hs = p3d.HostScene(path)
        hs.set_resolution(256, 256)
        a = hs.arrays()
        self.dev = p3d.DeviceScene(hs, bvh="device")
        kinds = a["prim_type"]
        tri, sph = np.nonzero(kinds == TRIANGLE)[0], np.nonzero(kinds == SPHERE)[0]
        self.spheres = len(sph) > len(tri)
        run = sph if self.spheres else tri
        assert np.array_equal(run, np.arange(run[0], run[0] + len(run)))
        self.first = int(run[0])
        rest = a["prim_v"][run, :4] if self.spheres else a["prim_v"][run].reshape(-1, 3)
        self.rest = torch.from_numpy(np.ascontiguousarray(rest, np.float32)).cuda()
        lo, hi = a["prim_bmin"][run].min(0).astype(np.float64), a["prim_bmax"][run].max(0).astype(np.float64)
        self.reach = 0.01 * float(np.linalg.norm(hi - lo))
        rng = np.random.default_rng(5)
        o = np.tile((lo + hi) / 2 + (hi - lo) * np.array([1.1, 0.9, 1.3]), (args.rays, 1))
        d = rng.uniform(lo, hi, (args.rays, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        self.o, self.d = torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()
        self.out = dict(hit_id=torch.empty(args.rays, dtype=torch.int32, device="cuda"), t=torch.empty(args.rays, dtype=torch.float32, device="cuda"))

    def pose(self, k):
        """The positions of step k, by a few torch operations on the current stream (radii stay)"""
        wave = torch.sin(self.rest * 3.0 + 0.37 * k)
        if self.spheres:
            wave = torch.cat([wave[:, :3], torch.zeros_like(wave[:, 3:])], 1)
        return (self.rest + self.reach * wave).contiguous()

    def waiting(self, pos):
        return self.dev.update_spheres(self.first, pos, mode=p3d.UPDATE_REFIT) if self.spheres else self.dev.update_triangles(self.first, pos, mode=p3d.UPDATE_REFIT)

    def streamed(self, pos, stream):
        (self.dev.refit_spheres if self.spheres else self.dev.refit_triangles)(self.first, pos, stream=stream)

    def trace(self, stream):
        self.dev.trace_closest_device(p3d.ACCEL_BVH, self.o, self.d, want=("hit_id", "t"), stream=stream, out=self.out)


def waiting_update_ms(case):
    poses = [case.pose(k) for k in range(args.warmup + args.steps)]
    torch.cuda.synchronize()
    return spread([case.waiting(p) for p in poses][args.warmup:])


def stream_gpu_ms(case, busy):
    side = torch.cuda.Stream()
    poses = [case.pose(k) for k in range(args.warmup + args.steps)]
    ballast = torch.linspace(0, 1, 1 << 24, device="cuda")
    torch.cuda.synchronize()
    out = []
    for p in poses:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if busy:  # about 0.3 ms of work in front of the first event: the call is enqueued long before the stream gets there
            with torch.cuda.stream(side):
                for _ in range(8):
                    ballast = torch.sin(ballast)
        e0.record(side)
        case.streamed(p, side)
        e1.record(side)
        side.synchronize()
        out.append(e0.elapsed_time(e1))
    return spread(out[args.warmup:])


def loop_wall_ms(case, streamed):
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for k in range(args.warmup + args.steps):
            if k == args.warmup:
                side.synchronize()
                t0 = time.perf_counter()
            pos = case.pose(k)
            if streamed:
                case.streamed(pos, side)
            else:
                case.waiting(pos)
            case.trace(side)
        side.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def kernel_stats(directory):
    """{kernel: {calls, mean_us, min_us, max_us}} of the update kernels, from the per-dispatch rows of a kernel trace"""
    import csv
    import glob
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Kernel_Name") or row.get("Name") or ""
            short = next((k for k in ("gather_geometry_args", "gather_geometry", "refit_kept_depth", "refit", "emit", "fillBuffer") if k in name), None)
            if short is None or "cost" in name:
                continue
            rows.setdefault(short, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return {k: dict(calls=len(v), mean_us=sum(v) / len(v), min_us=min(v), max_us=max(v)) for k, v in rows.items()}


def main():
    if not torch.cuda.is_available():
        sys.exit("stream_refit_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    tri = args.scene_file
    if not tri:
        import make_tri100k
        tri = os.path.join(tempfile.mkdtemp(), "tri.p3f")
        make_tri100k.generate(tri, n=args.triangles)
    scenes = (("tri%dk" % (args.triangles // 1000), tri), ("balls_low", os.path.join(args.root, "tests", "golden", "scenes", "balls_low.p3f")))
    if args.trace_only:
        case = Case(tri)
        side = torch.cuda.Stream()
        poses = [case.pose(k) for k in range(args.warmup + args.steps)]
        torch.cuda.synchronize()
        for p in poses:
            case.waiting(p)
        for p in poses:
            case.streamed(p, side)
        side.synchronize()
        return
    if args.waiting_only:
        with open(args.out, "w") as f:
            json.dump({name: waiting_update_ms(Case(path)) for name, path in scenes}, f)
        return
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, rays=args.rays, scenes={})
    for name, path in scenes:
        case = Case(path)
        r = dict(waiting_update_ms=waiting_update_ms(case), stream_gpu_ms=stream_gpu_ms(case, True), stream_gpu_ms_idle_stream=stream_gpu_ms(case, False))
        r["loop_wall_ms_per_step"] = dict(waiting=loop_wall_ms(case, False), stream=loop_wall_ms(case, True))
        r["loop_wall_ratio_waiting_over_stream"] = r["loop_wall_ms_per_step"]["waiting"] / r["loop_wall_ms_per_step"]["stream"]
        assert case.dev.status() == 0
        result["scenes"][name] = r
        print(name, json.dumps(r), flush=True)
    if args.parent_root:
        env = dict(os.environ)
        env.pop("P3D_LIB", None)
        runs = []
        for k in range(2):
            side = os.path.join(tempfile.mkdtemp(), "parent%d.json" % k)
            subprocess.run([sys.executable, HERE, "--root", args.parent_root, "--waiting-only", "--steps", str(args.steps), "--warmup", str(args.warmup),
                            "--rays", str(args.rays), "--triangles", str(args.triangles), "--scene-file", tri, "--out", side], env=env, check=True, timeout=300)
            runs.append(json.load(open(side)))
        for name, r in result["scenes"].items():
            a, b = runs[0][name], runs[1][name]
            r["parent_waiting_update_ms"] = [a, b]
            r["parent_spread_ms"] = abs(a["median"] - b["median"])
            bound = min(a["median"], b["median"]) + r["parent_spread_ms"]
            r["gpu_time_bound_ms"] = bound
            r["stream_gpu_within_bound"] = r["stream_gpu_ms"]["median"] <= bound
    if args.merge_kernel_stats:
        result["kernel_trace"] = kernel_stats(args.merge_kernel_stats)
    out = args.out or os.path.join(args.root, "profiles", "scene_update", "stream_refit.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
