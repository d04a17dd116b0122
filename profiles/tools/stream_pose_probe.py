#!/usr/bin/env python3
"""What posing a rigged scene costs once it is enqueued on the caller's stream (p3d_scene_set_rig + p3d_scene_pose_device)
instead of waited for (p3d_scene_transform_prims with P3D_UPDATE_REFIT).

    python profiles/tools/stream_pose_probe.py [--out profiles/scene_update/stream_pose.json] [--parent-root DIR]

Scenes: the 100k-triangle scene rigged as 256 bodies of equal size (n // 256 triangles each; the remainder is in no range) and
balls_low with every sphere a body of its own (each with a sphere_scale), 20 timed steps after 3 warm-up ones.  The matrices
of a step are produced by torch on the stream: a rotation about z and a translation per body.
1. GPU time: the stream form between two events on its stream, against the update_ms of the waiting form for the same numbers
   (read back to the host, as that form needs them) - from this tree, and, with --parent-root (a checkout of the commit before
   these entry points, with its library built), from the parent's library in two child processes of the same run.  The bound:
   the stream form's median may not exceed the larger of the parent's two medians plus the difference between them.
   The events bracket GPU work only: a short producer keeps the stream busy while the host is inside the call, so the first
   event is not stamped during the call's host prologue (`stream_gpu_ms`; `stream_gpu_ms_idle_stream` is the same without the
   producer, host prologue included).
2. Wall time per step of the loop "make the matrices on the stream, pose, trace_closest_device of 65 536 rays on the stream",
   with the waiting form (which copies the matrices to the host and waits for the device) and with the stream form, one
   synchronise at the end.  Not gated.
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
    ap.add_argument("--bodies", type=int, default=256)
    ap.add_argument("--waiting-only", action="store_true", help="update_ms of the waiting REFIT alone (what a parent checkout can do)")
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
    """A scene without a grid, its movable objects split into bodies, and a pose per step"""

    def __init__(self, path, rig):
        hs = p3d.HostScene(path)
        hs.set_resolution(256, 256)
        a = hs.arrays()
        self.dev = p3d.DeviceScene(hs, bvh="device")
        kinds = a["prim_type"]
        tri, sph = np.nonzero(kinds == TRIANGLE)[0], np.nonzero(kinds == SPHERE)[0]
        self.spheres = len(sph) > len(tri)
        run = sph if self.spheres else tri
        assert np.array_equal(run, np.arange(run[0], run[0] + len(run)))
        first = int(run[0])
        if self.spheres:
            self.ranges = [(first + k, 1, k) for k in range(len(run))]
        else:
            per = len(run) // args.bodies
            self.ranges = [(first + k * per, per, k) for k in range(args.bodies)]
        self.k = len(self.ranges)
        lo, hi = a["prim_bmin"][run].min(0).astype(np.float64), a["prim_bmax"][run].max(0).astype(np.float64)
        self.reach = 0.01 * float(np.linalg.norm(hi - lo))
        centre = np.stack([(a["prim_bmin"][f:f + c].min(0).astype(np.float64) + a["prim_bmax"][f:f + c].max(0).astype(np.float64)) / 2 for f, c, _ in self.ranges])
        self.centre = torch.from_numpy(centre.astype(np.float32)).cuda()
        self.phase = torch.arange(self.k, dtype=torch.float32, device="cuda")
        rng = np.random.default_rng(5)
        o = np.tile((lo + hi) / 2 + (hi - lo) * np.array([1.1, 0.9, 1.3]), (args.rays, 1))
        d = rng.uniform(lo, hi, (args.rays, 3)) - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        self.o, self.d = torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()
        self.out = dict(hit_id=torch.empty(args.rays, dtype=torch.int32, device="cuda"), t=torch.empty(args.rays, dtype=torch.float32, device="cuda"))
        if rig:
            self.dev.set_rig(self.ranges, self.k)

    def pose(self, step):
        """([K, 3, 4] matrices, [K] sphere scales or None) of a step, by a few torch operations on the current stream: every body
        turns about the vertical through its centre and slides"""
        ang = 0.05 * torch.sin(self.phase + 0.37 * step)
        c, s, z, one = torch.cos(ang), torch.sin(ang), torch.zeros_like(ang), torch.ones_like(ang)
        rot = torch.stack([torch.stack([c, -s, z], 1), torch.stack([s, c, z], 1), torch.stack([z, z, one], 1)], 1)  # [K, 3, 3]
        slide = self.reach * torch.stack([torch.sin(self.phase * 1.3 + 0.2 * step), torch.cos(self.phase * 0.7 + 0.3 * step), 0.5 * ang], 1)
        t = self.centre - torch.bmm(rot, self.centre.unsqueeze(2)).squeeze(2) + slide
        m = torch.cat([rot, t.unsqueeze(2)], 2).contiguous()
        return m, (1.0 + 0.1 * torch.sin(self.phase + 0.5 * step)).contiguous() if self.spheres else None

    def waiting(self, pose):
        m, sc = pose
        return self.dev.transform_prims(self.ranges, m.cpu().numpy(), p3d.UPDATE_REFIT, sphere_scale=None if sc is None else sc.cpu().numpy())

    def streamed(self, pose, stream):
        self.dev.pose_device(pose[0], pose[1], stream=stream)

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
            pose = case.pose(k)
            if streamed:
                case.streamed(pose, side)
            else:
                case.waiting(pose)
            case.trace(side)
        side.synchronize()
    return 1e3 * (time.perf_counter() - t0) / args.steps


def main():
    if not torch.cuda.is_available():
        sys.exit("stream_pose_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    tri = args.scene_file
    if not tri:
        import make_tri100k
        tri = os.path.join(tempfile.mkdtemp(), "tri.p3f")
        make_tri100k.generate(tri, n=args.triangles)
    scenes = (("tri%dk" % (args.triangles // 1000), tri), ("balls_low", os.path.join(args.root, "tests", "golden", "scenes", "balls_low.p3f")))
    if args.waiting_only:
        with open(args.out, "w") as f:
            json.dump({name: waiting_update_ms(Case(path, False)) for name, path in scenes}, f)
        return
    result = dict(device=torch.cuda.get_device_name(0), steps=args.steps, warmup=args.warmup, rays=args.rays, scenes={})
    for name, path in scenes:
        case = Case(path, True)
        r = dict(bodies=case.k, posed_objects=case.dev.rig()["n_posed_objects"], waiting_update_ms=waiting_update_ms(case),
                 stream_gpu_ms=stream_gpu_ms(case, True), stream_gpu_ms_idle_stream=stream_gpu_ms(case, False))
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
                            "--rays", str(args.rays), "--triangles", str(args.triangles), "--bodies", str(args.bodies), "--scene-file", tri, "--out", side],
                           env=env, check=True, timeout=300)
            runs.append(json.load(open(side)))
        for name, r in result["scenes"].items():
            a, b = runs[0][name], runs[1][name]
            r["parent_waiting_update_ms"] = [a, b]
            r["parent_spread_ms"] = abs(a["median"] - b["median"])
            bound = max(a["median"], b["median"]) + r["parent_spread_ms"]
            r["gpu_time_bound_ms"] = bound
            r["stream_gpu_within_bound"] = r["stream_gpu_ms"]["median"] <= bound
            print(name, "bound %.4f ms, stream %.4f ms: %s" % (bound, r["stream_gpu_ms"]["median"], "met" if r["stream_gpu_within_bound"] else "NOT met"), flush=True)
    out = args.out or os.path.join(args.root, "profiles", "scene_update", "stream_pose.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
