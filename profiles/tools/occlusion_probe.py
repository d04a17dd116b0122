#!/usr/bin/env python3
"""What hemisphere occlusion (p3d_occlusion_device) costs on the 100k-triangle scene (scenes/make_tri100k.py) with a tree built
on the device, through the BVH: the fused call at team 1, 16 and 64 against the two-call path it replaces -
occlusion_rays_device, then trace_any_device over the n x samples written rays with the limit repeated per sample (the
reduction of its answers to a count per point is left out of the time: it is in the caller's hands).

    python profiles/tools/occlusion_probe.py [--out profiles/ray_query/occlusion.json] [--points 65536] [--samples 64] [--repeats 20]
                                             [--warmup 3]

The points are the closest hits of rays aimed into the scene from 1.5 scene radii away, their normals the hit objects' turned
against the ray; the limit is 5 % of the scene's diagonal.  Before any time is taken the counts of the three team sizes must
equal each other and the per-point sums of the two-call path's answers, for every point.  Timing: a pair of events around
the call on the current stream and a host clock around call + synchronize; the forms are timed in alternation, round by round,
so that a drift of the machine falls on all of them.  Reported: median, min, max in ms."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import intersect_reference as ref  # noqa: E402
import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402

TEAMS = (1, 16, 64)


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


def surface_points(dev, centre, radius, n):
    """n points on the mesh with unit normals against the rays that found them, on the device"""
    rng = np.random.default_rng(1)
    m = 2 * n
    o = (centre + 1.5 * radius * ref._unit(rng, m)).astype(np.float32)
    d = ref.normalize32((centre + 0.5 * radius * ref._in_ball(rng, m)).astype(np.float32) - o)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hit = dev.trace_closest_device(p3d.ACCEL_BVH, d_o, d_d, want=("hit_point", "normal"))
    keep = torch.nonzero(hit["hit_id"] >= 0).flatten()[:n]
    if len(keep) < n:
        raise SystemExit("only %d of %d rays hit the mesh" % (len(keep), m))
    p, nrm, d_d = hit["hit_point"][keep], hit["normal"][keep], d_d[keep]
    nrm = torch.where(((nrm * d_d).sum(1) > 0)[:, None], -nrm, nrm)
    return p.contiguous(), nrm.contiguous()


def probe(path, n, samples, repeats, warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    centre, diagonal = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    d_p, d_n = surface_points(dev, centre, diagonal / 2, n)
    limit = np.float32(0.05 * diagonal)
    d_limit = torch.full((n,), limit, dtype=torch.float32, device="cuda")
    d_limit_rays = torch.full((n * samples,), limit, dtype=torch.float32, device="cuda")
    out = dict(points=n, samples=samples, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diagonal,
               limit=float(limit))
    B = p3d.ACCEL_BVH
    counts = {t: torch.empty(n, dtype=torch.int32, device="cuda") for t in TEAMS}
    rays = {"origin": torch.empty((n * samples, 3), device="cuda"), "direction": torch.empty((n * samples, 3), device="cuda")}
    occluded = {"occluded": torch.empty(n * samples, dtype=torch.uint8, device="cuda")}

    def fused(team):
        p3d.occlusion_device(dev, B, d_p, d_n, samples, max_dist=d_limit, seed=1, team=team, out={"unoccluded": counts[team]})

    def two_calls():
        p3d.occlusion_rays_device(dev, d_p, d_n, samples, seed=1, out=rays)
        dev.trace_any_device(B, rays["origin"], rays["direction"], t_max=d_limit_rays, out=occluded)

    # the answers first
    for team in TEAMS:
        fused(team)
    two_calls()
    torch.cuda.synchronize()
    want = samples - occluded["occluded"].reshape(n, samples).sum(1, dtype=torch.int32)
    out["counts_equal"] = {"team_%d" % t: bool((counts[t] == want).all()) for t in TEAMS}
    out["unoccluded"] = dict(mean=float(want.float().mean()), none_free=int((want == 0).sum()), all_free=int((want == samples).sum()))
    if not all(out["counts_equal"].values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the counts differ: no time is reported")

    calls = {"occlusion_device_team_%d" % t: (lambda t=t: fused(t)) for t in TEAMS}
    calls["occlusion_rays_device_then_trace_any_device"] = two_calls
    for name, res in timed_in_turn(calls, repeats, warmup).items():
        out["bvh_" + name] = res
    out["bytes_two_call_path"] = dict(rays_written_and_read=2 * n * samples * 24, answers=n * samples)
    out["bytes_fused"] = dict(read=n * 28, written=n * 4)
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "occlusion.json"))
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.points, args.samples, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
