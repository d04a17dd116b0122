#!/usr/bin/env python3
"""What the hits in order along a ray (p3d_trace_hits_device) cost on the 100k-triangle scene (scenes/make_tri100k.py) with a
tree built on the device, through the BVH: k = 1 without total against trace_closest_device with the same limit (the
yardstick, not a bar: it keeps one hit and ends its traversal differently), k = 4 and k = 16 with and without total, and
k = 0, the count alone - each without a limit and with the distance to the scene's centre as the limit (the near half of the
crossings).

    python profiles/tools/trace_hits_probe.py [--out profiles/ray_query/trace_hits.json] [--rays 1048576] [--repeats 20] [--warmup 3]
                                              [--check 128]

The rays start 1.5 scene radii from the centre and aim into the inner half of the scene, directions normalised in float32:
they cross the mesh several times.  Before any time is taken the BVH's answers (k = 16 with total, k = 4 without) must equal
the brute force's (P3D_ACCEL_NONE) in every bit on the first --check rays that the float64 model of tests/hits_reference.py
calls well-conditioned; the model visits every object per ray in numpy, hence a subset.  Over all the rays the number on which
the two back ends differ at all (k = 0, and k = 4 without total) is counted on the device and reported.  Timing: a pair of events around the
call on the current stream and a host clock around call + synchronize; the forms are timed in alternation, round by round, so
that a drift of the machine falls on all of them.  Reported: median, min, max in ms."""
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

import hits_reference as hr  # noqa: E402
import intersect_reference as ref  # noqa: E402
import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402

KS = (1, 4, 16)
LABELS = ("no_limit", "limit_at_centre")


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


def probe(path, n, repeats, warmup, n_check):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    centre, radius = (lo + hi) / 2, float(np.linalg.norm(hi - lo)) / 2
    rng = np.random.default_rng(1)
    o = (centre + 1.5 * radius * ref._unit(rng, n)).astype(np.float32)
    d = ref.normalize32((centre + 0.5 * radius * ref._in_ball(rng, n)).astype(np.float32) - o)
    d_o, d_d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    limit = np.float32(1.5 * radius)  # as far as the centre of the scene
    limits = {"no_limit": None, "limit_at_centre": torch.full((n,), limit, dtype=torch.float32, device="cuda")}
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    one = {"hit_id": torch.empty(n, **i32), "t": torch.empty(n, **f32)}
    total = {"total": torch.empty(n, **i32)}
    outs = {k: {"count": torch.empty(n, **i32), "object": torch.empty((n, k), **i32), "t": torch.empty((n, k), **f32)} for k in KS}
    with_total = {k: dict(outs[k], **total) for k in KS}
    out = dict(rays=n, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), radius=radius, limit=float(limit))

    # the answers first: the BVH against the brute force on the well-conditioned rays of a subset
    m = min(n_check, n)
    objs = ref.load_objects(path)
    table = ref._all(objs, o[:m], d[:m])
    equal = {}
    for label, lim in limits.items():
        lim_np = None if lim is None else np.full(m, limit, np.float32)
        ok = hr.all_hits_margin(objs, o[:m], d[:m], lim_np, table) >= ref.THRESHOLD
        out["checked_rays_" + label] = dict(rays=m, well_conditioned=int(ok.sum()))
        sub = None if lim is None else lim[:m]
        for k, want in ((16, ("t", "total")), (4, ("t",)), (0, ("total",))):
            got = {name: v.cpu().numpy() for name, v in dev.trace_hits_device(p3d.ACCEL_BVH, d_o[:m], d_d[:m], k, t_max=sub, want=want).items()}
            brute = {name: v.cpu().numpy() for name, v in dev.trace_hits_device(p3d.ACCEL_NONE, d_o[:m], d_d[:m], k, t_max=sub, want=want).items()}
            equal["bvh_equals_none_k%d_%s" % (k, label)] = all(got[name][ok].tobytes() == brute[name][ok].tobytes() for name in got)
            if k == 0:
                out["total_" + label] = dict(zero=int((brute["total"] == 0).sum()), mean=float(brute["total"].mean()), max=int(brute["total"].max()))
    # ... and ALL the rays that get timed, without the model's mask: on how many the two back ends differ (reported, no gate:
    # an ill-conditioned ray may differ).  The brute force visits every object per ray, once per form here
    for label, lim in limits.items():
        for k, want in ((0, ("total",)), (4, ("t",))):
            got = dev.trace_hits_device(p3d.ACCEL_BVH, d_o, d_d, k, t_max=lim, want=want)
            brute = dev.trace_hits_device(p3d.ACCEL_NONE, d_o, d_d, k, t_max=lim, want=want)
            differ = torch.zeros(n, dtype=torch.bool, device="cuda")
            for name in got:
                differ |= (got[name].reshape(n, -1) != brute[name].reshape(n, -1)).any(1)
            out["rays_differing_from_none_k%d_%s" % (k, label)] = int(differ.sum())
            del got, brute
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        dev.close()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    B = p3d.ACCEL_BVH
    for label, lim in limits.items():
        calls = {"trace_closest_device": lambda lim=lim: dev.trace_closest_device(B, d_o, d_d, t_max=lim, out=one),
                 "trace_hits_k0_total": lambda lim=lim: dev.trace_hits_device(B, d_o, d_d, 0, t_max=lim, want=("total",), out=total)}
        for k in KS:
            calls["trace_hits_k%d" % k] = lambda lim=lim, k=k: dev.trace_hits_device(B, d_o, d_d, k, t_max=lim, want=("t",), out=outs[k])
            if k > 1:
                calls["trace_hits_k%d_total" % k] = lambda lim=lim, k=k: dev.trace_hits_device(B, d_o, d_d, k, t_max=lim, want=("t", "total"), out=with_total[k])
        for name, res in timed_in_turn(calls, repeats, warmup).items():
            out["bvh_%s_%s" % (name, label)] = res
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query", "trace_hits.json"))
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--check", type=int, default=128)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.rays, args.repeats, args.warmup, args.check))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
