#!/usr/bin/env python3
"""What a filter costs the ray queries (p3d_trace_any_filtered_device, p3d_trace_hits_filtered_device,
p3d_occlusion_filtered_device) on the 100k-triangle scene (scenes/make_tri100k.py) with a tree built on the device, through the
BVH.  For each of the three, in one run and in alternation:

  the unfiltered entry point;
  the filtered kernel with a filter that names nothing (a list of eight -1 and a range with count 0): the filter's fixed cost,
  its answers checked to be the unfiltered call's bits before a time is printed;
  the filtered kernel with a filter that skips the ray's first hit (for occlusion: the triangle the point lies on), so that the
  walk goes on behind it.  The boxes are the whole scene's: a filter can make no walk shorter than the unfiltered one.

    python profiles/tools/ray_filter_probe.py [--out profiles/query_walk/ray_filter_probe.json] [--rays 1048576] [--points 65536] [--samples 16] [--repeats 20] [--warmup 3]

Timing as nearest_k_probe.py: a pair of HIP events around the call on the current stream, the forms in alternation round by
round; median, min, max in ms.  Every comparison is with the unfiltered call of the same run."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scenes"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402
from nearest_k_probe import timed_in_turn  # noqa: E402


def probe(path, n, n_points, samples, repeats, warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    B = p3d.ACCEL_BVH
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_o = cuda(rng.uniform(lo, hi, (n, 3)).astype(np.float32))
    direction = rng.normal(size=(n, 3))
    d_d = cuda((direction / np.linalg.norm(direction, axis=1, keepdims=True)).astype(np.float32))
    d_lim = torch.full((n,), np.float32(diag), dtype=torch.float32, device="cuda")
    nothing, no_range = cuda(np.full((n, 8), -1, np.int32)), cuda(np.zeros((n, 2), np.int32))
    out = dict(rays=n, points=n_points, samples=samples, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag)

    # the first hits: what the third form skips, and where the occlusion points lie
    first = dev.trace_hits_device(B, d_o, d_d, 1, t_max=d_lim, want=("hit_point", "normal"))
    d_first = first["object"].contiguous()  # (n, 1): -1 where the ray hits nothing, which names nothing
    hit = torch.nonzero(first["count"] > 0)[:n_points, 0]
    m = int(hit.numel())
    nrm = first["normal"][hit, 0]
    against = (nrm * d_d[hit]).sum(1, keepdim=True) > 0
    d_n = torch.where(against, -nrm, nrm).contiguous()
    d_p = first["hit_point"][hit, 0].contiguous()
    d_own = d_first[hit].contiguous()
    d_reach = torch.full((m,), np.float32(0.05 * diag), dtype=torch.float32, device="cuda")
    out.update(rays_that_hit=int((first["count"] > 0).sum()), occlusion_points=m)
    occ = dict(seed=7, max_dist=d_reach, want=("unoccluded", "bent"))

    equal = {}
    plain = dev.trace_any_device(B, d_o, d_d, t_max=d_lim)
    empty = p3d.trace_any_filtered_device(dev, B, d_o, d_d, t_max=d_lim, skip=nothing, skip_range=no_range)
    equal["any_empty_filter_equals_unfiltered"] = plain["occluded"].equal(empty["occluded"])
    behind = p3d.trace_any_filtered_device(dev, B, d_o, d_d, t_max=d_lim, skip=d_first)
    out["any_occluded_unfiltered"], out["any_occluded_without_the_first_hit"] = int(plain["occluded"].sum()), int(behind["occluded"].sum())
    for k, names in ((4, ("t", "total")), (4, ("t",)), (0, ("total",))):
        plain = dev.trace_hits_device(B, d_o, d_d, k, t_max=d_lim, want=names)
        empty = p3d.trace_hits_filtered_device(dev, B, d_o, d_d, k, t_max=d_lim, skip=nothing, skip_range=no_range, want=names)
        equal["hits_k%d_%s_empty_filter_equals_unfiltered" % (k, "_".join(names))] = all(plain[key].equal(empty[key]) for key in plain)
    second = p3d.trace_hits_filtered_device(dev, B, d_o, d_d, 1, t_max=d_lim, skip=d_first, want=("t",))
    two = dev.trace_hits_device(B, d_o, d_d, 2, t_max=d_lim, want=("t",))
    # (reported, not required: the two walks cull against different bounds, and a box test may decide in the last bits)
    out["hits_k1_without_the_first_differs_from_row_1_of_k2"] = int(((second["object"][:, 0] != two["object"][:, 1]) | (second["t"][:, 0] != two["t"][:, 1])).sum())
    plain = p3d.occlusion_device(dev, B, d_p, d_n, samples, **occ)
    empty = p3d.occlusion_filtered_device(dev, B, d_p, d_n, samples, skip=nothing[:m], skip_range=no_range[:m], **occ)
    equal["occlusion_empty_filter_equals_unfiltered"] = all(plain[key].equal(empty[key]) for key in plain)
    own = p3d.occlusion_filtered_device(dev, B, d_p, d_n, samples, skip=d_own, **occ)
    out["occlusion_free_unfiltered"], out["occlusion_free_without_the_own_triangle"] = int(plain["unoccluded"].sum()), int(own["unoccluded"].sum())
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    F = dict(skip=nothing, skip_range=no_range)
    calls = {
        "any_unfiltered": lambda: dev.trace_any_device(B, d_o, d_d, t_max=d_lim),
        "any_empty_filter": lambda: p3d.trace_any_filtered_device(dev, B, d_o, d_d, t_max=d_lim, **F),
        "any_skip_first_hit": lambda: p3d.trace_any_filtered_device(dev, B, d_o, d_d, t_max=d_lim, skip=d_first),
        "hits_k4_total_unfiltered": lambda: dev.trace_hits_device(B, d_o, d_d, 4, t_max=d_lim, want=("t", "total")),
        "hits_k4_total_empty_filter": lambda: p3d.trace_hits_filtered_device(dev, B, d_o, d_d, 4, t_max=d_lim, want=("t", "total"), **F),
        "hits_k4_total_skip_first_hit": lambda: p3d.trace_hits_filtered_device(dev, B, d_o, d_d, 4, t_max=d_lim, want=("t", "total"), skip=d_first),
        "hits_k1_unfiltered": lambda: dev.trace_hits_device(B, d_o, d_d, 1, t_max=d_lim, want=("t",)),
        "hits_k1_empty_filter": lambda: p3d.trace_hits_filtered_device(dev, B, d_o, d_d, 1, t_max=d_lim, want=("t",), **F),
        "hits_k1_skip_first_hit": lambda: p3d.trace_hits_filtered_device(dev, B, d_o, d_d, 1, t_max=d_lim, want=("t",), skip=d_first),
        "hits_k2_unfiltered_workaround": lambda: dev.trace_hits_device(B, d_o, d_d, 2, t_max=d_lim, want=("t",)),
        "occlusion_unfiltered": lambda: p3d.occlusion_device(dev, B, d_p, d_n, samples, **occ),
        "occlusion_empty_filter": lambda: p3d.occlusion_filtered_device(dev, B, d_p, d_n, samples, skip=nothing[:m], skip_range=no_range[:m], **occ),
        "occlusion_skip_own_triangle": lambda: p3d.occlusion_filtered_device(dev, B, d_p, d_n, samples, skip=d_own, **occ),
    }
    out.update(timed_in_turn(calls, repeats, warmup))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_walk", "ray_filter_probe.json"))
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.rays, args.points, args.samples, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
