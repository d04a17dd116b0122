#!/usr/bin/env python3
"""What a filter costs and saves (p3d_nearest_k_filtered_device, p3d_sweep_sphere_filtered_device) on the 100k-triangle scene
(scenes/make_tri100k.py) with a tree built on the device, through the BVH:

  (a) the filter's fixed cost: the filtered kernel with a filter that names nothing (a list of -1 and a range with count 0)
      against the unfiltered entry point, for the nearest query at k = 1 and for the sweep, on random points and rays;
  (b) self-proximity: the scene's own vertices, each skipping the triangle it belongs to (the scene is a soup: one triangle per
      vertex, n_skip = 1), at k = 1, against the workaround without a filter, nearest_k_device at k = 1 + n_skip, whose second
      row is the answer - that is checked before a time is printed;
  (c) the same for the sweep: a ball of radius 1 % of the diagonal round each vertex, skipping its own triangle, against the
      unfiltered sweep (which has no workaround: it answers T = 0 on the ball's own triangle).

    python profiles/tools/filtered_query_probe.py [--out profiles/query_walk/filtered_query_probe.json] [--points 1048576] [--repeats 20] [--warmup 3]

Timing as nearest_k_probe.py: a pair of events around the call on the current stream, the forms in alternation round by round;
median, min, max in ms."""
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


def probe(path, n, repeats, warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    B = p3d.ACCEL_BVH
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_p = cuda(rng.uniform(lo, hi, (n, 3)).astype(np.float32))
    d_o = cuda(rng.uniform(lo, hi, (n, 3)).astype(np.float32))
    direction = rng.normal(size=(n, 3))
    d_d = cuda((direction / np.linalg.norm(direction, axis=1, keepdims=True)).astype(np.float32))
    d_r = torch.full((n,), np.float32(0.01 * diag), dtype=torch.float32, device="cuda")
    d_lim = torch.full((n,), np.float32(diag), dtype=torch.float32, device="cuda")
    nothing, no_range = cuda(np.full((n, 8), -1, np.int32)), cuda(np.zeros((n, 2), np.int32))
    # the scene's own vertices: corner c of triangle j is row 3 j + c, and skips object j
    corners = a["prim_v"][:, :9].reshape(-1, 3).astype(np.float32)
    pick = rng.permutation(len(corners))[:n]
    d_v, d_own = cuda(corners[pick]), cuda((pick // 3).astype(np.int32)[:, None])
    m = len(pick)
    d_vd, d_vr, d_vlim = d_d[:m], d_r[:m], d_lim[:m]
    out = dict(points=n, vertices=m, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag)
    want = ("dist", "closest")

    # the answers first
    plain = dev.nearest_k_device(B, d_p, 1, want=want)
    empty = p3d.nearest_k_filtered_device(dev, B, d_p, 1, skip=nothing, skip_range=no_range, want=want)
    equal = {"nearest_empty_filter_equals_unfiltered": all(plain[k].equal(empty[k]) for k in plain)}
    plain = p3d.sweep_sphere_device(dev, B, d_o, d_d, d_r, t_max=d_lim, want=("t", "centre", "contact"))
    empty = p3d.sweep_sphere_filtered_device(dev, B, d_o, d_d, d_r, t_max=d_lim, skip=nothing, skip_range=no_range, want=("t", "centre", "contact"))
    equal["sweep_empty_filter_equals_unfiltered"] = all(plain[k].equal(empty[k]) for k in plain)
    own = p3d.nearest_k_filtered_device(dev, B, d_v, 1, skip=d_own, want=want)
    two = dev.nearest_k_device(B, d_v, 2, want=want)
    first_is_own = two["object"][:, 0] == d_own[:, 0]  # (a neighbour that touches the vertex may tie at 0 with a lower index)
    row = torch.where(first_is_own, 1, 0)
    pick_row = lambda t: t[torch.arange(m, device="cuda"), row]
    equal["self_proximity_equals_the_workaround"] = all(own[k][:, 0].equal(pick_row(two[k])) for k in ("object", "dist", "closest"))
    out["unfiltered_finds_own_triangle_at_0"] = int(((two["dist"][:, 0] == 0)).sum())
    swept = p3d.sweep_sphere_filtered_device(dev, B, d_v, d_vd, d_vr, t_max=d_vlim, skip=d_own, want=("t",))
    self_hit = p3d.sweep_sphere_device(dev, B, d_v, d_vd, d_vr, t_max=d_vlim, want=("t",))
    out["sweep_unfiltered_t0"] = int((self_hit["t"] == 0).sum())
    out["sweep_filtered_t0"] = int((swept["t"] == 0).sum())
    equal["sweep_filtered_never_names_its_own"] = bool((swept["object"] != d_own[:, 0]).all())
    torch.cuda.synchronize()
    out.update(equal)
    if not all(equal.values()) or dev.status() != 0:
        out["status_after"] = dev.status()
        print(json.dumps(out))
        raise SystemExit("the answers differ: no time is reported")

    calls = {
        "a_nearest_k1_unfiltered": lambda: dev.nearest_k_device(B, d_p, 1, want=want),
        "a_nearest_k1_empty_filter": lambda: p3d.nearest_k_filtered_device(dev, B, d_p, 1, skip=nothing, skip_range=no_range, want=want),
        "a_sweep_unfiltered": lambda: p3d.sweep_sphere_device(dev, B, d_o, d_d, d_r, t_max=d_lim, want=("t", "centre", "contact")),
        "a_sweep_empty_filter": lambda: p3d.sweep_sphere_filtered_device(dev, B, d_o, d_d, d_r, t_max=d_lim, skip=nothing, skip_range=no_range, want=("t", "centre", "contact")),
        "b_vertices_k1_skip_own": lambda: p3d.nearest_k_filtered_device(dev, B, d_v, 1, skip=d_own, want=want),
        "b_vertices_k2_workaround": lambda: dev.nearest_k_device(B, d_v, 2, want=want),
        "c_vertices_sweep_skip_own": lambda: p3d.sweep_sphere_filtered_device(dev, B, d_v, d_vd, d_vr, t_max=d_vlim, skip=d_own, want=("t", "centre", "contact")),
        "c_vertices_sweep_unfiltered": lambda: p3d.sweep_sphere_device(dev, B, d_v, d_vd, d_vr, t_max=d_vlim, want=("t", "centre", "contact")),
    }
    out.update(timed_in_turn(calls, repeats, warmup))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_walk", "filtered_query_probe.json"))
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, tri100k=probe(tri, args.points, args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
