#!/usr/bin/env python3
"""What a batch of nearest-surface queries (p3d_nearest_device) costs on the 100k-triangle scene (scenes/make_tri100k.py)
with a tree built on the device: the BVH traversal against the brute force (P3D_ACCEL_NONE), with and without a limit of 1 %
of the scene's diagonal, and one deformation step - refit, then ask - on one stream against the waiting forms.

    python profiles/tools/nearest_probe.py [--out profiles/nearest/nearest.json] [--points 1048576] [--repeats 20] [--warmup 3]
                                           [--none-repeats 5] [--none-warmup 1]

The points are uniform in the scene's bounding box.  The brute force visits 100 000 objects per point, so it gets fewer
repeats.  Timing: a pair of events around the call on the current stream (GPU time of what the call enqueues) and a host
clock around call + synchronize; the waiting refit waits by itself, so the step is compared by the host clock.
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


def probe(path, n, repeats, warmup, none_repeats, none_warmup):
    hs = p3d.HostScene(path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    diag = float(np.linalg.norm(hi - lo))
    rng = np.random.default_rng(1)
    d_p = torch.from_numpy(rng.uniform(lo, hi, (n, 3)).astype(np.float32)).cuda()
    d_lim = torch.full((n,), np.float32(0.01 * diag), dtype=torch.float32, device="cuda")
    outs = {"object": torch.empty(n, dtype=torch.int32, device="cuda"), "dist": torch.empty(n, dtype=torch.float32, device="cuda"),
            "closest": torch.empty((n, 3), dtype=torch.float32, device="cuda")}
    want = ("dist", "closest")
    out = dict(points=n, n_objects=int(a["n_prims"]), bvh_max_depth=int(dev.export_bvh()["bvh_max_depth"]), diagonal=diag, limit=0.01 * diag)
    answers = {}
    for accel_name, accel, r, w in (("bvh", p3d.ACCEL_BVH, repeats, warmup), ("none", p3d.ACCEL_NONE, none_repeats, none_warmup)):
        for label, lim in (("no_limit", None), ("limit_1_percent", d_lim)):
            out["%s_%s" % (accel_name, label)] = timed_device(lambda: dev.nearest_device(accel, d_p, max_dist=lim, want=want, out=outs), r, w)
            answers[accel_name, label] = {k: v.cpu().numpy().tobytes() for k, v in outs.items()}
            if accel_name == "bvh":
                out["found_" + label] = int((outs["object"] >= 0).sum())
    out["bvh_equals_none_bit_for_bit"] = all(answers["bvh", label] == answers["none", label] for label in ("no_limit", "limit_1_percent"))

    # one step of a deforming mesh: new positions, refit, ask - on one stream without a host wait, and with the waiting refit
    base = torch.from_numpy(a["prim_v"].reshape(-1, 3)).cuda()
    soups = [(base + np.float32(0.002 * diag) * torch.sin(base * (3.0 + k))).contiguous() for k in range(4)]
    side = torch.cuda.Stream()
    state = {"k": 0}

    def on_stream():
        state["k"] += 1
        with torch.cuda.stream(side):
            dev.refit_triangles(0, soups[state["k"] % 4], stream=side)
            dev.nearest_device(p3d.ACCEL_BVH, d_p, max_dist=d_lim, want=want, stream=side, out=outs)
        side.synchronize()

    def waiting():
        state["k"] += 1
        dev.update_triangles(0, soups[state["k"] % 4], mode=p3d.UPDATE_REFIT)
        dev.nearest_device(p3d.ACCEL_BVH, d_p, max_dist=d_lim, want=want, out=outs)
        torch.cuda.synchronize()

    for name, step in (("step_on_one_stream", on_stream), ("step_with_the_waiting_refit", waiting)):
        wall = []
        for i in range(warmup + repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            if i >= warmup:
                wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(wall_ms=spread(wall))
    out["status_after"] = dev.status()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest", "nearest.json"))
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--none-repeats", type=int, default=5)
    ap.add_argument("--none-warmup", type=int, default=1)
    args = ap.parse_args()
    tri = os.path.join(tempfile.mkdtemp(), "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup, none_repeats=args.none_repeats,
               none_warmup=args.none_warmup, tri100k=probe(tri, args.points, args.repeats, args.warmup, args.none_repeats, args.none_warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
