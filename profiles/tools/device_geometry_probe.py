#!/usr/bin/env python3
"""What a caller pays to deform a mesh that lives on the GPU: p3d_scene_update_geometry_device (the positions stay where they
are, one kernel gathers them) against the route there was before it, in the same process: the positions copied device ->
host, p3d_host_scene_set_geometry, the re-flattened descriptor and p3d_scene_update_prims with one 112-byte record per
object, each part timed.

    python profiles/tools/device_geometry_probe.py [--out profiles/scene_update/device_geometry.json] [--updates 20]

Scene: the 100k-triangle soup (scenes/make_tri100k.py).  Per mode (refit, rebuild) and form (soup, indexed; host): `updates`
timed calls after `warmup` untimed ones.  Every call sees new positions: a wave over the mesh, computed by torch on the
device before the clock starts.  Host wall-clock around each part; update_ms is the library's own GPU time (events around the
staging copy and the launches).  Reported: median, min, max.
"""
import argparse
import ctypes as C
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


def prim_table(hs):
    """The host scene's current p3d_prim records as an (n, 24) uint32 view (v 0-8, type 9): asking for it re-flattens"""
    d = hs.desc(False, False)
    return np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint32)), shape=(d.n_prims, C.sizeof(p3d.Prim) // 4))


def timed(hs, dev, mode, form, rest, index, amplitude, warmup, updates):
    """rest: (V, 3) float32 on the device; index: (F, 3) int32 on the device, or None for a soup (V = 3 F)"""
    L = p3d.lib()
    n = len(index) if index is not None else len(rest) // 3
    objs = np.arange(n, dtype=np.uint32)
    parts = dict(copy_to_host_ms=[], set_geometry_ms=[], flatten_ms=[], call_wall_ms=[], update_ms=[], total_wall_ms=[])
    for i in range(warmup + updates):
        pos = (rest + amplitude * torch.sin(4.0 * rest.roll(1, 1) + 0.3 * (i + 1))).contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if form != "host":
            ms = dev.update_triangles(0, pos, index, mode=mode)
            t4 = time.perf_counter()
            row = dict(call_wall_ms=t4 - t0, update_ms=ms / 1e3, total_wall_ms=t4 - t0)
        else:
            host = pos.cpu().numpy()
            t1 = time.perf_counter()
            hs.set_geometry(objs, host.reshape(-1, 9))
            t2 = time.perf_counter()
            recs = np.ascontiguousarray(prim_table(hs)[objs])
            t3 = time.perf_counter()
            gpu = C.c_float(0)
            if L.p3d_scene_update_prims(dev._h, len(objs), objs.ctypes.data, recs.ctypes.data, mode, C.byref(gpu)):
                raise RuntimeError(L.p3d_last_error().decode())
            t4 = time.perf_counter()
            row = dict(copy_to_host_ms=t1 - t0, set_geometry_ms=t2 - t1, flatten_ms=t3 - t2, call_wall_ms=t4 - t3, update_ms=gpu.value / 1e3,
                       total_wall_ms=t4 - t0)
        if i >= warmup:
            for k, v in row.items():
                parts[k].append(v * 1e3)
    return {k: spread(v) for k, v in parts.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update", "device_geometry.json"))
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("device_geometry_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    tmp = tempfile.mkdtemp()
    tri = os.path.join(tmp, "tri.p3f")
    make_tri100k.generate(tri, n=args.triangles)
    hs = p3d.HostScene(tri)
    hs.set_resolution(args.res, args.res)
    t = prim_table(hs).copy()
    rest_v = t[:, 0:9].copy().view(np.float32)
    n = len(rest_v)
    lo = t[:, 16:19].copy().view(np.float32).min(0).astype(np.float64)
    hi = t[:, 20:23].copy().view(np.float32).max(0).astype(np.float64)
    amplitude = 0.01 * float(np.linalg.norm(hi - lo))
    soup = torch.from_numpy(rest_v.reshape(-1, 3)).cuda()
    # the indexed form of the same mesh: positions in shuffled order, so that the gather is one
    order = np.random.default_rng(1).permutation(3 * n)
    shuffled = torch.from_numpy(np.ascontiguousarray(rest_v.reshape(-1, 3)[order])).cuda()
    index = torch.from_numpy(np.argsort(order).astype(np.int32).reshape(-1, 3)).cuda()
    result = dict(device=torch.cuda.get_device_name(0), updates=args.updates, warmup=args.warmup, objects=n,
                  bytes_per_object=dict(read_soup=36, read_indexed=72, written=112, host_route_upload=112))
    for mode, label in ((p3d.UPDATE_REFIT, "refit"), (p3d.UPDATE_REBUILD, "rebuild")):
        for form, rest, idx in (("soup", soup, None), ("indexed", shuffled, index), ("host", soup, None)):
            dev = p3d.DeviceScene(hs, bvh="device")
            result["%s_%s" % (label, form)] = timed(hs, dev, mode, form, rest, idx, amplitude, args.warmup, args.updates)
            dev.close()
            hs.set_geometry(np.arange(n, dtype=np.uint32), rest_v)  # back to the rest pose
            print(label, form, json.dumps(result["%s_%s" % (label, form)]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
