#!/usr/bin/env python3
"""What a caller pays to turn the objects of a live scene: p3d_scene_transform_prims (64 bytes per transform, the arithmetic on
the device) against the route there was before it, in the same process: the transform in numpy (p3d.transformed),
p3d_host_scene_set_geometry, the re-flattened descriptor (HostScene.arrays' source, p3d_host_scene_desc) and
p3d_scene_update_prims with one 112-byte record per object, each part timed.

    python profiles/tools/scene_transform_probe.py [--out profiles/scene_update/scene_transform.json] [--updates 20]

Scenes: the 100k-triangle soup (scenes/make_tri100k.py) and tests/golden/scenes/balls_low.p3f.  Per scene, mode and route:
`updates` timed calls after `warmup` untimed ones, each rotating ALL non-plane objects by one matrix about the scene centre (a
new angle per call, always from the rest pose).  Host wall-clock around each part; update_ms is the library's own GPU time
(events around the staging copy and the launches).  Reported: median, min, max.
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

PLANE = 3


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def prim_table(hs):
    """The host scene's current p3d_prim records as an (n, 24) uint32 view (v 0-8, type 9): asking for it re-flattens"""
    d = hs.desc(False, False)
    return np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint32)), shape=(d.n_prims, C.sizeof(p3d.Prim) // 4))


def runs(kinds):
    out, start = [], None
    for i, k in enumerate(list(kinds) + [PLANE]):
        if k != PLANE and start is None:
            start = i
        elif k == PLANE and start is not None:
            out.append((start, i - start, 0))
            start = None
    return out


def turn(centre, angle):
    """Rotation by `angle` about the y axis through `centre` -> (1, 3, 4) float32"""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    m = np.zeros((3, 4))
    m[:, :3] = rot
    m[:, 3] = centre - rot @ centre
    return m.astype(np.float32)[None]


def timed(hs, dev, mode, route, rest_type, rest_v, ranges, centre, warmup, updates):
    L = p3d.lib()
    parts = dict(numpy_ms=[], set_geometry_ms=[], flatten_ms=[], call_wall_ms=[], update_ms=[], total_wall_ms=[])
    for i in range(warmup + updates):
        m = turn(centre, 0.01 * (i + 1))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if route == "device":
            t3 = t0
            ms = dev.transform_prims(ranges, m, mode)
            t4 = time.perf_counter()
            row = dict(call_wall_ms=t4 - t3, update_ms=ms / 1e3, total_wall_ms=t4 - t0)
        else:
            objs, new_v = p3d.transformed(rest_type, rest_v, ranges, m)
            t1 = time.perf_counter()
            hs.set_geometry(objs, new_v)
            t2 = time.perf_counter()
            recs = np.ascontiguousarray(prim_table(hs)[objs])
            t3 = time.perf_counter()
            gpu = C.c_float(0)
            if L.p3d_scene_update_prims(dev._h, len(objs), objs.ctypes.data, recs.ctypes.data, mode, C.byref(gpu)):
                raise RuntimeError(L.p3d_last_error().decode())
            t4 = time.perf_counter()
            row = dict(numpy_ms=t1 - t0, set_geometry_ms=t2 - t1, flatten_ms=t3 - t2, call_wall_ms=t4 - t3, update_ms=gpu.value / 1e3,
                       total_wall_ms=t4 - t0)
        if i >= warmup:
            for k, v in row.items():
                parts[k].append(v * 1e3)
    return {k: spread(v) for k, v in parts.items() if v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update", "scene_transform.json"))
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--triangles", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_transform_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    tmp = tempfile.mkdtemp()
    tri = os.path.join(tmp, "tri.p3f")
    make_tri100k.generate(tri, n=args.triangles)
    result = dict(device=torch.cuda.get_device_name(0), updates=args.updates, warmup=args.warmup, scenes={})
    for name, path in (("tri%dk" % (args.triangles // 1000), tri), ("balls_low", os.path.join(ROOT, "tests", "golden", "scenes", "balls_low.p3f"))):
        hs = p3d.HostScene(path)
        hs.set_resolution(args.res, args.res)
        t = prim_table(hs).copy()
        rest_type, rest_v = t[:, 9].copy(), t[:, 0:9].copy().view(np.float32)
        movable = rest_type != PLANE
        lo = t[movable, 16:19].copy().view(np.float32).min(0).astype(np.float64)
        hi = t[movable, 20:23].copy().view(np.float32).max(0).astype(np.float64)
        ranges = runs(rest_type)
        covered = int(sum(c for _, c, _ in ranges))
        entry = dict(objects=int(len(rest_type)), objects_moved=covered, ranges=len(ranges),
                     upload_bytes=dict(device_route=64 + 16 * len(ranges), host_route=112 * covered))
        for mode, label in ((p3d.UPDATE_REFIT, "refit"), (p3d.UPDATE_REBUILD, "rebuild")):
            for route in ("host", "device"):
                dev = p3d.DeviceScene(hs, bvh="device")
                entry["%s_%s_route" % (label, route)] = timed(hs, dev, mode, route, rest_type, rest_v, ranges, (lo + hi) / 2, args.warmup,
                                                              args.updates)
                dev.close()
                hs.set_geometry(np.nonzero(movable)[0].astype(np.uint32), rest_v[movable])  # back to the rest pose
        result["scenes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
