#!/usr/bin/env python3
"""What the device-built uniform grid costs: p3d_scene_build_grid and p3d_scene_update_prims (REFIT, a third of the objects
moved) on a scene that has one, against the path there was before it for a scene rendered with accel = UGrid:
HostScene.set_geometry + desc(grid=True) (Grid::Build on the host) + a new DeviceScene(hs, bvh="device", grid=True).

    python profiles/tools/device_grid_probe.py [--out profiles/device_grid/device_grid.json] [--repeats 20] [--warmup 3]

Scenes: the 100k-triangle soup (scenes/make_tri100k.py: 125 cells with lists of about a thousand) and
tests/golden/scenes/path_glass.p3f (24 010 cells with short lists).  build_ms / update_ms are the library's own GPU times
(events around the launches; the read-backs between them are inside).  Wall-clock is taken with a host clock around the calls
named; every device call in them waits on both sides.  For the update paths the host scene's set_geometry is inside the
timed part of the old path (it cannot build its grid without it) and, for comparison, reported for the new path too.
Reported: median, min, max.
"""
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
import torch  # noqa: E402,F401  (initialised before the library's first HIP call)

import make_tri100k  # noqa: E402
import p3d_amd as p3d  # noqa: E402
from scene_update_helpers import random_moves  # noqa: E402


def spread(xs):
    return dict(median=float(np.median(xs)), min=float(np.min(xs)), max=float(np.max(xs)), n=len(xs))


def probe(path, repeats, warmup):
    hs = p3d.HostScene(path)
    hs.set_resolution(64, 64)
    a = hs.arrays(grid=True)
    out = dict(n_objects=int(a["n_prims"]), grid_n=list(a["grid_n"]), n_items=int(len(a["grid_cell_items"])))
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    build_ms, build_wall = [], []
    for i in range(warmup + repeats):
        t0 = time.perf_counter()
        ms = dev.build_grid()
        wall = (time.perf_counter() - t0) * 1e3
        if i >= warmup:
            build_ms.append(ms)
            build_wall.append(wall)
    out["build_grid"] = dict(build_ms=spread(build_ms), wall_ms=spread(build_wall))
    # the same updates on a scene without a grid: what the BVH work alone costs (created from a host scene of its own - this
    # one's descriptor carries the host's grid by now -, then fed this one's records)
    no_grid = p3d.DeviceScene(p3d.HostScene(path), bvh="device")
    no_grid.host = hs
    upd_ms, upd_wall, upd_total, bvh_only_ms, old_wall = [], [], [], [], []
    for i in range(warmup + repeats):
        objs, new_v = random_moves(hs.arrays(), 1000 + i)
        # the new path: move the host scene, hand the records to the live scene
        t0 = time.perf_counter()
        hs.set_geometry(objs, new_v)
        t1 = time.perf_counter()
        ms = dev.update_prims(objs, p3d.UPDATE_REFIT)
        t2 = time.perf_counter()
        ms_bvh = no_grid.update_prims(objs, p3d.UPDATE_REFIT)
        # the old path for the next move: a new scene with the host's grid
        objs2, new_v2 = random_moves(hs.arrays(), 5000 + i)
        t3 = time.perf_counter()
        hs.set_geometry(objs2, new_v2)
        hs.desc(False, True)
        fresh = p3d.DeviceScene(hs, bvh="device", grid=True)
        t4 = time.perf_counter()
        fresh.close()
        dev.update_prims(objs2, p3d.UPDATE_REFIT)  # keep the live scenes in step with the host scene
        no_grid.update_prims(objs2, p3d.UPDATE_REFIT)
        if i >= warmup:
            upd_ms.append(ms)
            upd_wall.append((t2 - t1) * 1e3)
            upd_total.append((t2 - t0) * 1e3)
            bvh_only_ms.append(ms_bvh)
            old_wall.append((t4 - t3) * 1e3)
    want = hs.arrays(grid=True)
    got = dev.export_grid()
    assert all(got[k].tobytes() == want[k].tobytes() for k in ("grid_bmin", "grid_bmax", "grid_cell_start", "grid_cell_items"))
    out["update_refit_third"] = dict(update_ms=spread(upd_ms), update_ms_scene_without_grid=spread(bvh_only_ms),
                                     wall_ms_update_call=spread(upd_wall), wall_ms_with_set_geometry=spread(upd_total))
    out["old_path_set_geometry_host_grid_new_scene"] = dict(wall_ms=spread(old_wall))
    for s in (dev, no_grid):
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_grid", "device_grid.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    tri = os.path.join(tmp, "tri100k.p3f")
    make_tri100k.generate(tri)
    res = dict(device=torch.cuda.get_device_name(0), repeats=args.repeats, warmup=args.warmup,
               tri100k=probe(tri, args.repeats, args.warmup),
               path_glass=probe(os.path.join(ROOT, "tests", "golden", "scenes", "path_glass.p3f"), args.repeats, args.warmup))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
