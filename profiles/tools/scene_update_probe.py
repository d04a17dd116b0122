#!/usr/bin/env python3
"""What a caller pays to move objects of a live scene: p3d_scene_update_prims (refit / rebuild) against the only path there
was before it, p3d_scene_destroy + p3d_scene_create_device_bvh of the updated descriptor.

    python profiles/tools/scene_update_probe.py [--out profiles/scene_update/scene_update.json] [--updates 20] [--res 2048]

Scenes: the 100k-triangle soup (scenes/make_tri100k.py) and tests/golden/scenes/balls_low.p3f.  Per scene and path: `updates`
timed calls after `warmup` untimed ones, each moving a random tenth of the objects by 1 % of the scene diagonal.  Host
wall-clock is taken around the C call(s) alone - every one of them waits for the device before it starts and before it
returns, so both sides are synchronised - with the host scene already moved and its descriptor flattened (all three paths
need that; it is reported once as host_prepare_ms).  update_ms is the library's own GPU time (events around staging copy and
launches).  Reported: median, min, max.

Then, per scene: the kernel time of the next `res`^2 Whitted depth-4 frames after a REFIT that moved a tenth of the objects by
0.1 %, 1 % and 10 % of the diagonal, against the same frames after a REBUILD of the same scene: when refitting stops paying.
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
    """The host scene's current p3d_prim records as an (n, 24) uint32 view (v 0-8, type 9, bmin 16-18, bmax 20-22)"""
    d = hs.desc(False, False)
    return np.ctypeslib.as_array(C.cast(d.prims, C.POINTER(C.c_uint32)), shape=(d.n_prims, C.sizeof(p3d.Prim) // 4))


def move(hs, rng, fraction, reach):
    """Moves a random `fraction` of the non-plane objects of the host scene by `reach` x the scene diagonal -> their indices"""
    t = prim_table(hs)
    kinds = t[:, 9]
    movable = np.nonzero(kinds != PLANE)[0]
    lo = t[movable, 16:19].copy().view(np.float32).min(0).astype(np.float64)
    hi = t[movable, 20:23].copy().view(np.float32).max(0).astype(np.float64)
    objs = np.sort(rng.choice(movable, max(1, int(len(movable) * fraction)), replace=False))
    d = rng.standard_normal((len(objs), 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True) * reach * np.linalg.norm(hi - lo)).astype(np.float32)
    v = t[objs, 0:9].copy().view(np.float32)
    kind = kinds[objs]
    for cols, k in (((0,), 0), ((0, 3, 6), 1), ((0, 3), 2)):
        for c in cols:
            v[kind == k, c:c + 3] += d[kind == k]
    hs.set_geometry(objs, v)
    return objs.astype(np.uint32)


def records(hs, objs):
    """The p3d_prim records of `objs` from the host scene's current descriptor, as one contiguous buffer"""
    return np.ascontiguousarray(prim_table(hs)[objs])


def timed_updates(L, hs, scene_h, rng, mode, warmup, updates):
    wall, gpu, prep = [], [], []
    for i in range(warmup + updates):
        t0 = time.perf_counter()
        objs = move(hs, rng, 0.1, 0.01)
        recs = records(hs, objs)
        t1 = time.perf_counter()
        ms = C.c_float(0)
        rc = L.p3d_scene_update_prims(scene_h, len(objs), objs.ctypes.data, recs.ctypes.data, mode, C.byref(ms))
        t2 = time.perf_counter()
        if rc:
            raise RuntimeError(L.p3d_last_error().decode())
        if i >= warmup:
            wall.append((t2 - t1) * 1e3)
            gpu.append(ms.value)
            prep.append((t1 - t0) * 1e3)
    return dict(wall_ms=spread(wall), update_ms=spread(gpu)), prep


def timed_recreate(L, hs, rng, warmup, updates):
    h = C.c_void_p()
    d = hs.desc(False, False)
    if L.p3d_scene_create_device_bvh(C.byref(d), 0, C.byref(h), None):
        raise RuntimeError(L.p3d_last_error().decode())
    wall, build = [], []
    for i in range(warmup + updates):
        move(hs, rng, 0.1, 0.01)
        d = hs.desc(False, False)
        torch.cuda.synchronize()
        ms = C.c_float(0)
        t1 = time.perf_counter()
        L.p3d_scene_destroy(h)
        h = C.c_void_p()
        rc = L.p3d_scene_create_device_bvh(C.byref(d), 0, C.byref(h), C.byref(ms))  # ends in host waits of its own
        t2 = time.perf_counter()
        if rc:
            raise RuntimeError(L.p3d_last_error().decode())
        if i >= warmup:
            wall.append((t2 - t1) * 1e3)
            build.append(ms.value)
    L.p3d_scene_destroy(h)
    return dict(wall_ms=spread(wall), build_ms=spread(build))


def frame_ms(dev, cfg, buf, frames):
    out = []
    for i in range(frames + 2):  # the first frame after an update records the tile costs, the second is the first scheduled one
        st = p3d.Stats()
        dev.render_device(cfg, dev.full_tile(), d_rgb=buf.data_ptr(), stats=st)
        if i >= 2:
            out.append(st.kernel_ms)
    return spread(out)


def frames_after(path, res, reach, frames, seed):
    hs = p3d.HostScene(path)
    hs.set_resolution(res, res)
    dev = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
    buf = torch.empty((res, res, 3), dtype=torch.float32, device="cuda")
    objs = move(hs, np.random.default_rng(seed), 0.1, reach)
    out = dict(displacement=reach, objects_moved=int(len(objs)))
    out["refit_update_ms"] = dev.update_prims(objs, p3d.UPDATE_REFIT)
    out["frame_ms_after_refit"] = frame_ms(dev, cfg, buf, frames)
    out["rebuild_update_ms"] = dev.update_prims([], p3d.UPDATE_REBUILD)
    out["frame_ms_after_rebuild"] = frame_ms(dev, cfg, buf, frames)
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_update", "scene_update.json"))
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=100000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scene_update_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    L = p3d.lib()
    tmp = tempfile.mkdtemp()
    tri = os.path.join(tmp, "tri.p3f")
    make_tri100k.generate(tri, n=args.triangles)
    result = dict(device=torch.cuda.get_device_name(0), updates=args.updates, warmup=args.warmup, res=args.res, scenes={})
    for name, path in (("tri%dk" % (args.triangles // 1000), tri), ("balls_low", os.path.join(ROOT, "tests", "golden", "scenes", "balls_low.p3f"))):
        rng = np.random.default_rng(7)
        hs = p3d.HostScene(path)
        hs.set_resolution(args.res, args.res)
        entry = dict(objects=int(hs.desc(False, False).n_prims))
        entry["recreate"] = timed_recreate(L, hs, rng, args.warmup, args.updates)
        dev = p3d.DeviceScene(hs, bvh="device")
        entry["refit"], prep = timed_updates(L, hs, dev._h, rng, p3d.UPDATE_REFIT, args.warmup, args.updates)
        entry["rebuild"], _ = timed_updates(L, hs, dev._h, rng, p3d.UPDATE_REBUILD, args.warmup, args.updates)
        entry["host_prepare_ms"] = spread(prep)
        dev.close()
        entry["next_frame"] = [frames_after(path, args.res, reach, args.frames, 21) for reach in (0.001, 0.01, 0.1)]
        result["scenes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
