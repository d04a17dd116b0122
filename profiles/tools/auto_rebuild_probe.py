#!/usr/bin/env python3
"""When a refitted tree should be rebuilt: the SAH cost of the tree (p3d_scene_bvh_cost) against what it predicts, the time of
the next frames, and what the policy of p3d_scene_set_auto_rebuild costs an update.

    python profiles/tools/auto_rebuild_probe.py [--out profiles/scene_update/auto_rebuild.json] [--parent-root DIR]

Scenes and seeds are those of scene_update_probe.py: the 100k-triangle soup and balls_low, a random tenth of the objects
moved (seed 21).  Per scene and displacement (0.1, 0.3, 1, 3 and 10 % of the scene diagonal):
  sah_build, sah_refit, sah_rebuild   the cost of the tree at create, after the REFIT, after a REBUILD of the moved scene
  frame_ms_after_refit / _rebuild     kernel time of `res`^2 Whitted depth-4 frames, as scene_update_probe.py takes it
  update_ms                           the library's GPU time of the update from the rest pose to the moved one, `updates` times
                                      each (an untimed REBUILD back at the rest pose before every timed call): REFIT, REBUILD,
                                      and REFIT with the policy on at `ratio`, with how many of those were promoted
`ratio` is --ratio, or else the recommendation: the sah ratio of the first displacement of the 100k scene at which
(frame after refit - frame after rebuild) exceeds (REBUILD update_ms - REFIT update_ms), rounded down to two digits.
--parent-root: a checkout of the commit before these entry points, with its library built.  A child process measures the
same REFIT and REBUILD calls there (`parent_update_ms`), in the same run: what the bookkeeping costs a caller with the policy off.
"""
import argparse
import ctypes as C
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.abspath(__file__)
LADDER = (0.001, 0.003, 0.01, 0.03, 0.1)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(HERE))), help="the checkout whose package is measured")
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--res", type=int, default=2048)
    ap.add_argument("--triangles", type=int, default=100000)
    ap.add_argument("--ratio", type=float, default=0.0)
    ap.add_argument("--updates-only", action="store_true", help="REFIT and REBUILD update_ms alone (what a parent checkout can do)")
    ap.add_argument("--scene-file", default=None, help="the generated triangle scene, if the caller has one")
    return ap.parse_args()


args = parse()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, "scenes"))
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))
import torch  # noqa: E402  (initialised before the library's first HIP call)

import p3d_amd as p3d  # noqa: E402
from scene_update_probe import frame_ms, move, records, spread  # noqa: E402


def update(L, dev, objs, recs, mode):
    ms = C.c_float(0)
    if L.p3d_scene_update_prims(dev._h, len(objs), objs.ctypes.data, recs.ctypes.data, mode, C.byref(ms)):
        raise RuntimeError(L.p3d_last_error().decode())
    return ms.value


def timed(L, dev, objs, rest, moved, mode, n):
    """update_ms of n updates from the rest pose (rebuilt there, untimed) to the moved one"""
    out, promoted = [], 0
    for i in range(n + 2):
        update(L, dev, objs, rest, p3d.UPDATE_REBUILD)
        ms = update(L, dev, objs, moved, mode)
        if i >= 2:
            out.append(ms)
            if hasattr(dev, "bvh_cost") and mode == p3d.UPDATE_REFIT:
                promoted += dev.bvh_cost()["last_update_rebuilt"]
    return out, promoted


def step(L, path, reach, ratio):
    hs = p3d.HostScene(path)
    hs.set_resolution(args.res, args.res)
    dev = p3d.DeviceScene(hs, bvh="device")
    out = dict(displacement=reach)
    full = not args.updates_only
    if full:
        out["sah_build"] = dev.bvh_cost()["sah"]
    rng = np.random.default_rng(21)
    objs = move(hs, rng, 0.1, 0.0)  # (the choice of objects comes first in the stream: reach 0 picks the same ones)
    rest = records(hs, objs)
    objs2 = move(hs, np.random.default_rng(21), 0.1, reach)
    assert np.array_equal(objs, objs2)
    moved = records(hs, objs)
    if full:
        cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
        buf = torch.empty((args.res, args.res, 3), dtype=torch.float32, device="cuda")
        update(L, dev, objs, moved, p3d.UPDATE_REFIT)
        out["sah_refit"] = dev.bvh_cost()["sah"]
        out["frame_ms_after_refit"] = frame_ms(dev, cfg, buf, args.frames)
        update(L, dev, objs[:0], moved[:0], p3d.UPDATE_REBUILD)
        out["sah_rebuild"] = dev.bvh_cost()["sah"]
        out["frame_ms_after_rebuild"] = frame_ms(dev, cfg, buf, args.frames)
        out["sah_refit_over_build"] = out["sah_refit"] / out["sah_build"]
    ms = {}
    ms["refit"] = spread(timed(L, dev, objs, rest, moved, p3d.UPDATE_REFIT, args.updates)[0])
    ms["rebuild"] = spread(timed(L, dev, objs, rest, moved, p3d.UPDATE_REBUILD, args.updates)[0])
    if full and ratio:
        dev.set_auto_rebuild(ratio)
        got, promoted = timed(L, dev, objs, rest, moved, p3d.UPDATE_REFIT, args.updates)
        ms["refit_policy_on"] = dict(spread(got), promoted=int(promoted), ratio=ratio)
        ms["rebuild_policy_on"] = spread(timed(L, dev, objs, rest, moved, p3d.UPDATE_REBUILD, args.updates)[0])
    out["update_ms"] = ms
    dev.close()
    return out


def recommend(steps):
    """The sah ratio of the first step from which a rebuild pays for itself within one frame, rounded down to two digits"""
    for s in steps:
        gain = s["frame_ms_after_refit"]["median"] - s["frame_ms_after_rebuild"]["median"]
        price = s["update_ms"]["rebuild"]["median"] - s["update_ms"]["refit"]["median"]
        if gain > price:
            return math.floor(s["sah_refit_over_build"] * 100) / 100
    return None


def main():
    if not torch.cuda.is_available():
        sys.exit("auto_rebuild_probe: no GPU; nothing here can be measured without one")
    torch.cuda.init()
    L = p3d.lib()
    tri = args.scene_file
    if not tri:
        import make_tri100k
        tri = os.path.join(tempfile.mkdtemp(), "tri.p3f")
        make_tri100k.generate(tri, n=args.triangles)
    scenes = (("tri%dk" % (args.triangles // 1000), tri), ("balls_low", os.path.join(args.root, "tests", "golden", "scenes", "balls_low.p3f")))
    if args.updates_only:
        result = {name: [step(L, path, reach, 0.0) for reach in LADDER] for name, path in scenes}
        with open(args.out, "w") as f:
            json.dump(result, f)
        return
    result = dict(device=torch.cuda.get_device_name(0), updates=args.updates, res=args.res, scenes={})
    ratio = args.ratio
    for name, path in scenes:
        steps = [step(L, path, reach, 0.0) for reach in LADDER]
        if name.startswith("tri"):
            result["recommended_ratio"] = recommend(steps)
            ratio = ratio or max(1.0, result["recommended_ratio"] or 0.0)  # (a ratio below 1 cannot be set; none found: 1)
        if ratio:  # the policy's share, now that the ratio is known
            for s, reach in zip(steps, LADDER):
                again = step(L, path, reach, ratio)["update_ms"]
                s["update_ms"]["refit_policy_on"], s["update_ms"]["rebuild_policy_on"] = again["refit_policy_on"], again["rebuild_policy_on"]
                s["update_ms"]["refit_second_run"], s["update_ms"]["rebuild_second_run"] = again["refit"], again["rebuild"]
        result["scenes"][name] = steps
        print(name, json.dumps(steps), flush=True)
    result["policy_ratio"] = ratio
    if args.parent_root:
        env = dict(os.environ)
        env.pop("P3D_LIB", None)
        side = os.path.join(tempfile.mkdtemp(), "parent.json")
        subprocess.run([sys.executable, HERE, "--root", args.parent_root, "--updates-only", "--updates", str(args.updates), "--res", str(args.res),
                        "--triangles", str(args.triangles), "--scene-file", tri, "--out", side], env=env, check=True, timeout=600)
        parent = json.load(open(side))
        for name, steps in parent.items():
            for s, p in zip(result["scenes"][name], steps):
                s["parent_update_ms"] = p["update_ms"]
    out = args.out or os.path.join(args.root, "profiles", "scene_update", "auto_rebuild.json")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
