"""What the tests of a live scene share (object updates, transforms, geometry from device memory, the stream refit and the stream
pose): their scenes and seeds, deterministic moves, the frame configurations a scene is compared in, and the comparison of
a scene with its twin.

A helper module: test modules import helper and reference modules only, never one another ("Layout of tests/")."""
import os

import numpy as np
import torch

import p3d_amd as p3d
from frame_checks import assert_same_frames, assert_same_grid, assert_same_tree, frames, gpu
from scene_update_helpers import BOX, PLANE, SPHERE, TRIANGLE

RES = 96
SCENES = ["balls_low", "tri5k", "balls_box", "cornell"]
GRID_SCENES = ("balls_low", "tri5k")
SEED = {"balls_low": 31, "tri5k": 32, "balls_box": 33, "cornell": 34}
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
LEAF = np.uint32(0x80000000)
TRACE_OUT = (("hit_id", torch.int32, None), ("t", torch.float32, None), ("hit_point", torch.float32, 3), ("normal", torch.float32, 3))
HEAD = ["bclr 0.1 0.2 0.3", "v", "from 0 -6 1", "at 0 0 0", "up 0 0 1", "angle 40", "hither 0.01", "resolution 64 64",
        "aperture 0", "focal 1", "l 3 -4 5 1 1 1", "f 0.8 0.3 0.3 0.7 1 1 1 0.3 20 0 1 0 0 0"]


def legacy(path):
    """balls_box.p3f, alone among these scenes, has 11-number `f` lines (HostScene's legacy_f11)"""
    return os.path.basename(path) == "balls_box.p3f"


def device(hs, name):
    return p3d.DeviceScene(hs, bvh="device", grid="device" if name in GRID_SCENES else False)


def runs(kinds, wanted):
    """Maximal runs of consecutive objects whose kind is in `wanted` -> [(first, count)]"""
    out, start = [], None
    for i, k in enumerate(list(kinds) + [None]):
        if k in wanted and start is None:
            start = i
        elif k not in wanted and start is not None:
            out.append((start, i - start))
            start = None
    return out


def rotation(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def rigid(a, rng, reach=0.05):
    """A seeded rotation about the centre of the non-plane objects plus a translation of `reach` x their diagonal -> (3, 4) float32"""
    movable = a["prim_type"] != PLANE
    lo = a["prim_bmin"][movable].min(0).astype(np.float64)
    hi = a["prim_bmax"][movable].max(0).astype(np.float64)
    centre = (lo + hi) / 2
    rot = rotation(rng)
    d = rng.standard_normal(3)
    d *= reach * np.linalg.norm(hi - lo) / np.linalg.norm(d)
    m = np.zeros((3, 4))
    m[:, :3] = rot
    m[:, 3] = centre - rot @ centre + d
    return m.astype(np.float32)


def box_move(a, rng):
    """A positive scale per axis and a translation: what a box takes"""
    m = np.zeros((3, 4), np.float32)
    m[:, :3] = np.diag(rng.uniform(0.7, 1.3, 3)).astype(np.float32)
    m[:, 3] = rng.uniform(-0.1, 0.1, 3).astype(np.float32)
    return m


def plan(a, seed):
    """Every sphere and triangle under one rigid move with sphere_scale 1.25, boxes in ranges of their own under a
    positive-diagonal one -> (ranges, xforms, sphere_scale)"""
    rng = np.random.default_rng(seed)
    xforms = np.stack([rigid(a, rng), box_move(a, rng)])
    ranges = [(f, c, 0) for f, c in runs(a["prim_type"], (SPHERE, TRIANGLE))] + [(f, c, 1) for f, c in runs(a["prim_type"], (BOX,))]
    return ranges, xforms, np.array([1.25, 1.0], np.float32)


def configs(name, accel=p3d.ACCEL_BVH):
    """(label, cfg): Whitted depth 4 in both stack modes, or the 4-spp path-traced frame of cornell"""
    if name == "cornell":
        return [("path trace 4 spp", p3d.pathtrace_config(accel=accel, spp_sqrt=2, max_depth=8, seed=3, collect_stats=1))]
    return [("whitted %s" % label, p3d.whitted_config(accel=accel, max_depth=4, stack_mode=mode, collect_stats=1))
            for label, mode in (("literal", p3d.STACK_LITERAL), ("per pixel", p3d.STACK_PER_PIXEL))]


def assert_same_scene(dev_a, dev_b, name, what):
    """Frames and trees, and for the scenes with a device grid the grids and one grid frame -> dev_b's BVH frames"""
    now = frames(dev_b, configs(name))
    assert_same_frames(frames(dev_a, configs(name)), now, what)
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), what)
    if name in GRID_SCENES:
        assert_same_grid(dev_a.export_grid(), dev_b.export_grid(), what)
        assert_same_frames(frames(dev_a, configs(name, p3d.ACCEL_GRID))[:1], frames(dev_b, configs(name, p3d.ACCEL_GRID))[:1], what + ", grid frame")
    return now


def host_route(hs, dev, rest, ranges, xforms, scale, mode):
    """What there was before: the transform in numpy from the REST geometry, the constructors on the host, 112 bytes per object"""
    objs, new_v = p3d.transformed(rest["prim_type"], rest["prim_v"], ranges, xforms, scale)
    hs.set_geometry(objs, new_v)
    return dev.update_prims(objs, mode)


def scene(hs):
    return p3d.DeviceScene(hs, bvh="device")


def assert_same_frames_and_tree(dev_a, dev_b, name, what):
    """assert_same_scene for scenes without a grid -> B's frames"""
    now = frames(dev_b, configs(name))
    assert_same_frames(frames(dev_a, configs(name)), now, what)
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), what)
    return now


def last_error():
    return p3d.lib().p3d_last_error().decode()


def produced(base, amount, rounds=50):
    """base + amount * a smooth field of it, by a chain of torch operations on the current stream"""
    wave = base
    for _ in range(rounds):
        wave = torch.sin(wave * 1.5 + 0.25)
    return (base + amount * wave).contiguous()


def kinds_of(a):
    tri, sph = np.nonzero(a["prim_type"] == TRIANGLE)[0], np.nonzero(a["prim_type"] == SPHERE)[0]
    for run in (tri, sph):
        assert len(run) == 0 or np.array_equal(run, np.arange(run[0], run[0] + len(run)))
    return tri, sph


def camera_rays(a, n, seed):
    lo, hi = a["prim_bmin"].min(0).astype(np.float64), a["prim_bmax"].max(0).astype(np.float64)
    rng = np.random.default_rng(seed)
    o = np.tile((lo + hi) / 2 + (hi - lo) * np.array([1.1, 0.9, 1.3]), (n, 1))
    d = rng.uniform(lo, hi, (n, 3)) - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return gpu(o.astype(np.float32)), gpu(d.astype(np.float32))


def trace_outputs(n):
    return {name: torch.zeros((n,) if cols is None else (n, cols), dtype=dtype, device="cuda") for name, dtype, cols in TRACE_OUT}
