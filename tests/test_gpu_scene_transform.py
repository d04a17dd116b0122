"""Transforms applied to a live scene's objects on the device (p3d_scene_transform_prims) on the GPU.

The yardstick is exact: the device route (ranges + matrices -> kernel -> BVH / grid work) must give, bit for bit, what the host
route gives for the same numbers (p3d.transformed -> HostScene.set_geometry -> update_prims): colours as uint32, hit IDs,
counters, the exported tree and the exported grid.  Every comparison here has tolerance 0."""
import ctypes as C

import numpy as np
import pytest

import p3d_amd as p3d
from conftest import scene_path
from scene_update_helpers import BOX, PLANE, SPHERE, TRIANGLE, random_moves
from frame_checks import CORNELL, PLANES, assert_same_frames, assert_same_tree, frames, frames_differ, load, rays
from live_scene_checks import (IDENTITY, RES, SCENES, SEED, assert_same_scene, configs, device, host_route, legacy, plan, rigid,
                               rotation, runs)

pytestmark = pytest.mark.gpu


@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "balls_box": scene_path("balls_box.p3f"), "cornell": CORNELL}


@pytest.mark.parametrize("name", SCENES)
def test_the_device_route_is_the_host_route(name, paths):
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    dev_a, dev_b = device(hs, name), device(hs, name)
    last = frames(dev_b, configs(name))
    for round_ in range(2):  # round two: A computes from the ORIGINAL prim_v, B from its rest copy - not from round one's result
        ranges, xforms, scale = plan(rest, SEED[name] + 100 * round_)
        assert host_route(hs, dev_a, rest, ranges, xforms, scale, p3d.UPDATE_REBUILD) > 0
        assert dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REBUILD, sphere_scale=scale) > 0
        now = assert_same_scene(dev_a, dev_b, name, "%s, round %d" % (name, round_))
        assert frames_differ(now, last), "the move changed no pixel"
        last = now
    assert dev_b.status() == 0


@pytest.mark.parametrize("name", SCENES)
def test_refit_keeps_the_topology_on_both_routes(name, paths):
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    dev_a, dev_b = device(hs, name), device(hs, name)
    t0 = dev_b.export_bvh()
    before = frames(dev_b, configs(name))
    ranges, xforms, scale = plan(rest, SEED[name] + 7)
    assert host_route(hs, dev_a, rest, ranges, xforms, scale, p3d.UPDATE_REFIT) > 0
    assert dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale) > 0
    now = assert_same_scene(dev_a, dev_b, name, "%s, refit" % name)
    t1 = dev_b.export_bvh()
    for k in ("bvh_index", "bvh_count_leaf", "bvh_order"):
        assert np.array_equal(t0[k], t1[k]), "%s: refit changed %s" % (name, k)
    assert t0["bvh_bmin"].tobytes() != t1["bvh_bmin"].tobytes()
    assert frames_differ(now, before), "the move changed no pixel"


@pytest.mark.parametrize("name", ["balls_low", "tri5k"])
def test_the_identity_brings_the_rest_pose_back(name, paths):
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    assert not (np.signbit(rest["prim_v"]) & (rest["prim_v"] == 0)).any()  # (1 * -0 + 0 is +0: the one value the identity changes)
    dev, fresh = device(hs, name), device(hs, name)
    ranges, xforms, scale = plan(rest, SEED[name] + 3)
    dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    assert frames_differ(frames(dev, configs(name)), frames(fresh, configs(name)))
    dev.transform_prims([(f, c, 0) for f, c, _ in ranges], IDENTITY[None], p3d.UPDATE_REBUILD)
    assert_same_scene(fresh, dev, name, "%s, identity after a move" % name)


@pytest.mark.parametrize("first", ["update", "transform"])
def test_update_prims_moves_the_rest_pose(first, paths):
    """update_prims of a few objects BEFORE the first transform (the rest copy is taken from what it left) and AFTER it (it
    writes the rest copy too): the identity then gives a fresh scene of the updated host scene"""
    name = "balls_low"
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    dev = device(hs, name)
    ranges, xforms, scale = plan(rest, SEED[name] + 5)
    if first == "transform":
        dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    objs, new_v = random_moves(rest, 77, fraction=0.25)
    hs.set_geometry(objs, new_v)
    dev.update_prims(objs, p3d.UPDATE_REFIT)
    if first == "update":
        dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    fresh = device(hs, name)
    assert frames_differ(frames(dev, configs(name)), frames(fresh, configs(name)))
    dev.transform_prims([(f, c, 0) for f, c, _ in ranges], IDENTITY[None], p3d.UPDATE_REBUILD)
    assert_same_scene(fresh, dev, name, "identity after update_prims (%s first)" % first)


@pytest.mark.parametrize("name", ["tri5k", "balls_low"])
def test_every_object_finds_its_range(name, paths):
    """tri5k split at 1, 63, 64, 65 and 257 (one object, a wave's end, a block's end + 1), balls_low with one range per object;
    every range with a matrix of its own, in shuffled order"""
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    n = rest["n_prims"]
    assert (rest["prim_type"] != PLANE).all() and not (rest["prim_type"] == BOX).any()
    cuts = [0, 1, 63, 64, 65, 257, n] if name == "tri5k" else list(range(n + 1))
    assert n > 257 or name != "tri5k"
    rng = np.random.default_rng(SEED[name] + 11)
    xforms = np.stack([rigid(rest, rng, reach=0.02 + 0.01 * i) for i in range(len(cuts) - 1)])
    ranges = [(cuts[i], cuts[i + 1] - cuts[i], i) for i in range(len(cuts) - 1)]
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    dev_a, dev_b = device(hs, name), device(hs, name)
    host_route(hs, dev_a, rest, ranges, xforms, None, p3d.UPDATE_REBUILD)
    dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REBUILD)
    assert_same_scene(dev_a, dev_b, name, "%s, %d ranges" % (name, len(ranges)))


def test_unnamed_objects_are_untouched(paths):
    name = "tri5k"
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    n = rest["n_prims"]
    dev_a, dev_b = device(hs, name), device(hs, name)
    ranges = [(n // 3, n // 3, 0)]
    xforms = rigid(rest, np.random.default_rng(41))[None]
    host_route(hs, dev_a, rest, ranges, xforms, None, p3d.UPDATE_REBUILD)
    dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REBUILD)
    o, d = rays()
    hit_a, p_a, t_a = dev_a.trace_closest(p3d.ACCEL_BVH, o, d, want_t=True)
    hit_b, p_b, t_b = dev_b.trace_closest(p3d.ACCEL_BVH, o, d, want_t=True)
    assert np.array_equal(hit_a, hit_b) and (hit_a >= 0).sum() > len(o) // 100
    outside = (hit_b >= 0) & ((hit_b < n // 3) | (hit_b >= 2 * (n // 3)))
    assert outside.sum() > 100  # rays that end on objects no range named
    assert p_a.tobytes() == p_b.tobytes() and t_a.tobytes() == t_b.tobytes()
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), "a third of tri5k")


def _xf(m=IDENTITY, scale=1.0, reserved=(0, 0, 0)):
    x = p3d.Xform()
    x.m[:] = [float(v) for v in np.asarray(m, np.float32).reshape(12)]
    x.sphere_scale = scale
    x.reserved[:] = reserved
    return x


def _raw(dev, ranges, xforms, mode=p3d.UPDATE_REFIT, n_ranges=None, n_xforms=None, null_ranges=False, null_xforms=False):
    rg = (p3d.XformRange * max(len(ranges), 1))(*[p3d.XformRange(*r) for r in ranges])
    xf = (p3d.Xform * max(len(xforms), 1))(*xforms)
    ms = C.c_float(-1.0)
    return p3d.lib().p3d_scene_transform_prims(dev._h if dev is not None else None, len(ranges) if n_ranges is None else n_ranges,
                                               None if null_ranges else C.cast(rg, C.c_void_p), len(xforms) if n_xforms is None else n_xforms,
                                               None if null_xforms else C.cast(xf, C.c_void_p), mode, C.byref(ms))


def test_refusals_leave_the_scene_as_it_was(paths):
    name = "balls_box"
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    a = hs.arrays()
    n = a["n_prims"]
    box = int(np.nonzero(a["prim_type"] == BOX)[0][0])
    sphere = int(np.nonzero(a["prim_type"] == SPHERE)[0][0])
    dev = p3d.DeviceScene(hs, bvh="device")  # (before the host scene builds a grid: its descriptor carries one from then on)
    host_tree = p3d.DeviceScene(hs, bvh=True)
    with_grid = p3d.DeviceScene(hs, bvh="device", grid=True)
    hp = load(PLANES, RES)
    ap = hp.arrays()
    plane = int(np.nonzero(ap["prim_type"] == PLANE)[0][0])
    dev_planes = p3d.DeviceScene(hp, bvh="device")

    def state(s):
        return frames(s, configs(name))

    slide = IDENTITY.copy()
    slide[:, 3] = (0.25, 0.1, -0.2)
    good = [(sphere, 1, 0, 0)]
    for what, scene in (("a scene with the host's tree", host_tree), ("a scene with an uploaded grid", with_grid)):
        was = state(scene)
        assert _raw(scene, good, [_xf(slide)]) == -1, what
        assert_same_frames(state(scene), was, what)
    was_planes = state(dev_planes)
    assert _raw(dev_planes, [(plane, 1, 0, 0)], [_xf(slide)]) == -1, "a range that covers a plane"
    assert b"plane" in p3d.lib().p3d_last_error()
    assert_same_frames(state(dev_planes), was_planes, "a range that covers a plane")

    was, tree = state(dev), dev.export_bvh()
    rot = np.zeros((3, 4), np.float32)
    rot[:, :3] = rotation(np.random.default_rng(2))
    nan_m, inf_m, flipped, flat = slide.copy(), slide.copy(), slide.copy(), slide.copy()
    nan_m[1, 2] = np.nan
    inf_m[0, 3] = np.inf
    flipped[1, 1] = -1.0
    flat[2, 2] = 0.0
    cases = [
        ("an unknown mode", dict(ranges=good, xforms=[_xf(slide)], mode=2)),
        ("null ranges with a count", dict(ranges=good, xforms=[_xf(slide)], null_ranges=True)),
        ("null transforms with a count", dict(ranges=[], xforms=[_xf(slide)], null_xforms=True)),
        ("an empty range", dict(ranges=[(sphere, 0, 0, 0)], xforms=[_xf(slide)])),
        ("a range behind the last object", dict(ranges=[(n - 1, 2, 0, 0)], xforms=[_xf(slide)])),
        ("a range whose end wraps", dict(ranges=[(0xffffffff, 2, 0, 0)], xforms=[_xf(slide)])),
        ("a transform that is not there", dict(ranges=[(sphere, 1, 1, 0)], xforms=[_xf(slide)])),
        ("no transforms at all", dict(ranges=good, xforms=[], n_xforms=0)),
        ("reserved in a range", dict(ranges=[(sphere, 1, 0, 1)], xforms=[_xf(slide)])),
        ("overlapping ranges", dict(ranges=[(sphere, 3, 0, 0), (sphere + 2, 2, 0, 0)], xforms=[_xf(slide)])),
        ("overlapping ranges, shuffled", dict(ranges=[(sphere + 4, 2, 0, 0), (sphere, 6, 0, 0), (sphere + 20, 1, 0, 0)], xforms=[_xf(slide)])),
        ("the same range twice", dict(ranges=[(sphere, 1, 0, 0), (sphere, 1, 0, 0)], xforms=[_xf(slide)])),
        ("a NaN in m", dict(ranges=good, xforms=[_xf(nan_m)])),
        ("an infinite m", dict(ranges=good, xforms=[_xf(inf_m)])),
        ("a NaN in an unused transform", dict(ranges=good, xforms=[_xf(slide), _xf(nan_m)])),
        ("a NaN sphere_scale", dict(ranges=good, xforms=[_xf(slide, float("nan"))])),
        ("an infinite sphere_scale", dict(ranges=good, xforms=[_xf(slide, float("inf"))])),
        ("sphere_scale 0", dict(ranges=good, xforms=[_xf(slide, 0.0)])),
        ("a negative sphere_scale", dict(ranges=good, xforms=[_xf(slide, -1.0)])),
        ("reserved in a transform", dict(ranges=good, xforms=[_xf(slide, 1.0, (0, 0, 5))])),
        ("a rotated box", dict(ranges=[(box, 1, 0, 0)], xforms=[_xf(rot)])),
        ("a mirrored box", dict(ranges=[(box, 1, 0, 0)], xforms=[_xf(flipped)])),
        ("a flattened box", dict(ranges=[(box, 1, 0, 0)], xforms=[_xf(flat)])),
        ("a rotated box among spheres", dict(ranges=[(0, n, 0, 0)], xforms=[_xf(rot)])),
    ]
    for what, kw in cases:
        assert _raw(dev, **kw) == -1, what
        assert p3d.lib().p3d_last_error(), what
        assert_same_frames(state(dev), was, what)
    assert _raw(None, good, [_xf(slide)]) == -1
    assert_same_tree(dev.export_bvh(), tree, "after the refusals")
    assert dev.status() == 0
    # the same call without a fault is accepted: boxes too, and update_ms == NULL
    rg = (p3d.XformRange * 2)(p3d.XformRange(sphere, 1, 0, 0), p3d.XformRange(box, 1, 0, 0))
    xf = (p3d.Xform * 1)(_xf(slide))
    assert p3d.lib().p3d_scene_transform_prims(dev._h, 2, C.cast(rg, C.c_void_p), 1, C.cast(xf, C.c_void_p), p3d.UPDATE_REBUILD, None) == 0
    assert frames_differ(state(dev), was)
    # no ranges at all: a rebuild of what is already rebuilt (re-sorting what is sorted changes nothing)
    tree = dev.export_bvh()
    assert _raw(dev, [], [], mode=p3d.UPDATE_REBUILD) == 0
    assert_same_tree(dev.export_bvh(), tree, "a rebuild of nothing")


def test_an_object_that_overflows_keeps_its_geometry(paths):
    """Finite numbers that leave float32.  A translation of 3e38 alone does not (3e38 + radius is finite: the largest float32
    is 3.4e38), so the sphere also takes sphere_scale 3e38: its radius, and with it its box, becomes infinite.  The kernel
    leaves that object unwritten and counts it: no fault is provoked."""
    name = "balls_low"
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    spheres = np.nonzero(rest["prim_type"] == SPHERE)[0]
    victim = int(spheres[np.argmax(rest["prim_v"][spheres, 3])])
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e38) + rest["prim_v"][victim, 3] * np.float32(3e38))
    rng = np.random.default_rng(SEED[name] + 13)
    far = IDENTITY.copy()
    far[:, 3] = 3e38
    xforms = np.stack([rigid(rest, rng), far])
    scale = np.array([1.25, 3e38], np.float32)
    others = [(f, c, 0) for f, c in runs([int(k) if i != victim else -1 for i, k in enumerate(rest["prim_type"])], (SPHERE, TRIANGLE))]
    dev_a, dev_b = device(hs, name), device(hs, name)
    before = frames(dev_b, configs(name))
    host_route(hs, dev_a, rest, others, xforms, scale, p3d.UPDATE_REBUILD)  # A: the victim is left out of the move
    with pytest.raises(p3d.P3DError) as e:
        dev_b.transform_prims(others + [(victim, 1, 1)], xforms, p3d.UPDATE_REBUILD, sphere_scale=scale)
    assert e.value.code == -1 and "1 object" in str(e.value)
    assert dev_b.status() == 0
    now = assert_same_scene(dev_a, dev_b, name, "overflow of one sphere")  # the victim where it was, the others moved
    assert frames_differ(now, before)
    # the scene goes on: the next transform is exact again
    ranges, xforms, scale = plan(rest, SEED[name] + 14)
    host_route(hs, dev_a, rest, ranges, xforms, scale, p3d.UPDATE_REFIT)
    dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    assert_same_scene(dev_a, dev_b, name, "after the overflow")


def test_accumulators_refuse_passes_until_reset(paths):
    hs = load(CORNELL, 64)
    rest = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev.accumulator(cfg)
    ada = dev.adaptive(cfg, rel_error=0.05, min_samples=4)
    acc.render(2)
    ada.render(4)
    ranges, xforms, scale = plan(rest, SEED["cornell"] + 9)
    dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    for a, done in ((acc, 2), (ada, 4)):
        with pytest.raises(p3d.P3DError) as e:
            a.render(1)
        assert e.value.code == -1 and "moved" in str(e.value)
        assert a.samples_done == done
        a.reset()
    hs.set_geometry(*p3d.transformed(rest["prim_type"], rest["prim_v"], ranges, xforms, scale))
    fresh = p3d.DeviceScene(hs, bvh=dev.export_bvh())
    f_acc = fresh.accumulator(cfg)
    f_ada = fresh.adaptive(cfg, rel_error=0.05, min_samples=4)
    for n in (4, 5):
        got, want = acc.render(n), f_acc.render(n)
        assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
        g_ada, w_ada = ada.render(n), f_ada.render(n)
        assert np.array_equal(g_ada[1], w_ada[1]) and g_ada[0].tobytes() == w_ada[0].tobytes() and np.array_equal(g_ada[2], w_ada[2])
    for a in (acc, ada, f_acc, f_ada):
        a.close()


def test_recorded_schedules_are_forgotten_and_staging_is_kept(paths):
    """The one frame here that is not 96 x 96: a tile schedule is memoised only for a frame of thousands of tiles.  Rendered
    twice so that the memo exists; after the transform the cost-ordered frame is the frame-ordered one."""
    res = 1024
    name = "balls_low"
    hs = load(paths[name], res, legacy_f11=legacy(paths[name]))
    rest = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    cost = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, tile_order=p3d.TILE_ORDER_COST)
    plain = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, tile_order=p3d.TILE_ORDER_FRAME)
    for _ in range(2):
        old = dev.render(cost, stats=False)
    ranges, xforms, scale = plan(rest, SEED[name] + 21)
    assert dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale) > 0
    ranges, xforms, scale = plan(rest, SEED[name] + 22)
    assert dev.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale) > 0  # the same sizes: nothing is allocated
    want = dev.render(plain, stats=False)
    for _ in range(2):
        rgb, hit = dev.render(cost, stats=False)[:2]
        assert np.array_equal(hit, want[1]) and rgb.tobytes() == want[0].tobytes()
    assert rgb.tobytes() != old[0].tobytes()
