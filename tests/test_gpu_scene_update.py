"""Moving the objects of a live device scene (p3d_scene_update_prims, p3d_scene_export_bvh) on the GPU.

REBUILD must be a fresh p3d_scene_create_device_bvh of the moved descriptor, to the bit: frames, counters and the exported
tree.  REFIT keeps the topology and must be exact for it: every box the exact union of what lies below it, and a scene
uploaded with that exported tree (p3d_scene_create) renders and traces the same bits.  Between the two trees only what
cannot depend on a tree is compared, with the bounds test_device_built_bvh_finds_the_same_closest_hits uses (grazing rays,
Q8).  All comparisons of one tree against itself have tolerance 0."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, RENDER_COUNTERS, assert_same_frames, assert_same_tree, frames, frames_differ, load, rays
from lbvh_reference import check_boxes
from live_scene_checks import configs
from oracle import binding as ob
import p3d_amd as p3d
from scene_update_helpers import PLANE, SPHERE, random_moves, write_moved_p3f

pytestmark = pytest.mark.gpu

RES = 192
WHITTED_SCENES = ["balls_low", "tri5k", "path_glass"]
SEED = {"balls_low": 11, "tri5k": 12, "path_glass": 13, "cornell": 14}


@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "path_glass": scene_path("path_glass.p3f"),
            "cornell": CORNELL}


def emissive_spheres(a):
    lit = a["materials"][:, 12:15].sum(1) > 0
    return [i for i in range(a["n_prims"]) if a["prim_type"][i] == SPHERE and lit[a["prim_material"][i]]]


def moves(hs, name, round_=0):
    """A third of the objects, seeded; always with the emissive sphere of cornell among them, and elsewhere with the scene's
    first sphere: a Whitted frame of a scene without lights (path_glass) is black, and moving its floor alone changes no hit ID"""
    a = hs.arrays()
    spheres = np.nonzero(a["prim_type"] == SPHERE)[0][:1].tolist()
    return random_moves(a, SEED[name] + 100 * round_, include=emissive_spheres(a) if name == "cornell" else spheres)


@pytest.mark.parametrize("name", WHITTED_SCENES + ["cornell"])
def test_rebuild_is_a_fresh_create(name, paths):
    hs = load(paths[name], RES)
    dev = p3d.DeviceScene(hs, bvh="device")
    last = frames(dev, configs(name))
    for round_ in range(2):  # the second update runs in the workspace the first one allocated
        objs, new_v = moves(hs, name, round_)
        hs.set_geometry(objs, new_v)
        ms = dev.update_prims(objs, p3d.UPDATE_REBUILD)
        assert ms > 0
        fresh = p3d.DeviceScene(hs, bvh="device")
        now = frames(dev, configs(name))
        assert_same_frames(now, frames(fresh, configs(name)), "%s, rebuild %d" % (name, round_))
        assert_same_tree(dev.export_bvh(), fresh.export_bvh(), "%s, rebuild %d" % (name, round_))
        assert frames_differ(now, last), "the move changed no pixel"
        last = now
        fresh.close()
    # n = 0: re-sorting what is already sorted changes nothing
    tree = dev.export_bvh()
    assert dev.update_prims([], p3d.UPDATE_REBUILD) > 0
    assert_same_tree(dev.export_bvh(), tree, "rebuild of nothing")
    assert_same_frames(frames(dev, configs(name)), last, "rebuild of nothing")


@pytest.mark.parametrize("name", WHITTED_SCENES + ["cornell"])
def test_refit_is_exact_for_its_tree(name, paths):
    hs = load(paths[name], RES)
    dev = p3d.DeviceScene(hs, bvh="device")
    before = frames(dev, configs(name))
    t0 = dev.export_bvh()
    check_boxes(t0, hs.arrays(), "%s as created" % name)
    o, d = rays(axis_parallel=True)
    for round_ in range(2):
        objs, new_v = moves(hs, name, round_)
        hs.set_geometry(objs, new_v)
        assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0
        t1 = dev.export_bvh()
        for k in ("bvh_index", "bvh_count_leaf", "bvh_order"):
            assert np.array_equal(t0[k], t1[k]), "%s: refit changed %s" % (name, k)
        assert t0["bvh_max_depth"] == t1["bvh_max_depth"]
        assert t0["bvh_bmin"].tobytes() != t1["bvh_bmin"].tobytes()
        check_boxes(t1, hs.arrays(), "%s, refit %d" % (name, round_))
        twin = p3d.DeviceScene(hs, bvh=t1)  # p3d_scene_create of the exported tree and the moved objects
        now = frames(dev, configs(name))
        assert_same_frames(now, frames(twin, configs(name)), "%s, refit %d against the uploaded tree" % (name, round_))
        assert frames_differ(now, before), "the move changed no pixel"
        hit_a, p_a, t_a = dev.trace_closest(p3d.ACCEL_BVH, o, d, want_t=True)
        hit_b, p_b, t_b = twin.trace_closest(p3d.ACCEL_BVH, o, d, want_t=True)
        assert np.array_equal(hit_a, hit_b) and (hit_a >= 0).sum() > len(o) // 100
        assert p_a.tobytes() == p_b.tobytes() and t_a.tobytes() == t_b.tobytes()
        assert np.array_equal(dev.trace_any(p3d.ACCEL_BVH, o, d), twin.trace_any(p3d.ACCEL_BVH, o, d))
        before = now
        twin.close()


@pytest.mark.parametrize("name", WHITTED_SCENES)
def test_refit_finds_the_same_surfaces_as_rebuild(name, paths, tmp_path):
    hs = load(paths[name], RES)
    refit = p3d.DeviceScene(hs, bvh="device")
    rebuilt = p3d.DeviceScene(hs, bvh="device")
    a = hs.arrays()
    objs, new_v = moves(hs, name)
    hs.set_geometry(objs, new_v)
    refit.update_prims(objs, p3d.UPDATE_REFIT)
    rebuilt.update_prims(objs, p3d.UPDATE_REBUILD)
    o, d = rays(axis_parallel=True)
    hit_f, _ = refit.trace_closest(p3d.ACCEL_BVH, o, d)
    hit_b, _ = rebuilt.trace_closest(p3d.ACCEL_BVH, o, d)
    sc = ob.Scene(write_moved_p3f(paths[name], str(tmp_path / "moved.p3f"), a["prim_type"], objs, new_v))
    hit_n, _, _ = sc.trace_closest(0, o, d)  # the oracle's object loop over the moved scene: a tree-independent answer
    assert (hit_n >= 0).sum() > len(o) // 100
    for what, other in (("rebuild", hit_b), ("object loop", hit_n)):
        miss = float(((other >= 0) != (hit_f >= 0)).mean())
        diff = float((other != hit_f).mean())
        print("%s, refit against %s: hit/miss differs on %.3g of the rays, the object on %.3g" % (name, what, miss, diff))
        assert miss < 1e-4, what
        assert diff < 1e-3, what
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=0)
    _, img_f, _ = refit.render(cfg)
    _, img_b, _ = rebuilt.render(cfg)
    px = float((img_f != img_b).mean())
    print("%s: depth-0 hit_id images differ on %.3g of the pixels" % (name, px))
    assert px < 1e-3


@pytest.mark.parametrize("mode", [p3d.UPDATE_REFIT, p3d.UPDATE_REBUILD], ids=["refit", "rebuild"])
def test_recorded_schedules_are_forgotten(mode, paths):
    """A frame big enough for a memoised tile schedule, and a striped tile whose halo chain is memoised, rendered twice so
    that the memos exist; after the update both render what a scene without memos renders."""
    res = 1024
    hs = load(paths["balls_low"], res)
    dev = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, tile_order=p3d.TILE_ORDER_COST)
    stripe = p3d.stripe_tile((res, res), 1, 2, 8)
    for _ in range(2):
        old = dev.render(cfg, stats=False)
        dev.render(cfg, tile=stripe, stats=False)
    objs, new_v = moves(hs, "balls_low")
    hs.set_geometry(objs, new_v)
    dev.update_prims(objs, mode)
    fresh = p3d.DeviceScene(hs, bvh="device" if mode == p3d.UPDATE_REBUILD else dev.export_bvh())
    for tile in (None, stripe):
        for _ in range(2):
            rgb, hit = dev.render(cfg, tile=tile, stats=False)[:2]
            f_rgb, f_hit = fresh.render(cfg, tile=tile, stats=False)[:2]
            assert np.array_equal(hit, f_hit) and rgb.tobytes() == f_rgb.tobytes()
    assert dev.render(cfg, stats=False)[0].tobytes() != old[0].tobytes()  # (balls_low has lights)


def test_accumulators_refuse_passes_until_reset(paths):
    hs = load(CORNELL, 64)
    dev = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev.accumulator(cfg)
    ada = dev.adaptive(cfg, rel_error=0.05, min_samples=4)
    acc.render(2)
    ada.render(4)
    objs, new_v = moves(hs, "cornell")
    hs.set_geometry(objs, new_v)
    dev.update_prims(objs, p3d.UPDATE_REFIT)
    for a, done in ((acc, 2), (ada, 4)):
        with pytest.raises(p3d.P3DError) as e:
            a.render(1)
        assert e.value.code == -1 and "moved" in str(e.value)
        assert a.samples_done == done
        a.reset()
    fresh = p3d.DeviceScene(hs, bvh=dev.export_bvh())
    f_acc = fresh.accumulator(cfg)
    f_ada = fresh.adaptive(cfg, rel_error=0.05, min_samples=4)
    for n in (4, 5):
        got, want = acc.render(n), f_acc.render(n)
        assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
        g_ada, w_ada = ada.render(n), f_ada.render(n)
        assert np.array_equal(g_ada[1], w_ada[1]) and g_ada[0].tobytes() == w_ada[0].tobytes() and np.array_equal(g_ada[2], w_ada[2])
    assert acc.samples_done == 9 and got[0].tobytes() == fresh.render(cfg)[0].tobytes()  # the completed frame is the one-shot frame
    for a in (acc, ada, f_acc, f_ada):
        a.close()


def _update_raw(dev, objs, recs, mode=p3d.UPDATE_REFIT):
    objs = np.ascontiguousarray(objs, np.uint32)
    ms = C.c_float(-1.0)
    return p3d.lib().p3d_scene_update_prims(dev._h, len(objs), objs.ctypes.data, C.cast(recs, C.c_void_p), mode, C.byref(ms))


def test_refusals_leave_the_scene_as_it_was(paths):
    hs = load(paths["balls_low"], RES)
    d = hs.desc(False, False)
    n = d.n_prims

    def records(objs):
        recs = (p3d.Prim * len(objs))()
        for i, o in enumerate(objs):
            recs[i] = d.prims[int(o)]
        return recs

    mats = [d.prims[i].material for i in range(n)]
    types = [d.prims[i].type for i in range(n)]
    other_mat = next(i for i in range(n) if mats[i] != mats[n - 1])
    other_type = next(i for i in range(n) if types[i] != types[n - 1])
    dev = p3d.DeviceScene(hs, bvh="device")  # (before the host scene builds a grid: its descriptor carries one from then on)
    host_tree = p3d.DeviceScene(hs, bvh=True)
    with_grid = p3d.DeviceScene(hs, bvh="device", grid=True)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, collect_stats=1)

    def frame(s):
        rgb, hit, st = s.render(cfg)
        return rgb.tobytes(), hit.tobytes(), tuple(getattr(st, k) for k in RENDER_COUNTERS)

    moved = records([n - 1])
    moved[0].v[0] += 0.25
    moved[0].bmin[0] += 0.25
    moved[0].bmax[0] += 0.25
    for what, scene in (("a scene with the host's tree", host_tree), ("a scene with a grid", with_grid)):
        was = frame(scene)
        assert _update_raw(scene, [n - 1], moved) == -1, what
        assert frame(scene) == was, what
    was = frame(dev)
    tree = dev.export_bvh()
    material = records([n - 1]); material[0].material = mats[other_mat]
    kind = records([n - 1]); kind[0].type = types[other_type]
    twice = records([n - 1, 2, n - 1])
    nan_box = records([1, n - 1]); nan_box[1].bmax[1] = float("nan")
    inverted = records([n - 1]); inverted[0].bmin[2], inverted[0].bmax[2] = inverted[0].bmax[2], inverted[0].bmin[2]
    infinite = records([n - 1]); infinite[0].bmax[0] = float("inf")
    cases = [("a changed material", [n - 1], material, p3d.UPDATE_REFIT), ("a changed type", [n - 1], kind, p3d.UPDATE_REBUILD),
             ("a repeated index", [n - 1, 2, n - 1], twice, p3d.UPDATE_REFIT), ("a NaN box", [1, n - 1], nan_box, p3d.UPDATE_REBUILD),
             ("an inverted box", [n - 1], inverted, p3d.UPDATE_REFIT), ("an infinite box", [n - 1], infinite, p3d.UPDATE_REFIT),
             ("an index out of range", [n], moved, p3d.UPDATE_REFIT), ("an unknown mode", [n - 1], moved, 2)]
    for what, objs, recs, mode in cases:
        assert _update_raw(dev, objs, recs, mode) == -1, what
        assert frame(dev) == was, what
    lib = p3d.lib()
    assert lib.p3d_scene_update_prims(dev._h, 1, None, C.cast(moved, C.c_void_p), 0, None) == -1
    assert lib.p3d_scene_update_prims(dev._h, 1, np.array([n - 1], np.uint32).ctypes.data, None, 0, None) == -1
    assert frame(dev) == was
    assert_same_tree(dev.export_bvh(), tree, "after the refusals")
    with pytest.raises(p3d.P3DError) as e:
        host_tree.export_bvh()
    assert e.value.code == -1
    # the same record without the fault is accepted, with update_ms == NULL too
    assert lib.p3d_scene_update_prims(dev._h, 1, np.array([n - 1], np.uint32).ctypes.data, C.cast(moved, C.c_void_p), 0, None) == 0
    assert frame(dev) != was
