"""The uniform grid built on the GPU (p3d_scene_build_grid, p3d_scene_export_grid) and kept through p3d_scene_update_prims.

The yardstick is the host builder, Grid::Build, through HostScene.arrays(grid=True) (test_host_logic.py ties it to the oracle):
the device grid must be that grid to the bit, so every comparison here is equality of bytes - exported arrays, colour bits,
hit IDs, counters and query results against a scene created with the host's grid uploaded."""
import ctypes as C

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, RENDER_COUNTERS, assert_same_frames, assert_same_grid, frames, frames_differ, load, rays
import p3d_amd as p3d
from scene_update_helpers import SPHERE, random_moves, translated

pytestmark = pytest.mark.gpu

RES = 192
SCENES = ["balls_low", "path_glass", "cornell", "tri5k", "tri100k", "one_sphere"]
SEED = {"balls_low": 21, "tri5k": 22, "cornell": 24}
SHAPE = {"balls_low": (49, 49, 3), "path_glass": (49, 49, 10), "cornell": (5, 5, 5), "tri5k": (5, 5, 5), "tri100k": (5, 5, 5),
         "one_sphere": (1, 1, 1)}

ONE_SPHERE = """bclr 0.1 0.2 0.3
v
from 2 1.5 1
at 0 0 0
up 0 0 1
angle 40
hither 0.01
resolution 64 64
aperture 0
focal 1
l 3 2 4 1 1 1
f 0.9 0.5 0.2 1 1 1 0.6 0.3 20 0 1 0 0 0
s 0 0 0 0.2
"""
# 2 * 10000 + 1 cells along every axis: more than 2^28 in all
FAR_APART = ONE_SPHERE.replace("s 0 0 0 0.2\n", "s 0 0 0 0.01\ns 10000 10000 10000 0.01\n")


@pytest.fixture(scope="module")
def paths(tri5k_path, tri100k_path, tmp_path_factory):
    d = tmp_path_factory.mktemp("grid_scenes")
    out = {"balls_low": scene_path("balls_low.p3f"), "path_glass": scene_path("path_glass.p3f"), "cornell": CORNELL,
           "tri5k": tri5k_path, "tri100k": tri100k_path, "one_sphere": str(d / "one_sphere.p3f"), "far_apart": str(d / "far_apart.p3f")}
    with open(out["one_sphere"], "w") as f:
        f.write(ONE_SPHERE)
    with open(out["far_apart"], "w") as f:
        f.write(FAR_APART)
    return out


_hosts = {}


@pytest.fixture
def host(paths):
    """name -> (host scene, its arrays with the host's grid): loaded and built once for the tests that do not move anything"""
    def get(name):
        if name not in _hosts:
            hs = load(paths[name], 64 if name == "tri100k" else RES)
            _hosts[name] = (hs, hs.arrays(grid=True))
        return _hosts[name]
    return get


def lists(a):
    return np.diff(a["grid_cell_start"].astype(np.int64))


def grid_configs(name):
    out = [("whitted", p3d.whitted_config(accel=p3d.ACCEL_GRID, max_depth=4, collect_stats=1))]
    if name == "cornell":
        out.append(("path trace 4 spp", p3d.pathtrace_config(accel=p3d.ACCEL_GRID, spp_sqrt=2, max_depth=8, seed=3, collect_stats=1)))
    return out


def assert_same_queries(a, b, what):
    o, d = rays(axis_parallel=True)
    hit_a, p_a, t_a = a.trace_closest(p3d.ACCEL_GRID, o, d, want_t=True)
    hit_b, p_b, t_b = b.trace_closest(p3d.ACCEL_GRID, o, d, want_t=True)
    assert np.array_equal(hit_a, hit_b), what
    assert p_a.tobytes() == p_b.tobytes() and t_a.tobytes() == t_b.tobytes(), what
    assert np.array_equal(a.trace_any(p3d.ACCEL_GRID, o, d), b.trace_any(p3d.ACCEL_GRID, o, d)), what


@pytest.mark.parametrize("name", SCENES)
def test_device_grid_is_the_host_grid(name, host):
    hs, want = host(name)
    assert tuple(want["grid_n"]) == SHAPE[name]
    # what each scene is here for, asserted on the host's arrays: a changed generator cannot hollow the test out
    if name == "balls_low":
        assert (lists(want) == 0).any()
    if name == "tri5k":
        assert lists(want).max() > 64  # longer than a wave
    if name == "tri100k":
        assert lists(want).max() > 1024  # longer than a workgroup can be
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    assert dev.device_grid_ms > 0
    assert_same_grid(dev.export_grid(), want, name)
    dev.close()


@pytest.mark.parametrize("name", SCENES)
def test_grid_frames_match_the_uploaded_grid(name, host):
    hs, _ = host(name)
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    twin = p3d.DeviceScene(hs, bvh="device", grid=True)
    assert_same_frames(frames(dev, grid_configs(name), skip_unsupported=False), frames(twin, grid_configs(name), skip_unsupported=False), name)
    assert_same_queries(dev, twin, name)
    dev.close()
    twin.close()


def moves(hs, name, round_):
    a = hs.arrays()
    lit = a["materials"][:, 12:15].sum(1) > 0
    spheres = [i for i in range(a["n_prims"]) if a["prim_type"][i] == SPHERE]
    include = [i for i in spheres if lit[a["prim_material"][i]]] if name == "cornell" else spheres[:1]
    return random_moves(a, SEED[name] + 100 * round_, include=include)


@pytest.mark.parametrize("mode", [p3d.UPDATE_REFIT, p3d.UPDATE_REBUILD], ids=["refit", "rebuild"])
@pytest.mark.parametrize("name", ["balls_low", "tri5k", "cornell"])
def test_update_rebuilds_the_grid(name, mode, paths):
    hs = load(paths[name], RES)
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    last = frames(dev, grid_configs(name), skip_unsupported=False)
    for round_ in range(2):  # the second rebuild runs in the arrays the first ones left
        objs, new_v = moves(hs, name, round_)
        hs.set_geometry(objs, new_v)
        assert dev.update_prims(objs, mode) > 0
        what = "%s, update %d" % (name, round_)
        assert_same_grid(dev.export_grid(), hs.arrays(grid=True), what)
        fresh = p3d.DeviceScene(hs, bvh="device", grid=True)
        now = frames(dev, grid_configs(name), skip_unsupported=False)
        assert_same_frames(now, frames(fresh, grid_configs(name), skip_unsupported=False), what)
        assert frames_differ(now, last), "the move changed no pixel"
        last = now
        fresh.close()
    grid = dev.export_grid()
    dev.update_prims([], p3d.UPDATE_REBUILD)
    assert_same_grid(dev.export_grid(), grid, "update of nothing")
    dev.close()


def test_grid_arrays_grow_and_shrink(paths):
    hs = load(paths["balls_low"], RES)
    original = hs.arrays(grid=True)
    sphere = int(np.nonzero(original["prim_type"] == SPHERE)[0][0])
    objs = np.array([sphere], np.uint32)
    home = original["prim_v"][objs].copy()
    extent_z = float(original["grid_bmax"][2] - original["grid_bmin"][2])
    away = translated(original["prim_type"], original["prim_v"], objs, [(0.0, 0.0, 3.0)])
    assert 3.0 > extent_z
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    assert_same_grid(dev.export_grid(), original, "as created")
    hs.set_geometry(objs, away)
    grown = hs.arrays(grid=True)
    assert tuple(grown["grid_n"]) != tuple(original["grid_n"])
    assert len(grown["grid_cell_start"]) > len(original["grid_cell_start"]) and len(grown["grid_cell_items"]) > len(original["grid_cell_items"])
    dev.update_prims(objs, p3d.UPDATE_REFIT)
    assert_same_grid(dev.export_grid(), grown, "grown")
    twin = p3d.DeviceScene(hs, bvh="device", grid=True)
    assert_same_frames(frames(dev, grid_configs("balls_low"), skip_unsupported=False), frames(twin, grid_configs("balls_low"), skip_unsupported=False), "grown")
    twin.close()
    hs.set_geometry(objs, home)
    dev.update_prims(objs, p3d.UPDATE_REFIT)
    back = dev.export_grid()
    assert_same_grid(back, hs.arrays(grid=True), "moved back")
    assert_same_grid(back, original, "moved back, against the original")
    dev.close()


def _export_raw(dev, n_start, n_items):
    start = np.full(n_start + 4, 0xdeadbeef, np.uint32)
    items = np.full(n_items + 4, 0xdeadbeef, np.uint32)
    info = p3d.GridDesc()
    a, b = C.c_uint32(n_start), C.c_uint32(n_items)
    rc = p3d.lib().p3d_scene_export_grid(dev._h, C.byref(info), start.ctypes.data, C.byref(a), items.ctypes.data, C.byref(b))
    return rc, start, items, a.value, b.value


def test_refusals(paths):
    hs = load(paths["balls_low"], RES)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_GRID, max_depth=4, collect_stats=1)
    lib = p3d.lib()

    def frame(s, c=cfg):
        rgb, hit, st = s.render(c)
        return rgb.tobytes(), hit.tobytes(), tuple(getattr(st, k) for k in RENDER_COUNTERS)

    host_tree = p3d.DeviceScene(hs, bvh=True)
    with pytest.raises(p3d.P3DError) as e:
        host_tree.build_grid()
    assert e.value.code == -1
    uploaded = p3d.DeviceScene(hs, bvh="device", grid=True)
    was = frame(uploaded)
    for call in (uploaded.build_grid, uploaded.export_grid):
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1
    assert frame(uploaded) == was
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    # before any build: a scene created as `dev` was, without the build
    d = p3d.SceneDesc.from_buffer_copy(hs.desc(False, False))
    d.has_grid = 0
    h = C.c_void_p()
    assert lib.p3d_scene_create_device_bvh(C.byref(d), 0, C.byref(h), None) == 0
    info = p3d.GridDesc()
    n, m = C.c_uint32(0), C.c_uint32(0)
    assert lib.p3d_scene_export_grid(h, C.byref(info), None, C.byref(n), None, C.byref(m)) == -1
    assert b"no device-built grid" in lib.p3d_last_error()
    lib.p3d_scene_destroy(h)
    # capacities one too small: -4, the sizes are reported and nothing is written
    grid = dev.export_grid()
    n_start, n_items = len(grid["grid_cell_start"]), len(grid["grid_cell_items"])
    for a, b in ((n_start - 1, n_items), (n_start, n_items - 1)):
        rc, start, items, got_a, got_b = _export_raw(dev, a, b)
        assert rc == -4 and (got_a, got_b) == (n_start, n_items)
        assert (start == 0xdeadbeef).all() and (items == 0xdeadbeef).all()
    rc, start, items, _, _ = _export_raw(dev, n_start, n_items)
    assert rc == 0 and (start[n_start:] == 0xdeadbeef).all() and (items[n_items:] == 0xdeadbeef).all()
    assert start[:n_start].tobytes() == grid["grid_cell_start"].tobytes() and items[:n_items].tobytes() == grid["grid_cell_items"].tobytes()
    # a second build gives the same grid and the same frame
    was = frame(dev)
    assert dev.build_grid() > 0
    assert_same_grid(dev.export_grid(), grid, "built twice")
    assert frame(dev) == was
    for s in (host_tree, uploaded, dev):
        s.close()


def test_accumulators_refuse_passes_until_reset(paths):
    hs = load(CORNELL, 64)
    dev = p3d.DeviceScene(hs, bvh="device", grid="device")
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_GRID, spp_sqrt=3, max_depth=8, seed=9, stack_mode=p3d.STACK_PER_PIXEL)
    acc = dev.accumulator(cfg)
    acc.render(2)
    objs, new_v = moves(hs, "cornell", 0)
    hs.set_geometry(objs, new_v)
    dev.update_prims(objs, p3d.UPDATE_REFIT)
    with pytest.raises(p3d.P3DError) as e:
        acc.render(1)
    assert e.value.code == -1 and "moved" in str(e.value)
    assert acc.samples_done == 2
    acc.reset()
    fresh = p3d.DeviceScene(hs, bvh="device", grid=True)
    f_acc = fresh.accumulator(cfg)
    for n in (4, 5):
        got, want = acc.render(n), f_acc.render(n)
        assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
    assert acc.samples_done == 9 and got[0].tobytes() == fresh.render(cfg)[0].tobytes()
    for a in (acc, f_acc):
        a.close()
    dev.close()
    fresh.close()


def test_too_many_cells_are_refused_before_the_build(paths):
    """Two tiny spheres 10 000 apart: 20 001 cells along every axis.  Refused on the host side of the call, after the bounds
    came back and before anything is sized by them; the scene is left without a grid and with its BVH."""
    hs = load(paths["far_apart"], 64)
    dev = p3d.DeviceScene(hs, bvh="device")
    bvh_cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=2)
    was = dev.render(bvh_cfg)
    with pytest.raises(p3d.P3DError) as e:
        dev.build_grid()
    assert e.value.code == -4 and "2^28" in str(e.value)
    with pytest.raises(p3d.P3DError) as e:
        dev.export_grid()
    assert e.value.code == -1
    with pytest.raises(p3d.P3DError) as e:
        dev.render(p3d.whitted_config(accel=p3d.ACCEL_GRID, max_depth=2))
    assert e.value.code == -1 and "without a grid" in str(e.value)
    now = dev.render(bvh_cfg)
    assert now[0].tobytes() == was[0].tobytes() and np.array_equal(now[1], was[1])
    dev.close()
