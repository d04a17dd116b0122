"""Filtered queries (include/p3d_filter.h) without a GPU: the entry points are declared, exported and wrapped as functions; the
host forms - the statement of the semantics - are held to the float64 models of the scene WITHOUT the skipped objects
(filter_reference.masked hands the thinned tables to the existing check_k / check_sweep, with their scenes and tolerances);
a skip list alone equals the unfiltered rows with the skipped objects taken out, in every bit; filters that name nothing change
no bit; the vertices of a mesh and the spheres of a ball scene stop finding themselves; and what is refused."""
import os
import re

import numpy as np
import pytest

from api_checks import header_code, scene_without_a_library
from conftest import SCENES as GOLDEN_SCENES
from device_query_contract import FLT_MAX, INVALID, UNSUPPORTED
from frame_checks import as_bytes
import filter_reference as fr
import intersect_reference as ref
import nearest_k_reference as nk
import nearest_reference as near
import p3d_amd as p3d
import sweep_reference as sw

NEAREST_SCENES = ("mixed", "mixed_planes", "planes", "axis_aligned", "tri5k")  # the nearest-k CPU test's, with its seeds
SEED = {name: 400 + k for k, name in enumerate(NEAREST_SCENES)}
MESH = "mount_high.p3f"   # the fixture the self-proximity test holds for: 2048 triangles over 1089 vertices, at most 6 round one
BALLS = "balls_low.p3f"   # and the one whose spheres sweep from their own centres


def test_the_header_declares_them():
    code, main = header_code("p3d_filter.h"), header_code()
    assert re.search(r'#include\s+"p3d_filter.h"', main) and re.search(r"#define\s+P3D_ABI_VERSION\s+4u?\b", main)
    assert re.search(r"#define\s+P3D_FILTER_SKIP_MAX\s+8u\b", code)
    cf, f, i32, u32 = r"\s*const\s+float\s*\*\s*\w+\s*,", r"\s*float\s*\*\s*\w+\s*,", r"\s*int32_t\s*\*\s*\w+\s*,", r"\s*uint32_t\s+\w+\s*,"
    filt = r"\s*const\s+int32_t\s*\*\s*\w+\s*," + u32 + r"\s*const\s+int32_t\s*\*\s*\w+\s*,"
    assert re.search(r"\bint\s+p3d_nearest_k_filtered_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 * 3 + cf * 2 + filt + i32 * 2 + f * 3 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_sweep_sphere_filtered_device\s*\(\s*p3d_scene\s*\*\s*\w+," + u32 * 2 + cf * 4 + filt + i32 + f * 4 + r"\s*void\s*\*\s*\w+\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_nearest_k_filtered\s*\(\s*p3d_host_scene\s*\*\s*\w+," + u32 * 2 + cf * 2 + filt + i32 * 2 + f + r"\s*float\s*\*\s*\w+\s*\)", code)
    assert re.search(r"\bint\s+p3d_host_scene_sweep_sphere_filtered\s*\(\s*const\s+p3d_host_scene\s*\*\s*\w+," + u32 + cf * 4 + filt + i32 + f * 2 + r"\s*float\s*\*\s*\w+\s*\)", code)


def test_the_library_exports_them_and_python_wraps_them_as_functions():
    names = ("p3d_nearest_k_filtered_device", "p3d_sweep_sphere_filtered_device", "p3d_host_scene_nearest_k_filtered", "p3d_host_scene_sweep_sphere_filtered")
    lib = p3d.lib()
    for name in names:
        assert hasattr(lib, name), name
        assert name in p3d.EXPORTS_ADDED and name in p3d.PROTOTYPES and name not in p3d.EXPORTS, name
    assert [len(p3d.PROTOTYPES[name][1]) for name in names] == [15, 16, 12, 13]
    assert lib.p3d_abi_version() == 4 and p3d.FILTER_SKIP_MAX == 8
    for fn in ("nearest_k_filtered_device", "sweep_sphere_filtered_device", "host_nearest_k_filtered", "host_sweep_sphere_filtered"):
        assert callable(getattr(p3d, fn)), fn
        assert not hasattr(p3d.DeviceScene, fn) and not hasattr(p3d.HostScene, fn), fn
    assert lib.p3d_nearest_k_filtered_device(None, p3d.ACCEL_BVH, 4, 2, None, None, None, 0, None, *([None] * 6)) == INVALID
    assert b"p3d_nearest_k_filtered_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_sweep_sphere_filtered_device(None, p3d.ACCEL_BVH, 4, None, None, None, None, None, 0, None, *([None] * 6)) == INVALID
    assert b"p3d_sweep_sphere_filtered_device" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_host_scene_nearest_k_filtered(None, 0, 2, None, None, None, 0, None, *([None] * 4)) == INVALID
    assert b"p3d_host_scene_nearest_k_filtered" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()
    assert lib.p3d_host_scene_sweep_sphere_filtered(None, 0, None, None, None, None, None, 0, None, *([None] * 4)) == INVALID
    assert b"p3d_host_scene_sweep_sphere_filtered" in lib.p3d_last_error() and b"null scene" in lib.p3d_last_error()


# ---- 1. the host forms against the float64 models of the thinned scene ----------------------------------------------------------

@pytest.fixture(scope="module")
def nearest_worlds(tmp_path_factory, tri5k_path):
    """name -> (host scene, model objects, points, the model's table, its smallest distances sorted, the 16 nearest objects)"""
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("filter_nearest")), tri5k=tri5k_path)
    out = {}
    for name in NEAREST_SCENES:
        objs = ref.load_objects(paths[name])
        pts = near.scene_points(objs, SEED[name])
        tab = near.table(objs, pts)
        nearest = np.argsort(tab, axis=0, kind="stable")[:16].T
        out[name] = (p3d.HostScene(paths[name]), objs, pts, tab, nk.sorted_table(tab), nearest)
    return out


def assert_names_no_skipped_object(obj, named, what):
    """obj (n,) or (n, k), -1: no answer; named: filter_reference.skipped's table"""
    rows = np.broadcast_to(np.arange(len(obj)).reshape((-1,) + (1,) * (obj.ndim - 1)), obj.shape)
    found = obj >= 0
    assert not named[obj[found], rows[found]].any(), what + ": a skipped object is in the answer"


@pytest.mark.parametrize("k", nk.KS)
@pytest.mark.parametrize("name", NEAREST_SCENES)
def test_the_host_nearest_form_is_the_model_of_the_thinned_scene(name, k, nearest_worlds):
    hs, objs, pts, tab, srt, nearest = nearest_worlds[name]
    n = len(pts)
    limits = nk.draw_k_limits(srt, k, SEED[name] + 50 + k)
    changed = 0
    for n_skip in fr.N_SKIPS:
        for ranged in (False, True):
            skip, skip_range = fr.draw(n, len(objs), n_skip, ranged, SEED[name] + 7 * n_skip + ranged, answers=nearest)
            named = fr.skipped(len(objs), n, skip, skip_range)
            thinned = np.where(named, np.inf, tab)
            for lim in (None, limits):
                what = "%s, k = %d, n_skip = %d%s%s" % (name, k, n_skip, ", a range" if ranged else "", ", limits" if lim is not None else "")
                got = p3d.host_nearest_k_filtered(hs, pts, k, max_dist=lim, skip=skip, skip_range=skip_range)
                # (without a limit the model's count is the survivors': an infinite limit says that to count_bounds)
                nk.check_k(objs, pts, k, np.full(n, np.inf, np.float32) if lim is None else lim, got, what, tab=thinned)
                assert_names_no_skipped_object(got[1], named, what)
                changed += int((got[1] != hs.nearest_k(pts, k, max_dist=lim)[1]).any(1).sum())
    assert changed > n, "%s: the filters changed hardly an answer" % name


@pytest.fixture(scope="module")
def sweep_paths(tmp_path_factory):
    return sw.scene_paths(tmp_path_factory.mktemp("filter_sweep"))


@pytest.mark.parametrize("name", list(sw.SCENES))
def test_the_host_sweep_form_is_the_model_of_the_thinned_scene(name, sweep_paths):
    """The scenes, sets and tolerances of test_sweep_api.py.  A ball whose obstacle in front is skipped flies on, and in the scenes
    with planes it may meet the next plane tens of thousands of units out or at a grazing angle, where float32 cannot hold the
    answer to tolerances that are relative to max(1, r) and max(1, T) (filter_reference.holds_in_float32): such a ball keeps its place in the batch with a
    filter that names nothing, and the test counts how many there are"""
    c = sw.cases(sweep_paths[name], sw.SCENES[name][0] + 500)
    hs = p3d.HostScene(sweep_paths[name])
    n, n_objs = len(c.o), len(c.objects)
    first = sw.first_contact(c.free_T)[0][:, None]
    # (the model's unlimited window ends a hundred scene sizes out; where a ball gets to behind it, a longer window says)
    reach = 1e8 / np.maximum(np.linalg.norm(c.d.astype(np.float64), axis=1), 1e-30)
    T_far = sw.table(c.objects, c.o, c.d, c.r, reach)[0]
    changed = 0
    for n_skip in fr.N_SKIPS:
        for ranged in (False, True):
            skip, skip_range = fr.draw(n, n_objs, n_skip, ranged, sw.SCENES[name][0] + 7 * n_skip + ranged, answers=first)
            far = ~fr.holds_in_float32(c.objects, fr.masked(T_far, skip, skip_range, np.nan), c.o, c.d, c.r, sw.TOL["at_radius"], sw.TOL["t"])
            assert far.sum() <= n // 50, "%s: %d balls fly out of float32's reach" % (name, far.sum())
            skip, skip_range = fr.emptied(skip, skip_range, far)
            named = fr.skipped(n_objs, n, skip, skip_range)
            for lim, T, margin in ((None, c.free_T, c.free_margin), (c.limits, c.lim_T, c.lim_margin)):
                what = "%s, n_skip = %d%s%s" % (name, n_skip, ", a range" if ranged else "", ", limits" if lim is not None else "")
                got = p3d.host_sweep_sphere_filtered(hs, c.o, c.d, c.r, t_max=lim, skip=skip, skip_range=skip_range)
                # (the margin is that of the whole scene: a grazing pass of a skipped object leaves a case out that need not be)
                err, _ = sw.check_sweep(c.objects, c.o, c.d, c.r, np.where(named, np.nan, T), margin, got, what)
                print("%s: %d balls with an emptied filter" % (what, far.sum()))
                sw.assert_within(err, what)
                assert_names_no_skipped_object(got[0], named, what)
                changed += int((got[0] != p3d.host_sweep_sphere(hs, c.o, c.d, c.r, t_max=lim)[0]).sum())
    assert changed > n // 2, "%s: the filters changed hardly an answer" % name


# ---- 2. a list alone: the unfiltered rows without the skipped objects, every bit -------------------------------------------------

@pytest.mark.parametrize("name", NEAREST_SCENES)
def test_a_skip_list_takes_rows_out_of_the_longer_unfiltered_list(name, nearest_worlds):
    hs, objs, pts, tab, srt, nearest = nearest_worlds[name]
    for k, n_skip in ((1, 1), (1, 8), (4, 8), (8, 8), (15, 1), (5, 3)):
        skip, _ = fr.draw(len(pts), len(objs), n_skip, False, SEED[name] + k, answers=nearest)
        for lim in (None, nk.draw_k_limits(srt, k + n_skip, SEED[name] + 90 + k)):
            want = fr.without(hs.nearest_k(pts, k + n_skip, max_dist=lim), skip, k)
            got = p3d.host_nearest_k_filtered(hs, pts, k, max_dist=lim, skip=skip)
            for a, b, what in zip(got, want, ("count", "object", "dist", "closest")):
                assert a.dtype == b.dtype and as_bytes(a) == as_bytes(b), "%s, k = %d, n_skip = %d: %s" % (name, k, n_skip, what)


# ---- 3. filters that name nothing, and one that names everything --------------------------------------------------------------------

def same(a, b, what):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and as_bytes(x) == as_bytes(y), what


def test_filters_that_name_nothing_change_no_bit(nearest_worlds, sweep_paths):
    hs, objs, pts, tab, srt, _ = nearest_worlds["mixed"]
    n, n_objs = len(pts), len(objs)
    rng = np.random.default_rng(5)
    nothing = {
        "absent": {},
        "no columns": dict(skip=np.zeros((n, 0), np.int32)),
        "all -1": dict(skip=np.full((n, 8), -1, np.int32)),
        "past the object count": dict(skip=rng.integers(n_objs, 2 ** 31 - 1, (n, 5)).astype(np.int32)),
        "negative entries": dict(skip=rng.integers(-2 ** 31, 0, (n, 3)).astype(np.int32)),
        "count <= 0": dict(skip_range=np.stack([rng.integers(0, n_objs, n), rng.integers(-5, 1, n)], 1).astype(np.int32)),
        "a range outside": dict(skip=np.full((n, 1), -1, np.int32), skip_range=np.stack([np.full(n, n_objs), np.full(n, 2 ** 31 - 1)], 1).astype(np.int32)),
        "a range that ends below 0": dict(skip_range=np.stack([np.full(n, -2 ** 31), np.full(n, 2 ** 31 - 1)], 1).astype(np.int32)),
    }
    c = sw.cases(sweep_paths["mixed"], sw.SCENES["mixed"][0] + 500)
    hs_sweep = p3d.HostScene(sweep_paths["mixed"])
    assert len(c.o) == n and len(c.objects) <= n_objs  # the same filters serve both: what is past one scene's count is past the other's
    for what, filt in nothing.items():
        for k in (1, 4, 16):
            for lim in (None, nk.draw_k_limits(srt, k, 3)):
                same(p3d.host_nearest_k_filtered(hs, pts, k, max_dist=lim, **filt), hs.nearest_k(pts, k, max_dist=lim), "nearest, %s, k = %d" % (what, k))
        for lim in (None, c.limits):
            same(p3d.host_sweep_sphere_filtered(hs_sweep, c.o, c.d, c.r, t_max=lim, **filt), p3d.host_sweep_sphere(hs_sweep, c.o, c.d, c.r, t_max=lim), "sweep, " + what)
    # everything skipped: the exact no-answer values
    for whole in (np.stack([np.zeros(n), np.full(n, n_objs)], 1), np.stack([np.full(n, -7), np.full(n, 2 ** 31 - 1)], 1)):
        whole = whole.astype(np.int32)
        count, obj, dist, closest = p3d.host_nearest_k_filtered(hs, pts, 4, skip_range=whole)
        assert not count.any() and (obj == -1).all() and (dist == FLT_MAX).all() and as_bytes(closest) == as_bytes(np.zeros((n, 4, 3), np.float32))
        obj, t, centre, contact = p3d.host_sweep_sphere_filtered(hs_sweep, c.o, c.d, c.r, skip_range=whole)
        assert (obj == -1).all() and (t == FLT_MAX).all() and as_bytes(centre) == as_bytes(np.zeros((n, 3), np.float32)) and as_bytes(contact) == as_bytes(centre)


# ---- 4. self-contact ------------------------------------------------------------------------------------------------------------------

def test_a_vertex_of_the_mesh_finds_its_neighbours_and_a_sphere_not_itself():
    hs = p3d.HostScene(os.path.join(GOLDEN_SCENES, MESH), legacy_f11=True)
    a = hs.arrays()
    points, incident = fr.mesh_vertices(a["prim_type"], a["prim_v"])
    assert len(points) >= 64, "%s: %d vertices with at most 8 triangles round them, a wave needs 64" % (MESH, len(points))
    assert ((incident >= 0).sum(1) >= 1).all() and ((incident >= 0).sum(1) > 2).any()
    obj, dist, _ = hs.nearest(points)
    assert (dist == 0).all() and (obj[:, None] == incident).any(1).all(), MESH + ": unfiltered, a vertex finds a triangle of its own at distance 0"
    objs = fr.objects_of(a)
    thinned = fr.masked(near.table(objs, points), incident, None, np.inf)
    got = p3d.host_nearest_k_filtered(hs, points, 1, skip=incident)
    assert not (got[1] == incident).any() and (got[0] == 1).all(), MESH + ": filtered, a vertex still finds a triangle of its own"
    nk.check_k(objs, points, 1, np.full(len(points), np.inf, np.float32), got, MESH + ", its own vertices", tab=thinned)
    assert (got[2] > 0).sum() > len(points) // 2  # (a triangle that touches the vertex without owning it - a T-junction - is a neighbour too)

    balls = p3d.HostScene(os.path.join(GOLDEN_SCENES, BALLS))
    b = balls.arrays()
    spheres = np.nonzero(b["prim_type"] == 0)[0].astype(np.int32)
    assert len(spheres) >= 8
    centre, radius = b["prim_v"][spheres, :3].astype(np.float32), b["prim_v"][spheres, 3].astype(np.float32)
    d = np.tile(np.array([[0.3, -0.2, 0.1]], np.float32), (len(spheres), 1))
    obj, t, _, _ = p3d.host_sweep_sphere(balls, centre, d, radius)
    # (T = 0 for all; spheres that overlap tie at 0 and the lower index wins: those that report themselves are the test's)
    own = obj == spheres
    assert (t == 0).all() and own.sum() >= 4, BALLS + ": unfiltered, a sphere swept from its own centre meets itself at T = 0"
    got = p3d.host_sweep_sphere_filtered(balls, centre, d, radius, skip=spheres[:, None])
    assert (got[0] != spheres).all(), BALLS + ": filtered, a sphere still meets itself"
    ranged = p3d.host_sweep_sphere_filtered(balls, centre, d, radius, skip_range=np.stack([spheres, np.ones_like(spheres)], 1))
    same(ranged, got, BALLS + ": a range of one is that list")
    objects = fr.objects_of(b)
    met = 0
    for i, own_index in enumerate(spheres):  # the model of the scene without that sphere, one ball each (its margin then is not the sphere's own 0)
        others = [j for j in range(len(objects)) if j != own_index]
        T, margin = sw.table([objects[j] for j in others], centre[i:i + 1], d[i:i + 1], radius[i:i + 1])
        one = tuple(x[i:i + 1].copy() for x in got)
        if one[0][0] >= 0:
            one[0][0] = others.index(int(one[0][0]))
            met += 1
        if margin[0] >= sw.THRESHOLD:
            err, _ = sw.check_sweep([objects[j] for j in others], centre[i:i + 1], d[i:i + 1], radius[i:i + 1], T, margin, one, "%s, sphere %d" % (BALLS, own_index), mixed=False)
            sw.assert_within(err, "%s, sphere %d" % (BALLS, own_index))
            assert one[0][0] == sw.first_contact(T)[0][0]
    assert met > 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------

def test_refusals(tmp_path, nearest_worlds):
    hs, objs, pts, *_ = nearest_worlds["mixed"]
    lib = p3d.lib()
    n = 4
    p = np.ascontiguousarray(pts[:n])
    count, obj = np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
    nine = np.full((n, 9), -1, np.int32)
    o, d, r = p, np.ones((n, 3), np.float32), np.ones(n, np.float32)
    nearest = lambda skip, n_skip, rows=n: lib.p3d_host_scene_nearest_k_filtered(hs._h, rows, 2, p.ctypes.data, None, skip, n_skip, None, count.ctypes.data, obj.ctypes.data, None, None)
    (tmp_path / "plain.p3f").write_text(ref.HEAD + "s 0 0 0 1\ns 3 0 0 1\n")
    plain = p3d.HostScene(str(tmp_path / "plain.p3f"))
    sweep = lambda skip, n_skip, rows=n, scene=plain: lib.p3d_host_scene_sweep_sphere_filtered(scene._h, rows, o.ctypes.data, d.ctypes.data, r.ctypes.data, None, skip, n_skip, None, count.ctypes.data, None, None, None)
    for call, name in ((nearest, b"p3d_host_scene_nearest_k_filtered"), (sweep, b"p3d_host_scene_sweep_sphere_filtered")):
        assert call(nine.ctypes.data, 9) == INVALID and name in lib.p3d_last_error() and b"n_skip must be" in lib.p3d_last_error()
        assert call(nine.ctypes.data, 9, 0) == INVALID  # whatever n
        assert call(None, 3) == INVALID and name in lib.p3d_last_error() and b"null skip" in lib.p3d_last_error()
        assert call(None, 0) == 0 and call(None, 3, 0) == 0, lib.p3d_last_error()  # no list needs no pointer, and no rows none either
    with pytest.raises(p3d.P3DError) as e:
        p3d.host_nearest_k_filtered(hs, p, 2, skip=nine)
    assert e.value.code == INVALID and "n_skip must be" in str(e.value)
    (tmp_path / "boxed.p3f").write_text(ref.HEAD + "s 0 0 0 1\nbox -1 3 -1 1 5 1\n")
    boxed = p3d.HostScene(str(tmp_path / "boxed.p3f"))
    with pytest.raises(p3d.P3DError) as e:  # the box is refused although the filter names it
        p3d.host_sweep_sphere_filtered(boxed, o, d, 1.0, skip=np.ones((n, 1), np.int32))
    assert e.value.code == UNSUPPORTED and "object 1 is a box" in str(e.value)
    assert sweep(None, 0, 0, boxed) == UNSUPPORTED
    # the tensor wrappers, before the library is called
    import torch
    raw = (0x1000, 6)
    dev = scene_without_a_library()
    q, s = p3d.nearest_k_filtered_device, p3d.sweep_sphere_filtered_device
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    cases = [
        ("a raw list without its width", INVALID, "needs n_skip", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=raw)),
        ("a CPU list", INVALID, "skip: the tensor is in host memory", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=i32(6, 3))),
        ("a flat list", INVALID, "skip: shape", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=i32(6))),
        ("a float list", INVALID, "skip: dtype", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=i32(6, 3).float())),
        ("a list of other rows", INVALID, "6 points, 5 skip rows", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=(0x2000, 5), n_skip=3)),
        ("a width that is not the tensor's", INVALID, "n_skip says 2", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip=i32(6, 3), n_skip=2)),
        ("an (n, 3) range", INVALID, "skip_range: shape", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip_range=i32(6, 3))),
        ("ranges of other rows", INVALID, "6 points, 5 skip ranges", lambda: q(dev, p3d.ACCEL_BVH, raw, 2, skip_range=(0x2000, 5))),
        ("k = 17", INVALID, "k must be 1 .. 16", lambda: q(dev, p3d.ACCEL_BVH, raw, 17)),
        ("the sweep: a CPU range", INVALID, "skip_range: the tensor is in host memory", lambda: s(dev, p3d.ACCEL_BVH, raw, raw, raw, skip_range=i32(6, 2))),
        ("the sweep: lists of other rows", INVALID, "6 balls, 5 skip rows", lambda: s(dev, p3d.ACCEL_BVH, raw, raw, raw, skip=(0x2000, 5), n_skip=1)),
        ("the sweep: the grid", UNSUPPORTED, "grid", lambda: s(dev, p3d.ACCEL_GRID, raw, raw, raw)),
    ]
    for what, code, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == code and word in str(e.value), "%s: %s" % (what, e.value)
