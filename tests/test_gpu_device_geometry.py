"""Geometry from device memory (p3d_scene_update_geometry_device) on the GPU.

The yardstick is exact, as for the transform route: what the device route (torch tensors -> one kernel -> BVH / grid work)
leaves must be, bit for bit, what the host route leaves for the same float32 numbers (p3d.deformed -> HostScene.set_geometry
-> update_prims, same mode) on a twin scene: colours as uint32, hit IDs, the counters of test_gpu_scene_transform.py, the
exported tree and the exported grid.  Every comparison here has tolerance 0.  No triangle here is degenerate (the one case
whose normal bits are unspecified).  The sub-check "a second call of the same size allocates nothing" is not asserted: the
transform tests have no instrument for it either; the staging is reused by construction (Scratch::ensure)."""
import ctypes as C

import numpy as np
import pytest
import torch

from device_geometry_helpers import deformed_mesh, diagonal, moved_spheres
from frame_checks import CORNELL, assert_same_frames, assert_same_tree, frames, frames_differ, gpu, load
from live_scene_checks import GRID_SCENES, IDENTITY, LEAF, RES, assert_same_scene, configs, device, host_route, rigid
import p3d_amd as p3d
from scene_update_helpers import SPHERE, TRIANGLE, translated
from variant_scenes import scene_path

pytestmark = pytest.mark.gpu

MODES = [p3d.UPDATE_REFIT, p3d.UPDATE_REBUILD]


@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "cornell": CORNELL}


def twins(path, name):
    """(host scene, its arrays, scene A for the host route, scene B for the device route)"""
    hs = load(path, RES)
    return hs, hs.arrays(), device(hs, name), device(hs, name)


def host_triangles(hs, dev, a, first, positions, indices, mode, only=None):
    objs, rows = p3d.deformed(a["prim_v"], first, positions, indices)
    if only is not None:
        objs, rows = objs[only], rows[only]
    hs.set_geometry(objs, rows)
    return dev.update_prims(objs, mode)


def host_spheres(hs, dev, a, first, cr, mode, only=None):
    objs, rows = p3d.deformed_spheres(a["prim_v"], first, cr)
    if only is not None:
        objs, rows = objs[only], rows[only]
    hs.set_geometry(objs, rows)
    return dev.update_prims(objs, mode)


def assert_same(dev_a, dev_b, name, what):
    """Frames with the BVH in both stack modes (or the path-traced frame), tree, and for the scenes with a device grid the
    grid and the frames through it in both stack modes -> B's BVH frames"""
    now = assert_same_scene(dev_a, dev_b, name, what)
    if name in GRID_SCENES:
        assert_same_frames(frames(dev_a, configs(name, p3d.ACCEL_GRID)), frames(dev_b, configs(name, p3d.ACCEL_GRID)), what + ", grid frames")
    return now


# 1. soup, whole mesh
@pytest.mark.parametrize("mode", MODES)
def test_a_soup_of_the_whole_mesh(mode, paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    before = frames(dev_b, configs("tri5k"))
    _, _, soup = deformed_mesh(a, seed=11)
    moved = np.linalg.norm(soup.astype(np.float64) - a["prim_v"].reshape(-1, 3), axis=1).max()
    assert 0 < moved <= 0.02 * diagonal(a) * (1 + 1e-6)
    assert host_triangles(hs, dev_a, a, 0, soup, None, mode) > 0
    assert dev_b.update_triangles(0, gpu(soup), mode=mode) > 0
    now = assert_same(dev_a, dev_b, "tri5k", "soup, mode %d" % mode)
    assert frames_differ(now, before), "the deformation changed no pixel"
    assert dev_b.status() == 0


# 2. indexed, shared vertices
@pytest.mark.parametrize("dtype", [np.int32, np.uint32])
def test_indexed_equals_the_soup(dtype, paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    pos, idx, soup = deformed_mesh(a, seed=11)
    host_triangles(hs, dev_a, a, 0, soup, None, p3d.UPDATE_REBUILD)  # case 1's host route
    d_idx = gpu(idx.astype(dtype))
    assert d_idx.dtype == (torch.int32 if dtype is np.int32 else torch.uint32)
    assert dev_b.update_triangles(0, gpu(pos), d_idx, mode=p3d.UPDATE_REBUILD) > 0
    assert_same(dev_a, dev_b, "tri5k", "indexed, %s" % dtype.__name__)


def test_vertices_shared_between_triangles(paths):
    """Triangles 1000 .. 1063 are welded into a fan around one position, and 2000 .. 2009 reuse the corners of triangle 5"""
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    pos, idx, _ = deformed_mesh(a, seed=12)
    idx = idx.copy()
    idx[1000:1064, 0] = idx[999, 0]
    idx[2000:2010, 1:] = idx[5, 1:]
    assert len(np.unique(idx)) < idx.size
    host_triangles(hs, dev_a, a, 0, pos, idx, p3d.UPDATE_REFIT)
    dev_b.update_triangles(0, gpu(pos), gpu(idx.astype(np.int32)), mode=p3d.UPDATE_REFIT)
    assert_same(dev_a, dev_b, "tri5k", "welded triangles")


# 3. ranges and block edges
def test_sources_in_descending_order_and_untouched_objects(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    n = a["n_prims"]
    pos, idx, soup = deformed_mesh(a, seed=13, fraction=0.01)
    spans = [(0, 1), (10, 63), (100, 64), (200, 65), (n - 257, 257)]  # one object, a wave's end either side, a block + 1
    covered = np.zeros(n, bool)
    for first, count in spans:
        covered[first:first + count] = True
    tree0 = dev_b.export_bvh()
    keep = []  # the tensors live until the call has returned
    meshes = []
    for k, (first, count) in enumerate(spans):
        if k % 2:  # indexed into the whole position array
            host_triangles(hs, dev_a, a, first, pos, idx[first:first + count], p3d.UPDATE_REFIT)
            keep.append((gpu(pos), gpu(idx[first:first + count].astype(np.int32))))
        else:      # a soup of its own
            part = soup[3 * first:3 * (first + count)]
            host_triangles(hs, dev_a, a, first, part, None, p3d.UPDATE_REFIT)
            keep.append((gpu(part),))
        meshes.append((first,) + keep[-1])
    meshes.reverse()
    assert [m[0] for m in meshes] == sorted((m[0] for m in meshes), reverse=True)
    assert dev_b.update_triangles(meshes, mode=p3d.UPDATE_REFIT) > 0
    now = assert_same(dev_a, dev_b, "tri5k", "five sources")
    # the uncovered objects keep their exact bits: every leaf of the (refitted: same topology) tree that holds none of the
    # covered objects has the box it had
    tree1 = dev_b.export_bvh()
    for k in ("bvh_index", "bvh_count_leaf", "bvh_order"):
        assert np.array_equal(tree0[k], tree1[k]), k
    leaves = np.nonzero(tree1["bvh_count_leaf"] & LEAF)[0]
    untouched = [l for l in leaves
                 if not covered[tree1["bvh_order"][tree1["bvh_index"][l]:tree1["bvh_index"][l] + (tree1["bvh_count_leaf"][l] & ~LEAF)]].any()]
    assert len(untouched) > len(leaves) // 2
    for k in ("bvh_bmin", "bvh_bmax"):
        assert tree0[k][untouched].tobytes() == tree1[k][untouched].tobytes(), k
    kept = set(untouched)
    moved = [l for l in leaves if l not in kept]
    assert tree0["bvh_bmin"][moved].tobytes() != tree1["bvh_bmin"][moved].tobytes()
    # ... and the frames above are those of scene A, whose uncovered objects no update has ever written


# 4. spheres
@pytest.mark.parametrize("mode", MODES)
def test_spheres(mode, paths):
    hs, a, dev_a, dev_b = twins(paths["balls_low"], "balls_low")
    spheres = np.nonzero(a["prim_type"] == SPHERE)[0]
    first, count = int(spheres[0]), len(spheres)
    before = frames(dev_b, configs("balls_low"))
    cr = moved_spheres(a, first, count, seed=21)
    assert host_spheres(hs, dev_a, a, first, cr, mode) > 0
    assert dev_b.update_spheres(first, gpu(cr), mode=mode) > 0
    now = assert_same(dev_a, dev_b, "balls_low", "spheres, mode %d" % mode)
    assert frames_differ(now, before)


def test_triangles_and_spheres_in_one_call(paths):
    hs, a, dev_a, dev_b = twins(paths["cornell"], "cornell")
    kinds = a["prim_type"]
    tri, sph = np.nonzero(kinds == TRIANGLE)[0], np.nonzero(kinds == SPHERE)[0]
    t0, s0 = int(tri[0]), int(sph[0])
    assert np.array_equal(tri, np.arange(t0, t0 + len(tri))) and np.array_equal(sph, np.arange(s0, s0 + len(sph)))
    before = frames(dev_b, configs("cornell"))
    rng = np.random.default_rng(22)
    soup = a["prim_v"][tri].reshape(-1, 3).astype(np.float64)
    soup = (soup + rng.uniform(-1, 1, soup.shape) * 0.01 * diagonal(a, tri)).astype(np.float32)
    cr = moved_spheres(a, s0, len(sph), seed=23)
    host_triangles(hs, dev_a, a, t0, soup, None, p3d.UPDATE_REFIT)
    host_spheres(hs, dev_a, a, s0, cr, p3d.UPDATE_REFIT)
    d_soup, d_cr = gpu(soup), gpu(cr)
    assert dev_b.update_geometry_device([dev_b.sphere_source(s0, d_cr), dev_b.triangle_source(t0, d_soup)], p3d.UPDATE_REFIT) > 0
    # (A took two refits, B one: a refit depends on the boxes alone)
    now = assert_same(dev_a, dev_b, "cornell", "triangles and spheres")
    assert frames_differ(now, before)


# 5. per-object failures
def test_failed_objects_keep_their_geometry(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    n = a["n_prims"]
    pos, idx, _ = deformed_mesh(a, seed=31)
    idx = idx.copy()
    idx[100:105, 0] = idx[50, 0]       # 50 and 100 .. 104 share one position ...
    clean_pos, clean_idx = pos.copy(), idx.copy()
    pos[idx[50, 0]] = np.nan           # ... which is NaN
    idx[7, 1] = idx[4000, 2] = len(pos)  # two triangles with an index == n_elems
    nan_set, oob_set = [50, 100, 101, 102, 103, 104], [7, 4000]
    ok = np.ones(n, bool)
    ok[nan_set + oob_set] = False
    host_triangles(hs, dev_a, a, 0, clean_pos, clean_idx, p3d.UPDATE_REBUILD, only=ok)  # the other objects only
    with pytest.raises(p3d.P3DError) as e:
        dev_b.update_triangles(0, gpu(pos), gpu(idx.astype(np.uint32)), mode=p3d.UPDATE_REBUILD)
    assert e.value.code == -1, e.value
    assert "%d triangle(s) with an index" % len(oob_set) in str(e.value) and "%d object(s) with a non-finite" % len(nan_set) in str(e.value), e.value
    assert dev_b.status() == 0
    assert_same(dev_a, dev_b, "tri5k", "two bad indices and a NaN position")
    assert hs.arrays()["prim_v"][~ok].tobytes() == a["prim_v"][~ok].tobytes()  # (what A holds for the failed ones: the old bits)
    # the scene goes on: the next update is exact again
    _, _, soup = deformed_mesh(a, seed=32)
    host_triangles(hs, dev_a, a, 0, soup, None, p3d.UPDATE_REFIT)
    dev_b.update_triangles(0, gpu(soup), mode=p3d.UPDATE_REFIT)
    assert_same(dev_a, dev_b, "tri5k", "after the failures")


@pytest.mark.parametrize("radius", [-0.25, float("nan")])
def test_a_sphere_with_a_bad_radius_keeps_its_geometry(radius, paths):
    hs, a, dev_a, dev_b = twins(paths["balls_low"], "balls_low")
    spheres = np.nonzero(a["prim_type"] == SPHERE)[0]
    first, count = int(spheres[0]), len(spheres)
    cr = moved_spheres(a, first, count, seed=33)
    ok = np.ones(count, bool)
    ok[3] = False
    host_spheres(hs, dev_a, a, first, cr, p3d.UPDATE_REFIT, only=ok)
    cr[3, 3] = radius
    with pytest.raises(p3d.P3DError) as e:
        dev_b.update_spheres(first, gpu(cr), mode=p3d.UPDATE_REFIT)
    assert e.value.code == -1 and "0 triangle(s)" in str(e.value) and "1 object(s) with a non-finite or inverted box" in str(e.value), e.value
    assert_same(dev_a, dev_b, "balls_low", "one bad radius")


# 6. refusals, nothing changed
def _raw(dev, sources, mode=p3d.UPDATE_REFIT, n=None, null=False):
    arr = (p3d.GeomSource * max(len(sources), 1))(*sources)
    ms = C.c_float(-1.0)
    return p3d.lib().p3d_scene_update_geometry_device(dev._h if dev is not None else None, len(sources) if n is None else n,
                                                      None if null else C.cast(arr, C.c_void_p), mode, C.byref(ms))


def test_refusals_leave_the_scene_as_it_was(paths):
    name = "balls_low"
    hs = load(paths[name], RES)
    a = hs.arrays()
    n = a["n_prims"]
    tri, sph = np.nonzero(a["prim_type"] == TRIANGLE)[0], np.nonzero(a["prim_type"] == SPHERE)[0]
    t0, nt, s0, ns = int(tri[0]), len(tri), int(sph[0]), len(sph)
    assert t0 + nt == s0 and s0 + ns == n and nt >= 2 and ns >= 4
    dev = p3d.DeviceScene(hs, bvh="device")  # (before the host scene builds a grid: its descriptor carries one from then on)
    host_tree = p3d.DeviceScene(hs, bvh=True)
    with_grid = p3d.DeviceScene(hs, bvh="device", grid=True)
    cr = gpu(moved_spheres(a, s0, ns, seed=41))
    soup = gpu((a["prim_v"][tri].reshape(-1, 3) * np.float32(1.01)).astype(np.float32))
    index = gpu(np.arange(3 * nt, dtype=np.int32).reshape(-1, 3))
    host_cr = np.ascontiguousarray(moved_spheres(a, s0, ns, seed=41))  # numpy arrays: host memory
    host_index = np.arange(3 * nt, dtype=np.uint32)
    S, TRI = SPHERE, TRIANGLE

    def src(first, count, kind, n_elems, data, index=None, reserved=(0, 0)):
        return p3d.GeomSource(first, count, kind, n_elems, data, index, (C.c_uint64 * 2)(*reserved))

    good = [src(s0, ns, S, ns, cr.data_ptr())]
    for what, scene in (("a scene with the host's tree", host_tree), ("a scene with an uploaded grid", with_grid)):
        was = frames(scene, configs(name))
        assert _raw(scene, good) == -1, what
        assert_same_frames(frames(scene, configs(name)), was, what)
    assert _raw(None, good) == -1
    was, tree = frames(dev, configs(name)), dev.export_bvh()
    # Host memory must be refused BEFORE any launch.  Each such source goes in twice first: were the pointer check to let it
    # through, the overlap (found behind it) would still refuse the call, and no kernel would ever be given a host address.
    for what, bad in (("d_data", src(s0, ns, S, ns, host_cr.ctypes.data)),
                      ("d_index", src(t0, nt, TRI, 3 * nt, soup.data_ptr(), host_index.ctypes.data))):
        assert _raw(dev, [bad, bad]) == -1
        assert b"is host memory" in p3d.lib().p3d_last_error() and what.encode() in p3d.lib().p3d_last_error(), p3d.lib().p3d_last_error()
    cases = [
        ("an unknown mode", dict(sources=good, mode=2)),
        ("null sources with a count", dict(sources=good, null=True)),
        ("an empty source", [src(s0, 0, S, 0, cr.data_ptr())]),
        ("a source behind the last object", [src(n - 1, 2, S, 2, cr.data_ptr())]),
        ("a source whose end wraps", [src(0xffffffff, 2, S, 2, cr.data_ptr())]),
        ("a kind that is neither", [src(s0, 1, 2, 1, cr.data_ptr())]),
        ("a plane's kind", [src(s0, 1, 3, 1, cr.data_ptr())]),
        ("spheres named as triangles", [src(s0, 1, TRI, 3, soup.data_ptr())]),
        ("triangles named as spheres", [src(t0, 1, S, 1, cr.data_ptr())]),
        ("a source that runs from triangles into spheres", [src(t0, nt + 1, TRI, 3 * (nt + 1), soup.data_ptr())]),
        ("null d_data", [src(s0, ns, S, ns, None)]),
        ("d_data off by two bytes", [src(s0, ns - 1, S, ns - 1, cr.data_ptr() + 2)]),
        ("d_index off by one byte", [src(t0, 1, TRI, 3 * nt, soup.data_ptr(), index.data_ptr() + 1)]),
        ("d_index given for spheres", [src(s0, ns, S, ns, cr.data_ptr(), index.data_ptr())]),
        ("n_elems 0", [src(t0, nt, TRI, 0, soup.data_ptr(), index.data_ptr())]),
        ("a soup with too few positions", [src(t0, nt, TRI, 3 * nt - 1, soup.data_ptr())]),
        ("a soup with too many positions", [src(t0, 1, TRI, 3 * nt, soup.data_ptr())]),
        ("spheres with n_elems != count", [src(s0, ns - 1, S, ns, cr.data_ptr())]),
        ("reserved[0]", [src(s0, ns, S, ns, cr.data_ptr(), reserved=(1, 0))]),
        ("reserved[1]", [src(s0, ns, S, ns, cr.data_ptr(), reserved=(0, 1 << 40))]),
        ("overlapping sources", [src(s0, 3, S, 3, cr.data_ptr()), src(s0 + 2, 2, S, 2, cr.data_ptr())]),
        ("overlapping sources, shuffled", [src(s0 + 3, 1, S, 1, cr.data_ptr()), src(s0, ns, S, ns, cr.data_ptr()), src(t0, 1, TRI, 3, soup.data_ptr())]),
        ("the same source twice", good + good),
        ("a fault in the second source", good + [src(t0, nt, TRI, 3 * nt, None)]),
        ("host memory as d_data", [src(s0, ns, S, ns, host_cr.ctypes.data)]),
        ("host memory as d_index", [src(t0, nt, TRI, 3 * nt, soup.data_ptr(), host_index.ctypes.data)]),
        # (every index in `index` is valid: if the runtime could not report the range, the kernel would still read nothing
        # outside the tensor)
        ("positions that end behind their allocation", [src(t0, nt, TRI, 1 << 28, soup.data_ptr(), index.data_ptr())]),
    ]
    for what, kw in cases:
        kw = kw if isinstance(kw, dict) else dict(sources=kw)
        assert _raw(dev, **kw) == -1, what
        assert p3d.lib().p3d_last_error().startswith(b"p3d_scene_update_geometry_device"), what
        assert_same_frames(frames(dev, configs(name)), was, what)
    assert b"ends behind its allocation" in p3d.lib().p3d_last_error()
    assert_same_tree(dev.export_bvh(), tree, "after the refusals")
    assert dev.status() == 0
    # the same calls without a fault are accepted, in any order, with update_ms == NULL
    arr = (p3d.GeomSource * 2)(src(s0, ns, S, ns, cr.data_ptr()), src(t0, nt, TRI, 3 * nt, soup.data_ptr(), index.data_ptr()))
    assert p3d.lib().p3d_scene_update_geometry_device(dev._h, 2, C.cast(arr, C.c_void_p), p3d.UPDATE_REBUILD, None) == 0
    assert frames_differ(frames(dev, configs(name)), was)


# 7. rest pose
def test_a_deformed_object_rests_where_it_is_put(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    n = a["n_prims"]
    move = rigid(a, np.random.default_rng(51))
    for dev in (dev_a, dev_b):
        dev.transform_prims([(0, n, 0)], move[None], p3d.UPDATE_REFIT)  # makes the rest copy
    moved = frames(dev_b, configs("tri5k"))
    first, count = 300, 700
    _, _, soup = deformed_mesh(a, seed=52)
    part = soup[3 * first:3 * (first + count)]
    host_triangles(hs, dev_a, a, first, part, None, p3d.UPDATE_REFIT)
    dev_b.update_triangles(first, gpu(part), mode=p3d.UPDATE_REFIT)
    deformed = assert_same(dev_a, dev_b, "tri5k", "a deformation after a transform")
    assert frames_differ(deformed, moved)
    for dev in (dev_a, dev_b):
        dev.transform_prims([(first, count, 0)], IDENTITY[None], p3d.UPDATE_REFIT)
    back = assert_same(dev_a, dev_b, "tri5k", "the identity on the deformed objects")
    # the deformed geometry, not the original one (the identity of the ORIGINAL rest pose would show the unmoved triangles)
    assert_same_frames(back, deformed, "the identity returns what the device update put there")


# 8. policy and bookkeeping
def test_a_refit_the_policy_promotes(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    dev_c = device(hs, "tri5k")
    n = a["n_prims"]
    rng = np.random.default_rng(61)
    # every triangle thrown somewhere else in the scene: the refitted tree is far worse than a built one
    jump = rng.uniform(-0.4, 0.4, (n, 1, 3)) * diagonal(a)
    soup = (a["prim_v"].reshape(n, 3, 3).astype(np.float64) + jump).astype(np.float32).reshape(-1, 3)
    ratio = 1.0 + 1e-6
    for dev in (dev_a, dev_b):
        dev.set_auto_rebuild(ratio)
    dev_c.set_auto_rebuild(ratio)
    host_triangles(hs, dev_a, a, 0, soup, None, p3d.UPDATE_REFIT)
    assert dev_a.bvh_cost()["last_update_rebuilt"] == 1, "the deformation is too small: the host route's REFIT was not promoted"
    d_soup = gpu(soup)
    dev_b.update_triangles(0, d_soup, mode=p3d.UPDATE_REFIT)
    dev_c.update_triangles(0, d_soup, mode=p3d.UPDATE_REBUILD)
    cost_a, cost_b, cost_c = dev_a.bvh_cost(), dev_b.bvh_cost(), dev_c.bvh_cost()
    assert cost_b["last_update_rebuilt"] == 1 and cost_b["refits_since_build"] == 0
    assert cost_a == cost_b == cost_c, (cost_a, cost_b, cost_c)
    assert_same(dev_a, dev_b, "tri5k", "a promoted refit, host and device route")
    assert_same_tree(dev_b.export_bvh(), dev_c.export_bvh(), "a promoted refit and a rebuild")
    # a small deformation afterwards, under a ratio it cannot reach, is a plain refit on both routes
    for dev in (dev_a, dev_b):
        dev.set_auto_rebuild(4.0)
    _, _, small = deformed_mesh(dict(a, prim_v=soup.reshape(-1, 9)), seed=62, fraction=0.0005)
    host_triangles(hs, dev_a, a, 0, small, None, p3d.UPDATE_REFIT)
    dev_b.update_triangles(0, gpu(small), mode=p3d.UPDATE_REFIT)
    cost_a, cost_b = dev_a.bvh_cost(), dev_b.bvh_cost()
    assert cost_a == cost_b and cost_b["last_update_rebuilt"] == 0 and cost_b["refits_since_build"] == 1, (cost_a, cost_b)
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), "a refit that stays a refit")


def test_an_accumulator_refuses_passes_until_reset(paths):
    hs = load(paths["cornell"], 64)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev.accumulator(cfg)
    acc.render(2)
    sph = np.nonzero(a["prim_type"] == SPHERE)[0]
    cr = moved_spheres(a, int(sph[0]), len(sph), seed=63)
    dev.update_spheres(int(sph[0]), gpu(cr), mode=p3d.UPDATE_REFIT)
    with pytest.raises(p3d.P3DError) as e:
        acc.render(1)
    assert e.value.code == -1 and "moved" in str(e.value)
    assert acc.samples_done == 2
    acc.reset()
    hs.set_geometry(*p3d.deformed_spheres(a["prim_v"], int(sph[0]), cr))
    fresh = p3d.DeviceScene(hs, bvh=dev.export_bvh())
    f_acc = fresh.accumulator(cfg)
    got, want = acc.render(4), f_acc.render(4)
    assert np.array_equal(got[1], want[1]) and got[0].tobytes() == want[0].tobytes()
    acc.close()
    f_acc.close()


# 9. producer on another stream
def test_positions_produced_on_another_stream(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    base = gpu(a["prim_v"].reshape(-1, 3))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wave = base
        for _ in range(200):  # some work in front of the result, so that it is still being produced when the call begins
            wave = torch.sin(wave * 1.5 + 0.25)
        pos = (base + 0.02 * wave).contiguous()
    assert dev_b.update_triangles(0, pos, mode=p3d.UPDATE_REBUILD) > 0  # no synchronize: the call's own waits cover `side`
    bits = pos.cpu().numpy()
    assert np.isfinite(bits).all() and bits.tobytes() != a["prim_v"].tobytes()
    host_triangles(hs, dev_a, a, 0, bits, None, p3d.UPDATE_REBUILD)
    assert_same(dev_a, dev_b, "tri5k", "positions from a side stream")


# 10. degenerate calls
def test_no_sources_is_update_prims_of_nothing(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"], "tri5k")
    _, _, soup = deformed_mesh(a, seed=71, fraction=0.05)
    host_triangles(hs, dev_a, a, 0, soup, None, p3d.UPDATE_REFIT)
    d_soup = gpu(soup)
    dev_b.update_triangles(0, d_soup, mode=p3d.UPDATE_REFIT)
    refitted = dev_b.export_bvh()
    dev_a.update_prims([], p3d.UPDATE_REBUILD)
    dev_b.update_geometry_device([], p3d.UPDATE_REBUILD)
    assert_same(dev_a, dev_b, "tri5k", "a rebuild of nothing")
    assert dev_b.export_bvh()["bvh_order"].tobytes() != refitted["bvh_order"].tobytes()  # (the refit had kept the old order)
    assert dev_b.bvh_cost()["last_update_rebuilt"] == 1
    assert _raw(dev_b, [], mode=p3d.UPDATE_REFIT) == 0 and _raw(dev_b, [], mode=p3d.UPDATE_REFIT, null=True) == 0
    assert dev_b.update_triangles(0, d_soup, mode=p3d.UPDATE_REFIT) > 0  # the same size again: the staging is kept
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), "the same geometry once more")


# 11. the three routes in turn, through the one staging buffer they share
def test_the_three_routes_share_one_stage(paths):
    """transform_prims (the largest payload, and it leaves a non-zero counter block behind), update_spheres (a much smaller
    one: its own upload zeroes the counters again), update_prims, update_triangles: after each, scene B is scene A, which
    took the host route.  The identity at the end reads the rest copy the last three calls wrote."""
    hs, a, dev_a, dev_b = twins(paths["cornell"], "cornell")
    kinds, n = a["prim_type"], a["n_prims"]
    tri, sph = np.nonzero(kinds == TRIANGLE)[0], np.nonzero(kinds == SPHERE)[0]
    t0, s0 = int(tri[0]), int(sph[0])
    assert len(tri) + len(sph) == n and len(sph) >= 3
    assert np.array_equal(tri, np.arange(t0, t0 + len(tri))) and np.array_equal(sph, np.arange(s0, s0 + len(sph)))
    # 1. one range per object, every range with a matrix of its own; the largest sphere overflows (a radius below 1 times a
    # finite sphere_scale stays finite, so it is also moved by 3e38, as in test_an_object_that_overflows_keeps_its_geometry)
    victim = int(sph[np.argmax(a["prim_v"][sph, 3])])
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e38) + a["prim_v"][victim, 3] * np.float32(3e38))
    rng = np.random.default_rng(81)
    xforms = np.stack([rigid(a, rng, reach=0.02 + 0.002 * i) for i in range(n)])
    xforms[victim] = IDENTITY
    xforms[victim][:, 3] = 3e38
    scale = np.full(n, 1.25, np.float32)
    scale[victim] = 3e38
    ranges = [(i, 1, i) for i in range(n)]
    host_route(hs, dev_a, a, [r for r in ranges if r[0] != victim], xforms, scale, p3d.UPDATE_REFIT)  # A: the victim is left out
    with pytest.raises(p3d.P3DError) as e:
        dev_b.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    assert e.value.code == -1 and "1 object" in str(e.value), e.value
    moved = assert_same(dev_a, dev_b, "cornell", "step 1: a transform per object, one sphere overflows")
    # 2. two spheres with valid radii: returns normally
    cr = moved_spheres(a, s0, 2, seed=82)
    host_spheres(hs, dev_a, a, s0, cr, p3d.UPDATE_REFIT)
    assert dev_b.update_spheres(s0, gpu(cr), mode=p3d.UPDATE_REFIT) > 0
    now = assert_same(dev_a, dev_b, "cornell", "step 2: two spheres from device memory")
    assert frames_differ(now, moved)
    # 3. three objects from the host scene, which both scenes are bound to
    objs = np.array([t0, t0 + len(tri) // 2, s0 + 1], np.uint32)
    offsets = np.random.default_rng(83).uniform(-0.05, 0.05, (3, 3)).astype(np.float32)
    hs.set_geometry(objs, translated(kinds, hs.arrays()["prim_v"], objs, offsets))
    for dev in (dev_a, dev_b):
        assert dev.update_prims(objs, p3d.UPDATE_REBUILD) > 0
    assert_same(dev_a, dev_b, "cornell", "step 3: three records from the host")
    # 4. the whole triangle soup
    soup = a["prim_v"][tri].reshape(-1, 3).astype(np.float64)
    soup = (soup + np.random.default_rng(84).uniform(-1, 1, soup.shape) * 0.01 * diagonal(a, tri)).astype(np.float32)
    assert not (soup == 0).any()  # (1 * -0 + 0 is +0: the one value the identity below would change)
    host_triangles(hs, dev_a, a, t0, soup, None, p3d.UPDATE_REFIT)
    assert dev_b.update_triangles(t0, gpu(soup), mode=p3d.UPDATE_REFIT) > 0
    last = assert_same(dev_a, dev_b, "cornell", "step 4: the triangle soup")
    # the triangles rest where step 4 put them (not where step 3, step 1 or the scene's file had them)
    dev_b.transform_prims([(t0, len(tri), 0)], IDENTITY[None], p3d.UPDATE_REFIT)
    assert_same_frames(assert_same(dev_a, dev_b, "cornell", "the identity on the triangles"), last, "the identity moved a triangle")
    assert dev_b.status() == 0
