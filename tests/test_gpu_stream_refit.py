"""The refit of a live scene from device buffers on the caller's stream (p3d_scene_refit_device) on the GPU.

The yardstick is exact: scene B takes the stream form, its twin A takes update_triangles / update_spheres with UPDATE_REFIT
and the same float32 numbers, and the two are compared with the helpers of the device-geometry tests (frames in both stack
modes as uint32, hit IDs, counters, the exported tree).  Every comparison here has tolerance 0.  No triangle here is
degenerate.  The scenes have no device-built grid (the stream form refuses those: see the refusals).

Not asserted: that a second call allocates nothing.  There is no instrument for it; it holds by construction (the sources
travel as kernel arguments, the counter block and the builder's state are made by the first call), and the loop time of
profiles/tools/stream_refit_probe.py is the evidence."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import p3d_amd as p3d
from device_query_contract import CAPACITY, INVALID, UNSUPPORTED
from device_geometry_helpers import deformed_mesh, diagonal, moved_spheres
from scene_update_helpers import SPHERE, TRIANGLE
from frame_checks import CORNELL, RENDER_COUNTERS, assert_same_frames, assert_same_tree, frames, frames_differ, gpu, load
from live_scene_checks import (HEAD, IDENTITY, LEAF, RES, TRACE_OUT, assert_same_frames_and_tree, camera_rays, configs, kinds_of,
                               last_error, produced, rigid, scene, trace_outputs)
from variant_scenes import scene_path

pytestmark = pytest.mark.gpu



@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "cornell": CORNELL}


def twins(path):
    """(host scene arrays, scene A for the waiting form, scene B for the stream form)"""
    hs = load(path, RES)
    return hs.arrays(), scene(hs), scene(hs)


# 1. whole-mesh soup, produced on the stream the call is given
def test_a_soup_produced_on_the_side_stream(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    before = frames(dev_b, configs("tri5k"))
    base = gpu(a["prim_v"].reshape(-1, 3))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        pos = produced(base, 0.02 * diagonal(a) / np.sqrt(3.0))
        dev_b.refit_triangles(0, pos, stream=side)  # no synchronisation between producer and call
    side.synchronize()
    bits = pos.cpu().numpy()
    assert np.isfinite(bits).all() and bits.tobytes() != a["prim_v"].tobytes()
    assert dev_a.update_triangles(0, pos, mode=p3d.UPDATE_REFIT) > 0
    now = assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "a soup from the side stream")
    assert frames_differ(now, before), "the deformation changed no pixel"
    assert dev_b.status() == 0


# 2. sources and untouched objects
@pytest.mark.parametrize("dtype", [np.int32, np.uint32])
def test_indexed_triangles_with_shared_vertices(dtype, paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    pos, idx, _ = deformed_mesh(a, seed=12)
    idx = idx.copy()
    idx[1000:1064, 0] = idx[999, 0]      # a fan around one position
    idx[2000:2010, 1:] = idx[5, 1:]      # ... and ten triangles that reuse two corners of triangle 5
    assert len(np.unique(idx)) < idx.size
    d_pos, d_idx = gpu(pos), gpu(idx.astype(dtype))
    assert d_idx.dtype == (torch.int32 if dtype is np.int32 else torch.uint32)
    side = torch.cuda.Stream()
    dev_b.refit_triangles(0, d_pos, d_idx, stream=side)
    side.synchronize()
    dev_a.update_triangles(0, d_pos, d_idx, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "indexed, %s" % dtype.__name__)
    assert dev_b.status() == 0


def test_spheres(paths):
    a, dev_a, dev_b = twins(paths["balls_low"])
    _, sph = kinds_of(a)
    first, count = int(sph[0]), len(sph)
    before = frames(dev_b, configs("balls_low"))
    cr = gpu(moved_spheres(a, first, count, seed=21))
    side = torch.cuda.Stream()
    dev_b.refit_spheres(first, cr, stream=side)
    side.synchronize()
    dev_a.update_spheres(first, cr, mode=p3d.UPDATE_REFIT)
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, "balls_low", "spheres"), before)
    assert dev_b.status() == 0


def test_triangles_and_spheres_in_one_call(paths):
    a, dev_a, dev_b = twins(paths["cornell"])
    tri, sph = kinds_of(a)
    t0, s0 = int(tri[0]), int(sph[0])
    before = frames(dev_b, configs("cornell"))
    rng = np.random.default_rng(22)
    soup = a["prim_v"][tri].reshape(-1, 3).astype(np.float64)
    d_soup = gpu((soup + rng.uniform(-1, 1, soup.shape) * 0.01 * diagonal(a, tri)).astype(np.float32))
    d_cr = gpu(moved_spheres(a, s0, len(sph), seed=23))
    dev_b.refit_device([dev_b.sphere_source(s0, d_cr), dev_b.triangle_source(t0, d_soup)])  # the default stream
    dev_a.update_geometry_device([dev_a.sphere_source(s0, d_cr), dev_a.triangle_source(t0, d_soup)], p3d.UPDATE_REFIT)
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, "cornell", "triangles and spheres"), before)


def test_sources_in_descending_order_and_untouched_objects(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    n = a["n_prims"]
    pos, idx, soup = deformed_mesh(a, seed=13, fraction=0.01)
    spans = [(0, 1), (10, 63), (100, 64), (200, 65), (n - 257, 257)]  # one object, a wave's end either side, a block + 1
    covered = np.zeros(n, bool)
    for first, count in spans:
        covered[first:first + count] = True
    tree0 = dev_b.export_bvh()
    meshes = []
    for k, (first, count) in enumerate(spans):
        if k % 2:  # indexed into the whole position array
            meshes.append((first, gpu(pos), gpu(idx[first:first + count].astype(np.int32))))
        else:      # a soup of its own
            meshes.append((first, gpu(soup[3 * first:3 * (first + count)])))
    meshes.reverse()
    assert [m[0] for m in meshes] == sorted((m[0] for m in meshes), reverse=True)
    side = torch.cuda.Stream()
    dev_b.refit_triangles(meshes, stream=side)
    side.synchronize()
    dev_a.update_triangles(meshes, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "five sources")
    # the uncovered objects keep their exact bits: every leaf that holds none of the covered objects has the box it had
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


# 3. three steps in a row on one stream, no host wait between them


def test_three_steps_without_a_host_wait(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    n_rays = 4096
    o, d = camera_rays(a, n_rays, seed=31)
    steps = [gpu(deformed_mesh(a, seed=32 + k, fraction=0.03)[2]) for k in range(3)]
    want = [w for w, _, _ in TRACE_OUT]
    outs_b = [trace_outputs(n_rays) for _ in steps]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for pos, out in zip(steps, outs_b):
        dev_b.refit_triangles(0, pos, stream=side)
        dev_b.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, stream=side, out=out)
    side.synchronize()
    outs_a = []
    for pos in steps:
        dev_a.update_triangles(0, pos, mode=p3d.UPDATE_REFIT)
        outs_a.append(dev_a.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, out=trace_outputs(n_rays)))
        torch.cuda.synchronize()
    for k, (got, ref) in enumerate(zip(outs_b, outs_a)):
        assert (ref["hit_id"] >= 0).sum() > n_rays // 4, "step %d: the rays miss the mesh" % k
        for name in want:
            assert got[name].cpu().numpy().tobytes() == ref[name].cpu().numpy().tobytes(), "step %d: %s differs" % (k, name)
    # the steps are told apart by these rays: trace k saw update k, and neither its neighbour's
    for k in range(2):
        assert outs_a[k]["t"].cpu().numpy().tobytes() != outs_a[k + 1]["t"].cpu().numpy().tobytes()
    assert dev_b.status() == 0


# 4. the smallest trees


@pytest.mark.parametrize("kind", ["spheres", "triangles"])
@pytest.mark.parametrize("n_objs", [1, 2, 3])
def test_tiny_scenes(n_objs, kind, tmp_path):
    """One object: the root is the only leaf, and the fit returns early.  Two: one internal node, emitted as a leaf of two.
    Three: the first tree with an inner node above a leaf."""
    if kind == "spheres":
        objs = ["s %g 0 0 0.6" % (1.4 * k - 1.4) for k in range(n_objs)]
    else:
        objs = ["p 3 %g -0.2 -0.6 %g 0.1 -0.5 %g 0 0.7" % (1.4 * k - 1.9, 1.4 * k - 0.8, 1.4 * k - 1.4) for k in range(n_objs)]
    path = str(tmp_path / "tiny.p3f")
    with open(path, "w") as f:
        f.write("\n".join(HEAD + objs) + "\n")
    a, dev_a, dev_b = twins(path)
    assert a["n_prims"] == n_objs
    before = frames(dev_b, configs("tiny"))
    rng = np.random.default_rng(40 + n_objs)
    side = torch.cuda.Stream()
    if kind == "spheres":
        new = a["prim_v"][:, :4].copy()
        new[:, :3] += rng.uniform(-0.2, 0.2, (n_objs, 3)).astype(np.float32)
        new[:, 3] *= np.float32(0.8)
        d_new = gpu(new)
        dev_b.refit_spheres(0, d_new, stream=side)
        side.synchronize()
        dev_a.update_spheres(0, d_new, mode=p3d.UPDATE_REFIT)
    else:
        new = a["prim_v"].reshape(-1, 3) + rng.uniform(-0.2, 0.2, (3 * n_objs, 3)).astype(np.float32)
        d_new = gpu(new)
        dev_b.refit_triangles(0, d_new, stream=side)
        side.synchronize()
        dev_a.update_triangles(0, d_new, mode=p3d.UPDATE_REFIT)
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, "tiny", "%d %s" % (n_objs, kind)), before)
    assert dev_b.status() == 0


# 5. per-object failures
def test_failed_triangles_keep_their_geometry_and_show_in_status(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    pos, idx, _ = deformed_mesh(a, seed=51)
    idx = idx.copy()
    idx[100:105, 0] = idx[50, 0]         # 50 and 100 .. 104 share one position ...
    pos[idx[50, 0]] = np.nan             # ... which is NaN
    idx[7, 1] = idx[4000, 2] = len(pos)  # two triangles with an index == n_elems
    nan_set, oob_set = [50, 100, 101, 102, 103, 104], [7, 4000]
    d_pos, d_idx = gpu(pos), gpu(idx.astype(np.uint32))
    tree0 = dev_b.export_bvh()
    side = torch.cuda.Stream()
    assert p3d.lib().p3d_scene_refit_device(dev_b._h, 1, C.byref(dev_b.triangle_source(0, d_pos, d_idx)), C.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    with pytest.raises(p3d.P3DError) as e:  # the twin: the waiting form, which reports in its return code
        dev_a.update_triangles(0, d_pos, d_idx, mode=p3d.UPDATE_REFIT)
    assert e.value.code == INVALID and "%d triangle(s) with an index" % len(oob_set) in str(e.value)
    assert dev_b.status() == INVALID
    msg = last_error()
    assert "%d triangle(s) with an index >= n_elems" % len(oob_set) in msg and "%d object(s) with a non-finite or inverted box" % len(nan_set) in msg, msg
    assert dev_b.status() == 0
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "two bad indices and a NaN position")
    # the named objects kept their geometry, the others moved
    tree1 = dev_b.export_bvh()
    order = tree1["bvh_order"]
    leaves = np.nonzero(tree1["bvh_count_leaf"] & LEAF)[0]
    single = {int(order[tree1["bvh_index"][l]]): l for l in leaves if (tree1["bvh_count_leaf"][l] & ~LEAF) == 1}
    kept = [single[o] for o in nan_set + oob_set if o in single]
    assert tree0["bvh_bmin"][kept].tobytes() == tree1["bvh_bmin"][kept].tobytes()
    assert tree0["bvh_bmin"].tobytes() != tree1["bvh_bmin"].tobytes()
    # the counts are those since the last check: one more bad call counts from zero
    dev_b.refit_triangles(0, d_pos, d_idx, stream=side)
    assert dev_b.status() == INVALID and "%d triangle(s) with an index" % len(oob_set) in last_error()
    assert dev_b.status() == 0


def test_a_frame_with_stats_leaves_the_report_to_status(paths):
    """A render call with stats behind a refit that skipped an object is not failed by it, and does not swallow the report:
    p3d_scene_status still returns it, once."""
    a, dev_a, dev_b = twins(paths["balls_low"])
    _, sph = kinds_of(a)
    first, count = int(sph[0]), len(sph)
    cr = moved_spheres(a, first, count, seed=53)
    cr[5, 3] = -1.0
    d_cr = gpu(cr)
    side = torch.cuda.Stream()
    dev_b.refit_spheres(first, d_cr, stream=side)
    side.synchronize()
    with pytest.raises(p3d.P3DError):
        dev_a.update_spheres(first, d_cr, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "balls_low", "frames with stats before the status is asked")  # (B's renders return normally)
    assert dev_b.status() == INVALID and "1 object(s) with a non-finite or inverted box" in last_error(), last_error()
    assert dev_b.status() == 0


@pytest.mark.parametrize("radius", [-0.25, float("nan")])
def test_a_sphere_with_a_bad_radius_keeps_its_geometry(radius, paths):
    a, dev_a, dev_b = twins(paths["balls_low"])
    _, sph = kinds_of(a)
    first, count = int(sph[0]), len(sph)
    cr = moved_spheres(a, first, count, seed=52)
    cr[3, 3] = radius
    d_cr = gpu(cr)
    dev_b.refit_spheres(first, d_cr)  # returns normally
    with pytest.raises(p3d.P3DError) as e:
        dev_a.update_spheres(first, d_cr, mode=p3d.UPDATE_REFIT)
    assert e.value.code == INVALID
    assert dev_b.status() == INVALID
    assert "0 triangle(s)" in last_error() and "1 object(s) with a non-finite or inverted box" in last_error(), last_error()
    assert dev_b.status() == 0
    assert_same_frames_and_tree(dev_a, dev_b, "balls_low", "one bad radius")


# 6. refusals, nothing changed
def _raw(dev, sources, n=None, null=False, stream=None):
    arr = (p3d.GeomSource * max(len(sources), 1))(*sources)
    return p3d.lib().p3d_scene_refit_device(dev._h if dev is not None else None, len(sources) if n is None else n,
                                            None if null else C.cast(arr, C.c_void_p), stream)


def test_refusals_leave_the_scene_as_it_was(paths):
    name = "balls_low"
    hs = load(paths[name], RES)
    a = hs.arrays()
    n = a["n_prims"]
    tri, sph = kinds_of(a)
    t0, nt, s0, ns = int(tri[0]), len(tri), int(sph[0]), len(sph)
    assert t0 + nt == s0 and s0 + ns == n and nt >= 2 and ns >= 4
    dev, twin = scene(hs), scene(hs)
    host_tree = p3d.DeviceScene(hs, bvh=True)
    device_grid = p3d.DeviceScene(hs, bvh="device", grid="device")
    uploaded_grid = p3d.DeviceScene(hs, bvh="device", grid=True)
    cr = gpu(moved_spheres(a, s0, ns, seed=61))
    soup = gpu((a["prim_v"][tri].reshape(-1, 3) * np.float32(1.01)).astype(np.float32))
    index = gpu(np.arange(3 * nt, dtype=np.int32).reshape(-1, 3))
    host_cr = np.ascontiguousarray(moved_spheres(a, s0, ns, seed=61))  # numpy arrays: host memory
    host_index = np.arange(3 * nt, dtype=np.uint32)
    S, TRI = SPHERE, TRIANGLE

    def src(first, count, kind, n_elems, data, index=None, reserved=(0, 0)):
        return p3d.GeomSource(first, count, kind, n_elems, data, index, (C.c_uint64 * 2)(*reserved))

    good = [src(s0, ns, S, ns, cr.data_ptr())]
    for what, other, code in (("a scene with the host's tree", host_tree, INVALID), ("a scene with an uploaded grid", uploaded_grid, INVALID),
                              ("a scene with a device-built grid", device_grid, UNSUPPORTED)):
        was = frames(other, configs(name))
        assert _raw(other, good) == code, what
        assert last_error().startswith("p3d_scene_refit_device"), what
        assert_same_frames(frames(other, configs(name)), was, what)
    assert "p3d_scene_update_geometry_device" in last_error()  # the grid scene is pointed to the waiting form
    assert _raw(None, good) == INVALID
    was, tree = frames(dev, configs(name)), dev.export_bvh()
    # host memory is refused BEFORE any launch; each such source goes in twice (test_gpu_device_geometry.py says why)
    for what, bad in (("d_data", src(s0, ns, S, ns, host_cr.ctypes.data)),
                      ("d_index", src(t0, nt, TRI, 3 * nt, soup.data_ptr(), host_index.ctypes.data))):
        assert _raw(dev, [bad, bad]) == INVALID
        assert "is host memory" in last_error() and what in last_error(), last_error()
    cases = [
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
        ("positions that end behind their allocation", [src(t0, nt, TRI, 1 << 28, soup.data_ptr(), index.data_ptr())]),
    ]
    for what, kw in cases:
        kw = kw if isinstance(kw, dict) else dict(sources=kw)
        assert _raw(dev, **kw) == INVALID, what
        assert last_error().startswith("p3d_scene_refit_device"), what
        assert_same_frames(frames(dev, configs(name)), was, what)
        assert_same_tree(dev.export_bvh(), tree, what)
    assert _raw(dev, cases[-1][1]) == INVALID and "ends behind its allocation" in last_error()
    # the policy: refused while it is on, accepted again once it is off
    dev.set_auto_rebuild(1.01)
    assert _raw(dev, good) == UNSUPPORTED and "auto-rebuild" in last_error()
    dev.set_auto_rebuild(0)
    # no sources: nothing enqueued, nothing changed
    assert _raw(dev, []) == 0 and _raw(dev, [], null=True) == 0
    assert dev.refit_device([]) is None
    assert_same_tree(dev.export_bvh(), tree, "after the refusals")
    assert_same_frames(frames(dev, configs(name)), was, "after the refusals")
    cost = dev.bvh_cost()
    assert cost["refits_since_build"] == 0
    assert dev.status() == 0
    # the same calls without a fault are accepted, in any order
    assert _raw(dev, [src(s0, ns, S, ns, cr.data_ptr()), src(t0, nt, TRI, 3 * nt, soup.data_ptr(), index.data_ptr())]) == 0
    twin.update_geometry_device([twin.triangle_source(t0, soup, index), twin.sphere_source(s0, cr)], p3d.UPDATE_REFIT)
    assert frames_differ(assert_same_frames_and_tree(twin, dev, name, "the accepted call"), was)
    assert dev.status() == 0


def test_sixteen_sources_and_one_too_many(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    _, _, soup = deformed_mesh(a, seed=62)
    spans = [(290 * k, 1 + 17 * k) for k in range(17)]  # 1 .. 273 triangles each (the last two more than a block), gaps between them
    parts = [gpu(soup[3 * first:3 * (first + count)]) for first, count in spans]
    meshes = [(first, part) for (first, _), part in zip(spans, parts)]
    tree = dev_b.export_bvh()
    with pytest.raises(p3d.P3DError) as e:
        dev_b.refit_triangles(meshes)
    assert e.value.code == CAPACITY and "p3d_scene_update_geometry_device" in str(e.value), e.value
    assert_same_tree(dev_b.export_bvh(), tree, "seventeen sources")
    assert dev_b.bvh_cost()["refits_since_build"] == 0
    side = torch.cuda.Stream()
    dev_b.refit_triangles(meshes[:16][::-1], stream=side)
    side.synchronize()
    dev_a.update_triangles(meshes[:16], mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "sixteen sources")
    assert dev_b.export_bvh()["bvh_bmin"].tobytes() != tree["bvh_bmin"].tobytes()
    assert dev_b.status() == 0


# 7. the setup path
def test_the_first_update_of_a_scene(paths):
    a, dev_a, dev_b = twins(paths["cornell"])
    _, sph = kinds_of(a)
    cr = gpu(moved_spheres(a, int(sph[0]), len(sph), seed=71))
    dev_b.refit_spheres(int(sph[0]), cr)  # nothing has made the builder's state: this call does
    dev_a.update_spheres(int(sph[0]), cr, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "cornell", "the first update is a stream refit")


# 8. topology and depth of a new tree
def test_after_a_rebuild_that_changed_the_order(paths):
    a, dev_a, dev_b = twins(paths["tri5k"])
    n = a["n_prims"]
    rng = np.random.default_rng(81)
    jump = rng.uniform(-0.4, 0.4, (n, 1, 3)) * diagonal(a)  # every triangle thrown somewhere else in the scene
    far = gpu((a["prim_v"].reshape(n, 3, 3).astype(np.float64) + jump).astype(np.float32).reshape(-1, 3))
    side = torch.cuda.Stream()
    dev_b.refit_triangles(0, far, stream=side)
    side.synchronize()
    dev_a.update_triangles(0, far, mode=p3d.UPDATE_REFIT)
    refitted = dev_b.export_bvh()
    for dev in (dev_a, dev_b):
        dev.update_geometry_device([], p3d.UPDATE_REBUILD)
    built = dev_b.export_bvh()
    assert built["bvh_order"].tobytes() != refitted["bvh_order"].tobytes()
    _, _, small = deformed_mesh(dict(a, prim_v=far.cpu().numpy().reshape(-1, 9)), seed=82, fraction=0.002)
    d_small = gpu(small)
    dev_b.refit_triangles(0, d_small, stream=side)  # over the NEW topology, with the new tree's depth
    side.synchronize()
    dev_a.update_triangles(0, d_small, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "a stream refit of a rebuilt tree")
    assert dev_b.export_bvh()["bvh_order"].tobytes() == built["bvh_order"].tobytes()
    assert dev_b.status() == 0


# 9. no state leaks between the forms
def test_the_forms_in_turn(paths):
    a, dev_a, dev_b = twins(paths["cornell"])
    tri, sph = kinds_of(a)
    t0, s0 = int(tri[0]), int(sph[0])
    move = rigid(a, np.random.default_rng(91))
    for dev in (dev_a, dev_b):
        dev.transform_prims([(t0, len(tri), 0)], move[None], p3d.UPDATE_REFIT)  # makes the rest copy
    side = torch.cuda.Stream()
    soup = a["prim_v"][tri].reshape(-1, 3).astype(np.float64)
    soup = (soup + np.random.default_rng(92).uniform(-1, 1, soup.shape) * 0.01 * diagonal(a, tri)).astype(np.float32)
    assert not (soup == 0).any()  # (1 * -0 + 0 is +0: the one value the identity below would change)
    d_soup = gpu(soup)
    dev_b.refit_triangles(t0, d_soup, stream=side)
    side.synchronize()
    dev_a.update_triangles(t0, d_soup, mode=p3d.UPDATE_REFIT)
    deformed = assert_same_frames_and_tree(dev_a, dev_b, "cornell", "step 1: a stream refit")
    cr = gpu(moved_spheres(a, s0, 2, seed=93))
    for dev in (dev_a, dev_b):
        assert dev.update_spheres(s0, cr, mode=p3d.UPDATE_REFIT) > 0
    assert_same_frames_and_tree(dev_a, dev_b, "cornell", "step 2: the waiting form")
    for dev in (dev_a, dev_b):
        dev.transform_prims([(t0, len(tri), 0)], IDENTITY[None], p3d.UPDATE_REFIT)
    back = assert_same_frames_and_tree(dev_a, dev_b, "cornell", "step 3: the identity")
    # (B's identity read the rest copy the stream form wrote, A's the one the waiting form wrote: a deformed object rests
    # where it is put, on both)
    assert frames_differ(back, deformed)  # (step 2 moved two spheres)
    cr2 = gpu(moved_spheres(a, s0, len(sph), seed=94))
    dev_b.refit_spheres(s0, cr2, stream=side)
    side.synchronize()
    dev_a.update_spheres(s0, cr2, mode=p3d.UPDATE_REFIT)
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, "cornell", "step 4: a stream refit again"), deformed)
    assert dev_b.status() == 0


# 10. accumulators and the cost record
def test_accumulators_and_bvh_cost(paths):
    hs = load(paths["cornell"], 64)
    a = hs.arrays()
    dev_a, dev_b = scene(hs), scene(hs)
    _, sph = kinds_of(a)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    acc = dev_b.accumulator(cfg)
    acc.render(2)
    was = dev_b.bvh_cost()
    cr = gpu(moved_spheres(a, int(sph[0]), len(sph), seed=95))
    dev_b.refit_spheres(int(sph[0]), cr)
    with pytest.raises(p3d.P3DError) as e:
        acc.render(1)
    assert e.value.code == INVALID and "moved" in str(e.value)
    assert acc.samples_done == 2
    acc.reset()
    acc.render(1)
    acc.close()
    dev_a.update_spheres(int(sph[0]), cr, mode=p3d.UPDATE_REFIT)
    cost_a, cost_b = dev_a.bvh_cost(), dev_b.bvh_cost()
    assert cost_b["refits_since_build"] == was["refits_since_build"] + 1 and cost_b["last_update_rebuilt"] == 0
    assert np.float64(cost_b["sah"]).tobytes() == np.float64(cost_a["sah"]).tobytes() and cost_b["sah"] != was["sah"]
    assert cost_a == cost_b, (cost_a, cost_b)


# 11. a frame that reads the root box
def test_a_per_level_frame_after_a_stream_refit(paths):
    hs = load(paths["tri5k"], 128)
    a = hs.arrays()
    dev_a, dev_b = scene(hs), scene(hs)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, chain_launch=p3d.CHAIN_PER_LEVEL, collect_stats=1)
    before = dev_b.render(cfg)
    # the mesh grows by a fifth about a corner: the root box it is binned by moves
    corner = a["prim_bmin"].min(0)
    grown = gpu(((a["prim_v"].reshape(-1, 3) - corner) * np.float32(1.2) + corner).astype(np.float32))
    side = torch.cuda.Stream()
    dev_b.refit_triangles(0, grown, stream=side)
    side.synchronize()
    dev_a.update_triangles(0, grown, mode=p3d.UPDATE_REFIT)
    rgb_a, hit_a, st_a = dev_a.render(cfg)
    rgb_b, hit_b, st_b = dev_b.render(cfg)
    assert np.array_equal(hit_a, hit_b) and rgb_a.tobytes() == rgb_b.tobytes()
    assert {k: getattr(st_a, k) for k in RENDER_COUNTERS} == {k: getattr(st_b, k) for k in RENDER_COUNTERS}
    assert rgb_b.tobytes() != before[0].tobytes()
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), "the grown mesh")
    assert dev_b.status() == 0


# 12. the call does not wait
def test_the_call_returns_ahead_of_the_stream(paths):
    """A producer of 900 torch kernels over 2^24 floats stands in front of the call on the side stream.  Measured on an
    MI355X: 17.7 ms of GPU time for the producer, 0.029 ms of host time for the call (a factor of 600).  The assertion below asks for
    a factor of at least 100 between them, and for a stream that is still busy when the call is back."""
    a, dev_a, dev_b = twins(paths["tri5k"])
    base = gpu(a["prim_v"].reshape(-1, 3))
    amount = 0.02 * diagonal(a) / np.sqrt(3.0)
    big = torch.linspace(0, 1, 1 << 24, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev_b.refit_triangles(0, produced(base, 0.5 * amount, rounds=4), stream=side)  # the setup call: it may wait
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        begin.record(side)
        slow = produced(big, 1.0, rounds=300)
        end.record(side)
        pos = produced(base, amount, rounds=4) + 0.0 * slow[:base.numel()].view(-1, 3)
        t0 = time.perf_counter()
        dev_b.refit_triangles(0, pos, stream=side)
        call_s = time.perf_counter() - t0
        busy = not side.query()
    side.synchronize()
    producer_ms = begin.elapsed_time(end)
    print("producer %.3f ms on the GPU, call %.4f ms on the host" % (producer_ms, 1e3 * call_s))
    assert producer_ms >= 100 * 1e3 * call_s, (producer_ms, call_s)
    assert busy, "the stream had passed the call when it returned"
    dev_a.update_triangles(0, pos, mode=p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "a refit behind a long producer")
    assert dev_b.status() == 0
