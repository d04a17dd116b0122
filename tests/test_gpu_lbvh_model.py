"""The device BVH builder (csrc/lbvh.hpp) against an independent model of its tree (lbvh_reference.py) on the GPU.

The tree is a function of the object boxes, so p3d_scene_export_bvh must return the model's arrays to the byte and the
model's depth: after create, after a REBUILD, and, boxes only, after a REFIT.  The degenerate scenes (coincident centres, flat
axes, an outlier, cell edges, a deep chain) are traversed as well: closest hits over the device tree against the object
loop of the same scene, and Whitted frames of the two deepest against a scene uploaded with the exported tree."""

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, frames
import fuzz_scenes
import lbvh_reference as ref
import p3d_amd as p3d
from scene_update_helpers import SPHERE, random_moves

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513]
SYNTHETIC = [name for name, _, _ in ref.synthetic_scenes()]


@pytest.fixture(scope="module")
def paths(tmp_path_factory, tri5k_path):
    tmp = tmp_path_factory.mktemp("lbvh")
    out = {name: ref.write_p3f(str(tmp / (name + ".p3f")), objects, view) for name, objects, view in ref.synthetic_scenes()}
    for n in COUNTS:
        out["count%d" % n] = ref.write_p3f(str(tmp / ("count%d.p3f" % n)), ref.counts_scene(n))
    out["mixed"] = fuzz_scenes.random_scene(21, str(tmp / "mixed.p3f"), n_spheres=40, n_tris=60, n_boxes=20, n_planes=2)
    out.update(balls_low=scene_path("balls_low.p3f"), path_glass=scene_path("path_glass.p3f"), tri5k=tri5k_path, cornell=CORNELL)
    return out


def model(a):
    return ref.build(a["prim_bmin"], a["prim_bmax"])


# ---- a. the tree --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["balls_low", "path_glass", "tri5k", "cornell"] + SYNTHETIC + ["mixed"])
def test_the_device_tree_is_the_models(name, paths):
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    got = dev.export_bvh()
    print("%s: %d objects, the device reports depth %d" % (name, len(got["bvh_order"]), got["bvh_max_depth"]))
    ref.assert_same_tree(got, model(hs.arrays()), name)


@pytest.mark.parametrize("n", COUNTS)
def test_the_device_tree_is_the_models_around_the_block_edge(n, paths):
    """n leaves, n - 1 internal nodes, 256 threads per block"""
    hs = p3d.HostScene(paths["count%d" % n])
    ref.assert_same_tree(p3d.DeviceScene(hs, bvh="device").export_bvh(), model(hs.arrays()), "%d spheres" % n)


# ---- b. the tree after updates ------------------------------------------------------------------------------------------------

UPDATED = ["balls_low", "tri5k", "chain"]
SEED = {"balls_low": 31, "tri5k": 32, "chain": 33}


def move(hs, name, round_):
    a = hs.arrays()
    objs, new_v = random_moves(a, SEED[name] + 100 * round_, include=np.nonzero(a["prim_type"] == SPHERE)[0][:1].tolist())
    hs.set_geometry(objs, new_v)
    return objs


@pytest.mark.parametrize("name", UPDATED)
def test_a_rebuilt_tree_is_the_model_of_the_moved_boxes(name, paths):
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    for round_ in range(2):  # the second round runs in the kept workspace
        assert dev.update_prims(move(hs, name, round_), p3d.UPDATE_REBUILD) > 0
        ref.assert_same_tree(dev.export_bvh(), model(hs.arrays()), "%s, rebuild %d" % (name, round_))


@pytest.mark.parametrize("name", UPDATED)
def test_a_refitted_tree_is_the_models_topology_over_the_moved_boxes(name, paths):
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    t0 = model(hs.arrays())
    for round_ in range(2):
        assert dev.update_prims(move(hs, name, round_), p3d.UPDATE_REFIT) > 0
        a = hs.arrays()
        want = ref.refit(t0, a["prim_bmin"], a["prim_bmax"])
        assert want["bvh_bmin"].tobytes() != t0["bvh_bmin"].tobytes()
        ref.assert_same_tree(dev.export_bvh(), want, "%s, refit %d" % (name, round_))
    # ... and behind a REBUILD the topology a REFIT keeps is the rebuilt one
    assert dev.update_prims(move(hs, name, 2), p3d.UPDATE_REBUILD) > 0
    t1 = model(hs.arrays())
    ref.assert_same_tree(dev.export_bvh(), t1, "%s, rebuild behind two refits" % name)
    assert dev.update_prims(move(hs, name, 3), p3d.UPDATE_REFIT) > 0
    a = hs.arrays()
    ref.assert_same_tree(dev.export_bvh(), ref.refit(t1, a["prim_bmin"], a["prim_bmax"]), "%s, refit behind a rebuild" % name)


def test_a_transformed_range_gives_the_models_trees(paths):
    """p3d_scene_transform_prims, a rotation of objects 700 .. 3699 of the 5000 triangles about their middle, in both modes.
    The boxes the model sees are the host route's: p3d.transformed -> HostScene.set_geometry."""
    hs = p3d.HostScene(paths["tri5k"])
    rest = hs.arrays()
    refitted, rebuilt = p3d.DeviceScene(hs, bvh="device"), p3d.DeviceScene(hs, bvh="device")
    t0 = model(rest)
    ranges = [(700, 3000, 0)]
    lo, hi = rest["prim_bmin"][700:3700].min(0).astype(np.float64), rest["prim_bmax"][700:3700].max(0).astype(np.float64)
    c, s = np.cos(0.7), np.sin(0.7)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
    m = np.zeros((1, 3, 4), np.float32)
    m[0, :, :3] = rot
    m[0, :, 3] = (lo + hi) / 2 - rot @ ((lo + hi) / 2)
    hs.set_geometry(*p3d.transformed(rest["prim_type"], rest["prim_v"], ranges, m))
    a = hs.arrays()
    assert (a["prim_bmin"][700:3700] != rest["prim_bmin"][700:3700]).any() and np.array_equal(a["prim_bmin"][:700], rest["prim_bmin"][:700])
    assert refitted.transform_prims(ranges, m, p3d.UPDATE_REFIT) > 0
    ref.assert_same_tree(refitted.export_bvh(), ref.refit(t0, a["prim_bmin"], a["prim_bmax"]), "transform, refit")
    assert rebuilt.transform_prims(ranges, m, p3d.UPDATE_REBUILD) > 0
    ref.assert_same_tree(rebuilt.export_bvh(), model(a), "transform, rebuild")


# ---- c. traversal of the degenerate trees -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SYNTHETIC)
def test_closest_hits_over_a_degenerate_tree_are_the_object_loops(name, paths):
    """20 000 rays (lbvh_reference.scene_rays) through the device tree and through the object loop of the same scene.

    Without spheres no test re-normalises the ray (Q8) and the nearest t is a minimum over the same per-object values: hit or
    miss must be identical and t equal to the bit; the object may differ only where two objects give that same t (everywhere
    among the 600 duplicates, on no more than the seam share of 1e-3 of the rays elsewhere).  The oracle's own BVH and its own
    object loop agree in just this way on all four such scenes and these rays (run on the CPU: 0 of 20 000 hit-or-miss and t
    differences on each), so none of them needs the statistical bounds.
    With spheres: the bounds of test_device_built_bvh_finds_the_same_closest_hits, and more than 1 % of the rays hit."""
    hs = p3d.HostScene(paths[name])
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    o, d = ref.scene_rays(a)
    hit_b, _, t_b = dev.trace_closest(p3d.ACCEL_BVH, o, d, want_t=True)
    hit_n, _, t_n = dev.trace_closest(p3d.ACCEL_NONE, o, d, want_t=True)
    miss = float(((hit_b >= 0) != (hit_n >= 0)).mean())
    diff = float((hit_b != hit_n).mean())
    both = (hit_b >= 0) & (hit_n >= 0)
    t_diff = int((t_b[both].view(np.uint32) != t_n[both].view(np.uint32)).sum())
    print("%s (depth %d): %.3f of the rays hit; hit/miss differs on %.3g, the object on %.3g, t in some bit on %d rays" % (
        name, dev.export_bvh()["bvh_max_depth"], float((hit_n >= 0).mean()), miss, diff, t_diff))
    assert (hit_n >= 0).mean() > 0.01
    if (a["prim_type"] == SPHERE).any():
        assert miss < 1e-4
        assert diff < 1e-3
    else:
        assert miss == 0 and t_diff == 0
        assert name == "duplicates" or diff < 1e-3


def stack_modes(accel=p3d.ACCEL_BVH):
    """(label, cfg): Whitted depth 2 in both stack modes"""
    return [(label, p3d.whitted_config(accel=accel, max_depth=2, stack_mode=mode, collect_stats=1))
            for label, mode in (("literal", p3d.STACK_LITERAL), ("per pixel", p3d.STACK_PER_PIXEL))]


@pytest.mark.parametrize("name", ["chain", "outlier"])
def test_frames_over_a_deep_device_tree(name, paths):
    """A 64 x 64 Whitted frame at depth 2 in both stack modes over the tree the device built and sized its stacks for (the chain:
    depth above 40, so the spilling stack and the halo chains' backing array are in use), against a scene created from the
    exported tree, tolerance 0; the primary-hit image against the object loop's, with the seam bound."""
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    tree = dev.export_bvh()
    ref.assert_same_tree(tree, model(hs.arrays()), name)
    twin = p3d.DeviceScene(hs, bvh=tree)
    mine, theirs = frames(dev, stack_modes()), frames(twin, stack_modes())
    assert [f[0] for f in mine] == [f[0] for f in theirs]
    for (label, rgb_a, hit_a, st_a), (_, rgb_b, hit_b, st_b) in zip(mine, theirs):
        assert np.array_equal(hit_a, hit_b), "%s, %s: hit IDs differ in %d pixels" % (name, label, int((hit_a != hit_b).sum()))
        assert rgb_a.tobytes() == rgb_b.tobytes(), "%s, %s: max |diff| %g" % (name, label, float(np.abs(rgb_a - rgb_b).max()))
        assert st_a == st_b, "%s, %s: counters %s / %s" % (name, label, st_a, st_b)
    plain = frames(dev, stack_modes(p3d.ACCEL_NONE))[0][2]
    for label, _, hit, _ in mine:
        px = float((hit != plain).mean())
        print("%s, %s (depth %d): %.3f of the pixels hit, hit IDs differ from the object loop's on %.3g" % (
            name, label, tree["bvh_max_depth"], float((hit >= 0).mean()), px))
        assert (hit >= 0).mean() > 0.01
        assert px < 1e-3
