"""The SAH cost of a device-built tree (p3d_scene_bvh_cost) and the refit that rebuilds by itself (p3d_scene_set_auto_rebuild)
on the GPU.

The cost is stated on the exported tree (include/p3d.h); `statement` below is that statement in float64, summed exactly
(math.fsum), and carries nothing of the package's tree_cost.  The device sums the same non-negative terms in another order: N
additions, each rounded to 2^-53 of a partial sum that is no larger than the total, so the two differ by at most N 2^-53 of
the total - below 5e-10 for N <= 2^22.  The bound used is 1e-9.

A promoted update must leave what the same update leaves when called with UPDATE_REBUILD - the tree of a scene created fresh
from the moved objects, to the byte - and one that is not promoted what a plain UPDATE_REFIT leaves."""
import math

import numpy as np
import pytest

from conftest import scene_path
from frame_checks import CORNELL, RENDER_COUNTERS, f64_bytes
import fuzz_scenes
import lbvh_reference as ref
import p3d_amd as p3d
from scene_update_helpers import random_moves, translated

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 3, 4, 255, 256, 257, 513]
SCENES = ["count%d" % n for n in COUNTS] + ["balls_low", "cornell", "mixed", "tri100k"]
LEAF = 0x80000000
RATIO = 1.25
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)


@pytest.fixture(scope="module")
def paths(tmp_path_factory, tri100k_path):
    tmp = tmp_path_factory.mktemp("bvh_cost")
    out = {"count%d" % n: ref.write_p3f(str(tmp / ("count%d.p3f" % n)), ref.counts_scene(n)) for n in COUNTS}
    out["mixed"] = fuzz_scenes.random_scene(21, str(tmp / "mixed.p3f"), n_spheres=40, n_tris=60, n_boxes=20, n_planes=2)
    out.update(balls_low=scene_path("balls_low.p3f"), cornell=CORNELL, tri100k=tri100k_path)
    return out


def statement(tree):
    """-> (sah, n_inner, n_leaves) of an export_bvh() dict"""
    lo, hi = tree["bvh_bmin"].astype(np.float64), tree["bvh_bmax"].astype(np.float64)
    if len(lo) == 0:
        return 0.0, 0, 0
    dx, dy, dz = (hi - lo).T
    area = (dx * dy + dy * dz) + dz * dx
    leaf = (tree["bvh_count_leaf"] & LEAF) != 0
    count = (tree["bvh_count_leaf"] & 0x7fffffff).astype(np.float64)
    total = math.fsum(area[~leaf].tolist() + (count[leaf] * area[leaf]).tolist())  # (count is 1 or 2: the product is exact)
    return (total / area[0] if area[0] > 0 else 0.0), int((~leaf).sum()), int(leaf.sum())


def same_export(a, b):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in ref.TREE_KEYS) and \
        a["bvh_max_depth"] == b["bvh_max_depth"]


def small_move(hs):
    objs, new_v = random_moves(hs.arrays(), 7, reach=0.001)
    hs.set_geometry(objs, new_v)
    return objs


def big_offsets(a, seed=11):
    """Every third object, each axis by up to the diagonal of the scene -> (objects, offsets)"""
    rng = np.random.default_rng(seed)
    objs = np.arange(0, a["n_prims"], 3, dtype=np.uint32)
    diag = float(np.linalg.norm(a["prim_bmax"].max(0).astype(np.float64) - a["prim_bmin"].min(0).astype(np.float64)))
    return objs, (rng.uniform(-1, 1, (len(objs), 3)) * diag).astype(np.float32)


def big_move(hs):
    a = hs.arrays()
    objs, off = big_offsets(a)
    hs.set_geometry(objs, translated(a["prim_type"], a["prim_v"], objs, off))
    return objs


def frame_bytes(dev):
    out = []
    for mode in (p3d.STACK_LITERAL, p3d.STACK_PER_PIXEL):
        rgb, hit, st = dev.render(p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, stack_mode=mode, collect_stats=1))
        out.append((rgb.tobytes(), hit.tobytes(), {k: getattr(st, k) for k in RENDER_COUNTERS}))
    return out


# ---- 1. the cost against the statement ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_the_cost_is_the_statement_over_the_exported_tree(name, paths):
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    before = dev.export_bvh()
    c = dev.bvh_cost()
    tree = dev.export_bvh()
    assert same_export(before, tree), "%s: measuring changed the tree" % name
    want, n_inner, n_leaves = statement(tree)
    print("%s: %d objects, sah %.17g, the statement's %.17g (relative %.3g); %d inner nodes, %d leaves" % (
        name, len(tree["bvh_order"]), c["sah"], want, abs(c["sah"] - want) / want, c["n_inner"], c["n_leaves"]))
    assert abs(c["sah"] - want) <= 1e-9 * want
    assert (c["n_inner"], c["n_leaves"]) == (n_inner, n_leaves)
    assert c["n_inner"] + c["n_leaves"] == len(tree["bvh_index"])
    assert (c["refits_since_build"], c["last_update_rebuilt"]) == (0, 0)
    assert f64_bytes(c["sah_baseline"]) == f64_bytes(c["sah"])  # create, and no refit since
    if name == "count1":
        assert c["sah"] == 1.0 and (c["n_inner"], c["n_leaves"]) == (0, 1)
    if name == "count2":
        assert c["sah"] == 2.0 and (c["n_inner"], c["n_leaves"]) == (0, 1)  # the root is a leaf of two objects
    assert dev.bvh_cost() == c, "%s: a second call" % name
    # tri100k: the same host scene (loading it again costs more than the rest of this test)
    fresh = p3d.DeviceScene(hs if name == "tri100k" else p3d.HostScene(paths[name]), bvh="device")
    assert fresh.bvh_cost() == c, "%s: a fresh scene" % name


def test_the_second_stage_loops_on_the_big_scene(paths):
    """More than 256 partials: 256 threads of the one-block launch take more than one each"""
    n = p3d.HostScene(paths["tri100k"]).arrays()["n_prims"]
    assert (n - 1 + 255) // 256 > 256


# ---- 2. the same tree, the same bits ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["count513", "balls_low"])
def test_a_rebuilt_tree_costs_what_a_fresh_scenes_does(name, paths):
    hs = p3d.HostScene(paths[name])
    dev = p3d.DeviceScene(hs, bvh="device")
    objs = big_move(hs) if name == "count513" else small_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REBUILD) > 0
    got, want = dev.bvh_cost(), p3d.DeviceScene(hs, bvh="device").bvh_cost()
    assert f64_bytes(got["sah"]) == f64_bytes(want["sah"]) and (got["n_inner"], got["n_leaves"]) == (want["n_inner"], want["n_leaves"])
    assert (got["refits_since_build"], got["last_update_rebuilt"]) == (0, 1)
    assert abs(got["sah"] - statement(dev.export_bvh())[0]) <= 1e-9 * got["sah"]


def test_a_refitted_tree_costs_the_statement_and_counts_its_refits(paths):
    hs = p3d.HostScene(paths["count513"])
    dev = p3d.DeviceScene(hs, bvh="device")
    for k in (1, 2):
        assert dev.update_prims(small_move(hs), p3d.UPDATE_REFIT) > 0
        c = dev.bvh_cost()
        assert abs(c["sah"] - statement(dev.export_bvh())[0]) <= 1e-9 * c["sah"]
        assert (c["refits_since_build"], c["last_update_rebuilt"], c["sah_baseline"]) == (k, 0, 0.0)


# ---- 3 to 5. the policy ----------------------------------------------------------------------------------------------------------

def pair(paths, grid=False, ratio=RATIO):
    """(host scene, scene with the policy on, its twin with the policy off, sah at build)"""
    hs = p3d.HostScene(paths["count513"])
    dev, twin = p3d.DeviceScene(hs, bvh="device", grid=grid), p3d.DeviceScene(hs, bvh="device", grid=grid)
    assert dev.auto_rebuild() == 0.0
    before = dev.export_bvh()
    dev.set_auto_rebuild(ratio)
    assert dev.auto_rebuild() == ratio and twin.auto_rebuild() == 0.0
    assert same_export(dev.export_bvh(), before), "switching the policy on changed the tree"
    built = statement(before)[0]
    c = dev.bvh_cost()
    assert f64_bytes(c["sah_baseline"]) == f64_bytes(c["sah"]) and abs(c["sah"] - built) <= 1e-9 * built
    return hs, dev, twin, built


def check_kept(dev, twin, built):
    """The twin took the same REFIT: the policy scene must hold its tree"""
    ratio = statement(twin.export_bvh())[0] / built
    print("refitted / built: %.4f" % ratio)
    assert abs(ratio - 1) < 0.1
    assert same_export(dev.export_bvh(), twin.export_bvh())
    c = dev.bvh_cost()
    assert (c["last_update_rebuilt"], c["refits_since_build"]) == (0, 1)
    assert abs(c["sah_baseline"] - built) <= 1e-9 * built


def check_rebuilt(hs, dev, twin, built, grid=False):
    """hs holds the moved objects"""
    ratio = statement(twin.export_bvh())[0] / built
    print("refitted / built: %.4f" % ratio)
    assert ratio > 1.5
    a = hs.arrays()
    fresh = p3d.DeviceScene(hs, bvh="device", grid=grid)
    got = dev.export_bvh()
    ref.assert_same_tree(got, ref.build(a["prim_bmin"], a["prim_bmax"]), "promoted refit")
    assert same_export(got, fresh.export_bvh())
    assert not same_export(got, twin.export_bvh())
    c = dev.bvh_cost()
    assert (c["last_update_rebuilt"], c["refits_since_build"]) == (1, 0)
    assert f64_bytes(c["sah_baseline"]) == f64_bytes(c["sah"]) == f64_bytes(fresh.bvh_cost()["sah"])
    return fresh


def test_the_policy_keeps_a_good_tree(paths):
    hs, dev, twin, built = pair(paths)
    objs = small_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and twin.update_prims(objs, p3d.UPDATE_REFIT) > 0
    check_kept(dev, twin, built)


def test_the_policy_rebuilds_a_bad_tree(paths):
    hs, dev, twin, built = pair(paths)
    objs = big_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and twin.update_prims(objs, p3d.UPDATE_REFIT) > 0
    fresh = check_rebuilt(hs, dev, twin, built)
    for (rgb_a, hit_a, st_a), (rgb_b, hit_b, st_b) in zip(frame_bytes(dev), frame_bytes(fresh)):
        assert hit_a == hit_b and rgb_a == rgb_b
        assert st_a == st_b, "counters %s / %s" % (st_a, st_b)
    # ... and the topology a later REFIT keeps is the rebuilt one
    objs = small_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and fresh.update_prims(objs, p3d.UPDATE_REFIT) > 0
    assert same_export(dev.export_bvh(), fresh.export_bvh())
    assert (dev.bvh_cost()["last_update_rebuilt"], dev.bvh_cost()["refits_since_build"]) == (0, 1)


def test_a_rebuild_with_the_policy_on_records_the_baseline(paths):
    hs, dev, twin, built = pair(paths)
    objs = big_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REBUILD) > 0 and twin.update_prims(objs, p3d.UPDATE_REBUILD) > 0
    assert same_export(dev.export_bvh(), twin.export_bvh())
    c = dev.bvh_cost()
    assert f64_bytes(c["sah_baseline"]) == f64_bytes(c["sah"]) and c["sah"] != built
    assert (c["last_update_rebuilt"], c["refits_since_build"]) == (1, 0)


def test_the_policy_through_transforms(paths):
    """A slide of every object by a thousandth of the diagonal, then a scatter of every third by a matrix of its own"""
    hs, dev, twin, built = pair(paths)
    rest = hs.arrays()
    n = rest["n_prims"]
    objs, off = big_offsets(rest)
    diag = float(np.linalg.norm(rest["prim_bmax"].max(0).astype(np.float64) - rest["prim_bmin"].min(0).astype(np.float64)))
    slide = IDENTITY[None].copy()
    slide[0, :, 3] = (0.001 * diag, 0, 0)
    ranges = [(0, n, 0)]
    assert dev.transform_prims(ranges, slide, p3d.UPDATE_REFIT) > 0 and twin.transform_prims(ranges, slide, p3d.UPDATE_REFIT) > 0
    check_kept(dev, twin, built)
    scatter = np.repeat(IDENTITY[None], len(objs), 0)
    scatter[:, :, 3] = off
    ranges = [(int(o), 1, i) for i, o in enumerate(objs)]
    assert dev.transform_prims(ranges, scatter, p3d.UPDATE_REFIT) > 0 and twin.transform_prims(ranges, scatter, p3d.UPDATE_REFIT) > 0
    # the host route to the same objects: the slide for those no range of the second call names, the scatter for the others
    hs.set_geometry(*p3d.transformed(rest["prim_type"], rest["prim_v"], [(0, n, 0)], slide))
    hs.set_geometry(*p3d.transformed(rest["prim_type"], rest["prim_v"], ranges, scatter))
    check_rebuilt(hs, dev, twin, built)


def test_the_policy_on_a_scene_with_a_device_grid(paths):
    hs, dev, twin, built = pair(paths, grid="device")
    objs = big_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and twin.update_prims(objs, p3d.UPDATE_REFIT) > 0
    fresh = check_rebuilt(hs, dev, twin, built, grid="device")
    got, want = dev.export_grid(), fresh.export_grid()
    assert got["grid_n"] == want["grid_n"]
    for k in ("grid_bmin", "grid_bmax", "grid_cell_start", "grid_cell_items"):
        assert got[k].tobytes() == want[k].tobytes(), k


# ---- 6. ratio 0 and +inf -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ratio", [0.0, float("inf")])
def test_ratio_0_and_infinity_never_rebuild(ratio, paths):
    hs, dev, twin, built = pair(paths)
    dev.set_auto_rebuild(ratio)  # (0 after a set: off again)
    assert dev.auto_rebuild() == ratio
    objs = big_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and twin.update_prims(objs, p3d.UPDATE_REFIT) > 0
    assert statement(twin.export_bvh())[0] / built > 1.5
    assert same_export(dev.export_bvh(), twin.export_bvh())
    c = dev.bvh_cost()
    assert (c["last_update_rebuilt"], c["refits_since_build"]) == (0, 1)
    if ratio == 0.0:
        assert c["sah_baseline"] == 0.0  # nothing was measured
    else:
        assert abs(c["sah_baseline"] - built) <= 1e-9 * built
        dev.set_auto_rebuild(0)
        assert dev.auto_rebuild() == 0.0
    objs = small_move(hs)
    assert dev.update_prims(objs, p3d.UPDATE_REFIT) > 0 and twin.update_prims(objs, p3d.UPDATE_REFIT) > 0
    assert same_export(dev.export_bvh(), twin.export_bvh())
    assert dev.bvh_cost()["refits_since_build"] == 2


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals(paths):
    hs = p3d.HostScene(paths["count513"])
    uploaded = p3d.DeviceScene(hs, bvh=True)
    for call in (lambda: uploaded.set_auto_rebuild(2.0), uploaded.bvh_cost, uploaded.auto_rebuild):
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == -1
    dev = p3d.DeviceScene(hs, bvh="device")
    for start in (0.0, 2.0):
        dev.set_auto_rebuild(start)
        for bad in (0.5, float("nan"), -1.0, float("-inf"), 0.999):
            with pytest.raises(p3d.P3DError) as e:
                dev.set_auto_rebuild(bad)
            assert e.value.code == -1
            assert dev.auto_rebuild() == start
    dev.set_auto_rebuild(1.0)
    assert dev.auto_rebuild() == 1.0
