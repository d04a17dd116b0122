"""The pose of a rigged live scene from device matrices on the caller's stream (p3d_scene_set_rig, p3d_scene_pose_device) on
the GPU.

The yardstick is exact: scene B takes set_rig + pose_device with its numbers in device tensors, its twin A takes
transform_prims(the same ranges, the same float32 numbers, UPDATE_REFIT), and the two are compared with the helpers of the
transform and stream-refit tests (frames in both stack modes as uint32, hit IDs, counters, the exported tree).  Every
comparison here has tolerance 0.  The scenes have no device-built grid (the stream form refuses those: see the refusals).
Where the matrices are produced on the GPU, the twin is given the bits read back from the tensor the call was given.

status() returns the code of p3d_scene_status (it does not raise): a skipped object shows as status() == -1 with the two
counts in p3d_last_error, and a second status() is 0.

Not asserted: that a pose allocates nothing.  There is no instrument for it; it holds by construction (the rig, the rest
copy, the counter block and the builder's state are made by set_rig, the matrices are the caller's), and the loop time of
profiles/tools/stream_pose_probe.py is the evidence."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import p3d_amd as p3d
from conftest import scene_path
from device_query_contract import INVALID, UNSUPPORTED
from device_geometry_helpers import deformed_mesh
from scene_update_helpers import BOX, PLANE, SPHERE, TRIANGLE, random_moves
from frame_checks import CORNELL, PLANES, RENDER_COUNTERS, assert_same_frames, assert_same_tree, frames, frames_differ, gpu, load
from live_scene_checks import (HEAD, IDENTITY, LEAF, RES, SCENES, SEED, TRACE_OUT, assert_same_frames_and_tree, box_move,
                               camera_rays, configs, kinds_of, last_error, legacy, plan, produced, rigid, runs, scene,
                               trace_outputs)

pytestmark = pytest.mark.gpu

MOVABLE = (SPHERE, TRIANGLE)


@pytest.fixture
def paths(tri5k_path):
    return {"balls_low": scene_path("balls_low.p3f"), "tri5k": tri5k_path, "balls_box": scene_path("balls_box.p3f"), "cornell": CORNELL}


def twins(path, res=RES):
    """(host scene, its arrays, scene A for the waiting form, scene B for the stream form)"""
    hs = load(path, res, legacy_f11=legacy(path))
    return hs, hs.arrays(), scene(hs), scene(hs)


def both(dev_a, dev_b, ranges, xforms, scale=None, twin_ranges=None):
    """B: pose_device on a side stream with the numbers in device tensors; A: the waiting form with the same numbers"""
    xforms = np.ascontiguousarray(xforms, np.float32).reshape(-1, 3, 4)
    scale = None if scale is None else np.ascontiguousarray(scale, np.float32)
    d_x, d_s = gpu(xforms), None if scale is None else gpu(scale)
    side = torch.cuda.Stream()
    dev_b.pose_device(d_x, d_s, stream=side)
    side.synchronize()
    assert dev_a.transform_prims(ranges if twin_ranges is None else twin_ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale) > 0


def moves(a, seed, k, reach=0.05):
    rng = np.random.default_rng(seed)
    return np.stack([rigid(a, rng, reach=reach * (1 + 0.1 * i)) for i in range(k)])


def untouched_leaves(tree, covered):
    """The leaves of an exported tree that hold none of the `covered` objects, and the others"""
    leaves = np.nonzero(tree["bvh_count_leaf"] & LEAF)[0]
    free = [l for l in leaves
            if not covered[tree["bvh_order"][tree["bvh_index"][l]:tree["bvh_index"][l] + (tree["bvh_count_leaf"][l] & ~LEAF)]].any()]
    kept = set(free)
    return free, [l for l in leaves if l not in kept]


def covered_by(ranges, n):
    covered = np.zeros(n, bool)
    for first, count, _ in ranges:
        covered[first:first + count] = True
    return covered


# 1. every scene of the transform tests, the matrices produced on a stream that is still working on them
@pytest.mark.parametrize("name", SCENES)
def test_the_stream_form_is_the_waiting_form(name, paths):
    hs, a, dev_a, dev_b = twins(paths[name])
    before = frames(dev_b, configs(name))
    ranges, _, _ = plan(a, 0)  # spheres and triangles on slot 0, boxes on slot 1; a plane is in no range
    posed = sum(c for _, c, _ in ranges)
    assert posed == int((a["prim_type"] != PLANE).sum()) > 0
    assert dev_b.rig() == dict(n_ranges=0, n_xforms=0, n_posed_objects=0)
    dev_b.set_rig(ranges, 2)
    assert dev_b.rig() == dict(n_ranges=len(ranges), n_xforms=2, n_posed_objects=posed)
    assert_same_frames(frames(dev_b, configs(name)), before, "set_rig moves nothing")
    side = torch.cuda.Stream()
    ballast = torch.linspace(0, 1, 1 << 20, device="cuda")
    last = before
    for round_ in range(2):  # round two: both start from the REST pose, not from round one's result
        _, xforms, scale = plan(a, SEED[name] + 40 + 100 * round_)  # rigid + spheres that grow; positive-diagonal for boxes
        base_x, base_s = gpu(xforms), gpu(scale)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            slow = produced(ballast, 1.0, rounds=20)
            d_x = (base_x + 0.0 * slow[:24].view(2, 3, 4)).contiguous()
            d_s = (base_s + 0.0 * slow[24:26]).contiguous()
            dev_b.pose_device(d_x, d_s, stream=side)  # no synchronisation between producer and call
        side.synchronize()
        x_bits, s_bits = d_x.cpu().numpy(), d_s.cpu().numpy()
        assert np.isfinite(x_bits).all() and np.array_equal(x_bits, xforms) and np.array_equal(s_bits, scale)
        assert dev_a.transform_prims(ranges, x_bits, p3d.UPDATE_REFIT, sphere_scale=s_bits) > 0
        now = assert_same_frames_and_tree(dev_a, dev_b, name, "%s, round %d" % (name, round_))
        assert frames_differ(now, last), "the pose changed no pixel"
        last = now
    assert dev_b.status() == 0


# 2. the smallest trees
@pytest.mark.parametrize("kind", ["spheres", "triangles"])
@pytest.mark.parametrize("n_objs", [1, 2, 3])
def test_tiny_scenes(n_objs, kind, tmp_path):
    """One object: the root is the only leaf.  Two: one internal node, emitted as a leaf of two.  Three: the first tree with
    an inner node above a leaf.  Every object is a body of its own."""
    if kind == "spheres":
        objs = ["s %g 0 0 0.6" % (1.4 * k - 1.4) for k in range(n_objs)]
    else:
        objs = ["p 3 %g -0.2 -0.6 %g 0.1 -0.5 %g 0 0.7" % (1.4 * k - 1.9, 1.4 * k - 0.8, 1.4 * k - 1.4) for k in range(n_objs)]
    path = str(tmp_path / "tiny.p3f")
    with open(path, "w") as f:
        f.write("\n".join(HEAD + objs) + "\n")
    hs, a, dev_a, dev_b = twins(path, 64)
    assert a["n_prims"] == n_objs
    before = frames(dev_b, configs("tiny"))
    ranges = [(k, 1, n_objs - 1 - k) for k in range(n_objs)]
    dev_b.set_rig(ranges, n_objs)
    rng = np.random.default_rng(140 + n_objs)
    both(dev_a, dev_b, ranges, moves(a, 150 + n_objs, n_objs), rng.uniform(0.7, 1.2, n_objs))
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, "tiny", "%d %s" % (n_objs, kind)), before)
    assert dev_b.status() == 0


# 3. ranges and untouched objects
def test_range_boundaries_and_untouched_objects(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"])
    n = a["n_prims"]
    assert (n - 1) % 256 and n > 2000
    ranges, end = [], n  # one object, a wave's end either side, a block's end either side; gaps between them; descending
    for slot, count in enumerate((257, 256, 255, 65, 64, 63, 1)):
        ranges.append((end - count, count, slot))
        end -= count + 37
    assert ranges[0][0] + ranges[0][1] == n and [r[0] for r in ranges] == sorted((r[0] for r in ranges), reverse=True)
    covered = covered_by(ranges, n)
    tree0 = dev_b.export_bvh()
    dev_b.set_rig(ranges, len(ranges))
    assert dev_b.rig()["n_posed_objects"] == int(covered.sum())
    both(dev_a, dev_b, ranges, moves(a, 301, len(ranges), reach=0.02))
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "seven ranges")
    # the unnamed objects keep their exact bits: every leaf that holds none of the covered objects has the box it had
    tree1 = dev_b.export_bvh()
    for k in ("bvh_index", "bvh_count_leaf", "bvh_order"):
        assert np.array_equal(tree0[k], tree1[k]), k
    free, moved = untouched_leaves(tree1, covered)
    assert len(free) > len(moved) > 0
    for k in ("bvh_bmin", "bvh_bmax"):
        assert tree0[k][free].tobytes() == tree1[k][free].tobytes(), k
    assert tree0["bvh_bmin"][moved].tobytes() != tree1["bvh_bmin"][moved].tobytes()
    assert dev_b.status() == 0


def test_forty_ranges_and_shared_slots(paths):
    """More ranges than the 16 sources the argument route of refit_device carries; every slot is shared by two ranges"""
    hs, a, dev_a, dev_b = twins(paths["tri5k"])
    n = a["n_prims"]
    rng = np.random.default_rng(302)
    ranges = [(120 * k, 1 + 2 * k, k % 20) for k in range(40)]
    assert ranges[-1][0] + ranges[-1][1] <= n
    ranges = [ranges[i] for i in rng.permutation(len(ranges))]
    before = dev_b.export_bvh()
    dev_b.set_rig(ranges, 20)
    assert dev_b.rig() == dict(n_ranges=40, n_xforms=20, n_posed_objects=sum(c for _, c, _ in ranges))
    both(dev_a, dev_b, ranges, moves(a, 303, 20, reach=0.02))
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "forty ranges")
    assert dev_b.export_bvh()["bvh_bmin"].tobytes() != before["bvh_bmin"].tobytes()
    assert dev_b.status() == 0


# 4. the rest pose
def test_the_identity_brings_the_rest_pose_back_and_a_pose_is_idempotent(paths):
    name = "balls_low"
    hs, a, dev, fresh = twins(paths[name])
    assert not (np.signbit(a["prim_v"]) & (a["prim_v"] == 0)).any()  # (1 * -0 + 0 is +0: the one value the identity changes)
    ranges, xforms, scale = plan(a, SEED[name] + 43)
    dev.set_rig(ranges, 2)
    d_x, d_s = gpu(xforms), gpu(scale)
    dev.pose_device(d_x, d_s)
    once_frames, once_tree = frames(dev, configs(name)), dev.export_bvh()
    assert frames_differ(once_frames, frames(fresh, configs(name)))
    dev.pose_device(d_x, d_s)  # T(rest) again, not T(T(rest))
    assert_same_frames(frames(dev, configs(name)), once_frames, "the same pose twice")
    assert_same_tree(dev.export_bvh(), once_tree, "the same pose twice")
    dev.pose_device(gpu(np.stack([IDENTITY, IDENTITY])))  # no scales: 1 for every slot
    assert_same_frames_and_tree(fresh, dev, name, "the identity after a pose")
    assert dev.status() == 0


@pytest.mark.parametrize("route", ["update_prims", "refit_triangles"])
def test_another_route_moves_the_rest_pose(route, paths):
    """B is rigged first, so the other route has to write B's rest copy; A's rest copy is made by its first transform from
    what that route left.  The next pose starts from the new rest on both."""
    name = "balls_low" if route == "update_prims" else "tri5k"
    hs, a, dev_a, dev_b = twins(paths[name])
    n = a["n_prims"]
    ranges = [(f, c, k % 2) for k, (f, c) in enumerate(runs(a["prim_type"], MOVABLE))] if name == "balls_low" else [(0, n // 2, 0), (n // 2, n - n // 2, 1)]
    dev_b.set_rig(ranges, 2)
    if route == "update_prims":
        objs, new_v = random_moves(a, 77, fraction=0.5)
        hs.set_geometry(objs, new_v)
        for dev in (dev_a, dev_b):
            dev.update_prims(objs, p3d.UPDATE_REFIT)
    else:
        soup = gpu(deformed_mesh(a, seed=78, fraction=0.03)[2])
        side = torch.cuda.Stream()
        dev_b.refit_triangles(0, soup, stream=side)
        side.synchronize()
        dev_a.update_triangles(0, soup, mode=p3d.UPDATE_REFIT)
    moved = assert_same_frames_and_tree(dev_a, dev_b, name, "the other route")
    both(dev_a, dev_b, ranges, moves(a, 79, 2))
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, name, "a pose from the new rest"), moved)
    if route == "update_prims":  # the identity gives the updated host scene: after a rebuild, a fresh scene of it, tree and all
        assert not (np.signbit(hs.arrays()["prim_v"]) & (hs.arrays()["prim_v"] == 0)).any()
        dev_b.pose_device(gpu(np.stack([IDENTITY, IDENTITY])))
        dev_b.update_geometry_device([], p3d.UPDATE_REBUILD)
        assert_same_frames_and_tree(scene(hs), dev_b, name, "the identity after update_prims")
    assert dev_b.status() == 0


def test_after_a_rebuild_that_changed_the_order(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"])
    n = a["n_prims"]
    k = 25
    ranges = [(i * (n // k), n // k, i) for i in range(k)]
    dev_b.set_rig(ranges, k)
    both(dev_a, dev_b, ranges, moves(a, 304, k, reach=0.3))  # every body thrown somewhere else in the scene
    refitted = dev_b.export_bvh()
    for dev in (dev_a, dev_b):
        dev.update_geometry_device([], p3d.UPDATE_REBUILD)
    built = dev_b.export_bvh()
    assert built["bvh_order"].tobytes() != refitted["bvh_order"].tobytes()
    assert dev_b.rig()["n_ranges"] == k  # the rig stands: a rebuild reorders leaves, not objects
    both(dev_a, dev_b, ranges, moves(a, 305, k, reach=0.29))  # over the NEW topology, with the new tree's depth
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "a pose of a rebuilt tree")
    assert dev_b.export_bvh()["bvh_order"].tobytes() == built["bvh_order"].tobytes()
    assert dev_b.status() == 0


# 5. three steps in a row on one stream, no host wait between them
def test_three_steps_without_a_host_wait(paths):
    hs, a, dev_a, dev_b = twins(paths["tri5k"])
    n, k, n_rays = a["n_prims"], 8, 4096
    ranges = [(i * (n // k), n // k, i) for i in range(k)]
    o, d = camera_rays(a, n_rays, seed=31)
    base = [gpu(moves(a, 310 + step, k, reach=0.04)) for step in range(3)]
    want = [w for w, _, _ in TRACE_OUT]
    outs_b = [trace_outputs(n_rays) for _ in base]
    dev_b.set_rig(ranges, k)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    poses = []
    with torch.cuda.stream(side):
        for m, out in zip(base, outs_b):
            poses.append((m + 0.01 * torch.sin(3.0 * m)).contiguous())  # this step's matrices, made on the stream
            dev_b.pose_device(poses[-1], stream=side)
            dev_b.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, stream=side, out=out)
    side.synchronize()
    outs_a = []
    for x in poses:
        dev_a.transform_prims(ranges, x.cpu().numpy(), p3d.UPDATE_REFIT)
        outs_a.append(dev_a.trace_closest_device(p3d.ACCEL_BVH, o, d, want=want, out=trace_outputs(n_rays)))
        torch.cuda.synchronize()
    for step, (got, ref) in enumerate(zip(outs_b, outs_a)):
        # (a check of this test's rays, not of the pose: hundreds of them end on the mesh, which is sparse; that they tell
        # the steps apart is asserted below)
        assert (ref["hit_id"] >= 0).sum() > n_rays // 8, "step %d: the rays miss the mesh" % step
        for name in want:
            assert got[name].cpu().numpy().tobytes() == ref[name].cpu().numpy().tobytes(), "step %d: %s differs" % (step, name)
    for step in range(2):  # trace k saw pose k, and neither its neighbour's
        assert outs_a[step]["t"].cpu().numpy().tobytes() != outs_a[step + 1]["t"].cpu().numpy().tobytes()
    assert dev_b.status() == 0


# 6. per-object skips
def run_skip_case(a, dev_a, dev_b, name, ranges, first, xforms, scale, bad_slots, counts):
    """Both scenes are first posed well.  Then B is posed with everything, A with the ranges of the good slots only (and
    harmless numbers in the bad ones: the waiting form refuses the whole call otherwise): the skipped objects stay where the
    first pose put them, on both."""
    k = len(xforms)
    both(dev_a, dev_b, ranges, first)  # a good pose: what the skipped objects must keep
    posed = assert_same_frames_and_tree(dev_a, dev_b, name, "the good pose")
    xforms = np.ascontiguousarray(xforms, np.float32).reshape(k, 3, 4)
    scale = np.ones(k, np.float32) if scale is None else np.ascontiguousarray(scale, np.float32)
    d_x, d_s = gpu(xforms), gpu(scale)
    side = torch.cuda.Stream()
    assert p3d.lib().p3d_scene_pose_device(dev_b._h, k, d_x.data_ptr(), d_s.data_ptr(), C.c_void_p(side.cuda_stream)) == 0  # P3D_OK
    side.synchronize()
    good = [r for r in ranges if r[2] not in bad_slots]
    safe_x, safe_s = xforms.copy(), scale.copy()
    for s in bad_slots:
        safe_x[s], safe_s[s] = IDENTITY, 1.0
    assert dev_a.transform_prims(good, safe_x, p3d.UPDATE_REFIT, sphere_scale=safe_s) > 0
    # frames rendered with stats in between neither report the skips nor clear them (B's renders return normally)
    now = assert_same_frames_and_tree(dev_a, dev_b, name, "the skipped objects where they were, the others moved")
    assert frames_differ(now, posed)
    assert dev_b.status() == INVALID
    msg = last_error()
    assert "p3d_scene_pose_device: %d object(s) with an unusable transform" % counts[0] in msg, msg
    assert "%d object(s) with a non-finite or inverted box" % counts[1] in msg, msg
    assert dev_b.status() == 0
    # the scene goes on: the next pose is exact again, and the counts start from zero
    both(dev_a, dev_b, ranges, first)
    assert_same_frames_and_tree(dev_a, dev_b, name, "after the skips")
    assert dev_b.status() == 0


def three_bodies(a):
    """balls_low: the triangles on slot 0, the spheres in two halves on slots 1 and 2"""
    tri, sph = kinds_of(a)
    half = len(sph) // 2
    assert len(tri) >= 2 and half >= 2
    return [(int(tri[0]), len(tri), 0), (int(sph[0]), half, 1), (int(sph[0]) + half, len(sph) - half, 2)]


def test_a_nan_in_one_matrix(paths):
    name = "balls_low"
    hs, a, dev_a, dev_b = twins(paths[name])
    ranges = three_bodies(a)
    dev_b.set_rig(ranges, 3)
    xforms = moves(a, 321, 3)
    xforms[1, 2, 1] = np.nan
    run_skip_case(a, dev_a, dev_b, name, ranges, moves(a, 322, 3), xforms, [1.1, 1.2, 0.9], {1}, (ranges[1][1], 0))


@pytest.mark.parametrize("slot, value", [(2, 0.0), (2, -1.0), (2, float("nan")), (2, float("inf")), (0, -1.0)])
def test_a_bad_sphere_scale(slot, value, paths):
    """The scale is checked for every object of its slot, triangles too: the waiting form refuses such a transform whatever
    it moves (slot 0 holds the triangles)"""
    name = "balls_low"
    hs, a, dev_a, dev_b = twins(paths[name])
    ranges = three_bodies(a)
    dev_b.set_rig(ranges, 3)
    scale = np.array([1.0, 1.25, 0.8], np.float32)
    scale[slot] = value
    run_skip_case(a, dev_a, dev_b, name, ranges, moves(a, 323, 3), moves(a, 324, 3), scale, {slot}, (ranges[slot][1], 0))


def test_a_rotation_on_a_slot_that_holds_a_box(paths):
    """One body of spheres, triangles and a box: under a rotation the box stays, the others turn.  Under a positive-diagonal
    matrix the box goes along."""
    name = "balls_box"
    hs, a, dev_a, dev_b = twins(paths[name])
    n = a["n_prims"]
    kinds = a["prim_type"]
    assert not (kinds == PLANE).any()
    boxes = int((kinds == BOX).sum())
    assert boxes >= 1
    ranges = [(0, n, 0)]
    dev_b.set_rig(ranges, 1)
    first = box_move(a, np.random.default_rng(325))[None]
    k = 1
    both(dev_a, dev_b, ranges, first)
    posed = assert_same_frames_and_tree(dev_a, dev_b, name, "a positive-diagonal pose of everything")
    turn = moves(a, 326, 1)
    d_x = gpu(turn)
    assert p3d.lib().p3d_scene_pose_device(dev_b._h, k, d_x.data_ptr(), None, None) == 0
    assert dev_a.transform_prims([(f, c, 0) for f, c in runs(kinds, MOVABLE)], turn, p3d.UPDATE_REFIT) > 0
    assert frames_differ(assert_same_frames_and_tree(dev_a, dev_b, name, "the box where it was, the others turned"), posed)
    assert dev_b.status() == INVALID
    msg = last_error()
    assert "%d object(s) with an unusable transform" % boxes in msg and " 0 object(s) with a non-finite or inverted box" in msg, msg
    assert dev_b.status() == 0


def test_a_box_that_overflows(paths):
    """Finite numbers that leave float32: the box's x extent times 3e38 plus a translation of 3e38 is infinite at its upper
    end.  The kernel leaves the box unwritten and counts it in the second counter: no fault is provoked."""
    name = "balls_box"
    hs, a, dev_a, dev_b = twins(paths[name])
    kinds = a["prim_type"]
    ranges, _, _ = plan(a, 0)
    box_rows = a["prim_v"][kinds == BOX]
    far = IDENTITY.copy()
    far[0, 0], far[0, 3] = 3e38, 3e38
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(3e38) * box_rows[:, 3] + np.float32(3e38)).all()
    dev_b.set_rig(ranges, 2)
    rng = np.random.default_rng(327)
    first = np.stack([rigid(a, rng), box_move(a, rng)])
    xforms = np.stack([rigid(a, rng), far])
    run_skip_case(a, dev_a, dev_b, name, ranges, first, xforms, [1.25, 1.0], {1}, (0, len(box_rows)))


# 7. refusals, nothing changed
def _set_rig(dev, ranges, n_xforms, n=None, null=False):
    rg = (p3d.XformRange * max(len(ranges), 1))(*[p3d.XformRange(*r) for r in ranges])
    return p3d.lib().p3d_scene_set_rig(dev._h if dev is not None else None, len(ranges) if n is None else n,
                                       None if null else C.cast(rg, C.c_void_p), n_xforms)


def _pose(dev, k, d_x, d_s=None, stream=None):
    return p3d.lib().p3d_scene_pose_device(dev._h if dev is not None else None, k, d_x, d_s, stream)


def test_refusals_leave_the_scene_as_it_was(paths):
    name = "balls_box"
    hs = load(paths[name], RES, legacy_f11=legacy(paths[name]))
    a = hs.arrays()
    n = a["n_prims"]
    sphere = int(np.nonzero(a["prim_type"] == SPHERE)[0][0])
    box = int(np.nonzero(a["prim_type"] == BOX)[0][0])
    dev, twin, policy = scene(hs), scene(hs), scene(hs)  # (before the host scene builds a grid: its descriptor carries one from then on)
    host_tree = p3d.DeviceScene(hs, bvh=True)
    device_grid = p3d.DeviceScene(hs, bvh="device", grid="device")
    uploaded_grid = p3d.DeviceScene(hs, bvh="device", grid=True)
    hp = load(PLANES, RES)
    plane = int(np.nonzero(hp.arrays()["prim_type"] == PLANE)[0][0])
    dev_planes = scene(hp)
    slide = IDENTITY.copy()
    slide[:, 3] = (0.25, 0.1, -0.2)
    d_x = gpu(np.stack([slide, slide]))
    d_s = gpu(np.array([1.1, 1.0], np.float32))
    host_x = np.ascontiguousarray(np.stack([slide, slide]))  # numpy arrays: host memory
    host_s = np.ones(2, np.float32)
    good = [(sphere, 3, 0, 0), (box, 1, 1, 0)]
    none = dict(n_ranges=0, n_xforms=0, n_posed_objects=0)

    # set_rig
    for what, other in (("a scene with the host's tree", host_tree), ("a scene with an uploaded grid", uploaded_grid)):
        was = frames(other, configs(name))
        assert _set_rig(other, good, 2) == INVALID, what
        assert last_error().startswith("p3d_scene_set_rig"), what
        assert _pose(other, 2, d_x.data_ptr()) == INVALID, what
        assert last_error().startswith("p3d_scene_pose_device"), what
        assert other.rig() == none
        assert_same_frames(frames(other, configs(name)), was, what)
    assert _set_rig(None, good, 2) == INVALID and _pose(None, 2, d_x.data_ptr()) == INVALID
    was_planes = frames(dev_planes, configs(name))
    assert _set_rig(dev_planes, [(plane, 1, 0, 0)], 1) == INVALID and "plane" in last_error()
    assert dev_planes.rig() == none
    assert_same_frames(frames(dev_planes, configs(name)), was_planes, "a range that covers a plane")
    was, tree = frames(dev, configs(name)), dev.export_bvh()
    rig_cases = [
        ("null ranges with a count", dict(ranges=good, n_xforms=2, null=True)),
        ("ranges without transforms", dict(ranges=good, n_xforms=0)),
        ("an empty range", dict(ranges=[(sphere, 0, 0, 0)], n_xforms=1)),
        ("a range behind the last object", dict(ranges=[(n - 1, 2, 0, 0)], n_xforms=1)),
        ("a range whose end wraps", dict(ranges=[(0xffffffff, 2, 0, 0)], n_xforms=1)),
        ("a slot that is not there", dict(ranges=[(sphere, 1, 1, 0)], n_xforms=1)),
        ("the slot of an unrigged object", dict(ranges=[(sphere, 1, 0xffffffff, 0)], n_xforms=1)),
        ("reserved in a range", dict(ranges=[(sphere, 1, 0, 1)], n_xforms=1)),
        ("overlapping ranges", dict(ranges=[(sphere, 3, 0, 0), (sphere + 2, 2, 0, 0)], n_xforms=1)),
        ("overlapping ranges, shuffled", dict(ranges=[(sphere + 4, 2, 0, 0), (sphere, 6, 0, 0), (sphere + 20, 1, 0, 0)], n_xforms=1)),
        ("the same range twice", dict(ranges=[(sphere, 1, 0, 0), (sphere, 1, 0, 0)], n_xforms=1)),
        ("a fault in the second range", dict(ranges=[(sphere, 1, 0, 0), (sphere + 2, 1, 1, 0)], n_xforms=1)),
    ]
    for rigged in (False, True):  # without a rig, and with one that every refusal must leave standing
        for what, kw in rig_cases:
            assert _set_rig(dev, **kw) == INVALID, what
            assert last_error().startswith("p3d_scene_set_rig"), what
            assert dev.rig() == (dict(n_ranges=2, n_xforms=2, n_posed_objects=4) if rigged else none), what
        assert_same_frames(frames(dev, configs(name)), was, "set_rig refusals")
        assert_same_tree(dev.export_bvh(), tree, "set_rig refusals")
        if not rigged:
            # pose without a rig
            assert _pose(dev, 2, d_x.data_ptr(), d_s.data_ptr()) == INVALID and "no rig" in last_error()
            assert _set_rig(dev, good, 2) == 0
            assert_same_frames(frames(dev, configs(name)), was, "set_rig moves nothing")
    # overlap is worded as in the waiting form
    assert _set_rig(dev, [(sphere, 3, 0, 0), (sphere + 2, 2, 0, 0)], 1) == INVALID and "object %d is in two ranges" % (sphere + 2) in last_error()

    # pose_device, on the rigged scene
    big = 1 << 24
    pose_cases = [
        ("one transform too few", (1, d_x.data_ptr(), d_s.data_ptr())),
        ("one transform too many", (3, d_x.data_ptr(), d_s.data_ptr())),
        ("no transforms", (0, d_x.data_ptr(), None)),
        ("null d_xforms", (2, None, d_s.data_ptr())),
        ("d_xforms off by two bytes", (2, d_x.data_ptr() + 2, d_s.data_ptr())),
        ("d_sphere_scale off by one byte", (2, d_x.data_ptr(), d_s.data_ptr() + 1)),
        ("host memory as d_xforms", (2, host_x.ctypes.data, None)),
        ("host memory as d_sphere_scale", (2, d_x.data_ptr(), host_s.ctypes.data)),
    ]
    # Host memory must be refused BEFORE any launch.  It goes to the scene with a device grid first: were the pointer check to
    # let it through, the grid (checked behind it) would still refuse the call, and no kernel would ever be given a host address.
    device_grid.set_rig([r[:3] for r in good], 2)
    for what, px, ps in (("d_xforms", host_x.ctypes.data, None), ("d_sphere_scale", d_x.data_ptr(), host_s.ctypes.data)):
        assert _pose(device_grid, 2, px, ps) == INVALID, what
        assert "is host memory" in last_error() and what in last_error(), last_error()
    for what, (k, px, ps) in pose_cases:
        assert _pose(dev, k, px, ps) == INVALID, what
        assert last_error().startswith("p3d_scene_pose_device"), what
        assert_same_frames(frames(dev, configs(name)), was, what)
        assert_same_tree(dev.export_bvh(), tree, what)
    assert _pose(dev, 2, host_x.ctypes.data, None) == INVALID and "is host memory" in last_error() and "d_xforms" in last_error()
    # matrices that end behind their allocation: a rig of 2^24 slots whose ranges name the first two (were the runtime unable
    # to report the range, the kernel would still read nothing outside the tensor)
    assert _set_rig(dev, good, big) == 0
    assert _pose(dev, big, d_x.data_ptr(), None) == INVALID and "ends behind its allocation" in last_error(), last_error()
    assert _pose(dev, big, d_x.data_ptr(), d_s.data_ptr()) == INVALID
    assert_same_frames(frames(dev, configs(name)), was, "matrices that end behind their allocation")
    assert _set_rig(dev, good, 2) == 0
    # a device grid, and the policy: the stream form is refused, the waiting form works
    xf = np.stack([slide, slide])
    scale = np.array([1.1, 1.0], np.float32)
    plain = [r[:3] for r in good]
    assert device_grid.rig()["n_posed_objects"] == 4
    was_grid = frames(device_grid, configs(name))
    assert _pose(device_grid, 2, d_x.data_ptr(), d_s.data_ptr()) == UNSUPPORTED
    assert last_error().startswith("p3d_scene_pose_device") and "p3d_scene_transform_prims" in last_error()
    assert_same_frames(frames(device_grid, configs(name)), was_grid, "a scene with a device-built grid")
    assert device_grid.transform_prims(plain, xf, p3d.UPDATE_REFIT, sphere_scale=scale) > 0
    dev.set_auto_rebuild(1.01)
    assert _pose(dev, 2, d_x.data_ptr(), d_s.data_ptr()) == UNSUPPORTED and "auto-rebuild" in last_error()
    assert_same_frames(frames(dev, configs(name)), was, "the policy is on")
    policy.set_auto_rebuild(1.01)
    assert policy.transform_prims(plain, xf, p3d.UPDATE_REFIT, sphere_scale=scale) > 0
    dev.set_auto_rebuild(0)
    assert dev.bvh_cost()["refits_since_build"] == 0
    assert dev.status() == 0
    # the same call without a fault is accepted
    assert _pose(dev, 2, d_x.data_ptr(), d_s.data_ptr()) == 0
    twin.transform_prims(plain, xf, p3d.UPDATE_REFIT, sphere_scale=scale)
    assert frames_differ(assert_same_frames_and_tree(twin, dev, name, "the accepted call"), was)
    # no ranges: the rig goes, and rig() says so
    assert _set_rig(dev, [], 0) == 0 and dev.rig() == none
    assert _pose(dev, 2, d_x.data_ptr(), d_s.data_ptr()) == INVALID and "no rig" in last_error()
    dev.set_rig([], 5)
    assert dev.rig() == none
    assert_same_frames_and_tree(twin, dev, name, "after the rig is gone")
    assert dev.status() == 0


# 8. accumulators and the cost record
def test_accumulators_and_bvh_cost(paths):
    hs = load(paths["cornell"], 64)
    a = hs.arrays()
    dev_a, dev_b = scene(hs), scene(hs)
    ranges, xforms, scale = plan(a, SEED["cornell"] + 45)
    cfg = p3d.pathtrace_config(accel=p3d.ACCEL_BVH, spp_sqrt=3, max_depth=8, seed=9)
    dev_b.set_rig(ranges, 2)
    acc = dev_b.accumulator(cfg)
    acc.render(2)
    was = dev_b.bvh_cost()
    dev_b.pose_device(gpu(xforms), gpu(scale))
    with pytest.raises(p3d.P3DError) as e:
        acc.render(1)
    assert e.value.code == INVALID and "moved" in str(e.value)
    assert acc.samples_done == 2
    acc.reset()
    acc.render(1)
    acc.close()
    dev_a.transform_prims(ranges, xforms, p3d.UPDATE_REFIT, sphere_scale=scale)
    cost_a, cost_b = dev_a.bvh_cost(), dev_b.bvh_cost()
    assert cost_b["refits_since_build"] == was["refits_since_build"] + 1 and cost_b["last_update_rebuilt"] == 0
    assert np.float64(cost_b["sah"]).tobytes() == np.float64(cost_a["sah"]).tobytes() and cost_b["sah"] != was["sah"]
    assert cost_a == cost_b, (cost_a, cost_b)


# 9. a frame that reads the root box
def test_a_per_level_frame_after_a_pose(paths):
    hs = load(paths["tri5k"], 128)
    a = hs.arrays()
    n = a["n_prims"]
    dev_a, dev_b = scene(hs), scene(hs)
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4, chain_launch=p3d.CHAIN_PER_LEVEL, collect_stats=1)
    before = dev_b.render(cfg)
    # the mesh grows by a fifth about a corner: the root box it is binned by moves
    corner = a["prim_bmin"].min(0).astype(np.float32)
    grow = np.zeros((1, 3, 4), np.float32)
    grow[0, :, :3] = np.eye(3, dtype=np.float32) * np.float32(1.2)
    grow[0, :, 3] = corner - np.float32(1.2) * corner
    dev_b.set_rig([(0, n, 0)], 1)
    side = torch.cuda.Stream()
    dev_b.pose_device(gpu(grow), stream=side)
    side.synchronize()
    dev_a.transform_prims([(0, n, 0)], grow, p3d.UPDATE_REFIT)
    rgb_a, hit_a, st_a = dev_a.render(cfg)
    rgb_b, hit_b, st_b = dev_b.render(cfg)
    assert np.array_equal(hit_a, hit_b) and rgb_a.tobytes() == rgb_b.tobytes()
    assert {k: getattr(st_a, k) for k in RENDER_COUNTERS} == {k: getattr(st_b, k) for k in RENDER_COUNTERS}
    assert rgb_b.tobytes() != before[0].tobytes()
    assert_same_tree(dev_a.export_bvh(), dev_b.export_bvh(), "the grown mesh")
    assert dev_b.status() == 0


# 10. the call does not wait
def test_the_call_returns_ahead_of_the_stream(paths):
    """The method of the stream-refit test: a producer of 900 torch kernels over 2^24 floats (17.7 ms of GPU time there)
    stands in front of the call on the side stream.  The assertion asks for a factor of at least 100 between the producer's
    GPU time and the call's host time, and for a stream that is still busy when the call is back."""
    hs, a, dev_a, dev_b = twins(paths["tri5k"])
    n, k = a["n_prims"], 16
    ranges = [(i * (n // k), n // k, i) for i in range(k)]
    base = gpu(moves(a, 330, k, reach=0.03))
    big = torch.linspace(0, 1, 1 << 24, device="cuda")
    dev_b.set_rig(ranges, k)  # the setup call: it may wait
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        dev_b.pose_device(base, stream=side)
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        begin.record(side)
        slow = produced(big, 1.0, rounds=300)
        end.record(side)
        x = (base + 0.01 * torch.sin(2.0 * base) + 0.0 * slow[:base.numel()].view(base.shape)).contiguous()
        t0 = time.perf_counter()
        dev_b.pose_device(x, stream=side)
        call_s = time.perf_counter() - t0
        busy = not side.query()
    side.synchronize()
    producer_ms = begin.elapsed_time(end)
    print("producer %.3f ms on the GPU, call %.4f ms on the host" % (producer_ms, 1e3 * call_s))
    assert producer_ms >= 100 * 1e3 * call_s, (producer_ms, call_s)
    assert busy, "the stream had passed the call when it returned"
    dev_a.transform_prims(ranges, x.cpu().numpy(), p3d.UPDATE_REFIT)
    assert_same_frames_and_tree(dev_a, dev_b, "tri5k", "a pose behind a long producer")
    assert dev_b.status() == 0
