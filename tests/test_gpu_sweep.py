"""Sphere sweeps over device tensors (p3d_sweep_sphere_device) on the GPU.

The yardstick is exact: host_sweep_sphere, the brute force on the CPU that test_sweep_api.py holds to the float64 model.  Under
ACCEL_NONE object, t, centre and contact must be its bits, with and without limits; under ACCEL_BVH every output must be the
ACCEL_NONE bits, on uploaded and on device-built trees, through the spill path of a deep tree, for radii from 0 to larger than
the scene, and behind a refit or a pose enqueued on the same stream.  Every comparison here has tolerance 0; the model's checks
run once, on the kernel's outputs."""
import os

import numpy as np
import pytest
import torch

from conftest import SCENES as GOLDEN_SCENES
import device_query_contract as dq
from device_query_contract import SWEEP, UNSUPPORTED
from frame_checks import as_bytes, gpu
import fuzz_scenes
import intersect_reference as ref
import p3d_amd as p3d
import sweep_reference as sw

pytestmark = pytest.mark.gpu

ALL = SWEEP.optional
HOST = ("object", "t", "centre", "contact")  # the outputs the host form has, in its order
N = sw.N_RAYS


def world(path, trees, balls, seed, legacy=False):
    """N balls, their limits (drawn from the host form's T as the CPU suite draws them from the model's), and the host form's answers"""
    w = dq.World(path, trees, legacy=legacy)
    o, d, r = balls
    w.attach(d_origin=o, d_direction=d, d_radius=r)
    w.free = SWEEP.host_form(w.hs, w, N, False)
    T = np.where(w.free["object"] >= 0, w.free["t"].astype(np.float64), np.nan)
    step = np.maximum(np.linalg.norm(d.astype(np.float64), axis=1), 1e-30)
    w.attach(d_t_max=sw.draw_limits(T, 40.0 / step, seed + 50))
    w.limited = SWEEP.host_form(w.hs, w, N, True)
    return w


def bounds_balls(path, seed, legacy=False):
    a = p3d.HostScene(path, legacy_f11=legacy).arrays()
    return sw.box_balls(a["prim_bmin"].min(0), a["prim_bmax"].max(0), seed)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = sw.scene_paths(tmp_path_factory.mktemp("sweep"))
    w = {}
    for name, (seed, _, _, planes) in sw.SCENES.items():
        w[name] = world(paths[name], ("none",) if planes else ("host", "device"), sw.balls(ref.load_objects(paths[name]), seed + 500), seed)
    fuzz = fuzz_scenes.random_scene(86, os.path.join(os.path.dirname(paths["mixed"]), "sweep_mesh.p3f"), n_spheres=0, n_tris=300, n_boxes=0)
    for name, path, trees, seed in (("tri5k", tri5k_path, ("device",), 87), ("balls_low", os.path.join(GOLDEN_SCENES, "balls_low.p3f"), ("host", "device"), 88),
                                    ("tri_low", os.path.join(GOLDEN_SCENES, "tri_low.p3f"), ("host", "device"), 89), ("mesh", fuzz, ("host", "device"), 90)):
        legacy = name == "tri_low"  # 11-number `f` lines (P3D_LOAD_LEGACY_F11)
        w[name] = world(path, trees, bounds_balls(path, seed, legacy), seed, legacy)
    dq.assert_deep(w["tri5k"].devs["device"])
    return w


def ask(dev, accel, w, n=N, limits=False, want=None):
    return SWEEP.ask(dev, accel, SWEEP.inputs_of(w, n, limits), want)


def assert_normals(dev, got, what, most=16):
    obj = got["object"]
    for j in np.unique(obj[obj >= 0])[:most]:
        m = obj == j
        assert as_bytes(got["normal"][m]) == as_bytes(dev.object_normal(int(j), got["contact"][m])), "%s: the normal of object %d" % (what, j)


def assert_host_bits(got, want, what):
    """want: host_sweep_sphere's tuple, or the answers by name"""
    dq.assert_answers(got, want if isinstance(want, dict) else dict(zip(HOST, want)), SWEEP.table, what)


@pytest.mark.parametrize("name", list(sw.SCENES) + ["tri5k", "balls_low", "tri_low", "mesh"])
def test_the_kernel_is_the_host_form_and_the_tree_the_brute_force(name, worlds):
    w = worlds[name]
    for limits, want in ((False, w.free), (True, w.limited)):
        first = None
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                what = "%s, %s tree, accel %d%s" % (name, tree, accel, ", limits" if limits else "")
                got = ask(dev, accel, w, limits=limits)
                assert_host_bits(got, want, what)
                if first is None:
                    first = got
                    assert_normals(dev, got, what)
                dq.assert_same_bits(got, first, what + ", against the first back end")  # (the normals too, which the host form has not)
            assert dev.status() == 0
        met = want["object"] >= 0
        assert 0 < met.sum() < N, name + ": met and not met in one batch"
        assert (want["t"][met] == 0).any() and (want["t"][met] > 0).any(), name + ": contacts at the start and later ones"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block
def test_batches_that_are_no_multiple_of_the_block(n, worlds):
    for name in ("mixed", "tri5k"):
        dq.check_ragged_batches(SWEEP, worlds[name], n, None, worlds[name].limited, name)


def test_an_empty_batch_launches_nothing(worlds):
    dq.check_empty_batch(SWEEP, worlds["mixed"].devs["host"])


def test_streams_optional_outputs_one_radius_and_twice_the_same(worlds):
    w = worlds["mixed"]
    dev = w.devs["device"]
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        what = "mixed, accel %d" % accel
        whole = ask(dev, accel, w, limits=True)
        dq.assert_same_bits(ask(dev, accel, w, limits=True), whole, what + ", the same call again")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            res = p3d.sweep_sphere_device(dev, accel, w.dev["d_origin"], w.dev["d_direction"], w.dev["d_radius"], t_max=w.dev["d_t_max"], want=ALL, stream=side)
        side.synchronize()
        dq.assert_same_bits({k: v.cpu().numpy() for k, v in res.items()}, whole, what + ", a stream of its own")
        # the optional outputs may be left out, and outputs may be the caller's
        only = ask(dev, accel, w, limits=True, want=())
        assert list(only) == ["object"] and as_bytes(only["object"]) == as_bytes(whole["object"]), what
        for k in ALL:
            some = ask(dev, accel, w, limits=True, want=(k,))
            assert list(some) == ["object", k] and as_bytes(some["object"]) == as_bytes(whole["object"]) and as_bytes(some[k]) == as_bytes(whole[k]), what + ", only " + k
        dq.check_callers_outputs(SWEEP, dev, accel, SWEEP.inputs_of(w, N, True), whole, what, optional=("contact",))
        # one number for every radius: the wrapper fills a tensor, on the call's stream
        for stream in (0, side):
            one = p3d.sweep_sphere_device(dev, accel, w.dev["d_origin"], w.dev["d_direction"], 0.25, want=("t",), stream=stream)
            torch.cuda.synchronize()
            want = p3d.host_sweep_sphere(w.hs, w.host["d_origin"], w.host["d_direction"], 0.25)
            assert as_bytes(one["object"].cpu().numpy()) == as_bytes(want[0]) and as_bytes(one["t"].cpu().numpy()) == as_bytes(want[1]), what + ", one radius"
    assert dev.status() == 0


def test_inputs_that_find_nothing(worlds):
    w = worlds["mixed"]
    n = 515
    for tree, dev in w.devs.items():
        for accel in w.accels(tree):
            what = "mixed, %s tree, accel %d" % (tree, accel)
            for value in (0.0, -2.0, np.nan, -np.inf):
                got = {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, w.dev["d_origin"][:n], w.dev["d_direction"][:n], w.dev["d_radius"][:n], t_max=gpu(np.full(n, value, np.float32)), want=ALL).items()}
                assert (got["object"] == -1).all() and (got["t"] == dq.FLT_MAX).all() and not any(got[k].any() for k in ("centre", "contact", "normal")), "%s: a limit of %g" % (what, value)
            for value in (-1.0, np.nan):
                got = p3d.sweep_sphere_device(dev, accel, w.dev["d_origin"][:n], w.dev["d_direction"][:n], value, want=())
                assert (got["object"].cpu().numpy() == -1).all(), "%s: a radius of %g" % (what, value)
            bad = w.host["d_origin"][:n].copy()
            bad[::2, 1] = np.nan
            got = ask_raw(dev, accel, gpu(bad), w.dev["d_direction"][:n], w.dev["d_radius"][:n])
            assert (got["object"][::2] == -1).all() and as_bytes(got["object"][1::2]) == as_bytes(w.free["object"][1:n:2]), what + ": NaN origins"
            still = np.zeros((n, 3), np.float32)  # a ball that stands still meets only what it touches
            got = ask_raw(dev, accel, w.dev["d_origin"][:n], gpu(still), w.dev["d_radius"][:n])
            want = p3d.host_sweep_sphere(w.hs, w.host["d_origin"][:n], still, w.host["d_radius"][:n])
            assert as_bytes(got["object"]) == as_bytes(want[0]) and as_bytes(got["t"]) == as_bytes(want[1]), what + ": zero directions"
            assert ((want[0] >= 0) == (w.free["t"][:n] == 0)).all() and (want[1][want[0] >= 0] == 0).all()
            inf = ask(dev, accel, w, n=n)  # and an infinite limit is none
            got = {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, w.dev["d_origin"][:n], w.dev["d_direction"][:n], w.dev["d_radius"][:n], t_max=gpu(np.full(n, np.inf, np.float32)), want=ALL).items()}
            dq.assert_same_bits(got, inf, what + ", infinite limits")


def ask_raw(dev, accel, d_o, d_d, d_r):
    return {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, d_o, d_d, d_r, want=("t",)).items()}


def test_refusals_enqueue_nothing(tmp_path, worlds):
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    inputs = SWEEP.inputs_of(w, n)
    outs = dq.check_buffer_refusals(SWEEP, dev, inputs, n, planes=worlds["planes"])
    (tmp_path / "boxed.p3f").write_text(ref.HEAD + "s 0 0 0 1\nbox -1 3 -1 1 5 1\n")
    boxed = p3d.DeviceScene(p3d.HostScene(str(tmp_path / "boxed.p3f")), bvh=True)
    with_planes = p3d.DeviceScene(worlds["planes"].hs, bvh=True)
    gridded = p3d.DeviceScene(p3d.HostScene(w.path), bvh=True, grid=True)
    lib = p3d.lib()
    every = dict(inputs, **{"d_" + name: t for name, t in outs.items()})
    # the library's own refusals, behind the wrapper's back: a box through every accel, the grid, the tree over a plane
    for scene, accel, word in ((boxed, p3d.ACCEL_NONE, b"box"), (boxed, p3d.ACCEL_BVH, b"box"), (boxed, p3d.ACCEL_GRID, b"grid"), (gridded, p3d.ACCEL_GRID, b"grid"),
                               (with_planes, p3d.ACCEL_BVH, b"plane")):
        assert SWEEP.raw(scene, accel, n, **every) == UNSUPPORTED, (accel, lib.p3d_last_error())
        assert b"p3d_sweep_sphere_device" in lib.p3d_last_error() and word in lib.p3d_last_error(), lib.p3d_last_error()
    assert SWEEP.raw(boxed, p3d.ACCEL_NONE, 0) == UNSUPPORTED  # a box is refused whatever n
    dq.assert_refused([("the wrapper: %s" % what, UNSUPPORTED, word, lambda scene=scene, accel=accel: SWEEP.call(scene, accel, inputs, ALL, 0, outs))
                       for what, word, scene, accel in (("a box", "box", boxed, p3d.ACCEL_NONE), ("the grid", "grid", gridded, p3d.ACCEL_GRID),
                                                        ("a plane under the tree", "plane", with_planes, p3d.ACCEL_BVH))])
    dq.assert_untouched(outs)
    assert all(s.status() == 0 for s in (dev, boxed, with_planes, gridded))


def test_behind_a_refit_on_the_same_stream(worlds):
    """refit_triangles with moved positions on a side stream, the sweep behind it on that stream, nothing in between: the answers
    are those of a fresh scene of the moved geometry under ACCEL_NONE, and the host form's after set_geometry."""
    dq.check_behind_a_refit(SWEEP, worlds["tri5k"], N, what="tri5k behind a refit", before={False: worlds["tri5k"].free, True: worlds["tri5k"].limited})


def test_behind_a_pose_on_the_same_stream(worlds):
    dq.check_behind_a_pose(SWEEP, worlds["mixed"], N, what="mixed behind a pose", before={False: worlds["mixed"].free, True: worlds["mixed"].limited})


def test_the_kernels_outputs_meet_the_model(worlds):
    """The checks of the CPU suite (sweep_reference.check_sweep), once, on what the kernel wrote: a quarter of the mixed set"""
    w = worlds["mixed"]
    n = N // 4
    c = sw.cases(w.path, sw.SCENES["mixed"][0] + 500, n)
    dev = w.devs["device"]
    d_o, d_d, d_r, d_lim = gpu(c.o), gpu(c.d), gpu(c.r), gpu(c.limits)
    for limits, T, margin in ((None, c.free_T, c.free_margin), (d_lim, c.lim_T, c.lim_margin)):
        res = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, d_o, d_d, d_r, t_max=limits, want=ALL)
        got = tuple(res[k].cpu().numpy() for k in HOST)
        err, _ = sw.check_sweep(c.objects, c.o, c.d, c.r, T, margin, got, "mixed on the device%s" % ("" if limits is None else ", limits"))
        sw.assert_within(err, "mixed on the device")
        # the normal at the contact point: unit, and along centre - contact (either way: it is not turned) where the ball is away from the object
        nrm = res["normal"].cpu().numpy().astype(np.float64)
        away = (got[0] >= 0) & (got[1] > 0) & (c.r > 1e-3)
        push = (got[2] - got[3])[away].astype(np.float64)
        cos = np.abs((push * nrm[away]).sum(1)) / np.linalg.norm(push, axis=1)
        on_sphere = np.array([c.objects[j]["kind"] == sw.SPHERE for j in got[0][away]])  # a sphere's contact is always along its normal
        assert np.abs(np.linalg.norm(nrm[got[0] >= 0], axis=1) - 1).max() <= 1e-6
        assert on_sphere.sum() > 20 and (cos[on_sphere] >= 1 - 1e-4).all(), "a sphere's normal is not along centre - contact"
    # a triangle's contact is along its normal only inside the face, not on an edge or a vertex: the triangles set holds 138 such
    # contacts (every barycentric coordinate of the contact point above 0.05, in float64)
    w = worlds["triangles"]
    objects = ref.load_objects(w.path)
    got = ask(w.devs["device"], p3d.ACCEL_BVH, w)
    away = (got["object"] >= 0) & (got["t"] > 0) & (w.host["d_radius"] > 1e-3)
    push = (got["centre"] - got["contact"])[away].astype(np.float64)
    cos = np.abs((push * got["normal"][away].astype(np.float64)).sum(1)) / np.linalg.norm(push, axis=1)
    in_face = np.array([strictly_inside(objects[j], q) for j, q in zip(got["object"][away], got["contact"][away].astype(np.float64))])
    assert in_face.sum() >= 100 and (cos[in_face] >= 1 - 1e-4).all(), "a face contact's normal is not along centre - contact"
    assert (cos[~in_face] < 1 - 1e-4).any(), "no edge or vertex contact among the rest: the face test above proves less than it says"


def strictly_inside(ob, q, least=0.05):
    """q, a point of the triangle's plane, has every barycentric coordinate above `least` (float64)"""
    e1, e2, w = ob["p1"] - ob["p0"], ob["p2"] - ob["p0"], q - ob["p0"]
    n = np.cross(e1, e2)
    beta, gamma = np.cross(w, e2) @ n / (n @ n), np.cross(e1, w) @ n / (n @ n)
    return min(beta, gamma, 1 - beta - gamma) > least


def test_a_ball_dropped_on_a_triangle_by_hand(tmp_path):
    """The by-hand cases of the CPU suite that need the normal, which the host form does not report: dropped on the middle of a
    face the normal is the face normal, exactly; on an edge and on a vertex it is still the triangle's, and centre - contact is
    the push direction"""
    (tmp_path / "one.p3f").write_text(ref.HEAD + "p 3\n0 -1 0\n0 1 0\n-2 0 0\np 3\n50 50 50\n51 50 50\n50 51 50\n")  # object 0 in the plane z = 0, (P1-P0) x (P2-P0) = (0, 0, 4); object 1 far away
    hs = p3d.HostScene(str(tmp_path / "one.p3f"))
    o = np.array([[-0.5, 0, 5], [-0.5, 0, -5], [3, 0, 10], [0, 4, 10], [0.5, 0, 5]], np.float32)
    d = np.array([[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1]], np.float32)
    r = np.array([1, 1, 5, 5, 0], np.float32)
    want = p3d.host_sweep_sphere(hs, o, d, r)
    assert want[0].tolist() == [0, 0, 0, 0, -1] and want[1][:4].tolist() == [4, 4, 6, 6]
    for tree in (True, "device"):
        dev = p3d.DeviceScene(hs, bvh=tree)
        for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
            got = {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, gpu(o), gpu(d), gpu(r), want=ALL).items()}
            assert_host_bits(got, want, "by hand, tree %s, accel %d" % (tree, accel))
            assert got["normal"].tolist() == [[0, 0, 1]] * 4 + [[0, 0, 0]], got["normal"]  # the face normal, from below too: not turned
            assert got["contact"][:4].tolist() == [[-0.5, 0, 0], [-0.5, 0, 0], [0, 0, 0], [0, 1, 0]]
            assert (got["centre"] - got["contact"])[:4].tolist() == [[0, 0, 1], [0, 0, -1], [3, 0, 4], [0, 3, 4]]
        assert dev.status() == 0


def test_one_radius_is_not_handed_out_again_before_the_launch(worlds, monkeypatch):
    """The tensor the wrapper fills for a scalar radius must live until the kernel is enqueued: none of the outputs allocated by
    the same call may lie on it (torch's allocator hands a freed block of the same size straight back)"""
    w = worlds["mixed"]
    dev = w.devs["device"]
    seen, full = [], torch.full

    def recording(*args, **kw):
        t = full(*args, **kw)
        seen.append((t.data_ptr(), t.numel() * t.element_size()))
        return t

    monkeypatch.setattr(torch, "full", recording)
    res = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, w.dev["d_origin"], w.dev["d_direction"], 0.25, want=ALL)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(seen) == 1
    lo, size = seen[0]
    for name, t in res.items():
        assert t.data_ptr() + t.numel() * t.element_size() <= lo or t.data_ptr() >= lo + size, "the output %r lies on the radii" % name
    want = p3d.host_sweep_sphere(w.hs, w.host["d_origin"], w.host["d_direction"], 0.25)
    assert_host_bits({k: v.cpu().numpy() for k, v in res.items()}, want, "mixed, one radius")
