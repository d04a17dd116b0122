"""Sphere sweeps over device tensors (p3d_sweep_sphere_device) on the GPU.

The yardstick is exact: host_sweep_sphere, the brute force on the CPU that test_sweep_api.py holds to the float64 model.  Under
ACCEL_NONE object, t, centre and contact must be its bits, with and without limits; under ACCEL_BVH every output must be the
ACCEL_NONE bits, on uploaded and on device-built trees, through the spill path of a deep tree, for radii from 0 to larger than
the scene, and behind a refit or a pose enqueued on the same stream.  Every comparison here has tolerance 0; the model's checks
run once, on the kernel's outputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import SCENES as GOLDEN_SCENES
from device_geometry_helpers import deformed_mesh
from frame_checks import as_bytes, gpu
from live_scene_checks import plan
import p3d_amd as p3d
import sweep_reference as sw

pytestmark = pytest.mark.gpu

ALL = ("t", "centre", "contact", "normal")
HOST = ("object", "t", "centre", "contact")  # the outputs the host form has, in its order
FLT_MAX = sw.FLT_MAX
INVALID, UNSUPPORTED = -1, -3
N = sw.N_RAYS


class World:
    """One scene: host scene, device scenes by tree, N balls, their limits (drawn from the host form's T as the CPU suite draws
    them from the model's), and the host form's answers"""

    def __init__(self, name, path, trees, balls, seed, legacy=False):
        self.name, self.path = name, path
        self.hs = p3d.HostScene(path, legacy_f11=legacy)
        self.devs = {tree: p3d.DeviceScene(self.hs, bvh={"host": True, "device": "device", "none": False}[tree]) for tree in trees}
        self.o, self.d, self.r = balls
        self.free = p3d.host_sweep_sphere(self.hs, self.o, self.d, self.r)
        T = np.where(self.free[0] >= 0, self.free[1].astype(np.float64), np.nan)
        step = np.maximum(np.linalg.norm(self.d.astype(np.float64), axis=1), 1e-30)
        self.limits = sw.draw_limits(T, 40.0 / step, seed + 50)
        self.limited = p3d.host_sweep_sphere(self.hs, self.o, self.d, self.r, t_max=self.limits)
        self.d_o, self.d_d, self.d_r, self.d_limits = gpu(self.o), gpu(self.d), gpu(self.r), gpu(self.limits)

    def accels(self, tree):
        return [p3d.ACCEL_NONE] if tree == "none" else [p3d.ACCEL_NONE, p3d.ACCEL_BVH]


def bounds_balls(path, seed, legacy=False):
    a = p3d.HostScene(path, legacy_f11=legacy).arrays()
    return sw.box_balls(a["prim_bmin"].min(0), a["prim_bmax"].max(0), seed)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    import intersect_reference as ref
    paths = sw.scene_paths(tmp_path_factory.mktemp("sweep"))
    w = {}
    for name, (seed, _, _, planes) in sw.SCENES.items():
        trees = ("none",) if planes else ("host", "device")
        w[name] = World(name, paths[name], trees, sw.balls(ref.load_objects(paths[name]), seed + 500), seed)
    fuzz = __import__("fuzz_scenes").random_scene(86, os.path.join(os.path.dirname(paths["mixed"]), "sweep_mesh.p3f"), n_spheres=0, n_tris=300, n_boxes=0)
    for name, path, trees, seed in (("tri5k", tri5k_path, ("device",), 87), ("balls_low", os.path.join(GOLDEN_SCENES, "balls_low.p3f"), ("host", "device"), 88),
                                    ("tri_low", os.path.join(GOLDEN_SCENES, "tri_low.p3f"), ("host", "device"), 89), ("mesh", fuzz, ("host", "device"), 90)):
        legacy = name == "tri_low"  # 11-number `f` lines (P3D_LOAD_LEGACY_F11)
        w[name] = World(name, path, trees, bounds_balls(path, seed, legacy), seed, legacy)
    assert w["tri5k"].devs["device"].export_bvh()["bvh_max_depth"] > 16  # deeper than the LDS window: the spill path runs
    return w


def ask(dev, accel, w, n=N, limits=False, want=ALL, **kw):
    res = p3d.sweep_sphere_device(dev, accel, w.d_o[:n], w.d_d[:n], w.d_r[:n], t_max=w.d_limits[:n] if limits else None, want=want, **kw)
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_host_bits(got, want, what):
    n = len(got["object"])
    assert got["object"].dtype == np.int32
    for k, ref_ in zip(HOST, want):
        assert as_bytes(got[k]) == as_bytes(ref_[:n]), "%s: %s" % (what, k)
    none = got["object"] < 0
    zeros = as_bytes(np.zeros((int(none.sum()), 3), np.float32))
    assert (got["t"][none] == FLT_MAX).all() and all(as_bytes(got[k][none]) == zeros for k in ("centre", "contact", "normal")), what + ": the no-answer values"


def assert_normals(dev, got, what, most=16):
    obj = got["object"]
    for j in np.unique(obj[obj >= 0])[:most]:
        m = obj == j
        assert as_bytes(got["normal"][m]) == as_bytes(dev.object_normal(int(j), got["contact"][m])), "%s: the normal of object %d" % (what, j)


def assert_same(a, b, what):
    assert list(a) == list(b)
    for k in a:
        assert as_bytes(a[k]) == as_bytes(b[k]), "%s: %s" % (what, k)


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
                assert_same(got, first, what + ", against the first back end")  # (the normals too, which the host form has not)
            assert dev.status() == 0
        met = want[0] >= 0
        assert 0 < met.sum() < N, name + ": met and not met in one batch"
        assert (want[1][met] == 0).any() and (want[1][met] > 0).any(), name + ": contacts at the start and later ones"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block
def test_batches_that_are_no_multiple_of_the_block(n, worlds):
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                assert_host_bits(ask(dev, accel, w, n=n, limits=True), w.limited, "%s, %s tree, accel %d, %d balls" % (name, tree, accel, n))


def test_an_empty_batch_launches_nothing(worlds):
    dev = worlds["mixed"].devs["host"]
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):  # whatever the pointers
        assert p3d.lib().p3d_sweep_sphere_device(dev._h, accel, 0, *([None] * 10)) == 0
    assert dev.status() == 0


def test_streams_optional_outputs_one_radius_and_twice_the_same(worlds):
    w = worlds["mixed"]
    dev = w.devs["device"]
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        what = "mixed, accel %d" % accel
        whole = ask(dev, accel, w, limits=True)
        assert_same(ask(dev, accel, w, limits=True), whole, what + ", the same call again")
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            res = p3d.sweep_sphere_device(dev, accel, w.d_o, w.d_d, w.d_r, t_max=w.d_limits, want=ALL, stream=side)
        side.synchronize()
        assert_same({k: v.cpu().numpy() for k, v in res.items()}, whole, what + ", a stream of its own")
        # the optional outputs may be left out, and outputs may be the caller's
        only = ask(dev, accel, w, limits=True, want=())
        assert list(only) == ["object"] and as_bytes(only["object"]) == as_bytes(whole["object"]), what
        for k in ALL:
            some = ask(dev, accel, w, limits=True, want=(k,))
            assert list(some) == ["object", k] and as_bytes(some["object"]) == as_bytes(whole["object"]) and as_bytes(some[k]) == as_bytes(whole[k]), what + ", only " + k
        mine = {"object": torch.full((N,), 77, dtype=torch.int32, device="cuda"), "contact": torch.full((N, 3), 5.0, device="cuda")}
        back = p3d.sweep_sphere_device(dev, accel, w.d_o, w.d_d, w.d_r, t_max=w.d_limits, want=("contact",), out=mine)
        assert list(back) == ["object", "contact"] and back["object"] is mine["object"] and back["contact"] is mine["contact"]
        assert as_bytes(mine["object"].cpu().numpy()) == as_bytes(whole["object"]) and as_bytes(mine["contact"].cpu().numpy()) == as_bytes(whole["contact"])
        # one number for every radius: the wrapper fills a tensor, on the call's stream
        for stream in (0, side):
            one = p3d.sweep_sphere_device(dev, accel, w.d_o, w.d_d, 0.25, want=("t",), stream=stream)
            torch.cuda.synchronize()
            want = p3d.host_sweep_sphere(w.hs, w.o, w.d, 0.25)
            assert as_bytes(one["object"].cpu().numpy()) == as_bytes(want[0]) and as_bytes(one["t"].cpu().numpy()) == as_bytes(want[1]), what + ", one radius"
    assert dev.status() == 0


def test_inputs_that_find_nothing(worlds):
    w = worlds["mixed"]
    n = 515
    for tree, dev in w.devs.items():
        for accel in w.accels(tree):
            what = "mixed, %s tree, accel %d" % (tree, accel)
            for value in (0.0, -2.0, np.nan, -np.inf):
                got = {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, w.d_o[:n], w.d_d[:n], w.d_r[:n], t_max=gpu(np.full(n, value, np.float32)), want=ALL).items()}
                assert (got["object"] == -1).all() and (got["t"] == FLT_MAX).all() and not any(got[k].any() for k in ("centre", "contact", "normal")), "%s: a limit of %g" % (what, value)
            for value in (-1.0, np.nan):
                got = p3d.sweep_sphere_device(dev, accel, w.d_o[:n], w.d_d[:n], value, want=())
                assert (got["object"].cpu().numpy() == -1).all(), "%s: a radius of %g" % (what, value)
            bad = w.o[:n].copy()
            bad[::2, 1] = np.nan
            got = ask_raw(dev, accel, gpu(bad), w.d_d[:n], w.d_r[:n])
            assert (got["object"][::2] == -1).all() and as_bytes(got["object"][1::2]) == as_bytes(w.free[0][1:n:2]), what + ": NaN origins"
            still = np.zeros((n, 3), np.float32)  # a ball that stands still meets only what it touches
            got = ask_raw(dev, accel, w.d_o[:n], gpu(still), w.d_r[:n])
            want = p3d.host_sweep_sphere(w.hs, w.o[:n], still, w.r[:n])
            assert as_bytes(got["object"]) == as_bytes(want[0]) and as_bytes(got["t"]) == as_bytes(want[1]), what + ": zero directions"
            assert ((want[0] >= 0) == (w.free[1][:n] == 0)).all() and (want[1][want[0] >= 0] == 0).all()
            inf = ask(dev, accel, w, n=n)  # and an infinite limit is none
            got = {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, w.d_o[:n], w.d_d[:n], w.d_r[:n], t_max=gpu(np.full(n, np.inf, np.float32)), want=ALL).items()}
            assert_same(got, inf, what + ", infinite limits")


def ask_raw(dev, accel, d_o, d_d, d_r):
    return {k: v.cpu().numpy() for k, v in p3d.sweep_sphere_device(dev, accel, d_o, d_d, d_r, want=("t",)).items()}


HEAD = """bclr 0 0 0
v
from 0 0 20
at 0 0 0
up 0 1 0
angle 40
hither 0.01
resolution 32 32
aperture 0
focal 1
l 0 10 10 1 1 1
f 0.8 0.8 0.8 0.9 1 1 1 0.3 20 0 1 0 0 0
"""


def test_refusals_enqueue_nothing(tmp_path, worlds):
    w = worlds["mixed"]
    dev, no_tree = w.devs["host"], worlds["mixed_planes"].devs["none"]
    lib = p3d.lib()
    n = 129
    (tmp_path / "boxed.p3f").write_text(HEAD + "s 0 0 0 1\nbox -1 3 -1 1 5 1\n")
    boxed = p3d.DeviceScene(p3d.HostScene(str(tmp_path / "boxed.p3f")), bvh=True)
    with_planes = p3d.DeviceScene(worlds["planes"].hs, bvh=True)
    gridded = p3d.DeviceScene(p3d.HostScene(w.path), bvh=True, grid=True)
    outs = dict(object=torch.full((n,), 77, dtype=torch.int32, device="cuda"), t=torch.full((n,), 123.0, device="cuda"),
                centre=torch.full((n, 3), 123.0, device="cuda"), contact=torch.full((n, 3), 123.0, device="cuda"), normal=torch.full((n, 3), 123.0, device="cuda"))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    args = (ptr(w.d_o), ptr(w.d_d), ptr(w.d_r), None, ptr(outs["object"]), ptr(outs["t"]), ptr(outs["centre"]), ptr(outs["contact"]), ptr(outs["normal"]), None)
    # the library's own refusals, behind the wrapper's back: a box through every accel, the grid, the tree over a plane
    for scene, accel, code, word in ((boxed, p3d.ACCEL_NONE, UNSUPPORTED, b"box"), (boxed, p3d.ACCEL_BVH, UNSUPPORTED, b"box"), (boxed, p3d.ACCEL_GRID, UNSUPPORTED, b"grid"),
                                     (gridded, p3d.ACCEL_GRID, UNSUPPORTED, b"grid"), (with_planes, p3d.ACCEL_BVH, UNSUPPORTED, b"plane"),
                                     (no_tree, p3d.ACCEL_BVH, INVALID, b"without BVH"), (dev, 7, INVALID, b"accel")):
        assert lib.p3d_sweep_sphere_device(scene._h, accel, n, *args) == code, (accel, lib.p3d_last_error())
        assert b"p3d_sweep_sphere_device" in lib.p3d_last_error() or code == INVALID
        assert word in lib.p3d_last_error(), lib.p3d_last_error()
    assert lib.p3d_sweep_sphere_device(boxed._h, p3d.ACCEL_NONE, 0, *([None] * 10)) == UNSUPPORTED  # a box is refused whatever n
    for k in (0, 1, 2, 4):  # a null origin, direction, radius, object
        holed = list(args)
        holed[k] = None
        assert lib.p3d_sweep_sphere_device(dev._h, p3d.ACCEL_BVH, n, *holed) == INVALID and b"null argument" in lib.p3d_last_error()
    host = np.zeros((n, 3), np.float32)
    big = 0x00ffff00  # balls no buffer here holds
    huge = torch.empty((big, 3), device="cuda")  # (never read: every call it is given to is refused)
    q = lambda scene, accel, *a, **kw: p3d.sweep_sphere_device(scene, accel, *a, **kw)
    cases = [
        ("the wrapper: a box", UNSUPPORTED, "box", lambda: q(boxed, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], w.d_r[:n], want=ALL, out=outs)),
        ("the wrapper: the grid", UNSUPPORTED, "grid", lambda: q(gridded, p3d.ACCEL_GRID, w.d_o[:n], w.d_d[:n], w.d_r[:n], want=ALL, out=outs)),
        ("the wrapper: a plane under the tree", UNSUPPORTED, "plane", lambda: q(with_planes, p3d.ACCEL_BVH, w.d_o[:n], w.d_d[:n], w.d_r[:n], want=ALL, out=outs)),
        ("a misaligned radius", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_BVH, w.d_o[:n], w.d_d[:n], (w.d_r.data_ptr() + 2, n), want=ALL, out=outs)),
        ("a misaligned output", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], w.d_r[:n], want=ALL, out=dict(outs, t=(outs["t"].data_ptr() + 2, n)))),
        ("host origins", INVALID, "d_origin is host memory", lambda: q(dev, p3d.ACCEL_BVH, (host.ctypes.data, n), w.d_d[:n], w.d_r[:n], want=ALL, out=outs)),
        ("a host radius", INVALID, "d_radius is host memory", lambda: q(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], (host.ctypes.data, n), want=ALL, out=outs)),
        # too short: torch hands out pieces of larger allocations, so "behind the allocation" needs a count beyond any of them
        ("a radius too short", INVALID, "d_radius ends behind its allocation",
         lambda: q(dev, p3d.ACCEL_NONE, (huge.data_ptr(), big), (huge.data_ptr(), big), (w.d_r.data_ptr(), big), want=(), out={"object": (outs["object"].data_ptr(), big)})),
        ("an output too short", INVALID, "d_object ends behind its allocation",
         lambda: q(dev, p3d.ACCEL_BVH, (huge.data_ptr(), big), (huge.data_ptr(), big), (huge.data_ptr(), big), want=(), out={"object": (outs["object"].data_ptr(), big)})),
    ]
    for what, code, word, call in cases:
        with pytest.raises(p3d.P3DError) as e:
            call()
        assert e.value.code == code and word in str(e.value), "%s: %s" % (what, e.value)
    del huge
    # the planes are there for the brute force
    pw = worlds["planes"]
    assert as_bytes(ask(with_planes, p3d.ACCEL_NONE, pw, n=n, want=())["object"]) == as_bytes(pw.free[0][:n])
    torch.cuda.synchronize()
    assert bool((outs["object"] == 77).all()) and all(bool((outs[k] == 123.0).all()) for k in ALL)
    assert all(s.status() == 0 for s in (dev, boxed, with_planes, gridded))


def test_behind_a_refit_on_the_same_stream(worlds, tri5k_path):
    """refit_triangles with moved positions on a side stream, the sweep behind it on that stream, nothing in between: the answers
    are those of a fresh scene of the moved geometry under ACCEL_NONE, and the host form's after set_geometry."""
    w = worlds["tri5k"]
    hs = p3d.HostScene(tri5k_path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    soup = deformed_mesh(a, seed=91, fraction=0.03)[2]
    base, d_soup = gpu(a["prim_v"].reshape(-1, 3)), gpu(soup)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wave = base
        for _ in range(50):  # some work in front, so that the positions are still being produced when the calls begin
            wave = torch.sin(wave * 1.5 + 0.25)
        moved = (d_soup + 0.0 * wave).contiguous()
        dev.refit_triangles(0, moved, stream=side)
        res = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, w.d_r, t_max=w.d_limits, want=ALL, stream=side)
    side.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    hs.set_geometry(*p3d.deformed(a["prim_v"], 0, soup))
    want = p3d.host_sweep_sphere(hs, w.o, w.d, w.r, t_max=w.limits)
    assert_host_bits(got, want, "tri5k behind a refit")
    assert as_bytes(want[1]) != as_bytes(w.limited[1]), "the refit moved nothing the balls can meet"
    fresh = p3d.DeviceScene(hs, bvh=False)
    assert_same(got, ask(fresh, p3d.ACCEL_NONE, w, limits=True), "tri5k behind a refit, against a fresh scene")
    assert dev.status() == 0 and fresh.status() == 0


def test_behind_a_pose_on_the_same_stream(worlds):
    w = worlds["mixed"]
    hs = p3d.HostScene(w.path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    ranges, xforms, scale = plan(a, 93)  # spheres and triangles under a rigid move
    dev.set_rig(ranges, 2)
    side = torch.cuda.Stream()
    d_x, d_s = gpu(xforms), gpu(scale)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev.pose_device(d_x, d_s, stream=side)
        res = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, w.d_r, want=ALL, stream=side)
        res_lim = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, w.d_r, t_max=w.d_limits, want=ALL, stream=side)
    side.synchronize()
    got, lim = ({k: v.cpu().numpy() for k, v in r.items()} for r in (res, res_lim))
    hs.set_geometry(*p3d.transformed(a["prim_type"], a["prim_v"], ranges, xforms, scale))
    want = p3d.host_sweep_sphere(hs, w.o, w.d, w.r)
    assert_host_bits(got, want, "mixed behind a pose")
    assert_host_bits(lim, p3d.host_sweep_sphere(hs, w.o, w.d, w.r, t_max=w.limits), "mixed behind a pose, limits")
    assert as_bytes(want[1]) != as_bytes(w.free[1]), "the pose moved nothing"
    fresh = p3d.DeviceScene(hs, bvh=False)
    assert_same(got, ask(fresh, p3d.ACCEL_NONE, w), "mixed behind a pose, against a fresh scene")
    assert dev.status() == 0 and fresh.status() == 0


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
    import intersect_reference as ref
    w = worlds["triangles"]
    objects = ref.load_objects(w.path)
    got = ask(w.devs["device"], p3d.ACCEL_BVH, w)
    away = (got["object"] >= 0) & (got["t"] > 0) & (w.r > 1e-3)
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
    (tmp_path / "one.p3f").write_text(HEAD + "p 3\n0 -1 0\n0 1 0\n-2 0 0\np 3\n50 50 50\n51 50 50\n50 51 50\n")  # object 0 in the plane z = 0, (P1-P0) x (P2-P0) = (0, 0, 4); object 1 far away
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
    res = p3d.sweep_sphere_device(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, 0.25, want=ALL)
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert len(seen) == 1
    lo, size = seen[0]
    for name, t in res.items():
        assert t.data_ptr() + t.numel() * t.element_size() <= lo or t.data_ptr() >= lo + size, "the output %r lies on the radii" % name
    want = p3d.host_sweep_sphere(w.hs, w.o, w.d, 0.25)
    assert_host_bits({k: v.cpu().numpy() for k, v in res.items()}, want, "mixed, one radius")
