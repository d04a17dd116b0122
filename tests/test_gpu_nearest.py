"""Nearest-surface queries over device tensors (p3d_nearest_device) on the GPU.

The yardstick is exact: HostScene.nearest, the brute force on the CPU that test_nearest_reference.py holds to the float64
model.  Under ACCEL_NONE object, dist and closest must be its bits at every batch size, with and without limits; under
ACCEL_BVH they must be the ACCEL_NONE bits, on uploaded and on device-built trees, through the spill path of a deep tree, and
behind a refit or a pose enqueued on the same stream.  Every comparison here has tolerance 0.

The library's debug hooks expose no scratch sizes, so "a second call of the same n allocates nothing" is not tested here."""
import ctypes as C

import numpy as np
import pytest
import torch

from device_geometry_helpers import deformed_mesh
from frame_checks import as_bytes, gpu
import intersect_reference as ref
from live_scene_checks import plan
import nearest_reference as near
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 129, 4099]  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block of many
ALL = ("object", "dist", "closest", "normal")
FLT_MAX = near.FLT_MAX
INVALID, UNSUPPORTED = -1, -3
SEED = {"mixed": 400, "mixed_planes": 401, "planes": 402, "axis_aligned": 403, "tri5k": 404}  # the CPU suite's


class World:
    """One scene: host scene, device scenes by tree, max(BATCHES) points (the CPU suite's 2 000 first), their limits (drawn
    from the host form's distances as the CPU suite draws them from the model's), and the host form's answers"""

    def __init__(self, name, path, trees):
        self.name = name
        self.path = path
        self.hs = p3d.HostScene(path)
        objs = ref.load_objects(path)
        self.planes = any(ob["kind"] == ref.PLANE for ob in objs)
        self.devs = {tree: p3d.DeviceScene(self.hs, bvh={"host": True, "device": "device", "none": False}[tree]) for tree in trees}
        self.p = np.concatenate([near.scene_points(objs, SEED[name]), near.scene_points(objs, SEED[name] + 1000, max(BATCHES) - near.N_POINTS)])
        self.free = self.hs.nearest(self.p)
        self.limits = near.draw_limits(self.free[1].astype(np.float64), SEED[name] + 50)
        self.limited = self.hs.nearest(self.p, max_dist=self.limits)
        self.d_p, self.d_limits = gpu(self.p), gpu(self.limits)

    def accels(self, tree):
        return [p3d.ACCEL_NONE] if tree == "none" else [p3d.ACCEL_NONE, p3d.ACCEL_BVH]


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest")), tri5k=tri5k_path)
    trees = {"mixed": ("host", "device"), "axis_aligned": ("host",), "tri5k": ("device",), "mixed_planes": ("none",), "planes": ("none",)}
    w = {name: World(name, paths[name], trees[name]) for name in trees}
    assert w["tri5k"].devs["device"].export_bvh()["bvh_max_depth"] > 16  # deeper than the LDS window: the spill path runs
    return w


def ask(dev, accel, d_p, d_limits=None, want=ALL, **kw):
    return {k: v.cpu().numpy() for k, v in dev.nearest_device(accel, d_p, max_dist=d_limits, want=want, **kw).items()}


def assert_answers(got, want, what):
    """object, dist and closest equal `want` = (object, dist, closest) bit for bit; the no-answer values are exact"""
    n = len(got["object"])
    assert got["object"].dtype == np.int32 and (got["object"] == want[0][:n]).all(), what + ": object"
    assert as_bytes(got["dist"]) == as_bytes(want[1][:n]), what + ": dist"
    assert as_bytes(got["closest"]) == as_bytes(want[2][:n]), what + ": closest"
    none = got["object"] < 0
    assert (got["dist"][none] == FLT_MAX).all() and as_bytes(got["closest"][none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), what + ": the no-answer values"


def assert_normals(dev, got, what, most=24):
    obj, q, nrm = got["object"], got["closest"], got["normal"]
    none = obj < 0
    assert as_bytes(nrm[none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), what + ": a normal where nothing was found"
    for j in np.unique(obj[~none])[:most]:
        m = obj == j
        assert as_bytes(nrm[m]) == as_bytes(dev.object_normal(int(j), q[m])), "%s: the normal of object %d" % (what, j)


@pytest.mark.parametrize("n", BATCHES)
def test_the_device_form_is_the_host_form(n, worlds):
    for name, w in worlds.items():
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                what = "%s, %s tree, accel %d, %d points" % (name, tree, accel, n)
                got = ask(dev, accel, w.d_p[:n])
                assert_answers(got, w.free, what)
                assert (got["object"] >= 0).all()
                assert_normals(dev, got, what)
                lim = ask(dev, accel, w.d_p[:n], w.d_limits[:n])
                assert_answers(lim, w.limited, what + ", limits")
                assert_normals(dev, lim, what + ", limits")
                if n >= 63:
                    assert 0 < (lim["object"] >= 0).sum() < n, what + ": found and not found in one batch"
                # the optional outputs may be left out, and outputs may be the caller's
                mine = {"object": torch.full((n,), 77, dtype=torch.int32, device="cuda"), "closest": torch.full((n, 3), 5.0, device="cuda")}
                back = dev.nearest_device(accel, w.d_p[:n], max_dist=w.d_limits[:n], want=("closest",), out=mine)
                assert list(back) == ["object", "closest"] and back["object"] is mine["object"] and back["closest"] is mine["closest"]
                assert (mine["object"].cpu().numpy() == w.limited[0][:n]).all() and as_bytes(mine["closest"].cpu().numpy()) == as_bytes(w.limited[2][:n]), what
                only = dev.nearest_device(accel, w.d_p[:n], want=())
                assert list(only) == ["object"] and (only["object"].cpu().numpy() == w.free[0][:n]).all(), what
            assert dev.status() == 0


def test_limits_that_keep_nothing_or_everything(worlds):
    for name, w in worlds.items():
        n = 515
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                what = "%s, %s tree, accel %d" % (name, tree, accel)
                for value in (0.0, -2.0, np.nan, -np.inf):
                    got = ask(dev, accel, w.d_p[:n], gpu(np.full(n, value, np.float32)))
                    assert (got["object"] == -1).all() and (got["dist"] == FLT_MAX).all(), "%s: a limit of %g" % (what, value)
                    for k in ("closest", "normal"):
                        assert as_bytes(got[k]) == as_bytes(np.zeros((n, 3), np.float32)), "%s: a limit of %g, %s" % (what, value, k)
                assert_answers(ask(dev, accel, w.d_p[:n], gpu(np.full(n, np.inf, np.float32))), w.free, what + ", infinite limits")
                # the limit at the distance itself (d2 against the float32 square of sqrtf(d2): the host form says which way), and twice it
                d = w.free[1][:n]
                same = ask(dev, accel, w.d_p[:n], gpu(d))
                assert_answers(same, w.hs.nearest(w.p[:n], max_dist=d), what + ", the distance as the limit")
                twice = ask(dev, accel, w.d_p[:n], gpu(np.where(d > 0, 2 * d, np.float32(1e-3))))
                assert_answers(twice, w.free, what + ", twice the distance as the limit")


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


def test_an_empty_scene_and_an_empty_batch(tmp_path, worlds):
    path = tmp_path / "empty.p3f"
    path.write_text(HEAD)
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh=False)
    got = ask(dev, p3d.ACCEL_NONE, gpu(np.zeros((65, 3), np.float32)))
    assert (got["object"] == -1).all() and (got["dist"] == FLT_MAX).all() and not got["closest"].any() and not got["normal"].any()
    lib = p3d.lib()
    w = worlds["mixed"]
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):  # whatever the pointers
        assert lib.p3d_nearest_device(w.devs["host"]._h, accel, 0, None, None, None, None, None, None, None) == 0


def test_refusals_enqueue_nothing(worlds):
    w = worlds["mixed"]
    dev, no_tree = w.devs["host"], worlds["mixed_planes"].devs["none"]
    with_planes = p3d.DeviceScene(worlds["planes"].hs, bvh=True)
    lib = p3d.lib()
    n = 129
    d_p, d_m = w.d_p[:n], w.d_limits[:n]
    outs = dict(object=torch.full((n,), 77, dtype=torch.int32, device="cuda"), dist=torch.full((n,), 123.0, device="cuda"),
                closest=torch.full((n, 3), 123.0, device="cuda"), normal=torch.full((n, 3), 123.0, device="cuda"))
    host = np.zeros((n, 3), np.float32)
    huge = torch.empty((0x00ffff00, 3), device="cuda")  # (never read: every call it is given to is refused)
    big = 0x00ffff00  # points no buffer here holds: 200 MB of them
    # Host memory must be refused BEFORE any launch.  It goes in first with a count no buffer here can serve: were the pointer
    # check to let it through, the object buffer would end behind its allocation: no kernel would ever be given a host address.
    assert lib.p3d_nearest_device(dev._h, p3d.ACCEL_BVH, big, C.c_void_p(host.ctypes.data), None, C.c_void_p(outs["object"].data_ptr()),
                                  None, None, None, None) == INVALID
    assert b"d_point is host memory" in lib.p3d_last_error(), lib.p3d_last_error()
    cases = [
        ("the grid", UNSUPPORTED, "grid", lambda: dev.nearest_device(p3d.ACCEL_GRID, d_p, want=ALL, out=outs)),
        ("a tree over a scene with planes", UNSUPPORTED, "plane", lambda: with_planes.nearest_device(p3d.ACCEL_BVH, d_p, want=ALL, out=outs)),
        ("a scene without a tree", INVALID, "without BVH", lambda: no_tree.nearest_device(p3d.ACCEL_BVH, d_p, want=ALL, out=outs)),
        ("an unknown accel", INVALID, "accel", lambda: dev.nearest_device(7, d_p, want=ALL, out=outs)),
        ("misaligned points", INVALID, "aligned", lambda: dev.nearest_device(p3d.ACCEL_BVH, (d_p.data_ptr() + 2, n), want=ALL, out=outs)),
        ("a misaligned limit", INVALID, "aligned", lambda: dev.nearest_device(p3d.ACCEL_NONE, d_p, max_dist=(d_m.data_ptr() + 1, n), want=ALL, out=outs)),
        ("a misaligned output", INVALID, "aligned",
         lambda: dev.nearest_device(p3d.ACCEL_BVH, d_p, want=ALL, out=dict(outs, dist=(outs["dist"].data_ptr() + 2, n)))),
        ("host points", INVALID, "d_point is host memory", lambda: dev.nearest_device(p3d.ACCEL_BVH, (host.ctypes.data, n), want=ALL, out=outs)),
        ("a host limit", INVALID, "d_max_dist is host memory", lambda: dev.nearest_device(p3d.ACCEL_NONE, d_p, max_dist=(host.ctypes.data, n), want=ALL, out=outs)),
        # too short: torch hands out pieces of larger allocations, so "behind the allocation" needs a count beyond any of them
        ("points too short", INVALID, "d_point ends behind its allocation",
         lambda: dev.nearest_device(p3d.ACCEL_BVH, (d_p.data_ptr(), big), want=(), out={"object": (outs["object"].data_ptr(), big)})),
        ("a limit too short", INVALID, "d_max_dist ends behind its allocation",
         lambda: dev.nearest_device(p3d.ACCEL_NONE, (huge.data_ptr(), big), max_dist=(d_m.data_ptr(), big), want=(), out={"object": (outs["object"].data_ptr(), big)})),
        ("an output too short", INVALID, "d_object ends behind its allocation",
         lambda: dev.nearest_device(p3d.ACCEL_NONE, (huge.data_ptr(), big), want=(), out={"object": (outs["object"].data_ptr(), big)})),
    ]
    for what, code, word, call in cases:
        try:
            call()
            raised = None
        except p3d.P3DError as e:
            raised = e
        assert raised is not None, what + ": accepted"
        assert raised.code == code and word in str(raised), "%s: %s" % (what, raised)
    del huge
    args = (C.c_void_p(outs["dist"].data_ptr()), C.c_void_p(outs["closest"].data_ptr()), C.c_void_p(outs["normal"].data_ptr()), None)
    assert lib.p3d_nearest_device(dev._h, p3d.ACCEL_BVH, n, C.c_void_p(d_p.data_ptr()), None, None, *args) == INVALID  # null d_object
    assert b"null argument" in lib.p3d_last_error()
    assert lib.p3d_nearest_device(dev._h, p3d.ACCEL_BVH, n, None, None, C.c_void_p(outs["object"].data_ptr()), *args) == INVALID
    # the planes are there for the brute force
    assert (ask(with_planes, p3d.ACCEL_NONE, worlds["planes"].d_p[:n], want=())["object"] == worlds["planes"].free[0][:n]).all()
    torch.cuda.synchronize()
    assert bool((outs["object"] == 77).all()) and all(bool((outs[k] == 123.0).all()) for k in ("dist", "closest", "normal"))
    assert dev.status() == 0 and with_planes.status() == 0


def test_behind_a_refit_on_the_same_stream(worlds, tri5k_path):
    """refit_triangles with moved positions on a side stream, the query behind it on that stream, nothing in between: the
    answers are those of a fresh scene of the moved geometry under ACCEL_NONE, and the host form's after set_geometry."""
    w = worlds["tri5k"]
    hs = p3d.HostScene(tri5k_path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    soup = deformed_mesh(a, seed=91, fraction=0.03)[2]
    base, d_soup = gpu(a["prim_v"].reshape(-1, 3)), gpu(soup)
    n = 4099
    outs = {k: (torch.empty((n,) if c is None else (n, c), dtype=getattr(torch, t), device="cuda")) for k, (t, c) in p3d._NEAREST_OUTPUTS.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wave = base
        for _ in range(50):  # some work in front, so that the positions are still being produced when the calls begin
            wave = torch.sin(wave * 1.5 + 0.25)
        moved = (d_soup + 0.0 * wave).contiguous()
        dev.refit_triangles(0, moved, stream=side)
        dev.nearest_device(p3d.ACCEL_BVH, w.d_p[:n], max_dist=w.d_limits[:n], want=ALL, stream=side, out=outs)
    side.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    assert as_bytes(moved.cpu().numpy()) == as_bytes(soup)
    hs.set_geometry(*p3d.deformed(a["prim_v"], 0, soup))
    want = hs.nearest(w.p[:n], max_dist=w.limits[:n])
    assert_answers(got, want, "tri5k behind a refit")
    assert (want[0] != w.limited[0][:n]).any() or as_bytes(want[1]) != as_bytes(w.limited[1][:n]), "the refit moved nothing the points can see"
    fresh = p3d.DeviceScene(hs, bvh=False)
    again = ask(fresh, p3d.ACCEL_NONE, w.d_p[:n], w.d_limits[:n])
    for k in ALL:
        assert as_bytes(got[k]) == as_bytes(again[k]), "tri5k behind a refit, against a fresh scene: " + k
    assert 0 < (got["object"] >= 0).sum() < n
    assert dev.status() == 0 and fresh.status() == 0


def test_behind_a_pose_on_the_same_stream(worlds):
    w = worlds["mixed"]
    hs = p3d.HostScene(w.path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    ranges, xforms, scale = plan(a, 93)  # spheres and triangles under a rigid move, boxes under a positive-diagonal one
    dev.set_rig(ranges, 2)
    n = 4099
    side = torch.cuda.Stream()
    d_x, d_s = gpu(xforms), gpu(scale)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev.pose_device(d_x, d_s, stream=side)
        res = dev.nearest_device(p3d.ACCEL_BVH, w.d_p[:n], want=ALL, stream=side)
        res_lim = dev.nearest_device(p3d.ACCEL_BVH, w.d_p[:n], max_dist=w.d_limits[:n], want=ALL, stream=side)
    side.synchronize()
    got, lim = ({k: v.cpu().numpy() for k, v in r.items()} for r in (res, res_lim))
    hs.set_geometry(*p3d.transformed(a["prim_type"], a["prim_v"], ranges, xforms, scale))
    want = hs.nearest(w.p[:n])
    assert_answers(got, want, "mixed behind a pose")
    assert_answers(lim, hs.nearest(w.p[:n], max_dist=w.limits[:n]), "mixed behind a pose, limits")
    assert as_bytes(want[1]) != as_bytes(w.free[1][:n]), "the pose moved nothing"
    fresh = p3d.DeviceScene(hs, bvh=False)
    again = ask(fresh, p3d.ACCEL_NONE, w.d_p[:n])
    for k in ALL:
        assert as_bytes(got[k]) == as_bytes(again[k]), "mixed behind a pose, against a fresh scene: " + k
    assert dev.status() == 0 and fresh.status() == 0
