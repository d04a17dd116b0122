"""The k nearest surfaces over device tensors (p3d_nearest_k_device) on the GPU.

The yardstick is exact: HostScene.nearest_k, the brute force on the CPU that test_nearest_k_reference.py holds to the float64
model.  Under ACCEL_NONE and under ACCEL_BVH - uploaded and device-built trees, through the spill path of a deep tree, behind
a refit or a pose enqueued on the same stream - count, object, dist and closest must be its bits at every batch size and k,
with and without limits; at k = 1 the four outputs must be nearest_device's.  Every comparison here has tolerance 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from device_geometry_helpers import deformed_mesh
from frame_checks import as_bytes, gpu
import intersect_reference as ref
from live_scene_checks import plan
import nearest_k_reference as nk
import nearest_reference as near
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 129, 4099]  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block of many
KS = (1, 2, 5, 16)
ALL = ("count", "object", "dist", "closest", "normal")
FLT_MAX = near.FLT_MAX
INVALID, UNSUPPORTED = -1, -3
SEED = {"mixed": 400, "mixed_planes": 401, "planes": 402, "axis_aligned": 403, "tri5k": 404}  # the CPU suite's
TREES = {"mixed": ("host", "device"), "axis_aligned": ("host",), "tri5k": ("device",), "mixed_planes": ("none",), "planes": ("none",)}


class World:
    """One scene: host scene, device scenes by tree, max(BATCHES) points (the CPU suite's 2 000 first), the model's smallest
    distances to them (computed once, only to draw the limits from), and per k the limits and the host form's answers"""

    def __init__(self, name, path, trees):
        self.name = name
        self.path = path
        self.hs = p3d.HostScene(path)
        objs = ref.load_objects(path)
        self.n_objs = len(objs)
        self.devs = {tree: p3d.DeviceScene(self.hs, bvh={"host": True, "device": "device", "none": False}[tree]) for tree in trees}
        self.p = np.concatenate([near.scene_points(objs, SEED[name]), near.scene_points(objs, SEED[name] + 1000, max(BATCHES) - near.N_POINTS)])
        self.srt = nk.sorted_table(near.table(objs, self.p), 2 * max(KS))
        self.d_p = gpu(self.p) if trees else None
        self._limits, self._free, self._limited = {}, {}, {}

    def accels(self, tree):
        return [p3d.ACCEL_NONE] if tree == "none" else [p3d.ACCEL_NONE, p3d.ACCEL_BVH]

    def limits(self, k):
        if k not in self._limits:
            lim = nk.draw_k_limits(self.srt, k, SEED[self.name] + 50 + k)
            self._limits[k] = (lim, gpu(lim) if self.devs else None)
        return self._limits[k]

    def free(self, k):
        if k not in self._free:
            self._free[k] = self.hs.nearest_k(self.p, k)
        return self._free[k]

    def limited(self, k):
        if k not in self._limited:
            self._limited[k] = self.hs.nearest_k(self.p, k, max_dist=self.limits(k)[0])
        return self._limited[k]


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest_k")), tri5k=tri5k_path)
    w = {name: World(name, paths[name], TREES[name]) for name in TREES}
    assert w["tri5k"].devs["device"].export_bvh()["bvh_max_depth"] > 16  # deeper than the LDS window: the spill path runs
    return w


def ask(dev, accel, d_p, k, d_limits=None, want=ALL, **kw):
    return {name: v.cpu().numpy() for name, v in dev.nearest_k_device(accel, d_p, k, max_dist=d_limits, want=want, **kw).items()}


def assert_answers(got, want, k, what):
    """count, object, dist and closest equal `want` = (count, object, dist, closest) bit for bit; the no-answer values are exact"""
    n = len(got["count"])
    assert got["count"].dtype == np.int32 and got["count"].shape == (n,) and (got["count"] == want[0][:n]).all(), what + ": count"
    assert got["object"].dtype == np.int32 and got["object"].shape == (n, k) and (got["object"] == want[1][:n]).all(), what + ": object"
    assert got["dist"].shape == (n, k) and as_bytes(got["dist"]) == as_bytes(want[2][:n]), what + ": dist"
    assert got["closest"].shape == (n, k, 3) and as_bytes(got["closest"]) == as_bytes(want[3][:n]), what + ": closest"
    none = np.arange(k)[None, :] >= got["count"][:, None]
    assert (got["object"][none] == -1).all() and (got["object"][~none] >= 0).all(), what + ": the rows behind count"
    assert (got["dist"][none] == FLT_MAX).all() and as_bytes(got["closest"][none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), what + ": the no-answer values"


def assert_normals(dev, got, what, most=24):
    obj, q, nrm = got["object"], got["closest"], got["normal"]
    assert nrm.shape == q.shape
    none = obj < 0
    assert as_bytes(nrm[none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), what + ": a normal in a row behind count"
    for j in np.unique(obj[~none])[:most]:
        m = obj == j
        assert as_bytes(nrm[m]) == as_bytes(dev.object_normal(int(j), q[m])), "%s: the normal of object %d" % (what, j)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", BATCHES)
def test_the_device_form_is_the_host_form(n, k, worlds):
    for name, w in worlds.items():
        lim, d_lim = w.limits(k)
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                what = "%s, %s tree, accel %d, %d points, k = %d" % (name, tree, accel, n, k)
                got = ask(dev, accel, w.d_p[:n], k)
                assert_answers(got, w.free(k), k, what)
                assert (got["count"] == min(k, w.n_objs)).all()
                assert_normals(dev, got, what)
                lim_got = ask(dev, accel, w.d_p[:n], k, d_lim[:n])
                assert_answers(lim_got, w.limited(k), k, what + ", limits")
                assert_normals(dev, lim_got, what + ", limits")
                if n >= 63 and w.n_objs >= k:
                    c = lim_got["count"]
                    assert (c == 0).any() and (c == k).any() and (k == 1 or ((c > 0) & (c < k)).any()), what + ": the three sorts of point in one batch"
                # outputs may be the caller's, and the optional ones may be left out
                mine = {"count": torch.full((n,), 77, dtype=torch.int32, device="cuda"), "object": torch.full((n, k), 77, dtype=torch.int32, device="cuda"),
                        "closest": torch.full((n, k, 3), 5.0, device="cuda")}
                back = dev.nearest_k_device(accel, w.d_p[:n], k, max_dist=d_lim[:n], want=("closest",), out=mine)
                assert list(back) == ["count", "object", "closest"] and all(back[key] is mine[key] for key in mine)
                want = w.limited(k)
                assert (mine["count"].cpu().numpy() == want[0][:n]).all() and (mine["object"].cpu().numpy() == want[1][:n]).all(), what
                assert as_bytes(mine["closest"].cpu().numpy()) == as_bytes(want[3][:n]), what
                only = dev.nearest_k_device(accel, w.d_p[:n], k, want=())
                assert list(only) == ["count", "object"] and (only["object"].cpu().numpy() == w.free(k)[1][:n]).all(), what
                assert (only["count"].cpu().numpy() == w.free(k)[0][:n]).all(), what
            assert dev.status() == 0


def test_k_1_is_nearest_device(worlds):
    w = worlds["tri5k"]
    dev = w.devs["device"]
    n = max(BATCHES)
    lim, d_lim = w.limits(1)
    host = {False: w.hs.nearest(w.p), True: w.hs.nearest(w.p, max_dist=lim)}
    for accel in w.accels("device"):
        for d_m in (None, d_lim):
            one = {name: v.cpu().numpy() for name, v in dev.nearest_device(accel, w.d_p, max_dist=d_m, want=("object", "dist", "closest", "normal")).items()}
            got = ask(dev, accel, w.d_p, 1, d_m)
            for name in ("object", "dist", "closest", "normal"):
                assert as_bytes(got[name]) == as_bytes(one[name]), "accel %d, %s: %s" % (accel, "no limit" if d_m is None else "limits", name)
            assert (got["count"] == (one["object"] >= 0)).all()
            assert d_m is None or 0 < got["count"].sum() < n
            # (nearest_device is the k = 1 launch of the same kernel: the independent statement is the host's k = 1 brute force)
            h_object, h_dist, h_closest = host[d_m is not None]
            assert (got["object"][:, 0] == h_object).all(), "accel %d: HostScene.nearest's object" % accel
            assert as_bytes(got["dist"][:, 0]) == as_bytes(h_dist) and as_bytes(got["closest"][:, 0]) == as_bytes(h_closest), "accel %d: HostScene.nearest's bits" % accel
    assert dev.status() == 0


def test_limits_that_keep_nothing_or_everything(worlds):
    n, k = 515, 5
    for name, w in worlds.items():
        for tree, dev in w.devs.items():
            for accel in w.accels(tree):
                what = "%s, %s tree, accel %d" % (name, tree, accel)
                for value in (0.0, -2.0, np.nan, -np.inf):
                    got = ask(dev, accel, w.d_p[:n], k, gpu(np.full(n, value, np.float32)))
                    assert (got["count"] == 0).all() and (got["object"] == -1).all() and (got["dist"] == FLT_MAX).all(), "%s: a limit of %g" % (what, value)
                    for key in ("closest", "normal"):
                        assert as_bytes(got[key]) == as_bytes(np.zeros((n, k, 3), np.float32)), "%s: a limit of %g, %s" % (what, value, key)
                assert_answers(ask(dev, accel, w.d_p[:n], k, gpu(np.full(n, np.inf, np.float32))), w.free(k), k, what + ", infinite limits")


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
    got = ask(dev, p3d.ACCEL_NONE, gpu(np.zeros((65, 3), np.float32)), 3)
    assert (got["count"] == 0).all() and (got["object"] == -1).all() and (got["dist"] == FLT_MAX).all() and not got["closest"].any() and not got["normal"].any()
    lib = p3d.lib()
    w = worlds["mixed"]
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):  # whatever the pointers, once k is valid
        assert lib.p3d_nearest_k_device(w.devs["host"]._h, accel, 0, 3, None, None, None, None, None, None, None, None) == 0
        for k in (0, 17):
            assert lib.p3d_nearest_k_device(w.devs["host"]._h, accel, 0, k, None, None, None, None, None, None, None, None) == INVALID
            assert b"k must be" in lib.p3d_last_error()


def test_refusals_enqueue_nothing(worlds):
    w = worlds["mixed"]
    dev, no_tree = w.devs["host"], worlds["mixed_planes"].devs["none"]
    with_planes = p3d.DeviceScene(worlds["planes"].hs, bvh=True)
    lib = p3d.lib()
    n, k = 129, 2
    d_p, d_m = w.d_p[:n], w.limits(k)[1][:n]
    outs = dict(count=torch.full((n,), 77, dtype=torch.int32, device="cuda"), object=torch.full((n, k), 77, dtype=torch.int32, device="cuda"),
                dist=torch.full((n, k), 123.0, device="cuda"), closest=torch.full((n, k, 3), 123.0, device="cuda"),
                normal=torch.full((n, k, 3), 123.0, device="cuda"))
    ptr = lambda name: C.c_void_p(outs[name].data_ptr())
    host = np.zeros((n, k * 3), np.float32)
    big = 0x00ffff00  # points no buffer of this call's outputs holds
    huge = torch.empty((big, 3), device="cuda")  # (never read: every call it is given to is refused)
    counts = torch.empty(big, dtype=torch.int32, device="cuda")  # (never written)
    # Host memory must be refused BEFORE any launch.  It goes in first with a count no output buffer here can serve: were the
    # pointer check to let it through, the count buffer would end behind its allocation: no kernel would ever be given a host address.
    assert lib.p3d_nearest_k_device(dev._h, p3d.ACCEL_BVH, big, k, C.c_void_p(host.ctypes.data), None, ptr("count"), ptr("object"),
                                    None, None, None, None) == INVALID
    assert b"d_point is host memory" in lib.p3d_last_error(), lib.p3d_last_error()
    q = lambda scene, accel, points, kk=k, **kw: scene.nearest_k_device(accel, points, kk, want=kw.pop("want", ALL), out=kw.pop("out", outs), **kw)
    short = lambda **over: dict({"count": (counts.data_ptr(), big), "object": (outs["object"].data_ptr(), big)}, **over)
    cases = [
        ("the grid", UNSUPPORTED, "grid", lambda: q(dev, p3d.ACCEL_GRID, d_p)),
        ("a tree over a scene with planes", UNSUPPORTED, "plane", lambda: q(with_planes, p3d.ACCEL_BVH, d_p)),
        ("a scene without a tree", INVALID, "without BVH", lambda: q(no_tree, p3d.ACCEL_BVH, d_p)),
        ("an unknown accel", INVALID, "accel", lambda: q(dev, 7, d_p)),
        ("k = 0", INVALID, "k must be", lambda: q(dev, p3d.ACCEL_BVH, d_p, 0, out={name: (v.data_ptr(), n) for name, v in outs.items()})),
        ("k = 17", INVALID, "k must be", lambda: q(dev, p3d.ACCEL_NONE, d_p, 17, out={name: (v.data_ptr(), n) for name, v in outs.items()})),
        ("misaligned points", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_BVH, (d_p.data_ptr() + 2, n))),
        ("a misaligned limit", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_NONE, d_p, max_dist=(d_m.data_ptr() + 1, n))),
        ("a misaligned count", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_BVH, d_p, out=dict(outs, count=(outs["count"].data_ptr() + 2, n)))),
        ("a misaligned output", INVALID, "aligned", lambda: q(dev, p3d.ACCEL_BVH, d_p, out=dict(outs, dist=(outs["dist"].data_ptr() + 2, n)))),
        ("host points", INVALID, "d_point is host memory", lambda: q(dev, p3d.ACCEL_BVH, (host.ctypes.data, n))),
        ("a host limit", INVALID, "d_max_dist is host memory", lambda: q(dev, p3d.ACCEL_NONE, d_p, max_dist=(host.ctypes.data, n))),
        ("a host count", INVALID, "d_count is host memory", lambda: q(dev, p3d.ACCEL_NONE, d_p, out=dict(outs, count=(host.ctypes.data, n)))),
        ("a host object", INVALID, "d_object is host memory", lambda: q(dev, p3d.ACCEL_BVH, d_p, out=dict(outs, object=(host.ctypes.data, n)))),
        ("a host dist", INVALID, "d_dist is host memory", lambda: q(dev, p3d.ACCEL_BVH, d_p, out=dict(outs, dist=(host.ctypes.data, n)))),
        ("a host closest", INVALID, "d_closest is host memory", lambda: q(dev, p3d.ACCEL_NONE, d_p, out=dict(outs, closest=(host.ctypes.data, n)))),
        ("a host normal", INVALID, "d_normal is host memory", lambda: q(dev, p3d.ACCEL_BVH, d_p, out=dict(outs, normal=(host.ctypes.data, n)))),
        # too short: torch hands out pieces of larger allocations, so "behind the allocation" needs a count beyond any of them
        ("points too short", INVALID, "d_point ends behind its allocation", lambda: q(dev, p3d.ACCEL_BVH, (d_p.data_ptr(), big), want=(), out=short())),
        ("a limit too short", INVALID, "d_max_dist ends behind its allocation",
         lambda: q(dev, p3d.ACCEL_NONE, (huge.data_ptr(), big), max_dist=(d_m.data_ptr(), big), want=(), out=short())),
        ("a count too short", INVALID, "d_count ends behind its allocation",
         lambda: q(dev, p3d.ACCEL_NONE, (huge.data_ptr(), big), want=(), out=short(count=(outs["count"].data_ptr(), big)))),
        ("an object too short", INVALID, "d_object ends behind its allocation", lambda: q(dev, p3d.ACCEL_NONE, (huge.data_ptr(), big), want=(), out=short())),
        # n rows of n*k: the sizes are those of this call, not of p3d_nearest_device (the count buffer serves n * 1, not n * k)
        ("an object of n, not n k, elements", INVALID, "d_object ends behind its allocation",
         lambda: q(dev, p3d.ACCEL_NONE, (huge.data_ptr(), big), want=(), out=short(object=(counts.data_ptr(), big)))),
    ]
    for what, code, word, call in cases:
        try:
            call()
            raised = None
        except p3d.P3DError as e:
            raised = e
        assert raised is not None, what + ": accepted"
        assert raised.code == code and word in str(raised), "%s: %s" % (what, raised)
    del huge, counts
    tail = (ptr("dist"), ptr("closest"), ptr("normal"), None)
    d = C.c_void_p(d_p.data_ptr())
    assert lib.p3d_nearest_k_device(dev._h, p3d.ACCEL_BVH, n, k, d, None, None, ptr("object"), *tail) == INVALID  # a null d_count
    assert b"null argument" in lib.p3d_last_error()
    assert lib.p3d_nearest_k_device(dev._h, p3d.ACCEL_BVH, n, k, d, None, ptr("count"), None, *tail) == INVALID  # a null d_object
    assert b"null argument" in lib.p3d_last_error()
    assert lib.p3d_nearest_k_device(dev._h, p3d.ACCEL_BVH, n, k, None, None, ptr("count"), ptr("object"), *tail) == INVALID
    # the planes are there for the brute force
    pw = worlds["planes"]
    assert (ask(with_planes, p3d.ACCEL_NONE, pw.d_p[:n], k, want=())["object"] == pw.free(k)[1][:n]).all()
    torch.cuda.synchronize()
    assert bool((outs["count"] == 77).all()) and bool((outs["object"] == 77).all())
    assert all(bool((outs[name] == 123.0).all()) for name in ("dist", "closest", "normal"))
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
    n, k = 4099, 4
    lim, d_lim = w.limits(k)
    shapes = {"count": (n,), "object": (n, k), "dist": (n, k), "closest": (n, k, 3), "normal": (n, k, 3)}
    outs = {name: torch.empty(shape, dtype=torch.int32 if name in ("count", "object") else torch.float32, device="cuda") for name, shape in shapes.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        wave = base
        for _ in range(50):  # some work in front, so that the positions are still being produced when the calls begin
            wave = torch.sin(wave * 1.5 + 0.25)
        moved = (d_soup + 0.0 * wave).contiguous()
        dev.refit_triangles(0, moved, stream=side)
        dev.nearest_k_device(p3d.ACCEL_BVH, w.d_p[:n], k, max_dist=d_lim[:n], want=ALL, stream=side, out=outs)
    side.synchronize()
    got = {name: v.cpu().numpy() for name, v in outs.items()}
    assert as_bytes(moved.cpu().numpy()) == as_bytes(soup)
    hs.set_geometry(*p3d.deformed(a["prim_v"], 0, soup))
    want = hs.nearest_k(w.p[:n], k, max_dist=lim[:n])
    assert_answers(got, want, k, "tri5k behind a refit")
    before = w.limited(k)
    assert (want[1] != before[1][:n]).any() or as_bytes(want[2]) != as_bytes(before[2][:n]), "the refit moved nothing the points can see"
    fresh = p3d.DeviceScene(hs, bvh=False)
    again = ask(fresh, p3d.ACCEL_NONE, w.d_p[:n], k, d_lim[:n])
    for name in ALL:
        assert as_bytes(got[name]) == as_bytes(again[name]), "tri5k behind a refit, against a fresh scene: " + name
    assert (got["count"] == 0).any() and (got["count"] == k).any() and ((got["count"] > 0) & (got["count"] < k)).any()
    assert dev.status() == 0 and fresh.status() == 0


def test_behind_a_pose_on_the_same_stream(worlds):
    w = worlds["mixed"]
    hs = p3d.HostScene(w.path)
    a = hs.arrays()
    dev = p3d.DeviceScene(hs, bvh="device")
    ranges, xforms, scale = plan(a, 93)  # spheres and triangles under a rigid move, boxes under a positive-diagonal one
    dev.set_rig(ranges, 2)
    n, k = 4099, 4
    lim, d_lim = w.limits(k)
    side = torch.cuda.Stream()
    d_x, d_s = gpu(xforms), gpu(scale)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev.pose_device(d_x, d_s, stream=side)
        res = dev.nearest_k_device(p3d.ACCEL_BVH, w.d_p[:n], k, want=ALL, stream=side)
        res_lim = dev.nearest_k_device(p3d.ACCEL_BVH, w.d_p[:n], k, max_dist=d_lim[:n], want=ALL, stream=side)
    side.synchronize()
    got, lim_got = ({name: v.cpu().numpy() for name, v in r.items()} for r in (res, res_lim))
    hs.set_geometry(*p3d.transformed(a["prim_type"], a["prim_v"], ranges, xforms, scale))
    want = hs.nearest_k(w.p[:n], k)
    assert_answers(got, want, k, "mixed behind a pose")
    assert_answers(lim_got, hs.nearest_k(w.p[:n], k, max_dist=lim[:n]), k, "mixed behind a pose, limits")
    assert as_bytes(want[2]) != as_bytes(w.free(k)[2][:n]), "the pose moved nothing"
    fresh = p3d.DeviceScene(hs, bvh=False)
    for d_m, mine in ((None, got), (d_lim[:n], lim_got)):
        again = ask(fresh, p3d.ACCEL_NONE, w.d_p[:n], k, d_m)
        for name in ALL:
            assert as_bytes(mine[name]) == as_bytes(again[name]), "mixed behind a pose, against a fresh scene: " + name
    assert dev.status() == 0 and fresh.status() == 0
