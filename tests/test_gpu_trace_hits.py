"""The hits in order along a ray over device tensors (p3d_trace_hits_device) on the GPU.

Under ACCEL_NONE the yardstick is exact: the brute force over the CPU oracle's per-object test (hits_reference.brute_hits),
every ray, count, total, object and t in bits.  The BVH traversal is held to that GPU brute force on the rays the float64
model calls well-conditioned (hits_reference.all_hits_margin, under the 5 % cap of intersect_reference.py): every output in
bits, with and without total (the two cull bounds), with and without limits, on uploaded and device-built trees and through
the spill path of a deep tree.  The slats fill a list of sixteen; the closed cube gives the parity of the crossings."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import device_query_contract as dq
from device_query_contract import FLT_MAX, INVALID, UNSUPPORTED
from frame_checks import as_bytes, gpu
import hits_reference as hr
import intersect_reference as ref
import p3d_amd as p3d
from ray_query_checks import BATCHES, CLOSEST_ALL, N_MESH, N_MODEL, World, limit_sets
from scene_update_helpers import BOX, SPHERE, TRIANGLE
import segment_reference as seg

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 16)
ROWS = ("count", "object", "t", "hit_point", "normal")
ALL = ROWS + ("total",)
INF = np.float32(np.inf)


class RayWorld(World):
    """World with rays of the caller's"""

    def __init__(self, path, trees, o, d, oracle=True):
        super().__init__(path, trees, n=8, oracle=oracle)
        self.set_rays(o, d)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("trace_hits")
    w = {name: World(path, ("host", "device") if name == "mixed" else ("host",)) for name, path in ref.scene_paths(tmp).items()}
    w["slats"] = RayWorld(hr.write_slats(tmp / "slats.p3f"), ("device",), *hr.slat_rays(21, max(BATCHES)))
    return w


@pytest.fixture(scope="module")
def cube(tmp_path_factory):
    o, d, inside = hr.cube_rays(23, N_MESH)
    w = RayWorld(hr.write_cube(tmp_path_factory.mktemp("trace_hits_cube") / "cube.p3f"), ("device",), o, d, oracle=False)
    w.inside = inside
    return w


def through_rays(objs, seed, n):
    """n rays from 1.5 scene radii out, aimed into the inner half of the scene: they cross a mesh several times"""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([np.stack([ob["p0"], ob["p1"], ob["p2"]]) for ob in objs])
    c, r = (pts.min(0) + pts.max(0)) / 2, np.linalg.norm(pts.max(0) - pts.min(0)) / 2
    o = (c + 1.5 * r * ref._unit(rng, n)).astype(np.float32)
    return o, ref.normalize32((c + 0.5 * r * ref._in_ball(rng, n)).astype(np.float32) - o)


@pytest.fixture(scope="module")
def mesh(tri5k_path):
    """A few thousand triangles under a tree built on the device, deeper than the 16-entry LDS window of the stack"""
    w = RayWorld(tri5k_path, ("device",), *through_rays(ref.load_objects(tri5k_path), 9, N_MESH), oracle=False)
    assert w.devs["device"].export_bvh()["bvh_max_depth"] > 16
    return w


def ask(dev, accel, d_o, d_d, k, t_max=None, want=ALL, **kw):
    t_max = gpu(np.asarray(t_max, np.float32)) if isinstance(t_max, np.ndarray) else t_max
    return {name: v.cpu().numpy() for name, v in dev.trace_hits_device(accel, d_o, d_d, k, t_max=t_max, want=want, **kw).items()}


def assert_rows(got, k, what):
    """shapes and dtypes, and the rows behind count hold the miss values"""
    n = len(got["count"])
    assert got["count"].dtype == np.int32 and got["count"].shape == (n,) and got["object"].dtype == np.int32 and got["object"].shape == (n, k), what
    none = np.arange(k)[None, :] >= got["count"][:, None]
    assert (got["object"][none] == -1).all() and (got["object"][~none] >= 0).all(), what + ": the rows behind count"
    if "t" in got:
        assert got["t"].shape == (n, k) and (got["t"][none] == FLT_MAX).all(), what + ": t behind count"
    for name in ("hit_point", "normal"):
        if name in got:
            assert got[name].shape == (n, k, 3) and as_bytes(got[name][none]) == as_bytes(np.zeros((int(none.sum()), 3), np.float32)), "%s: %s behind count" % (what, name)
    if "total" in got:
        assert got["total"].dtype == np.int32 and (got["count"] == np.minimum(got["total"], k)).all(), what + ": count = min(total, k)"


def assert_is_brute(got, want, k, what):
    count, total, obj, t = want
    assert_rows(got, k, what)
    assert (got["count"] == count).all(), "%s: count, first at ray %d" % (what, int(np.argmax(got["count"] != count)))
    assert (got["total"] == total).all(), "%s: total, first at ray %d" % (what, int(np.argmax(got["total"] != total)))
    assert (got["object"] == obj).all(), "%s: object, first at ray %d" % (what, int(np.argmax((got["object"] != obj).any(1))))
    assert as_bytes(got["t"]) == as_bytes(t), what + ": t"


# ---- accel None: the oracle's brute force on every ray ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "mixed_planes", "planes", "axis_aligned"])
def test_brute_force_equals_the_oracle(name, worlds):
    w = worlds[name]
    dev = w.devs["host"]
    n = N_MODEL
    sets, has = limit_sets(w, n)
    sets["no limit"] = None
    for what, t_max in sets.items():
        for k in KS:
            label = "%s, limits %s, k = %d" % (name, what, k)
            want = hr.brute_hits(w.tests, t_max, k)
            got = ask(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], k, t_max, want=("count", "object", "t", "total"))
            assert_is_brute(got, want, k, label)
            if what in ("zero", "NaN"):
                assert not got["count"].any() and not got["total"].any()
            if what == "t itself":  # strict: the nearest hit itself is out, and with it every hit
                assert not got["total"][has].any()
            if what == "the float above t":
                t_near = seg.nearest(w.tests)[0]
                assert (got["total"][has] >= 1).all() and as_bytes(got["t"][has, 0]) == as_bytes(t_near[has])
            if what == "the float below t":
                assert not got["total"][has].any()
            if what in ("inf", "no limit"):
                assert as_bytes(got["t"][has, 0]) == as_bytes(seg.nearest(w.tests)[0][has]) and (got["count"][~has] == 0).all()
        free, unlimited = ask(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], 5, None), ask(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], 5, sets["inf"])
    assert all(as_bytes(free[key]) == as_bytes(unlimited[key]) for key in ALL)
    assert (hr.brute_hits(w.tests, None, 0)[1] >= 2).any()  # hits behind the first one
    assert dev.status() == 0


# ---- the slats: full lists ----------------------------------------------------------------------------------------------------------

def test_slats_fill_the_list(worlds):
    w = worlds["slats"]
    dev = w.devs["device"]
    n = N_MODEL
    d_o, d_d = w.d_o[:n], w.d_d[:n]
    limits = hr.slat_limits(w.table(n), 22)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        for what, t_max in (("no limit", None), ("limits", limits)):
            label = "slats, accel %d, %s" % (accel, what)
            want = hr.brute_hits(w.tests, t_max, 16)
            full = ask(dev, accel, d_o, d_d, 16, t_max)
            assert_is_brute(full, want, 16, label)
            if t_max is None:
                assert (full["total"] == hr.N_SLATS).all() and (full["count"] == 16).all() and (full["object"] == np.arange(16)[None, :]).all()
            else:
                assert full["total"].min() < 16 < full["total"].max()
            for k in (1, 4):
                part = ask(dev, accel, d_o, d_d, k, t_max)
                assert_rows(part, k, label)
                assert (part["total"] == full["total"]).all() and (part["count"] == np.minimum(full["total"], k)).all(), label + ": k = %d" % k
                for key in ("object", "t", "hit_point", "normal"):
                    assert as_bytes(part[key]) == as_bytes(full[key][:, :k]), "%s: %s of k = %d is no prefix of k = 16" % (label, key, k)
            assert (ask(dev, accel, d_o, d_d, 0, t_max, want=("total",))["total"] == full["total"]).all(), label + ": k = 0"
            # without total a full list culls against its last entry: the same count, object and t
            for k in (1, 4, 16):
                lean = ask(dev, accel, d_o, d_d, k, t_max, want=ROWS)
                assert "total" not in lean
                assert_rows(lean, k, label)
                assert (lean["count"] == np.minimum(full["total"], k)).all(), label
                for key in ("object", "t", "hit_point", "normal"):
                    assert as_bytes(lean[key]) == as_bytes(full[key][:, :k]), "%s: %s without total, k = %d" % (label, key, k)
    assert dev.status() == 0


# ---- the BVH against the GPU's own brute force, which the tests above pin -----------------------------------------------------

def assert_bvh_is_brute(got, want, ok, what):
    for key in got:
        a, b = got[key], want[key]
        wrong = ok & (a.reshape(len(a), -1).view(np.uint32) != b.reshape(len(b), -1).view(np.uint32)).any(1)
        assert not wrong.any(), "%s: %s differs from the brute force on %d well-conditioned rays, first at ray %d" % (
            what, key, int(wrong.sum()), int(np.nonzero(wrong)[0][0]))


@pytest.mark.parametrize("name,tree", [("mixed", "host"), ("mixed", "device"), ("axis_aligned", "host"), ("slats", "device")])
def test_bvh_equals_the_brute_force(name, tree, worlds):
    w = worlds[name]
    dev = w.devs[tree]
    full = len(w.o)
    table = w.table(full)
    drawn = hr.slat_limits(table, 24) if name == "slats" else seg.draw_limits(w.objs, w.o, w.d, 19, table=table)
    for limits in (None, drawn):
        margin = hr.all_hits_margin(w.objs, w.o, w.d, limits, table)
        for n in BATCHES:
            t_max = None if limits is None else limits[:n]
            for want_names in (ALL, ROWS):
                for k in KS:
                    what = "%s, %s tree, %d rays, k = %d, %s, %s total" % (name, tree, n, k, "no limit" if limits is None else "limits",
                                                                            "with" if "total" in want_names else "without")
                    got = ask(dev, p3d.ACCEL_BVH, w.d_o[:n], w.d_d[:n], k, t_max, want=want_names)
                    want = ask(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], k, t_max, want=want_names)
                    assert_rows(got, k, what)
                    if n == 1:
                        assert all(as_bytes(got[key]) == as_bytes(want[key]) for key in got) or margin[0] < ref.THRESHOLD, what
                        continue
                    ok, left = ref.well_conditioned(margin[:n], what)
                    assert_bvh_is_brute(got, want, ok, what)
                    if n >= 63 and name != "slats":  # (every ray crosses the slats)
                        assert (want["count"][ok] == 0).any() and (want["count"][ok] > 0).any(), what + ": the rays all hit or all miss"
        assert (ask(dev, p3d.ACCEL_NONE, w.d_o, w.d_d, 0, limits, want=("total",))["total"] >= 2).any()
    assert dev.status() == 0


def test_through_a_deep_device_tree(mesh):
    """A few thousand triangles: the traversal spills past its LDS window; the brute-force side is the GPU's own, held to the model"""
    w, dev = mesh, mesh.devs["device"]
    n = len(w.o)
    table = w.table(n)
    for limits in (None, seg.draw_limits(w.objs, w.o, w.d, 20, table=table)):
        ok, left = ref.well_conditioned(hr.all_hits_margin(w.objs, w.o, w.d, limits, table), "tri5k through-rays")
        for want_names in (ALL, ROWS):
            got = ask(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, 2, limits, want=want_names)
            want = ask(dev, p3d.ACCEL_NONE, w.d_o, w.d_d, 2, limits, want=want_names)
            assert_rows(got, 2, "tri5k, k = 2")
            assert_bvh_is_brute(got, want, ok, "tri5k, device tree, k = 2, %s total" % ("with" if "total" in want_names else "without"))
        got = ask(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, 0, limits, want=("total",))
        want = ask(dev, p3d.ACCEL_NONE, w.d_o, w.d_d, 0, limits, want=("total",))
        assert_bvh_is_brute(got, want, ok, "tri5k, device tree, k = 0")
        m_total = hr.model_hits(table, limits, 0)[0]
        assert (want["total"][ok] == m_total[ok]).all(), "tri5k: the brute force's total against the model's"
        assert (m_total[ok] == 0).any() and (m_total[ok] >= 3).any()
        print("tri5k: %d rays, %d left out, up to %d hits" % (n, left, int(m_total.max())))
    assert dev.status() == 0


# ---- the two segment traversals against each other ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "mesh"])
def test_some_hit_is_a_total_above_zero(name, worlds, mesh):
    """occluded of the segment any-hit = (total of the hit list > 0), on EVERY ray: both run the same per-object test on fresh
    copies of the ray, and with total wanted the hit list culls with the same box test against the same limit, so it reaches
    every leaf the any-hit reaches before it stops.  Always with a t_max tensor: without one the any-hit is the feeler"""
    w = mesh if name == "mesh" else worlds[name]
    dev = w.devs["device"]
    first = dev.trace_closest_device(p3d.ACCEL_NONE, w.d_o[:N_MESH], w.d_d[:N_MESH], want=("t",))["t"].cpu().numpy()
    with np.errstate(over="ignore"):  # (a miss: FLT_MAX, twice that: inf)
        scaled = {by: np.where(first > 0, first * np.float32(by), INF).astype(np.float32) for by in (0.5, 2)}
    sets = {"inf": np.full(N_MESH, INF, np.float32), "half the first hit": scaled[0.5], "twice the first hit": scaled[2]}
    assert all(((t_max > 0) & ~np.isnan(t_max)).all() for t_max in sets.values())
    for what, t_max in sets.items():
        for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
            for n in (1, 65, N_MESH):
                d_t = gpu(t_max[:n])
                occluded = dev.trace_any_device(accel, w.d_o[:n], w.d_d[:n], t_max=d_t)["occluded"].cpu().numpy()
                total = ask(dev, accel, w.d_o[:n], w.d_d[:n], 0, d_t, want=("total",))["total"]
                differ = (occluded != 0) != (total > 0)
                assert not differ.any(), "%s, accel %d, %d rays, limits %s: %d rays differ, first at ray %d" % (
                    name, accel, n, what, int(differ.sum()), int(np.argmax(differ)))
                if n == N_MESH and what != "half the first hit":
                    assert occluded.any() and not occluded.all(), "%s, limits %s: the rays all hit or all miss" % (name, what)
    assert dev.status() == 0


# ---- hit_point and normal ---------------------------------------------------------------------------------------------------------

def test_hit_points_and_normals(worlds):
    w = worlds["mixed"]
    dev = w.devs["host"]
    n, k = N_MODEL, 5
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        got = ask(dev, accel, w.d_o[:n], w.d_d[:n], k)
        assert_rows(got, k, "mixed, accel %d" % accel)
        obj, hp, nrm = got["object"], got["hit_point"], got["normal"]
        assert (obj[:, 1:] >= 0).any() and (obj[:, 0] < 0).any()  # hits behind the first one, and rays that hit nothing
        for j in np.unique(obj[obj >= 0]):
            m = obj == j
            assert as_bytes(nrm[m]) == as_bytes(dev.object_normal(int(j), hp[m])), "accel %d: the normal of object %d" % (accel, j)
    # a lone object on a triangle-only scene reports the closest-hit query's bits: the slats under a limit behind the first one
    s = worlds["slats"]
    sdev = s.devs["device"]
    table = s.table(n)
    ts = np.sort(np.where(table[0], table[1], np.inf), axis=0)
    limit = ((ts[0] + ts[1]) / 2).astype(np.float32)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        got = ask(sdev, accel, s.d_o[:n], s.d_d[:n], 3, limit)
        one = {key: v.cpu().numpy() for key, v in sdev.trace_closest_device(accel, s.d_o[:n], s.d_d[:n], t_max=gpu(limit), want=CLOSEST_ALL).items()}
        assert (got["total"] == 1).all() and (got["count"] == 1).all() and (one["hit_id"] == 0).all()
        assert (got["object"][:, 0] == one["hit_id"]).all() and as_bytes(got["t"][:, 0]) == as_bytes(one["t"])
        assert as_bytes(got["hit_point"][:, 0]) == as_bytes(one["hit_point"]) and as_bytes(got["normal"][:, 0]) == as_bytes(one["normal"])


# ---- inside or outside: the parity of the crossings of a closed mesh -----------------------------------------------------------

def test_parity_tells_inside_from_outside(cube):
    w, dev = cube, cube.devs["device"]
    ok, left = ref.well_conditioned(hr.all_hits_margin(w.objs, w.o, w.d, None, w.table(len(w.o))), "the cube's rays")
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        total = ask(dev, accel, w.d_o, w.d_d, 0, want=("total",))["total"]
        assert ((total[ok] & 1) == w.inside[ok]).all(), "accel %d" % accel
        assert (total[ok & w.inside] == 1).all() and np.isin(total[ok & ~w.inside], (0, 2)).all() and (total[ok & ~w.inside] == 2).any()
    assert w.inside[ok].sum() > 200 and (~w.inside)[ok].sum() > 200


# ---- on a side stream, behind an update ---------------------------------------------------------------------------------------------

def model_objects(a):
    """intersect_reference's objects from HostScene.arrays() (no planes)"""
    out = []
    for kind, v in zip(a["prim_type"], np.asarray(a["prim_v"], np.float64).reshape(-1, 9)):
        if kind == TRIANGLE:
            out.append(dict(kind=ref.TRIANGLE, p0=v[0:3], p1=v[3:6], p2=v[6:9]))
        elif kind == SPHERE:
            out.append(dict(kind=ref.SPHERE, c=v[:3], r=v[3]))
        else:
            assert kind == BOX
            out.append(dict(kind=ref.BOX, mn=v[:3], mx=v[3:6]))
    return out


def tree_is_brute_where_well_conditioned(got, brute, hs, w, n, limited, what):
    """device_query_contract's assert_tree: the tree's answers behind an update are the fresh scene's brute force on the rays the
    model of the moved geometry calls well-conditioned (the brute force itself is held to that scene on every ray, in every bit)"""
    objs = model_objects(hs.arrays())
    o, d = w.o[:n], w.d[:n]
    ok, left = ref.well_conditioned(hr.all_hits_margin(objs, o, d, w.host["d_t_max"][:n] if limited else None, ref._all(objs, o, d)), what)
    assert_bvh_is_brute(got, brute, ok, what)


FOUR_HITS = dq.trace_hits(4, assert_tree=tree_is_brute_where_well_conditioned)


def test_behind_a_refit_on_the_same_stream(worlds):
    n = 4099
    s = copy.copy(worlds["slats"])  # (the limits are this test's: the module's world stays as it is)
    s.host, s.dev = dict(s.host), dict(s.dev)
    s.attach(d_t_max=hr.slat_limits(s.table(n), 25))
    dq.check_behind_a_refit(FOUR_HITS, s, n, soup=lambda a: (a["prim_v"].reshape(-1, 3) + np.float32([0.3, -0.2, 0.11])).astype(np.float32), what="slats behind a refit")


def test_behind_a_pose_on_the_same_stream(worlds):
    dq.check_behind_a_pose(FOUR_HITS, worlds["mixed"], 4099, limits=(False,), what="mixed behind a pose")


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def hip_runtime():
    """The HIP runtime this process has loaded (the one torch and libp3d.so allocate through), for an allocation of an exact size"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime is loaded"
    hip = C.CDLL(paths[0])
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemGetAddressRange.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_void_p]
    return hip


def test_refusals_enqueue_nothing(worlds):
    w = worlds["mixed"]
    dev = w.devs["host"]
    lib = p3d.lib()
    n, k = 129, 2
    d_o, d_d = w.d_o[:n], w.d_d[:n]
    # what every device query refuses: host memory first, every input misaligned, in host memory and too short, the required
    # outputs too short, an unknown accel, a missing tree, the null pointers
    outs = dq.check_buffer_refusals(dq.trace_hits(k), dev, {"d_origin": d_o, "d_direction": d_d, "d_t_max": torch.full((n,), 3.0, device="cuda")}, n)
    ptr = lambda name: C.c_void_p(outs[name].data_ptr())
    host = np.zeros((n, k * 3), np.float32)
    big = dq.BIG
    huge = torch.empty((big, 3), device="cuda")  # (never read: every call it is given to is refused)
    raws = {name: (v.data_ptr(), n) for name, v in outs.items()}
    q = lambda accel, o=d_o, d=d_d, kk=k, **kw: dev.trace_hits_device(accel, o, d, kk, want=kw.pop("want", ALL), out=kw.pop("out", outs), **kw)
    far = (huge.data_ptr(), big)
    dq.assert_refused(
        [("the grid", UNSUPPORTED, "grid", lambda: q(p3d.ACCEL_GRID)),
         ("k = 17", INVALID, "k must be", lambda: q(p3d.ACCEL_NONE, kk=17, out=raws)),
         ("a misaligned total", INVALID, "aligned", lambda: q(p3d.ACCEL_BVH, out=dict(outs, total=(outs["total"].data_ptr() + 2, n)))),
         ("a host total, k = 0", INVALID, "d_total is host memory", lambda: q(p3d.ACCEL_BVH, kk=0, want=("total",), out={"total": (host.ctypes.data, n)})),
         ("a total too short", INVALID, "d_total ends behind its allocation",
          lambda: q(p3d.ACCEL_NONE, o=far, d=far, kk=0, want=("total",), out={name: (v.data_ptr(), big) for name, v in outs.items()}))] +
        [("a host " + name, INVALID, "d_%s is host memory" % name, lambda name=name: q(p3d.ACCEL_BVH, out=dict(outs, **{name: (host.ctypes.data, n)}))) for name in outs])
    # a buffer short by one element: an allocation of its own, straight from the runtime, which therefore knows where it ends
    # (torch hands out pieces of larger segments).  Every call is refused: none may be accepted with a buffer shorter than the
    # kernel would write, so the extent the runtime reports is asserted before the library sees the pointer
    hip = hip_runtime()
    head = (dev._h, p3d.ACCEL_NONE, n, k, C.c_void_p(d_o.data_ptr()), C.c_void_p(d_d.data_ptr()), None)
    names = ("count", "total", "object", "t", "hit_point", "normal")
    for name, elems in (("count", n), ("total", n), ("object", n * k), ("t", n * k), ("hit_point", n * k * 3), ("normal", n * k * 3)):
        nbytes = (elems - 1) * 4
        lean = C.c_void_p()
        assert hip.hipMalloc(C.byref(lean), C.c_size_t(nbytes)) == 0 and lean.value
        try:
            base, size = C.c_void_p(), C.c_size_t()
            assert hip.hipMemGetAddressRange(C.byref(base), C.byref(size), lean) == 0
            assert base.value == lean.value and size.value == nbytes, "the runtime reports %d bytes for an allocation of %d" % (size.value, nbytes)
            assert hip.hipMemset(lean, 5, C.c_size_t(nbytes)) == 0 and hip.hipDeviceSynchronize() == 0
            rc = lib.p3d_trace_hits_device(*head, *[lean if key == name else ptr(key) for key in names], None)
            assert rc == INVALID and ("d_%s ends behind its allocation" % name).encode() in lib.p3d_last_error(), "%s: %d, %s" % (name, rc, lib.p3d_last_error())
            back = np.zeros(nbytes, np.uint8)
            assert hip.hipDeviceSynchronize() == 0 and hip.hipMemcpy(C.c_void_p(back.ctypes.data), lean, C.c_size_t(nbytes), 2) == 0  # device to host
            assert (back == 5).all(), name + ": the short buffer was written"
        finally:
            assert hip.hipFree(lean) == 0
    del huge
    o_, d_ = C.c_void_p(d_o.data_ptr()), C.c_void_p(d_d.data_ptr())
    rows = (ptr("t"), ptr("hit_point"), ptr("normal"), None)
    call = lib.p3d_trace_hits_device
    assert call(dev._h, p3d.ACCEL_BVH, n, 17, o_, d_, None, ptr("count"), ptr("total"), ptr("object"), *rows) == INVALID and b"k must be" in lib.p3d_last_error()
    assert call(dev._h, p3d.ACCEL_BVH, n, 0, o_, d_, None, ptr("count"), None, ptr("object"), *rows) == INVALID  # k = 0 without total
    assert b"d_total is needed" in lib.p3d_last_error()
    assert call(dev._h, p3d.ACCEL_BVH, n, k, o_, d_, None, None, ptr("total"), ptr("object"), *rows) == INVALID  # a null d_count
    assert b"null argument" in lib.p3d_last_error()
    assert call(dev._h, p3d.ACCEL_NONE, n, k, o_, d_, None, ptr("count"), ptr("total"), None, *rows) == INVALID  # a null d_object
    assert b"null argument" in lib.p3d_last_error()
    assert call(dev._h, p3d.ACCEL_NONE, n, k, None, d_, None, ptr("count"), ptr("total"), ptr("object"), *rows) == INVALID
    assert call(dev._h, p3d.ACCEL_GRID, n, k, o_, d_, None, ptr("count"), ptr("total"), ptr("object"), *rows) == UNSUPPORTED
    # an empty batch is fine, whatever the pointers, once k is valid
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        assert call(dev._h, accel, 0, 3, *([None] * 10)) == 0 and call(dev._h, accel, 0, 0, *([None] * 10)) == 0
        assert call(dev._h, accel, 0, 17, *([None] * 10)) == INVALID
    torch.cuda.synchronize()
    assert all(bool((outs[name] == 77).all()) for name in ("count", "total", "object"))
    assert all(bool((outs[name] == 123.0).all()) for name in ("t", "hit_point", "normal"))
    # k = 0 takes the row pointers as they come - they are ignored - and the planes are there for the brute force and not refused
    # under the tree
    total = torch.full((n,), 77, dtype=torch.int32, device="cuda")
    assert call(dev._h, p3d.ACCEL_BVH, n, 0, o_, d_, None, None, C.c_void_p(total.data_ptr()), None, None, None, None, None) == 0
    assert call(dev._h, p3d.ACCEL_BVH, n, 0, o_, d_, None, C.c_void_p(host.ctypes.data), C.c_void_p(total.data_ptr()), C.c_void_p(1), None, None, None, None) == 0
    torch.cuda.synchronize()
    assert (total.cpu().numpy() == ask(dev, p3d.ACCEL_BVH, d_o, d_d, 1, want=("total",))["total"]).all()
    pw = worlds["planes"]
    with_planes = pw.devs["host"]
    none = ask(with_planes, p3d.ACCEL_NONE, pw.d_o[:n], pw.d_d[:n], 0, want=("total",))["total"]
    tree = ask(with_planes, p3d.ACCEL_BVH, pw.d_o[:n], pw.d_d[:n], 0, want=("total",))["total"]
    assert (none == hr.brute_hits((pw.tests[0][:, :n], pw.tests[1][:, :n]), None, 0)[1]).all() and (tree <= none).all()
    assert dev.status() == 0 and with_planes.status() == 0
