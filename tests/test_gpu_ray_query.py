"""Ray queries over device tensors (p3d_trace_closest_device, p3d_trace_any_device) on the GPU.

Without a limit the device forms must equal the host forms (p3d_trace_closest, p3d_trace_any) bit for bit, for the three back
ends, at every batch size, on uploaded and on device-built trees.  With t_max the closest hit is the unlimited one filtered by
t < t_max; the any-hit is the segment query, whose yardsticks are the exact brute force over the CPU oracle's per-object test
(accel None: every ray, no cap) and, for the BVH traversal, that brute force on the rays the float64 model of
segment_reference.py calls well-conditioned, under the 5 % cap of intersect_reference.py.

The library's debug hooks (csrc/p3d_debug.h) expose no scratch sizes, so "a second call of the same n allocates nothing" is
not tested here."""
import numpy as np
import pytest
import torch

import device_query_contract as dq
from device_query_contract import ANY, CLOSEST, FLT_MAX, UNSUPPORTED
from frame_checks import ACCELS, gpu, same_bits_or_nan
import intersect_reference as ref
from oracle import binding as ob
import p3d_amd as p3d
from ray_query_checks import BATCHES, CLOSEST_ALL, INF, N_MESH, N_MODEL, World, limit_sets
import segment_reference as seg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_query")
    paths = ref.scene_paths(tmp)
    return {name: World(path, ("host", "device") if name == "mixed" else ("host",)) for name, path in paths.items()}


@pytest.fixture(scope="module")
def mesh(tri5k_path):
    """A few thousand triangles under a tree built on the device, deeper than the 16-entry LDS window of the stack"""
    w = World(tri5k_path, ("device",), seed=9, n=N_MESH, oracle=False)
    assert w.devs["device"].export_bvh()["bvh_max_depth"] > 16
    return w


def scenes_of(worlds, mesh):
    """(label, world, device scene, accels whose answers mean something bit for bit: all of them)"""
    out = [("%s, %s tree" % (name, tree), w, dev) for name, w in worlds.items() for tree, dev in w.devs.items()]
    return out + [("tri5k, device tree", mesh, mesh.devs["device"])]


# ---- without a limit: the host forms, bit for bit ---------------------------------------------------------------------------------

def assert_normals(dev, hit, hp, nrm, what, most=24):
    miss = hit < 0
    assert not nrm[miss].any() and not np.signbit(nrm[miss]).any(), what + ": a normal on a miss"
    for obj in np.unique(hit[~miss])[:most]:
        m = hit == obj
        assert same_bits_or_nan(nrm[m], dev.object_normal(int(obj), hp[m])).all(), "%s: the normal of object %d" % (what, obj)


@pytest.mark.parametrize("n", BATCHES)
def test_device_forms_equal_the_host_forms(n, worlds, mesh):
    for label, w, dev in scenes_of(worlds, mesh):
        n_here = min(n, len(w.o))
        o, d = w.o[:n_here], w.d[:n_here]
        d_o, d_d = w.d_o[:n_here], w.d_d[:n_here]
        for accel_name, accel in ACCELS.items():
            what = "%s over %s, %d rays" % (label, accel_name, n_here)
            hit, hp, t = dev.trace_closest(accel, o, d, want_t=True)
            got = {k: v.cpu().numpy() for k, v in dev.trace_closest_device(accel, d_o, d_d, want=CLOSEST_ALL).items()}
            assert (got["hit_id"] == hit).all(), what + ": hit_id"
            assert same_bits_or_nan(got["t"], t).all(), what + ": t"
            assert same_bits_or_nan(got["hit_point"], hp).all(), what + ": hit_point"
            assert (got["t"][hit < 0] == FLT_MAX).all() and not got["hit_point"][hit < 0].any(), what + ": the miss values"
            assert_normals(dev, hit, hp, got["normal"], what)
            occ = dev.trace_any_device(accel, d_o, d_d)["occluded"].cpu().numpy()
            assert occ.dtype == np.uint8 and (occ == dev.trace_any(accel, o, d)).all(), what + ": occluded"
            if n_here >= 63 and not any(m["kind"] == ref.PLANE for m in w.objs):
                assert 0 < (hit >= 0).sum() < n_here and 0 < occ.sum() < n_here, what + ": hits and misses in one batch"
            dq.check_callers_outputs(CLOSEST, dev, accel, {"d_origin": d_o, "d_direction": d_d}, {"hit_id": hit}, what)


# ---- closest hit with a limit -------------------------------------------------------------------------------------------------

def limits_around(t, seed):
    """Per ray one of: t itself (a miss: strict), its upper neighbour (a hit), 0, inf, NaN, half, double"""
    rng = np.random.default_rng(seed)
    t = np.asarray(t, np.float32)
    with np.errstate(over="ignore"):
        choices = np.stack([t, np.nextafter(t, INF), np.zeros_like(t), np.full_like(t, INF), np.full_like(t, np.nan),
                            (t * np.float32(0.5)).astype(np.float32), (t * np.float32(2)).astype(np.float32)])
    pick = rng.integers(0, len(choices), len(t))
    return choices[pick, np.arange(len(t))], pick


@pytest.mark.parametrize("accel_name", list(ACCELS))
def test_closest_hit_with_a_limit(accel_name, worlds, mesh):
    accel = ACCELS[accel_name]
    for label, w, dev in scenes_of(worlds, mesh):
        what = "%s over %s" % (label, accel_name)
        free = {k: v.cpu().numpy() for k, v in dev.trace_closest_device(accel, w.d_o, w.d_d, want=CLOSEST_ALL).items()}
        t_max, pick = limits_around(free["t"], 31)
        got = {k: v.cpu().numpy() for k, v in dev.trace_closest_device(accel, w.d_o, w.d_d, t_max=gpu(t_max), want=CLOSEST_ALL).items()}
        with np.errstate(invalid="ignore"):
            keep = (free["hit_id"] >= 0) & (free["t"] < t_max)
        hits = free["hit_id"] >= 0
        assert not keep[hits & (pick == 0)].any() and keep[hits & (pick == 1)].all() and not keep[np.isin(pick, (2, 4))].any()
        assert keep[hits & (pick == 3)].all() and (0 < keep.sum() < hits.sum() or not hits.any()), what
        assert (got["hit_id"] == np.where(keep, free["hit_id"], -1)).all(), what + ": hit_id"
        assert same_bits_or_nan(got["t"], np.where(keep, free["t"], FLT_MAX)).all(), what + ": t"
        for k in ("hit_point", "normal"):
            assert same_bits_or_nan(got[k], np.where(keep[:, None], free[k], np.float32(0))).all(), "%s: %s" % (what, k)


# ---- the segment query, accel None: the oracle's brute force on every ray ---------------------------------------------------------

def segment(dev, accel, d_o, d_d, t_max):
    return dev.trace_any_device(accel, d_o, d_d, t_max=gpu(np.asarray(t_max, np.float32)))["occluded"].cpu().numpy().astype(bool)


@pytest.mark.parametrize("name", ["mixed", "mixed_planes", "planes", "axis_aligned"])
def test_segment_any_hit_by_brute_force_equals_the_oracle(name, worlds):
    w = worlds[name]
    dev = w.devs["host"]
    n = N_MODEL
    sets, has = limit_sets(w, n)
    for what, t_max in sets.items():
        want = seg.brute_force(w.tests, t_max)
        got = segment(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], t_max)
        assert (got == want).all(), "%s, limits %s: %d rays differ from the oracle's brute force, first at ray %d" % (
            name, what, int((got != want).sum()), int(np.nonzero(got != want)[0][0]))
        if what in ("zero", "NaN"):
            assert not got.any()
        if what == "the float above t":
            assert got[has].all()  # the nearest hit itself lies in front of it
        if what == "draws":
            assert 0 < got.sum() < n
    # without a limit it is the feeler: where no sphere re-normalises the ray under way, the unlimited segment query's answer
    assert (seg.brute_force(w.tests, np.full(n, INF)) == (w.tests[0] & ~np.isnan(w.tests[1])).any(0)).all()


def test_segment_any_hit_on_the_exact_cases(tmp_path):
    """EDGES: hits whose float32 arithmetic is exact, turned into limits either side of their t"""
    path = tmp_path / "edges.p3f"
    path.write_text(ref.EDGES)
    hs, sc = p3d.HostScene(str(path)), ob.Scene(str(path))
    dev = p3d.DeviceScene(hs, bvh=True, grid=True)
    cases = [c for c in ref.EXACT_RAYS if c[3]]
    o = np.array([c[1] for c in cases], np.float32)
    d = np.array([c[2] for c in cases], np.float32)
    t = np.array([c[4] for c in cases], np.float32)
    tests = seg.per_object(sc.object_intercepts, len(ref.load_objects(str(path))), o, d)
    for k, c in enumerate(cases):
        assert tests[0][c[0], k] and tests[1][c[0], k] == t[k]  # (a hit at t = 0 may be -0.0)
    same, up, down = seg.tie_limits(t)
    for what, t_max in (("t itself", same), ("the float above t", up), ("the float below t", down)):
        got = segment(dev, p3d.ACCEL_NONE, gpu(o), gpu(d), t_max)
        assert (got == seg.brute_force(tests, t_max)).all(), "EDGES, limits %s" % what
        if what == "the float above t":
            assert got.all()
    # the listed object alone decides wherever no other object of the scene lies in front of it
    alone = (tests[0] & (tests[1] < t[None, :])).sum(0) == 0
    assert alone.any() and not segment(dev, p3d.ACCEL_NONE, gpu(o), gpu(d), same)[alone].any()


# ---- the segment query through the BVH --------------------------------------------------------------------------------------------

def assert_bvh_segment(w, table, t_max, got, want, what):
    """got == want on the rays the model calls well-conditioned (5 % cap), both occluded and free among them -> left out"""
    n = len(got)
    _, margin = seg.occluded_within(w.objs, w.o[:n], w.d[:n], t_max, table=table)
    ok, left = ref.well_conditioned(margin, what)
    wrong = ok & (got != want)
    print("%s: %d rays, %d occluded, %d left out by the model, %d of those differ" % (what, n, int(want.sum()), left, int((~ok & (got != want)).sum())))
    assert not wrong.any(), "%s: %d well-conditioned rays differ from the brute force, first at ray %d (margin %g)" % (
        what, int(wrong.sum()), int(np.nonzero(wrong)[0][0]), float(margin[wrong][0]))
    if n >= 63:
        assert 0 < want[ok].sum() < ok.sum(), what + ": the rays are all occluded or all free"
    return left


@pytest.mark.parametrize("name,tree", [("mixed", "host"), ("mixed", "device"), ("axis_aligned", "host")])
def test_segment_any_hit_through_the_bvh(name, tree, worlds):
    w = worlds[name]
    dev = w.devs[tree]
    # the oracle's brute force, on the CPU suite's rays and limits
    n = N_MODEL
    t_max = seg.draw_limits(w.objs, w.o[:n], w.d[:n], 18, table=w.table(n))
    got = segment(dev, p3d.ACCEL_BVH, w.d_o[:n], w.d_d[:n], t_max)
    assert_bvh_segment(w, w.table(n), t_max, got, seg.brute_force(w.tests, t_max), "segment any-hit %s, %s tree, %d rays" % (name, tree, n))
    # every batch size, against the GPU's own brute force, which the test above pins
    full = len(w.o)
    t_all = seg.draw_limits(w.objs, w.o, w.d, 19, table=w.table(full))
    for n in BATCHES:
        got = segment(dev, p3d.ACCEL_BVH, w.d_o[:n], w.d_d[:n], t_all[:n])
        want = segment(dev, p3d.ACCEL_NONE, w.d_o[:n], w.d_d[:n], t_all[:n])
        if n == 1:
            assert (got == want).all() or seg.occluded_within(w.objs, w.o[:1], w.d[:1], t_all[:1], table=w.table(1))[1][0] < ref.THRESHOLD
            continue
        assert_bvh_segment(w, w.table(n), t_all[:n], got, want, "segment any-hit %s, %s tree, %d rays" % (name, tree, n))


def test_segment_any_hit_through_a_deep_device_tree(mesh):
    """A few thousand triangles: the traversal spills past its LDS window; the brute-force side is the GPU's own"""
    w, dev = mesh, mesh.devs["device"]
    n = len(w.o)
    t_max = seg.draw_limits(w.objs, w.o, w.d, 20, table=w.table(n))
    got = segment(dev, p3d.ACCEL_BVH, w.d_o, w.d_d, t_max)
    want = segment(dev, p3d.ACCEL_NONE, w.d_o, w.d_d, t_max)
    assert_bvh_segment(w, w.table(n), t_max, got, want, "segment any-hit tri5k, device tree, %d rays" % n)
    # ... and that brute force is the model's on its well-conditioned rays
    seg.check_segment(w.objs, w.o, w.d, t_max, want, "segment any-hit tri5k, accel none, %d rays" % n)


# ---- what it is for ---------------------------------------------------------------------------------------------------------------

def test_an_occluder_behind_the_target_does_not_shadow_it(tmp_path):
    """A at the origin looks at B = (0, 0, -5); a sphere stands behind B.  The feeler, which has no limit, calls A shadowed."""
    path = tmp_path / "behind.p3f"
    path.write_text(ref.HEAD + "s 0 0 -10 1\ns 50 0 0 1\ns -50 3 0 1\n")
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh=True, grid=True)
    a, b = np.zeros((1, 3), np.float32), np.array([[0, 0, -5]], np.float32)
    d = ref.normalize32(b - a)
    dist = np.linalg.norm(b - a, axis=1).astype(np.float32)
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        assert dev.trace_any(accel, a, d).tolist() == [1]
        assert dev.trace_any_device(accel, gpu(a), gpu(d))["occluded"].cpu().tolist() == [1]
        assert segment(dev, accel, gpu(a), gpu(d), dist).tolist() == [False]
        assert segment(dev, accel, gpu(a), gpu(d), dist + 5).tolist() == [True]  # ... and B would not see (0, 0, -10)


def test_a_query_on_a_side_stream_and_after_an_update(tmp_path):
    """Rays produced on a side stream, the query behind them on that stream, the result read after stream.synchronize() only;
    then update_triangles moves the occluder away and the same query reports free."""
    tris = np.array([[[-1, -1, -5], [1, -1, -5], [0, 1, -5]], [[9, 9, -5], [10, 9, -5], [9, 10, -5]], [[-9, 9, -4], [-10, 9, -4], [-9, 10, -4]]], np.float32)
    path = tmp_path / "wall.p3f"
    path.write_text(ref.HEAD + "".join("p 3\n" + "".join("%g %g %g\n" % tuple(v) for v in t) for t in tris))
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh="device")
    n = 4099
    base = gpu(np.random.default_rng(5).uniform(-0.2, 0.2, (n, 3)).astype(np.float32))
    aim = gpu(np.array([[0, 0, -1]], np.float32)).expand(n, 3)
    limit = torch.full((n,), 10.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()

    def ask():
        with torch.cuda.stream(side):
            wave = base
            for _ in range(200):  # some work in front of the rays, so that they are still being produced when the call begins
                wave = torch.sin(wave * 1.5 + 0.25)
            o = (base + 0.01 * wave).contiguous()
            d = (aim + 0.0 * wave).contiguous()
            res = {accel: dev.trace_any_device(accel, o, d, t_max=limit, stream=side)["occluded"] for accel in (p3d.ACCEL_BVH, p3d.ACCEL_NONE)}
            hit = dev.trace_closest_device(p3d.ACCEL_BVH, o, d, t_max=limit, stream=side)["hit_id"]
        side.synchronize()
        return res, hit

    res, hit = ask()
    assert all(bool(r.all()) for r in res.values()) and bool((hit == 0).all())
    away = gpu((tris[0] + np.float32([0, 40, 0])).reshape(3, 3))
    dev.update_triangles(0, away)
    res, hit = ask()
    assert not any(bool(r.any()) for r in res.values()) and bool((hit == -1).all())
    assert dev.status() == 0


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals_enqueue_nothing(worlds):
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    inputs = dict(CLOSEST.inputs_of(w, n), d_t_max=torch.full((n,), 3.0, dtype=torch.float32, device="cuda"))
    outs = [dq.check_buffer_refusals(query, dev, inputs, n) for query in (CLOSEST, ANY)]
    dq.assert_refused([("the grid with a limit", UNSUPPORTED, "grid", lambda: ANY.call(dev, p3d.ACCEL_GRID, inputs, (), 0, outs[1]))])
    for query, out in zip((CLOSEST, ANY), outs):
        dq.check_empty_batch(query, dev)
        dq.assert_untouched(out)
