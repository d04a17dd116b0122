"""The filtered ray queries over device tensors (p3d_trace_any_filtered_device, p3d_trace_hits_filtered_device,
p3d_occlusion_filtered_device) on the GPU.  Every comparison has tolerance 0.

The yardstick is ray_filter_reference.py: the per-object (hit, t) tables of the unfiltered scene with the entries the filters
name set to "no hit", handed to the brute forces of hits_reference / segment_reference.  Under ACCEL_NONE every ray equals it;
the BVH equals ACCEL_NONE on every ray whose margin in the thinned float64 table is above intersect_reference.THRESHOLD, under
the 5 % cap the unfiltered tests of these scenes have (intersect_reference.well_conditioned asserts it; the CPU suite shows
with the model alone that these rays and filters stay within it).  A second statement: the unfiltered call over a scene from
which a range is taken out, indices mapped back.  Planes: the unfiltered segment family does not refuse a plane under the tree
(the BVH loses it, Q12), so neither do the filtered forms; the scene with planes goes through ACCEL_NONE, and the tree's
answer is checked to be what the unfiltered tree call does: accepted, with no more hits than the brute force."""
import copy
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import SCENES as GOLDEN_SCENES
import device_query_contract as dq
from device_query_contract import BATCHES, BVH, INVALID, NONE, UNSUPPORTED
from frame_checks import as_bytes, gpu
import filter_reference as fr
import hits_reference as hr
import intersect_reference as ref
import occlusion_checks as oc
import p3d_amd as p3d
from ray_query_checks import N_MESH, N_MODEL, World
import ray_filter_reference as rf
from scene_update_helpers import BOX, SPHERE, TRIANGLE
import segment_reference as seg

pytestmark = pytest.mark.gpu

KS = (0, 1, 4, 16)
ROWS = ("count", "object", "t", "hit_point", "normal")
ALL = ROWS + ("total",)
INF = np.float32(np.inf)
FILTERS = [(n_skip, ranged) for n_skip in fr.N_SKIPS for ranged in (False, True)]
SAMPLES = 16


def dev_filter(skip, skip_range):
    return dict(skip=None if skip is None else gpu(skip), skip_range=None if skip_range is None else gpu(skip_range))


def limits_of(t_max):
    return gpu(np.asarray(t_max, np.float32)) if isinstance(t_max, np.ndarray) else t_max


def hits(dev, accel, d_o, d_d, k, t_max=None, skip=None, skip_range=None, want=ALL, **kw):
    want = tuple(w for w in want if k or w == "total")
    res = p3d.trace_hits_filtered_device(dev, accel, d_o, d_d, k, t_max=limits_of(t_max), want=want, **dev_filter(skip, skip_range), **kw)
    return {name: v.cpu().numpy() for name, v in res.items()}


def plain_hits(dev, accel, d_o, d_d, k, t_max=None, want=ALL):
    want = tuple(w for w in want if k or w == "total")
    return {name: v.cpu().numpy() for name, v in dev.trace_hits_device(accel, d_o, d_d, k, t_max=limits_of(t_max), want=want).items()}


def occluded(dev, accel, d_o, d_d, t_max=None, skip=None, skip_range=None, **kw):
    return p3d.trace_any_filtered_device(dev, accel, d_o, d_d, t_max=limits_of(t_max), **dev_filter(skip, skip_range), **kw)["occluded"].cpu().numpy()


def plain_occluded(dev, accel, d_o, d_d, t_max):
    return dev.trace_any_device(accel, d_o, d_d, t_max=limits_of(t_max))["occluded"].cpu().numpy()


def inf_limits(n):
    return np.full(n, INF, np.float32)


def same(a, b, what):
    dq.assert_same_bits(a, b, what)


def assert_hits_are_brute(got, want, k, what):
    count, total, obj, t = want
    assert (got["total"] == total).all(), "%s: total, first at ray %d" % (what, int(np.argmax(got["total"] != total)))
    if k:
        assert (got["count"] == count).all(), "%s: count, first at ray %d" % (what, int(np.argmax(got["count"] != count)))
        assert (got["object"] == obj).all(), "%s: object, first at ray %d" % (what, int(np.argmax((got["object"] != obj).any(1))))
        assert as_bytes(got["t"]) == as_bytes(t), what + ": t"


def assert_same_where(got, want, ok, what):
    for key in got:
        a, b = np.ascontiguousarray(got[key]), np.ascontiguousarray(want[key])
        wrong = ok & (a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(1)
        assert not wrong.any(), "%s: %s differs from the brute force on %d well-conditioned rays, first at ray %d" % (
            what, key, int(wrong.sum()), int(np.nonzero(wrong)[0][0]))


class RayWorld(World):
    """World with rays of the caller's"""

    def __init__(self, path, trees, o, d, oracle=False):
        super().__init__(path, trees, n=8, oracle=oracle)
        self.set_rays(o, d)


def device_tests(dev, n_objs, o, d):
    """segment_reference.per_object's (hit, t) tables from p3d_object_intercepts: every object on fresh copies of all rays"""
    hit, t = np.zeros((n_objs, len(o)), bool), np.zeros((n_objs, len(o)), np.float32)
    for j in range(n_objs):
        hit[j], t[j], _ = dev.object_intercepts(j, o, d)
    return hit, t


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_filters")
    paths = ref.scene_paths(tmp)
    w = {name: World(paths[name], ("host", "device") if name == "mixed" else ("host",)) for name in rf.SEED}
    for name, world in w.items():
        world.case = rf.Case(paths[name], rf.SEED[name], objs=world.objs, rays=(world.o, world.d))
        o, d = rf.scene_rays(world.objs)
        assert as_bytes(o) == as_bytes(world.o) and as_bytes(d) == as_bytes(world.d), name + ": the CPU suite speaks of other rays"
    w["tmp"] = tmp
    return w


@pytest.fixture(scope="module")
def slats(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ray_filters_slats")
    w = RayWorld(hr.write_slats(tmp / "slats.p3f"), ("device",), *hr.slat_rays(21, max(BATCHES)))
    w.tmp = tmp
    return w


# ---- 1. accel None: the masked brute force on every ray ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rf.SEED))
def test_brute_force_equals_the_masked_oracle(name, worlds):
    w = worlds[name]
    dev, c, n = w.devs["host"], w.case, N_MODEL
    d_o, d_d = w.d_o[:n], w.d_d[:n]
    changed = 0
    for n_skip, ranged in FILTERS:
        skip, skip_range = rf.draw(c, n_skip, ranged, n)
        tests = rf.mask_tests(w.tests, skip, skip_range)
        for t_max in (None, c.limits[:n]):
            for k in KS:
                what = "%s, n_skip = %d%s, k = %d%s" % (name, n_skip, ", a range" if ranged else "", k, ", limits" if t_max is not None else "")
                got = hits(dev, NONE, d_o, d_d, k, t_max, skip, skip_range, want=("count", "object", "t", "total"))
                assert_hits_are_brute(got, hr.brute_hits(tests, t_max, k), k, what)
                if k == 1:
                    changed += int((got["object"] != plain_hits(dev, NONE, d_o, d_d, 1, t_max)["object"]).sum()) if n_skip or ranged else 0
            lim = inf_limits(n) if t_max is None else t_max
            got = occluded(dev, NONE, d_o, d_d, lim, skip, skip_range)
            assert (got.astype(bool) == seg.brute_force(tests, lim)).all(), "%s: the any-hit" % what
    assert changed > n, name + ": the filters changed hardly an answer"
    if name == "mixed_planes":  # planes under the tree: accepted as the unfiltered calls accept them, and the tree finds no more than the loop
        skip, skip_range = rf.draw(c, 8, True, n)
        tree = hits(dev, BVH, d_o, d_d, 0, None, skip, skip_range, want=("total",))["total"]
        loop = hits(dev, NONE, d_o, d_d, 0, None, skip, skip_range, want=("total",))["total"]
        lost = plain_hits(dev, BVH, d_o, d_d, 0, want=("total",))["total"] < plain_hits(dev, NONE, d_o, d_d, 0, want=("total",))["total"]
        assert lost.any(), "the unfiltered tree call is accepted and loses the planes: what the filtered one has to do as well"
        assert (tree <= loop).all() and (tree < loop).any()
    assert dev.status() == 0


# ---- 2. the BVH against the brute force, which the test above pins --------------------------------------------------------------------

@pytest.mark.parametrize("name,tree", [("mixed", "host"), ("mixed", "device"), ("axis_aligned", "host")])
def test_bvh_equals_the_brute_force(name, tree, worlds):
    w = worlds[name]
    dev, c = w.devs[tree], w.case
    for n_skip, ranged in FILTERS:
        skip, skip_range = rf.draw(c, n_skip, ranged)
        masked = rf.mask_table(c.table, skip, skip_range)
        for limits in (None, c.limits):
            label = "%s, %s tree, n_skip = %d%s, %s" % (name, tree, n_skip, ", a range" if ranged else "", "no limit" if limits is None else "limits")
            margin = rf.hits_margin(c.objs, c.o, c.d, limits, masked)
            any_limits = inf_limits(c.n) if limits is None else limits
            any_margin = rf.model_occluded(c.objs, c.o, c.d, any_limits, masked)[1]
            for n in BATCHES:
                f = (None if skip is None else skip[:n], None if skip_range is None else skip_range[:n])
                t_max = None if limits is None else limits[:n]
                if n == 1:
                    ok, any_ok = margin[:1] >= ref.THRESHOLD, any_margin[:1] >= ref.THRESHOLD
                else:
                    ok, left = ref.well_conditioned(margin[:n], label)  # (asserts the cap on the share left out)
                    any_ok, any_left = ref.well_conditioned(any_margin[:n], label + ", the any-hit")
                    if n == max(BATCHES):
                        print("%s: %d of %d rays left out of the hit lists, %d of the any-hit (cap %g)" % (label, left, n, any_left, ref.MAX_LEFT_OUT))
                for k in KS:
                    for want_names in ((ALL, ROWS) if k in (1, 16) else (ALL,)):
                        what = "%s, %d rays, k = %d, %s total" % (label, n, k, "with" if "total" in want_names else "without")
                        got = hits(dev, BVH, w.d_o[:n], w.d_d[:n], k, t_max, *f, want=want_names)
                        want = hits(dev, NONE, w.d_o[:n], w.d_d[:n], k, t_max, *f, want=want_names)
                        assert_same_where(got, want, ok, what)
                a = occluded(dev, BVH, w.d_o[:n], w.d_d[:n], any_limits[:n], *f)
                b = occluded(dev, NONE, w.d_o[:n], w.d_d[:n], any_limits[:n], *f)
                assert not (any_ok & (a != b)).any(), label + ", %d rays: the any-hit" % n
    assert dev.status() == 0


def test_through_a_deep_device_tree(tri5k_path):
    """A few thousand triangles under a device-built tree: the traversal spills past its LDS window with a filter in registers"""
    objs = ref.load_objects(tri5k_path)
    rng = np.random.default_rng(9)
    pts = np.concatenate([np.stack([ob["p0"], ob["p1"], ob["p2"]]) for ob in objs])
    centre, r = (pts.min(0) + pts.max(0)) / 2, np.linalg.norm(pts.max(0) - pts.min(0)) / 2
    o = (centre + 1.5 * r * ref._unit(rng, N_MESH)).astype(np.float32)
    d = ref.normalize32((centre + 0.5 * r * ref._in_ball(rng, N_MESH)).astype(np.float32) - o)
    w = RayWorld(tri5k_path, ("device",), o, d)
    dev = w.devs["device"]
    dq.assert_deep(dev)
    c = rf.Case(tri5k_path, 640, objs=objs, rays=(w.o, w.d))
    for n_skip, ranged in ((8, False), (1, True)):
        skip, skip_range = rf.draw(c, n_skip, ranged)
        masked = rf.mask_table(c.table, skip, skip_range)
        for limits in (None, c.limits):
            what = "tri5k, n_skip = %d%s%s" % (n_skip, ", a range" if ranged else "", "" if limits is None else ", limits")
            ok, left = ref.well_conditioned(rf.hits_margin(c.objs, c.o, c.d, limits, masked), what)
            for k, want_names in ((2, ALL), (2, ROWS), (0, ("total",))):
                got, want = (hits(dev, accel, w.d_o, w.d_d, k, limits, skip, skip_range, want=want_names) for accel in (BVH, NONE))
                assert_same_where(got, want, ok, what + ", k = %d" % k)
            m_total = hr.model_hits(masked, limits, 0)[0]
            assert (want["total"][ok] == m_total[ok]).all(), what + ": the brute force's total against the thinned model's"
            assert (m_total != hr.model_hits(c.table, limits, 0)[0]).any(), what + ": the filters changed no total"
            any_limits = inf_limits(c.n) if limits is None else limits
            any_ok, _ = ref.well_conditioned(rf.model_occluded(c.objs, c.o, c.d, any_limits, masked)[1], what + ", the any-hit")
            a, b = (occluded(dev, accel, w.d_o, w.d_d, any_limits, skip, skip_range) for accel in (BVH, NONE))
            assert not (any_ok & (a != b)).any() and ((b != 0) == (want["total"] > 0)).all(), what + ": the any-hit"
    assert dev.status() == 0


GOLDEN = "balls_low.p3f"  # ten spheres and two triangles


def test_a_golden_scene_of_spheres_and_triangles():
    """The fixture the smoke run renders: the masked brute force over p3d_object_intercepts on every ray, and the trees against it"""
    w = dq.World(os.path.join(GOLDEN_SCENES, GOLDEN), ("host", "device"))
    objs = fr.objects_of(w.hs.arrays())
    c = rf.Case(w.path, 650, objs=objs)
    w.attach(d_origin=c.o, d_direction=c.d)
    tests = device_tests(w.devs["host"], len(objs), c.o, c.d)
    for n_skip, ranged in FILTERS:
        skip, skip_range = rf.draw(c, n_skip, ranged)
        masked, thinned = rf.mask_table(c.table, skip, skip_range), rf.mask_tests(tests, skip, skip_range)
        for limits in (None, c.limits):
            what = "%s, n_skip = %d%s%s" % (GOLDEN, n_skip, ", a range" if ranged else "", "" if limits is None else ", limits")
            ok = ref.well_conditioned(rf.hits_margin(objs, c.o, c.d, limits, masked), what)[0]
            any_limits = inf_limits(c.n) if limits is None else limits
            any_ok = ref.well_conditioned(rf.model_occluded(objs, c.o, c.d, any_limits, masked)[1], what + ", the any-hit")[0]
            for tree, dev in w.devs.items():
                for k in KS:
                    brute = hits(dev, NONE, w.dev["d_origin"], w.dev["d_direction"], k, limits, skip, skip_range)
                    assert_hits_are_brute(brute, hr.brute_hits(thinned, limits, k), k, "%s, %s tree, k = %d" % (what, tree, k))
                    assert_same_where(hits(dev, BVH, w.dev["d_origin"], w.dev["d_direction"], k, limits, skip, skip_range), brute, ok, "%s, %s tree, k = %d" % (what, tree, k))
                loop = occluded(dev, NONE, w.dev["d_origin"], w.dev["d_direction"], any_limits, skip, skip_range)
                assert (loop.astype(bool) == seg.brute_force(thinned, any_limits)).all(), what + ": the any-hit"
                assert not (any_ok & (occluded(dev, BVH, w.dev["d_origin"], w.dev["d_direction"], any_limits, skip, skip_range) != loop)).any(), what
    assert all(dev.status() == 0 for dev in w.devs.values())


# ---- 3. the thinned scene as a scene of its own -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["mixed", "mixed_planes"])
def test_a_shared_range_is_the_scene_without_it(name, worlds):
    w = worlds[name]
    dev, c, n = w.devs["host"], w.case, N_MODEL
    d_o, d_d = w.d_o[:n], w.d_d[:n]
    for first, count in rf.shared_ranges(len(c.objs)):
        keep = rf.kept(len(c.objs), first, count)
        thin = p3d.DeviceScene(p3d.HostScene(rf.write_thinned(worlds["tmp"] / ("%s_%d_%d.p3f" % (name, first, count)), c.objs, keep)), bvh=False)
        skip_range = np.tile(np.int32([first, count]), (n, 1))
        for t_max in (None, c.limits[:n]):
            what = "%s without %d objects from %d%s" % (name, count, first, "" if t_max is None else ", limits")
            for k in KS:
                got = hits(dev, NONE, d_o, d_d, k, t_max, None, skip_range)
                want = plain_hits(thin, NONE, d_o, d_d, k, t_max)
                if k:
                    want["object"] = rf.mapped_back(want["object"], keep)
                same(got, want, what + ", k = %d" % k)
            lim = inf_limits(n) if t_max is None else t_max
            same(occluded(dev, NONE, d_o, d_d, lim, None, skip_range), plain_occluded(thin, NONE, d_o, d_d, lim), what + ": the any-hit")
        assert thin.status() == 0


# ---- 4. the slats: a full list is refilled from behind the skipped ones ---------------------------------------------------------------

def slat_filters(n):
    """Sixteen of the forty slats per ray: eight on the list and eight in the range, which begin at a slat that differs from ray
    to ray -> (skip, skip_range, named (40, n))"""
    start = (np.arange(n) * 7) % (hr.N_SLATS - 16)
    skip = (start[:, None] + np.arange(8)[None, :]).astype(np.int32)
    skip_range = np.stack([start + 8, np.full(n, 8)], 1).astype(np.int32)
    return skip, skip_range, fr.skipped(hr.N_SLATS, n, skip, skip_range)


def test_slats_refill_a_full_list(slats):
    w, dev, n = slats, slats.devs["device"], N_MESH
    d_o, d_d = w.d_o[:n], w.d_d[:n]
    skip, skip_range, named = slat_filters(n)
    assert (named.sum(0) == 16).all()
    survivors = np.stack([np.nonzero(~named[:, i])[0][:16] for i in range(n)])  # a ray along +z meets the slats in file order
    tests = rf.mask_tests(device_tests(dev, hr.N_SLATS, w.o[:n], w.d[:n]), skip, skip_range)
    for accel in (NONE, BVH):
        full = hits(dev, accel, d_o, d_d, 16, None, skip, skip_range)
        what = "slats, accel %d" % accel
        assert (full["total"] == hr.N_SLATS - 16).all() and (full["count"] == 16).all(), what
        assert (full["object"] == survivors).all(), what + ": the sixteen nearest slats that are not skipped"
        assert_hits_are_brute(full, hr.brute_hits(tests, None, 16), 16, what)
        unfiltered = plain_hits(dev, accel, d_o, d_d, 16)
        assert (unfiltered["object"] == np.arange(16)[None, :]).all() and named[unfiltered["object"], np.arange(n)[:, None]].any()
        for k in (1, 4, 16):  # without total a full list culls against its last entry, which no skipped slat may have set
            lean = hits(dev, accel, d_o, d_d, k, None, skip, skip_range, want=ROWS)
            for key in ROWS[1:]:
                assert as_bytes(lean[key]) == as_bytes(full[key][:, :k]), "%s: %s without total, k = %d" % (what, key, k)
        assert (hits(dev, accel, d_o, d_d, 0, None, skip, skip_range)["total"] == hr.N_SLATS - 16).all()
        # a limit between the first survivor and the second: one hit, and the any-hit sees it; below the first survivor: none
        t = full["t"]
        for lim, found in (((t[:, 0] + t[:, 1]) / 2, 1), (t[:, 0], 0)):
            lim = lim.astype(np.float32)
            assert (hits(dev, accel, d_o, d_d, 4, lim, skip, skip_range)["total"] == found).all(), what
            assert (occluded(dev, accel, d_o, d_d, lim, skip, skip_range) == found).all(), what + ": the any-hit"
            assert (plain_occluded(dev, accel, d_o, d_d, lim) == (1 if found else (survivors[:, 0] > 0))).all()
    assert dev.status() == 0


# ---- 5. inside or outside, without the asking body ---------------------------------------------------------------------------------------

def test_parity_without_the_asking_body(tmp_path):
    o_c, d_c, inside = hr.cube_rays(23, N_MESH)
    o_b, d_b = rf.body_rays(29, N_MESH)
    path = rf.write_cube_and_body(tmp_path / "two_bodies.p3f")
    objs = ref.load_objects(path)
    assert len(objs) == 2 * rf.CUBE_TRIANGLES
    cube = np.tile(np.int32([0, rf.CUBE_TRIANGLES]), (N_MESH, 1))
    for o, d, in_cube, in_body in ((o_c, d_c, inside, np.zeros(N_MESH, bool)), (o_b, d_b, np.zeros(N_MESH, bool), np.ones(N_MESH, bool))):
        w = RayWorld(path, ("device",), o, d)
        dev = w.devs["device"]
        table = ref._all(objs, w.o, w.d)
        ok = ref.well_conditioned(hr.all_hits_margin(objs, w.o, w.d, None, table), "two bodies")[0]
        ok &= ref.well_conditioned(rf.hits_margin(objs, w.o, w.d, None, rf.mask_table(table, None, cube)), "two bodies without the cube")[0]
        for accel in (NONE, BVH):
            whole = plain_hits(dev, accel, w.d_o, w.d_d, 0, want=("total",))["total"]
            without = hits(dev, accel, w.d_o, w.d_d, 0, None, None, cube, want=("total",))["total"]
            assert ((whole[ok] & 1) == (in_cube | in_body)[ok]).all(), "accel %d: unfiltered, the parity counts the cube" % accel
            assert ((without[ok] & 1) == in_body[ok]).all(), "accel %d: without the cube's range the parity is the second body's" % accel
            if in_cube.any():
                assert (without[ok & in_cube] == 0).sum() > 50 and np.isin(without[ok & in_cube], (0, 2)).all()
        assert dev.status() == 0


# ---- 6. filters stay with their lanes; filters that name nothing; no filter ------------------------------------------------------------

def occlusion_inputs(w, count=129):
    p, nrm, limits = oc.choose_points(w, count, SAMPLES, oc.drawn_limits)
    return p, nrm, limits


def ask_occlusion(dev, accel, p, nrm, limits, skip=None, skip_range=None, team=0, want=("unoccluded", "bent"), **kw):
    res = p3d.occlusion_filtered_device(dev, accel, gpu(p), gpu(nrm), SAMPLES, max_dist=limits_of(limits), seed=oc.SEED, sample_begin=oc.BEGIN,
                                        team=team, want=want, **dev_filter(skip, skip_range), **kw)
    return {name: v.cpu().numpy() for name, v in res.items()}


def test_filters_do_not_leak_between_lanes(worlds, slats):
    """Neighbouring lanes hold different filters: the batch reversed gives the rows reversed, and a ray answers alone as it
    does in the batch"""
    w = worlds["mixed"]
    dev, c = w.devs["device"], w.case
    for n in (65, 129):
        skip, skip_range = rf.draw(c, 8, True, n)
        back = lambda a: None if a is None else np.ascontiguousarray(a[::-1])
        o, d, lim = w.o[:n], w.d[:n], c.limits[:n]
        for accel in (NONE, BVH):
            for k in (1, 4):
                fwd = hits(dev, accel, gpu(o), gpu(d), k, lim, skip, skip_range)
                rev = hits(dev, accel, gpu(back(o)), gpu(back(d)), k, back(lim), back(skip), back(skip_range))
                same(fwd, {name: v[::-1] for name, v in rev.items()}, "mixed, accel %d, k = %d: the batch reversed" % (accel, k))
                for i in (0, 1, 63, 64):
                    one = hits(dev, accel, gpu(o[i:i + 1]), gpu(d[i:i + 1]), k, lim[i:i + 1], skip[i:i + 1], skip_range[i:i + 1])
                    same(one, {name: v[i:i + 1] for name, v in fwd.items()}, "mixed, accel %d, k = %d: ray %d alone" % (accel, k, i))
            fwd = occluded(dev, accel, gpu(o), gpu(d), lim, skip, skip_range)
            rev = occluded(dev, accel, gpu(back(o)), gpu(back(d)), back(lim), back(skip), back(skip_range))
            same(fwd, rev[::-1], "mixed, accel %d: the any-hit, the batch reversed" % accel)
    # the slats: every lane skips another sixteen; the answer of a lane is that of its own filter alone
    n = 129
    skip, skip_range, named = slat_filters(n)
    sdev = slats.devs["device"]
    for accel in (NONE, BVH):
        got = hits(sdev, accel, slats.d_o[:n], slats.d_d[:n], 16, None, skip, skip_range)
        assert not named[got["object"], np.arange(n)[:, None]].any(), "accel %d: a lane lists a slat of its own filter" % accel
        left = np.stack([np.nonzero(~named[:, i])[0][:16] for i in range(n)])
        assert (got["object"] == left).all() and len(np.unique(left, axis=0)) > 16, "accel %d: a lane answers with a neighbour's filter" % accel
    # occlusion: one row per point, whatever the team
    p, nrm, limits = occlusion_inputs(w)
    m = len(p)
    skip, skip_range = rf.draw(c, 8, True, m)
    for accel in (NONE, BVH):
        for team in (1, 16, 64):
            fwd = ask_occlusion(dev, accel, p, nrm, limits, skip, skip_range, team=team, point_offset=0)
            # (the sample streams follow the point's index: reversed points keep theirs through a split into single points)
            for i in (0, 1, 63, 64, m - 1):
                one = ask_occlusion(dev, accel, p[i:i + 1], nrm[i:i + 1], limits[i:i + 1], skip[i:i + 1], skip_range[i:i + 1], team=team, point_offset=i)
                same(one, {name: v[i:i + 1] for name, v in fwd.items()}, "occlusion, accel %d, team %d: point %d alone" % (accel, team, i))
    assert dev.status() == 0 and sdev.status() == 0


def nothing_filters(n, n_objs):
    rng = np.random.default_rng(5)
    return {
        "absent": {},
        "no columns": dict(skip=np.zeros((n, 0), np.int32)),
        "all -1": dict(skip=np.full((n, 8), -1, np.int32)),
        "past the object count": dict(skip=rng.integers(n_objs, 2 ** 31 - 1, (n, 5)).astype(np.int32)),
        "negative entries": dict(skip=rng.integers(-2 ** 31, 0, (n, 3)).astype(np.int32)),
        "count <= 0": dict(skip_range=np.stack([rng.integers(0, n_objs, n), rng.integers(-5, 1, n)], 1).astype(np.int32)),
        "a range past the end that overflows 32 bits": dict(skip=np.full((n, 1), -1, np.int32),
                                                            skip_range=np.tile(np.int32([2 ** 31 - 2, 2 ** 31 - 1]), (n, 1))),
        "a range that ends below 0": dict(skip_range=np.tile(np.array([-2 ** 31, 2 ** 31 - 1], np.int64).astype(np.int32), (n, 1))),
    }


@pytest.mark.parametrize("tree", ["host", "device"])
def test_a_filter_that_names_nothing_changes_no_bit(tree, worlds):
    w = worlds["mixed"]
    dev, c, n = w.devs[tree], w.case, 129
    d_o, d_d, lim = w.d_o[:n], w.d_d[:n], c.limits[:n]
    p, nrm, limits = occlusion_inputs(w)
    for what, filt in nothing_filters(n, len(c.objs)).items():
        f = (filt.get("skip"), filt.get("skip_range"))
        for accel in (NONE, BVH):
            label = "%s tree, accel %d, %s" % (tree, accel, what)
            for k in KS:
                for t_max in (None, lim):
                    same(hits(dev, accel, d_o, d_d, k, t_max, *f), plain_hits(dev, accel, d_o, d_d, k, t_max), label + ", k = %d" % k)
            same(hits(dev, accel, d_o, d_d, 4, lim, *f, want=ROWS), plain_hits(dev, accel, d_o, d_d, 4, lim, want=ROWS), label + ", without total")
            for t_max in (lim, inf_limits(n)):
                same(occluded(dev, accel, d_o, d_d, t_max, *f), plain_occluded(dev, accel, d_o, d_d, t_max), label + ": the any-hit")
            for team in (1, 16, 64):
                plain = p3d.occlusion_device(dev, accel, gpu(p), gpu(nrm), SAMPLES, max_dist=gpu(limits), seed=oc.SEED, sample_begin=oc.BEGIN, team=team,
                                             want=("unoccluded", "bent"))
                same(ask_occlusion(dev, accel, p, nrm, limits, *f, team=team), {name: v.cpu().numpy() for name, v in plain.items()},
                     label + ": occlusion, team %d" % team)
    # t_max = None: the wrapper's own +inf limits
    same(occluded(dev, BVH, d_o, d_d, None), plain_occluded(dev, BVH, d_o, d_d, inf_limits(n)), "the wrapper's +inf limits")
    assert dev.status() == 0


# ---- 7. occlusion ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,tree", [("mixed", "host"), ("mixed", "device"), ("axis_aligned", "host")])
def test_occlusion_counts_equal_the_filtered_any_hit_over_its_rays(name, tree, worlds):
    w = worlds[name]
    dev, c = w.devs[tree], w.case
    p, nrm, limits = occlusion_inputs(w)
    m = len(p)
    rays = p3d.occlusion_rays_device(dev, gpu(p), gpu(nrm), SAMPLES, sample_begin=oc.BEGIN, seed=oc.SEED)
    host_o, host_d = p3d.occlusion_rays(p, nrm, SAMPLES, sample_begin=oc.BEGIN, seed=oc.SEED)
    assert as_bytes(rays["origin"].cpu().numpy()) == as_bytes(host_o) and as_bytes(rays["direction"].cpu().numpy()) == as_bytes(host_d)
    per_ray = lambda a: None if a is None else np.repeat(a, SAMPLES, axis=0)
    changed = 0
    for n_skip, ranged in FILTERS:
        skip, skip_range = rf.draw(c, n_skip, ranged, m)
        if skip is not None:  # the objects the points lie on, and those their rays meet first: what a point of a body skips
            first = hits(dev, NONE, rays["origin"], rays["direction"], 1, per_ray(limits))["object"].reshape(m, SAMPLES)
            rows = np.arange(m) % 4 != 3
            skip[rows, :] = np.where(first[rows, :n_skip] >= 0, first[rows, :n_skip], skip[rows, :])
        for lim in (None, limits):
            label = "%s, %s tree, n_skip = %d%s%s" % (name, tree, n_skip, ", a range" if ranged else "", "" if lim is None else ", limits")
            ray_limits = inf_limits(m * SAMPLES) if lim is None else per_ray(lim)
            occ = {accel: occluded(dev, accel, rays["origin"], rays["direction"], ray_limits, per_ray(skip), per_ray(skip_range)) for accel in (NONE, BVH)}
            agree = (occ[NONE] == occ[BVH]).reshape(m, SAMPLES).all(1)
            assert agree.sum() >= m - m // 8, label + ": the accels disagree on too many points for the bent normals to be compared"
            bent = {}
            for accel in (NONE, BVH):
                counts = oc.counts_from(occ[accel], SAMPLES)
                for team in (1, 16, 64):
                    got = ask_occlusion(dev, accel, p, nrm, lim, skip, skip_range, team=team)
                    assert got["unoccluded"].dtype == np.int32 and (got["unoccluded"] == counts).all(), "%s, accel %d, team %d: the counts" % (label, accel, team)
                    err = np.abs(got["bent"].astype(np.float64) - oc.bent_from(occ[accel], host_d, SAMPLES)).max()
                    assert err <= oc.bent_bound(SAMPLES), "%s, accel %d, team %d: bent" % (label, accel, team)
                    bent[accel, team] = got["bent"]
            for team in (1, 16, 64):
                assert as_bytes(bent[NONE, team][agree]) == as_bytes(bent[BVH, team][agree]), "%s, team %d: bent across the accels" % (label, team)
            if n_skip or ranged:
                plain = p3d.occlusion_device(dev, NONE, gpu(p), gpu(nrm), SAMPLES, max_dist=limits_of(lim), seed=oc.SEED, sample_begin=oc.BEGIN)
                changed += int((plain["unoccluded"].cpu().numpy() != oc.counts_from(occ[NONE], SAMPLES)).sum())
    assert changed > 0, "%s: the filters opened no point" % name
    assert dev.status() == 0


def test_a_sphere_of_the_scene_is_open_on_its_own_shell(tmp_path):
    """A particle that is a sphere of the scene, points on its own shell, bias 0: with itself skipped it is fully open where
    nothing else is near; unfiltered, a point that float32 puts on or inside the shell meets the shell at t = 0 (under the tree
    only where the ray also passes the box test of the sphere's leaf: an origin on a face of that box, heading out, misses it)"""
    (tmp_path / "particles.p3f").write_text(ref.HEAD + "s 0 0 0 1\ns 4 0 0 1\np 3\n-1 -1 9\n1 -1 9\n0 1 9\ns 0 7 0 0.5\n")
    hs = p3d.HostScene(str(tmp_path / "particles.p3f"))
    rng = np.random.default_rng(33)
    axes = np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)  # |p|^2 = 1 exactly: c = 0 in the sphere's test, a hit at t = 0
    nrm = np.concatenate([axes, ref.normalize32(ref._unit(rng, 123).astype(np.float32))])
    p = nrm.copy()  # the unit sphere at the origin: a point of the shell is its own normal
    n = len(p)
    limits = np.full(n, 1.5, np.float32)  # the nearest other surface is 2 away
    own = np.zeros((n, 1), np.int32)
    for tree in (True, "device"):
        dev = p3d.DeviceScene(hs, bvh=tree)
        for accel in (NONE, BVH):
            for team in (1, 16, 64):
                ask = lambda **f: ask_occlusion(dev, accel, p, nrm, limits, team=team, bias=0.0, **f)["unoccluded"]
                plain = ask()
                if accel == NONE:
                    assert (plain[:6] == 0).all() and (plain < SAMPLES).sum() >= 6, "unfiltered, the shell shadows its own points"
                assert (ask(skip=own) == SAMPLES).all(), "accel %d, team %d: a sphere that skips itself is still shadowed" % (accel, team)
                assert (ask(skip_range=np.tile(np.int32([0, 1]), (n, 1))) == SAMPLES).all()
                other = ask(skip=np.full((n, 1), 1, np.int32))  # another sphere's index opens nothing
                assert (other == plain).all()
        assert dev.status() == 0


# ---- 8. the contract every device query keeps ------------------------------------------------------------------------------------------

N_SKIP = 3
FILTER_INPUTS = (dq.Input("d_skip", N_SKIP, False, "int32"), dq.Input("d_skip_range", 2, False, "int32"))
RAY_INPUTS = (dq.Input("d_origin", 3, True), dq.Input("d_direction", 3, True), dq.Input("d_t_max", None, False))


def with_filters(required=("d_origin", "d_direction"), limit="d_t_max"):
    """Query.inputs_of for a world whose filters are attached: the required inputs, the limit if asked for, and both filters"""
    def inputs_of(w, n, limited=False):
        names = list(required) + ([limit] if limited else []) + ["d_skip", "d_skip_range"]
        return {name: w.dev[name][:n] for name in names}
    return inputs_of


def model_objects(a):
    """intersect_reference's objects from HostScene.arrays() (no planes)"""
    out = []
    for kind, v in zip(a["prim_type"], np.asarray(a["prim_v"], np.float64).reshape(-1, 9)):
        assert kind in (TRIANGLE, SPHERE, BOX)
        out.append(dict(kind=ref.TRIANGLE, p0=v[0:3], p1=v[3:6], p2=v[6:9]) if kind == TRIANGLE else
                   dict(kind=ref.SPHERE, c=v[:3], r=v[3]) if kind == SPHERE else dict(kind=ref.BOX, mn=v[:3], mx=v[3:6]))
    return out


def tree_is_brute_where_well_conditioned(got, brute, hs, w, n, limited, what):
    """assert_tree: the tree's answers behind an update are the fresh scene's brute force on the rays the thinned model of the
    moved geometry calls well-conditioned"""
    objs = model_objects(hs.arrays())
    o, d = w.o[:n], w.d[:n]
    masked = rf.mask_table(ref._all(objs, o, d), w.host["d_skip"][:n], w.host["d_skip_range"][:n])
    limits = w.host["d_t_max"][:n] if limited else None
    if "occluded" in got:
        margin = rf.model_occluded(objs, o, d, inf_limits(n) if limits is None else limits, masked)[1]
    else:
        margin = rf.hits_margin(objs, o, d, limits, masked)
    assert_same_where(got, brute, ref.well_conditioned(margin, what)[0], what)


def filtered_hits(k, width=0):
    """width: the n_skip of the RAW calls (0: the contract's raw calls pass no list); the wrapper's calls bring lists N_SKIP wide"""
    return dq.Query(
        "trace_hits_filtered_device", (k, "d_origin", "d_direction", "d_t_max", "d_skip", width, "d_skip_range", "d_count", "d_total", "d_object", "d_t",
                                       "d_hit_point", "d_normal"),
        RAY_INPUTS + FILTER_INPUTS, p3d._trace_hits_outputs(k), ("count", "total", "object", "t", "hit_point", "normal"), ("count", "object"),
        limit="d_t_max", witness="t", on_stream=(BVH, NONE), assert_tree=tree_is_brute_where_well_conditioned, inputs_of=with_filters(),
        call=lambda dev, accel, i, want, stream, out: p3d.trace_hits_filtered_device(
            dev, accel, i["d_origin"], i["d_direction"], k, t_max=i.get("d_t_max"), skip=i.get("d_skip"), skip_range=i.get("d_skip_range"),
            n_skip=N_SKIP if i.get("d_skip") is not None else None, want=want, stream=stream, out=out))


def filtered_any(width=0):
    """The limit is a required input here: every call, limited or not in the contract's words, brings the world's d_t_max"""
    return dq.Query(
        "trace_any_filtered_device", ("d_origin", "d_direction", "d_t_max", "d_skip", width, "d_skip_range", "d_occluded"),
        (dq.Input("d_origin", 3, True), dq.Input("d_direction", 3, True), dq.Input("d_t_max", None, True)) + FILTER_INPUTS,
        {"occluded": ("uint8", None)}, ("occluded",), ("occluded",), limit="d_t_max", witness="occluded", on_stream=(BVH, NONE),
        assert_tree=tree_is_brute_where_well_conditioned,
        inputs_of=lambda w, n, limited=False: {name: w.dev[name][:n] for name in ("d_origin", "d_direction", "d_t_max", "d_skip", "d_skip_range")},
        call=lambda dev, accel, i, want, stream, out: p3d.trace_any_filtered_device(
            dev, accel, i["d_origin"], i["d_direction"], t_max=i.get("d_t_max"), skip=i.get("d_skip"), skip_range=i.get("d_skip_range"),
            n_skip=N_SKIP if i.get("d_skip") is not None else None, stream=stream, out=out))


def occlusion_tree(got, brute, hs, w, n, limited, what):
    """assert_tree of the occlusion query: the counts of the tree are the brute force's on the points all of whose rays the
    thinned model of the moved geometry calls well-conditioned"""
    objs = model_objects(hs.arrays())
    o, d = p3d.occlusion_rays(w.host["d_point"][:n], w.host["d_normal"][:n], SAMPLES)
    per_ray = lambda a: np.repeat(a[:n], SAMPLES, axis=0)
    masked = rf.mask_table(ref._all(objs, o, d), per_ray(w.host["d_skip"]), per_ray(w.host["d_skip_range"]))
    limits = per_ray(w.host["d_max_dist"]) if limited else inf_limits(n * SAMPLES)
    ok = (rf.model_occluded(objs, o, d, limits, masked)[1] >= ref.THRESHOLD).reshape(n, SAMPLES).all(1)
    # (a point lies 1e-4 above its own surface, which some of its sixteen rays graze: about one point in four passes on these scenes)
    assert ok.sum() > n // 10, what + ": too few points are well-conditioned in all their rays"
    assert_same_where(got, brute, ok, what)


def filtered_occlusion(width=0):
    params = p3d.OcclusionParams(seed=0, samples=SAMPLES, sample_begin=0, point_offset=0, flags=0, bias=1e-4, team=0)  # (held here: the raw calls pass its address)
    q = dq.Query(
        "occlusion_filtered_device", ("d_point", "d_normal", "d_max_dist", C.byref(params), "d_skip", width, "d_skip_range", "d_unoccluded", "d_bent"),
        (dq.Input("d_point", 3, True), dq.Input("d_normal", 3, True), dq.Input("d_max_dist", None, False)) + FILTER_INPUTS, p3d._OCCLUSION_OUTPUTS,
        ("unoccluded", "bent"), ("unoccluded",), limit="d_max_dist", witness="unoccluded", on_stream=(BVH, NONE), assert_tree=occlusion_tree,
        inputs_of=with_filters(required=("d_point", "d_normal"), limit="d_max_dist"),
        call=lambda dev, accel, i, want, stream, out: p3d.occlusion_filtered_device(
            dev, accel, i["d_point"], i["d_normal"], SAMPLES, max_dist=i.get("d_max_dist"), skip=i.get("d_skip"), skip_range=i.get("d_skip_range"),
            n_skip=N_SKIP if i.get("d_skip") is not None else None, want=want, stream=stream, out=out))
    q.params = params
    return q


FOUR_HITS, FILTERED_ANY, OCCLUSION = filtered_hits(4), filtered_any(), filtered_occlusion()
RAW_WIDTH = {"trace_hits_filtered_device": lambda width: filtered_hits(2, width), "trace_any_filtered_device": filtered_any,
             "occlusion_filtered_device": filtered_occlusion}


def well_conditioned_world(w, tmp):
    """A copy of a World with rays every back end answers alike: those whose thinned margins - of the hit list and of the
    any-hit, without and with limits - are all above the threshold, with N_SKIP-wide lists and ranges drawn round their first hits"""
    c = w.case
    skip, skip_range = fr.draw(c.n, len(c.objs), N_SKIP, True, 77, answers=rf.first_hits(c.table))
    masked = rf.mask_table(c.table, skip, skip_range)
    margins = [rf.hits_margin(c.objs, c.o, c.d, lim, masked) for lim in (None, c.limits)]
    margins += [rf.model_occluded(c.objs, c.o, c.d, lim, masked)[1] for lim in (inf_limits(c.n), c.limits)]
    ok = np.min(margins, axis=0) >= ref.THRESHOLD
    assert ok.sum() >= 0.8 * c.n
    rows = np.concatenate([np.nonzero(ok)[0], np.nonzero(ok)[0]])[:c.n]  # (filled up with a second round of the same rays)
    out = copy.copy(w)
    out.host, out.dev = {}, {}
    out.set_rays(w.o[rows], w.d[rows])
    out.attach(d_t_max=c.limits[rows], d_skip=skip[rows], d_skip_range=skip_range[rows])
    return out


@pytest.fixture(scope="module")
def contract(worlds):
    w = well_conditioned_world(worlds["mixed"], worlds["tmp"])
    w.device_tests = device_tests(w.devs["host"], len(w.objs), w.o, w.d)
    return w


@pytest.fixture(scope="module")
def occlusion_contract(contract):
    """The contract's world with max(BATCHES) surface points (the world's own, round after round), their limits and filters, and
    the yardstick by limits: the counts of the masked brute force over p3d_object_intercepts on the written rays, the float64
    bent sum, and the points all of whose rays the thinned model calls well-conditioned (where the tree has to agree)"""
    w = copy.copy(contract)
    w.host, w.dev = dict(contract.host), dict(contract.dev)
    p, nrm = oc.surface_points(contract)
    rows = np.arange(max(BATCHES)) % len(p)
    p, nrm = np.ascontiguousarray(p[rows]), np.ascontiguousarray(nrm[rows])
    m = len(p)
    w.attach(d_point=p, d_normal=nrm, d_max_dist=oc.drawn_limits(m))
    o, d = p3d.occlusion_rays(p, nrm, SAMPLES)
    per_ray = lambda a: np.repeat(a, SAMPLES, axis=0)
    skip, skip_range = per_ray(w.host["d_skip"]), per_ray(w.host["d_skip_range"])
    tests = rf.mask_tests(device_tests(w.devs["host"], len(w.objs), o, d), skip, skip_range)
    masked = rf.mask_table(ref._all(w.objs, o, d), skip, skip_range)
    w.yardstick = {}
    for limited in (False, True):
        limits = per_ray(w.host["d_max_dist"]) if limited else inf_limits(m * SAMPLES)
        occ = seg.brute_force(tests, limits)
        ok = (rf.model_occluded(w.objs, o, d, limits, masked)[1] >= ref.THRESHOLD).reshape(m, SAMPLES).all(1)
        w.yardstick[limited] = (oc.counts_from(occ, SAMPLES).astype(np.int32), oc.bent_from(occ, d, SAMPLES), ok)
    return w


@pytest.mark.parametrize("n", BATCHES)
def test_ragged_batches_of_points_through_every_back_end(n, occlusion_contract):
    """Filtered occlusion at every batch size, team and back end: the loop's counts are the masked brute force's on every point,
    the tree's on the points whose rays are all well-conditioned, and there the bent normals of the two are the same bits"""
    w = occlusion_contract
    for limited in (False, True):
        counts, bent, ok = (a[:n] for a in w.yardstick[limited])
        inputs = OCCLUSION.inputs_of(w, n, limited)
        for team in (1, 16, 64):
            loop = {}
            for tree, dev, accel in w.back_ends():
                what = "filtered occlusion, %s tree, accel %d, team %d, %d points%s" % (tree, accel, team, n, ", limits" if limited else "")
                got = {name: v.cpu().numpy() for name, v in p3d.occlusion_filtered_device(
                    dev, accel, inputs["d_point"], inputs["d_normal"], SAMPLES, max_dist=inputs.get("d_max_dist"), skip=inputs["d_skip"],
                    skip_range=inputs["d_skip_range"], team=team, want=("unoccluded", "bent")).items()}
                assert got["unoccluded"].dtype == np.int32 and got["unoccluded"].shape == (n,) and got["bent"].shape == (n, 3), what
                where = np.ones(n, bool) if accel == NONE else ok
                assert (got["unoccluded"][where] == counts[where]).all(), what + ": the counts"
                assert np.abs(got["bent"].astype(np.float64) - bent)[where].max(initial=0.0) <= oc.bent_bound(SAMPLES), what + ": bent"
                if accel == NONE:
                    loop[tree] = got
                else:
                    assert as_bytes(got["bent"][ok]) == as_bytes(loop[tree]["bent"][ok]), what + ": bent against the loop's"
    if n == max(BATCHES):
        # (a point lies 1e-4 above its own surface, which some of its sixteen rays graze: the float64 model alone says 26 % pass here)
        assert all(w.yardstick[limited][2].mean() > 0.1 for limited in (False, True)), "too few points are well-conditioned in all their rays"
        assert (w.yardstick[True][0] != w.yardstick[False][0]).any() and 0 < w.yardstick[True][0].mean() < SAMPLES
    assert all(dev.status() == 0 for dev in w.devs.values())


@pytest.mark.parametrize("n", BATCHES)
def test_ragged_batches_through_every_back_end(n, contract):
    w = contract
    tests = rf.mask_tests((w.device_tests[0][:, :n], w.device_tests[1][:, :n]), w.host["d_skip"][:n], w.host["d_skip_range"][:n])
    lim = w.host["d_t_max"][:n]
    for k in (1, 4, 16):
        answers = [dict(zip(("count", "total", "object", "t"), hr.brute_hits(tests, t_max, k))) for t_max in (None, lim)]
        dq.check_ragged_batches(filtered_hits(k), w, n, *answers, "filtered hits, k = %d" % k)
    any_limited = {"occluded": seg.brute_force(tests, lim).astype(np.uint8)}  # (check_ragged_batches wants an object or a hit_id among the outputs)
    for tree, dev, accel in w.back_ends():
        same(FILTERED_ANY.ask(dev, accel, FILTERED_ANY.inputs_of(w, n)), any_limited, "the filtered any-hit, %s tree, accel %d, %d rows" % (tree, accel, n))


def test_empty_batches_and_the_callers_outputs(contract, occlusion_contract):
    w, dev = contract, contract.devs["host"]
    for q in (FOUR_HITS, FILTERED_ANY, OCCLUSION):
        dq.check_empty_batch(q, dev)
    lib = p3d.lib()
    assert lib.p3d_trace_hits_filtered_device(dev._h, BVH, 0, 2, None, None, None, None, 9, None, *([None] * 7)) == INVALID  # whatever n
    assert b"n_skip must be" in lib.p3d_last_error()
    n = 129
    tests = rf.mask_tests((w.device_tests[0][:, :n], w.device_tests[1][:, :n]), w.host["d_skip"][:n], w.host["d_skip_range"][:n])
    want = dict(zip(("count", "total", "object", "t"), hr.brute_hits(tests, w.host["d_t_max"][:n], 4)))
    for accel in (NONE, BVH):
        dq.check_callers_outputs(FOUR_HITS, dev, accel, FOUR_HITS.inputs_of(w, n, True), want, "filtered hits, accel %d" % accel, optional=("total", "t"))
        dq.check_callers_outputs(FILTERED_ANY, dev, accel, FILTERED_ANY.inputs_of(w, n), {"occluded": seg.brute_force(tests, w.host["d_t_max"][:n]).astype(np.uint8)},
                                 "the filtered any-hit, accel %d" % accel)
        # occlusion: the answers the ragged batches pin (every point of the loop's, the well-conditioned ones of the tree's) into the caller's tensors
        points = OCCLUSION.inputs_of(occlusion_contract, n, True)
        answers = OCCLUSION.ask(dev, accel, points)
        counts, _, ok = (a[:n] for a in occlusion_contract.yardstick[True])
        where = np.ones(n, bool) if accel == NONE else ok
        assert (answers["unoccluded"][where] == counts[where]).all()
        dq.check_callers_outputs(OCCLUSION, dev, accel, points, answers, "filtered occlusion, accel %d" % accel, optional=("bent",))
    assert dev.status() == 0


def test_refusals_enqueue_nothing(contract, worlds):
    w, dev = contract, contract.devs["host"]
    n = 129
    lib = p3d.lib()
    ins = {"d_origin": w.d_o[:n], "d_direction": w.d_d[:n], "d_t_max": w.dev["d_t_max"][:n], "d_skip": w.dev["d_skip"][:n], "d_skip_range": w.dev["d_skip_range"][:n]}
    p, nrm = gpu(w.o[:n]), gpu(ref.normalize32(w.d[:n]))
    for q, inputs in ((filtered_hits(2), ins), (FILTERED_ANY, ins), (OCCLUSION, {"d_point": p, "d_normal": nrm, "d_skip": ins["d_skip"], "d_skip_range": ins["d_skip_range"]})):
        outs = dq.check_buffer_refusals(q, dev, inputs, n)
        good = {name: inputs[name] for name in inputs if name not in ("d_skip", "d_skip_range")}
        good.update({"d_" + name: t for name, t in outs.items()})
        nine = torch.full((n, 9), -1, dtype=torch.int32, device="cuda")
        # the filter's own refusals, worded once for all three
        assert RAW_WIDTH[q.name](9).raw(dev, BVH, n, **good, d_skip=nine) == INVALID and b"n_skip must be 0 .. P3D_FILTER_SKIP_MAX (8)" in lib.p3d_last_error()
        assert q.entry.encode() in lib.p3d_last_error()
        assert RAW_WIDTH[q.name](N_SKIP).raw(dev, BVH, n, **good) == INVALID and b"d_skip is needed with n_skip > 0" in lib.p3d_last_error()  # a null list
        with pytest.raises(p3d.P3DError) as e:
            q.call(dev, p3d.ACCEL_GRID, {name: t for name, t in inputs.items()}, (), 0, None)
        assert e.value.code == UNSUPPORTED and "grid" in str(e.value), q.name
        with pytest.raises(p3d.P3DError) as e:
            q.call(dev, NONE, dict(inputs, d_skip=nine), (), 0, None)
        assert e.value.code == INVALID and "n_skip says" in str(e.value)
        dq.assert_untouched(outs)
    # the any-hit needs its limit: the half-line without one is the feeler, which takes no filter
    occ = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    assert filtered_any(N_SKIP).raw(dev, BVH, n, d_origin=ins["d_origin"], d_direction=ins["d_direction"], d_skip=ins["d_skip"], d_occluded=occ) == INVALID
    assert b"pass +inf for a half-line" in lib.p3d_last_error()
    assert FILTERED_ANY.raw(dev, BVH, n, d_origin=ins["d_origin"], d_direction=ins["d_direction"], d_occluded=occ) == INVALID  # (no filter at all: still the segment query)
    assert b"pass +inf for a half-line" in lib.p3d_last_error()
    torch.cuda.synchronize()
    assert bool((occ == 77).all()) and dev.status() == 0


def test_behind_a_refit_on_the_same_stream(slats):
    n = 4099
    s = copy.copy(slats)
    s.host, s.dev = dict(s.host), dict(s.dev)
    skip, skip_range, _ = slat_filters(n)
    s.attach(d_t_max=hr.slat_limits(s.table(n), 25), d_skip=skip[:, :N_SKIP], d_skip_range=skip_range)
    lift = lambda a: (a["prim_v"].reshape(-1, 3) + np.float32([0.3, -0.2, 0.2])).astype(np.float32)
    dq.check_behind_a_refit(FOUR_HITS, s, n, soup=lift, what="filtered hits over the slats behind a refit")
    dq.check_behind_a_refit(FILTERED_ANY, s, n, soup=lift, what="the filtered any-hit over the slats behind a refit")
    # occlusion: points under the stack, looking up, with limits round the first slat their filters leave
    m = 515
    rng = np.random.default_rng(41)
    p = np.concatenate([rng.uniform(-0.5, 0.5, (m, 2)), rng.uniform(-1.5, -0.5, (m, 1))], 1).astype(np.float32)
    nrm = np.tile(np.float32([0, 0, 1]), (m, 1))
    wide = np.concatenate([skip[:m, :N_SKIP - 1], skip[:m, 7:8]], 1)
    first_left = np.argmax(~fr.skipped(hr.N_SLATS, m, wide, skip_range[:m]), axis=0) * hr.SLAT_GAP  # the height of the first slat a point's filter leaves
    limits = (first_left - p[:, 2] + rng.uniform(0.05, 0.5, m)).astype(np.float32)
    s.attach(d_point=p, d_normal=nrm, d_max_dist=limits, d_skip=wide, d_skip_range=skip_range[:m])
    dq.check_behind_a_refit(OCCLUSION, s, m, soup=lift, what="filtered occlusion under the slats behind a refit")


def test_behind_a_pose_on_the_same_stream(contract):
    dq.check_behind_a_pose(FOUR_HITS, contract, 4099, what="filtered hits behind a pose")
    dq.check_behind_a_pose(FILTERED_ANY, contract, 4099, limits=(True,), what="the filtered any-hit behind a pose")
    w = copy.copy(contract)
    w.host, w.dev = dict(w.host), dict(w.dev)
    p, nrm, limits = occlusion_inputs(contract)
    m = len(p)
    w.attach(d_point=p, d_normal=nrm, d_max_dist=limits, d_skip=contract.host["d_skip"][:m], d_skip_range=contract.host["d_skip_range"][:m])
    dq.check_behind_a_pose(OCCLUSION, w, m, what="filtered occlusion behind a pose")
