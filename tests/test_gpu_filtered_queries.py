"""Filtered queries over device tensors (p3d_nearest_k_filtered_device, p3d_sweep_sphere_filtered_device) on the GPU.

The yardstick is exact: host_nearest_k_filtered and host_sweep_sphere_filtered, the brute force on the CPU that
test_filter_api.py holds to the float64 models of the thinned scene.  Under ACCEL_NONE and ACCEL_BVH, on uploaded and
device-built trees and through the spill path of a deep tree, at every batch size, k and list width, the outputs the host forms
have must be their bits; filters that differ from lane to lane must not leak; an absent filter is the unfiltered query; and
what every device query promises is device_query_contract.py's.  Every comparison here has tolerance 0."""
import os

import numpy as np
import pytest

from conftest import SCENES as GOLDEN_SCENES
import device_query_contract as dq
from device_query_contract import BATCHES, INVALID, SWEEP, Input, nearest_k
from frame_checks import gpu
import filter_reference as fr
import intersect_reference as ref
import nearest_reference as near
import p3d_amd as p3d
import sweep_reference as sw

pytestmark = pytest.mark.gpu

N = max(BATCHES)
KS = (1, 4, 16)
K_CONTRACT, SKIP_CONTRACT = 3, 2  # (a required input of the shared refusals has at most 12 bytes per row)
NEAREST_HOST, SWEEP_HOST = ("count", "object", "dist", "closest"), ("object", "t", "centre", "contact")


def _filter_of(i):
    return dict(skip=i.get("d_skip"), skip_range=i.get("d_skip_range"))


def _host_filter(w, n, n_skip):
    return dict(skip=w.host["d_skip"][:n, :n_skip] if n_skip else None, skip_range=w.host["d_skip_range"][:n])


def nearest_k_filtered(k, n_skip):
    """p3d_nearest_k_filtered_device at this k and list width: the list is the first n_skip columns of the world's"""
    def inputs_of(w, n, limited=False):
        i = {"d_point": w.dev["d_point"][:n], "d_skip_range": w.dev["d_skip_range"][:n]}
        if n_skip:
            i["d_skip"] = w.lists[n_skip][:n]
        if limited:
            i["d_max_dist"] = w.dev["d_max_dist"][:n]
        return i

    return dq.Query(
        "nearest_k_filtered_device", (k, "d_point", "d_max_dist", "d_skip", n_skip, "d_skip_range", "d_count", "d_object", "d_dist", "d_closest", "d_normal"),
        (Input("d_point", 3, True), Input("d_max_dist", None, False), Input("d_skip", n_skip, n_skip > 0, "int32"), Input("d_skip_range", 2, False, "int32")),
        p3d._nearest_k_outputs(k), ("count", "object", "dist", "closest", "normal"), ("count", "object"), limit="d_max_dist", witness="dist",
        refuses_planes=True, inputs_of=inputs_of,
        call=lambda dev, accel, i, want, stream, out: p3d.nearest_k_filtered_device(dev, accel, i["d_point"], k, max_dist=i.get("d_max_dist"), n_skip=n_skip if "d_skip" in i else None,
                                                                                   want=want, stream=stream, out=out, **_filter_of(i)),
        host_form=lambda hs, w, n, limited: dict(zip(NEAREST_HOST, p3d.host_nearest_k_filtered(
            hs, w.host["d_point"][:n], k, max_dist=w.host["d_max_dist"][:n] if limited else None, **_host_filter(w, n, n_skip)))))


def sweep_filtered(n_skip):
    def inputs_of(w, n, limited=False):
        i = {name: w.dev[name][:n] for name in ("d_origin", "d_direction", "d_radius", "d_skip_range")}
        if n_skip:
            i["d_skip"] = w.lists[n_skip][:n]
        if limited:
            i["d_t_max"] = w.dev["d_t_max"][:n]
        return i

    return dq.Query(
        "sweep_sphere_filtered_device", ("d_origin", "d_direction", "d_radius", "d_t_max", "d_skip", n_skip, "d_skip_range", "d_object", "d_t", "d_centre", "d_contact", "d_normal"),
        (Input("d_origin", 3, True), Input("d_direction", 3, True), Input("d_radius", None, True), Input("d_t_max", None, False),
         Input("d_skip", n_skip, n_skip > 0, "int32"), Input("d_skip_range", 2, False, "int32")),
        p3d._SWEEP_OUTPUTS, ("object", "t", "centre", "contact", "normal"), ("object",), limit="d_t_max", witness="t", refuses_planes=True, inputs_of=inputs_of,
        call=lambda dev, accel, i, want, stream, out: p3d.sweep_sphere_filtered_device(dev, accel, i["d_origin"], i["d_direction"], i["d_radius"], t_max=i.get("d_t_max"),
                                                                                      n_skip=n_skip if "d_skip" in i else None, want=want, stream=stream, out=out, **_filter_of(i)),
        host_form=lambda hs, w, n, limited: dict(zip(SWEEP_HOST, p3d.host_sweep_sphere_filtered(
            hs, w.host["d_origin"][:n], w.host["d_direction"][:n], w.host["d_radius"][:n], t_max=w.host["d_t_max"][:n] if limited else None,
            **_host_filter(w, n, n_skip)))))


def world(path, trees, seed):
    """One scene with N points and N balls, limits for both, and filters drawn round the unfiltered answers: the list's first
    columns are the objects each query would find (three rows in four), so that a filter changes what is found"""
    w = dq.World(path, trees)
    a = w.hs.arrays()
    n_objs = int(a["n_prims"])
    lo, hi = a["prim_bmin"].min(0), a["prim_bmax"].max(0)
    rng = np.random.default_rng(seed)
    points = (lo + (hi - lo) * rng.uniform(-0.1, 1.1, (N, 3))).astype(np.float32)
    o, d, r = sw.box_balls(lo, hi, seed + 1, N)
    w.attach(d_point=points, d_origin=o, d_direction=d, d_radius=r)
    count, nearest, dist, _ = w.hs.nearest_k(points, 16)
    contact, T, _, _ = p3d.host_sweep_sphere(w.hs, o, d, r)
    with np.errstate(invalid="ignore"):
        far = np.where(count > 0, dist[np.arange(N), np.maximum(count - 1, 0)], 1.0)
        lim = (far * rng.choice([0.4, 0.8, 1.5], N)).astype(np.float32)
    lim[0::75], lim[25::75], lim[50::75] = 0.0, -1.5, np.nan
    step = np.maximum(np.linalg.norm(d.astype(np.float64), axis=1), 1e-30)
    w.attach(d_max_dist=lim, d_t_max=sw.draw_limits(np.where(contact >= 0, T.astype(np.float64), np.nan), 40.0 / step, seed + 2))
    answers = nearest.copy()
    answers[1::2, 0] = np.where(contact[1::2] >= 0, contact[1::2], answers[1::2, 0])  # every other row: the ball's contact first
    skip, skip_range = fr.draw(N, n_objs, 8, True, seed + 3, answers=answers)
    w.attach(d_skip=skip, d_skip_range=skip_range)
    w.lists = {s: gpu(np.ascontiguousarray(skip[:, :s])) for s in (1, SKIP_CONTRACT, 8)}  # (a list is contiguous: its first columns are a copy)
    w.n_objs, w.unfiltered = n_objs, (nearest, contact)
    return w


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = sw.scene_paths(tmp_path_factory.mktemp("filtered"))
    w = {"mixed": world(paths["mixed"], ("host", "device"), 700), "tri5k": world(tri5k_path, ("device",), 701),
         "planes": world(paths["planes"], ("none",), 702)}
    dq.assert_deep(w["tri5k"].devs["device"])  # deeper than the stack window: the spill path runs with a filter
    return w


@pytest.fixture(scope="module")
def host_answers(worlds):
    """(scene, query name, k, n_skip, limited) -> the host form's answers for all N rows, computed once"""
    cache = {}

    def get(name, query, key, limited):
        full = (name, query.name) + key + (limited,)
        if full not in cache:
            cache[full] = query.host_form(worlds[name].hs, worlds[name], N, limited)
        return cache[full]
    return get


@pytest.mark.parametrize("n_skip", fr.N_SKIPS)
@pytest.mark.parametrize("k", KS)
def test_nearest_is_the_host_form(k, n_skip, worlds, host_answers):
    query = nearest_k_filtered(k, n_skip)
    for name in ("mixed", "tri5k"):
        free, limited = host_answers(name, query, (k, n_skip), False), host_answers(name, query, (k, n_skip), True)
        for n in BATCHES:
            dq.check_ragged_batches(query, worlds[name], n, free, limited, "%s, k = %d, n_skip = %d" % (name, k, n_skip))
        named = fr.skipped(worlds[name].n_objs, N, worlds[name].host["d_skip"][:, :n_skip], worlds[name].host["d_skip_range"])
        found = free["object"] >= 0
        assert not named[free["object"][found], np.nonzero(found)[0]].any() and found.any()


@pytest.mark.parametrize("n_skip", fr.N_SKIPS)
def test_the_sweep_is_the_host_form(n_skip, worlds, host_answers):
    query = sweep_filtered(n_skip)
    for name in ("mixed", "tri5k"):
        free, limited = host_answers(name, query, (n_skip,), False), host_answers(name, query, (n_skip,), True)
        for n in BATCHES:
            dq.check_ragged_batches(query, worlds[name], n, free, limited, "%s, n_skip = %d" % (name, n_skip))
        named = fr.skipped(worlds[name].n_objs, N, worlds[name].host["d_skip"][:, :n_skip], worlds[name].host["d_skip_range"])
        found = free["object"] >= 0
        assert not named[free["object"][found], np.nonzero(found)[0]].any() and found.any()
        assert (free["object"] != worlds[name].unfiltered[1]).any(), name + ": the filters changed no contact"


def test_neighbouring_lanes_skip_each_others_answers(worlds):
    """Lane i skips what lane i ^ 1 finds without a filter, and nothing else: where the two answers differ, lane i must still find
    its own - a filter held in a wave-uniform value, or read from the neighbour's row, would take it away"""
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        n = 4098
        swap = np.arange(n) ^ 1
        nearest, contact = w.unfiltered[0][:n, 0], w.unfiltered[1][:n]
        for accel in w.accels("device"):
            dev = w.devs["device"]
            skip = np.ascontiguousarray(nearest[swap][:, None].astype(np.int32))
            got = p3d.nearest_k_filtered_device(dev, accel, w.dev["d_point"][:n], 1, skip=gpu(skip), want=("dist", "closest"))
            got = {key: v.cpu().numpy() for key, v in got.items()}
            want = p3d.host_nearest_k_filtered(w.hs, w.host["d_point"][:n], 1, skip=skip)
            dq.assert_answers(got, dict(zip(NEAREST_HOST, want)), p3d._nearest_k_outputs(1), "%s, accel %d: nearest, swapped lists" % (name, accel))
            differ = nearest != nearest[swap]
            assert differ.sum() > n // 4 and (got["object"][differ, 0] == nearest[differ]).all() and (got["object"][~differ, 0] != nearest[~differ]).all()
            skip = np.ascontiguousarray(contact[swap][:, None].astype(np.int32))
            got = p3d.sweep_sphere_filtered_device(dev, accel, w.dev["d_origin"][:n], w.dev["d_direction"][:n], w.dev["d_radius"][:n], skip=gpu(skip),
                                                   want=("t", "centre", "contact"))
            got = {key: v.cpu().numpy() for key, v in got.items()}
            want = p3d.host_sweep_sphere_filtered(w.hs, w.host["d_origin"][:n], w.host["d_direction"][:n], w.host["d_radius"][:n], skip=skip)
            dq.assert_answers(got, dict(zip(SWEEP_HOST, want)), p3d._SWEEP_OUTPUTS, "%s, accel %d: sweep, swapped lists" % (name, accel))
            differ = (contact != contact[swap]) & (contact >= 0)
            assert differ.sum() > 16 and (got["object"][differ] == contact[differ]).all()
        assert dev.status() == 0


def test_an_absent_filter_is_the_unfiltered_query(worlds):
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        for tree, dev, accel in w.back_ends():
            what = "%s, %s tree, accel %d" % (name, tree, accel)
            for k in KS:
                plain = nearest_k(k)
                for limited in (False, True):
                    lim = w.dev["d_max_dist"] if limited else None
                    want = {key: v.cpu().numpy() for key, v in dev.nearest_k_device(accel, w.dev["d_point"], k, max_dist=lim, want=plain.optional).items()}
                    got = {key: v.cpu().numpy() for key, v in p3d.nearest_k_filtered_device(dev, accel, w.dev["d_point"], k, max_dist=lim, want=plain.optional).items()}
                    dq.assert_same_bits(got, want, "%s, nearest, k = %d" % (what, k))
            for limited in (False, True):
                lim = w.dev["d_t_max"] if limited else None
                args = (dev, accel, w.dev["d_origin"], w.dev["d_direction"], w.dev["d_radius"])
                want = {key: v.cpu().numpy() for key, v in p3d.sweep_sphere_device(*args, t_max=lim, want=SWEEP.optional).items()}
                got = {key: v.cpu().numpy() for key, v in p3d.sweep_sphere_filtered_device(*args, t_max=lim, want=SWEEP.optional).items()}
                dq.assert_same_bits(got, want, what + ", sweep")
                # and filters that name nothing, through the filtered kernel
                none = p3d.sweep_sphere_filtered_device(*args, t_max=lim, want=SWEEP.optional, skip=gpu(np.full((N, 8), -1, np.int32)),
                                                        skip_range=gpu(np.tile(np.array([[w.n_objs, 5]], np.int32), (N, 1))))
                dq.assert_same_bits({key: v.cpu().numpy() for key, v in none.items()}, want, what + ", sweep, filters that name nothing")
            assert dev.status() == 0


@pytest.mark.parametrize("which", ("nearest", "sweep"))
def test_the_contract_of_every_device_query(which, worlds):
    query = nearest_k_filtered(K_CONTRACT, SKIP_CONTRACT) if which == "nearest" else sweep_filtered(SKIP_CONTRACT)
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    outs = dq.check_buffer_refusals(query, dev, query.inputs_of(w, n, True), n, planes=worlds["planes"])
    dq.check_empty_batch(query, dev)
    # the filter's own refusals, through the entry point: nothing is enqueued
    every = dict(query.inputs_of(w, n), **{"d_" + name: t for name, t in outs.items()})
    at = query.layout.index("d_skip") + 1  # n_skip stands behind its buffer
    assert query.layout[at] == SKIP_CONTRACT
    nine = dq.Query(query.name, query.layout[:at] + (9,) + query.layout[at + 1:], query.inputs, query.table, query.order, query.required, query.call)
    for rows in (n, 0):
        assert nine.raw(dev, p3d.ACCEL_BVH, rows, **every) == INVALID and b"n_skip must be" in p3d.lib().p3d_last_error()
    assert query.raw(dev, p3d.ACCEL_NONE, n, **dict(every, d_skip=None)) == INVALID and b"d_skip is needed" in p3d.lib().p3d_last_error()
    dq.assert_untouched(outs)
    whole = query.ask(dev, p3d.ACCEL_BVH, query.inputs_of(w, N, True))
    dq.check_callers_outputs(query, dev, p3d.ACCEL_BVH, query.inputs_of(w, N, True), whole, which, optional=("closest",) if which == "nearest" else ("contact",))
    dq.check_behind_a_refit(query, worlds["tri5k"], N, what="tri5k behind a refit")
    dq.check_behind_a_pose(query, w, N, what="mixed behind a pose")
    assert dev.status() == 0


def test_a_vertex_of_the_mesh_and_a_sphere_of_the_balls_on_the_device():
    """test_filter_api.py's self-contact cases, on the device: bit for bit the host forms, which that test holds to the model"""
    hs = p3d.HostScene(os.path.join(GOLDEN_SCENES, "mount_high.p3f"), legacy_f11=True)
    a = hs.arrays()
    points, incident = fr.mesh_vertices(a["prim_type"], a["prim_v"])
    assert len(points) >= 64
    want = p3d.host_nearest_k_filtered(hs, points, 1, skip=incident)
    balls = p3d.HostScene(os.path.join(GOLDEN_SCENES, "balls_low.p3f"))
    b = balls.arrays()
    spheres = np.nonzero(b["prim_type"] == 0)[0].astype(np.int32)
    centre, radius = np.ascontiguousarray(b["prim_v"][spheres, :3], np.float32), np.ascontiguousarray(b["prim_v"][spheres, 3], np.float32)
    d = np.tile(np.array([[0.3, -0.2, 0.1]], np.float32), (len(spheres), 1))
    want_sweep = p3d.host_sweep_sphere_filtered(balls, centre, d, radius, skip=spheres[:, None])
    for tree in (True, "device"):
        dev = p3d.DeviceScene(hs, bvh=tree)
        for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
            plain = dev.nearest_device(accel, gpu(points))
            assert (plain["dist"].cpu().numpy() == 0).all() and (plain["object"].cpu().numpy()[:, None] == incident).any(1).all()
            got = {key: v.cpu().numpy() for key, v in p3d.nearest_k_filtered_device(dev, accel, gpu(points), 1, skip=gpu(incident), want=("dist", "closest")).items()}
            dq.assert_answers(got, dict(zip(NEAREST_HOST, want)), p3d._nearest_k_outputs(1), "the mesh's own vertices, accel %d" % accel)
            assert not (got["object"] == incident).any()
        assert dev.status() == 0
    dev = p3d.DeviceScene(balls, bvh=False)
    plain = p3d.sweep_sphere_device(dev, p3d.ACCEL_NONE, gpu(centre), gpu(d), gpu(radius))
    assert (plain["t"].cpu().numpy() == 0).all()
    got = {key: v.cpu().numpy() for key, v in p3d.sweep_sphere_filtered_device(dev, p3d.ACCEL_NONE, gpu(centre), gpu(d), gpu(radius), skip=gpu(spheres[:, None]),
                                                                              want=("t", "centre", "contact")).items()}
    dq.assert_answers(got, dict(zip(SWEEP_HOST, want_sweep)), p3d._SWEEP_OUTPUTS, "the balls' own spheres")
    assert (got["object"] != spheres).all() and dev.status() == 0
