"""Nearest surfaces to a segment over device tensors (p3d_nearest_segment_k_device) on the GPU.

The yardstick is exact: host_nearest_segment_k, the brute force on the CPU that test_nearest_segment_reference.py holds to the
float64 model.  Under ACCEL_NONE and ACCEL_BVH, on uploaded and device-built trees and through the spill path of a deep tree, at
every batch size, k and list width, the outputs the host form has must be its bits; the pierce-built and the a == b segments are
in every batch; filters differ from lane to lane and are drawn round the unfiltered answers; an absent filter is the kernel
without filter code; and what every device query promises is device_query_contract.py's.  Every comparison here has tolerance 0."""
import numpy as np
import pytest

import device_query_contract as dq
from device_query_contract import BATCHES, INVALID, UNSUPPORTED, Input
from frame_checks import gpu
import filter_reference as fr
import intersect_reference as ref
import nearest_segment_reference as seg
import p3d_amd as p3d
import sweep_reference as sw

pytestmark = pytest.mark.gpu

N = max(BATCHES)
KS = (1, 4, 16)
K_CONTRACT, SKIP_CONTRACT = 3, 2  # (a required input of the shared refusals has at most 12 bytes per row)
HOST = ("count", "object", "dist", "param", "on_segment", "closest")


def nearest_segment_k(k, n_skip, ranged=True):
    """p3d_nearest_segment_k_device at this k and list width: the list is the first n_skip columns of the world's"""
    def inputs_of(w, n, limited=False):
        i = {"d_a": w.dev["d_a"][:n], "d_b": w.dev["d_b"][:n]}
        if ranged:
            i["d_skip_range"] = w.dev["d_skip_range"][:n]
        if n_skip:
            i["d_skip"] = w.lists[n_skip][:n]
        if limited:
            i["d_max_dist"] = w.dev["d_max_dist"][:n]
        return i

    def host_form(hs, w, n, limited):
        return dict(zip(HOST, p3d.host_nearest_segment_k(
            hs, w.host["d_a"][:n], w.host["d_b"][:n], k, max_dist=w.host["d_max_dist"][:n] if limited else None,
            skip=w.host["d_skip"][:n, :n_skip] if n_skip else None, skip_range=w.host["d_skip_range"][:n] if ranged else None)))

    return dq.Query(
        "nearest_segment_k_device",
        (k, "d_a", "d_b", "d_max_dist", "d_skip", n_skip, "d_skip_range", "d_count", "d_object", "d_dist", "d_param", "d_on_segment", "d_closest", "d_normal"),
        (Input("d_a", 3, True), Input("d_b", 3, True), Input("d_max_dist", None, False), Input("d_skip", n_skip, n_skip > 0, "int32"),
         Input("d_skip_range", 2, False, "int32")),
        p3d._nearest_segment_k_outputs(k), ("count", "object", "dist", "param", "on_segment", "closest", "normal"), ("count", "object"),
        limit="d_max_dist", witness="dist", refuses_planes=True, inputs_of=inputs_of, host_form=host_form,
        call=lambda dev, accel, i, want, stream, out: p3d.nearest_segment_k_device(
            dev, accel, i["d_a"], i["d_b"], k, max_dist=i.get("d_max_dist"), skip=i.get("d_skip"), skip_range=i.get("d_skip_range"),
            n_skip=n_skip if "d_skip" in i else None, want=want, stream=stream, out=out))


def world(path, trees, seed):
    """One scene with N segments (every fifth built to pierce, a == b among the others: nearest_segment_reference.scene_segments),
    limits, and filters drawn round the unfiltered answers: the list's first columns are the objects each segment would find
    (three rows in four), so that a filter changes what is found"""
    w = dq.World(path, trees)
    a, b, pierced = seg.scene_segments(ref.load_objects(path), seed, N)
    assert (pierced[:5] >= 0).any() and (a[:8] == b[:8]).all(1).any()  # both sorts in every batch but the lone lane's
    w.attach(d_a=a, d_b=b)
    count, nearest, dist, _, _, _ = p3d.host_nearest_segment_k(w.hs, a, b, 16)
    rng = np.random.default_rng(seed + 1)
    far = np.where(count > 0, dist[np.arange(N), np.maximum(count - 1, 0)], 1.0)
    lim = (np.where(far > 0, far, 1.0) * rng.choice([0.4, 0.8, 1.5], N)).astype(np.float32)
    lim[0::75], lim[25::75], lim[50::75] = 0.0, -1.5, np.nan
    n_objs = int(w.hs.arrays()["n_prims"])
    skip, skip_range = fr.draw(N, n_objs, 8, True, seed + 3, answers=nearest)
    w.attach(d_max_dist=lim, d_skip=skip, d_skip_range=skip_range)
    w.lists = {s: gpu(np.ascontiguousarray(skip[:, :s])) for s in (1, SKIP_CONTRACT, 8)}  # (a list is contiguous: its first columns are a copy)
    w.n_objs, w.unfiltered, w.pierced = n_objs, nearest, pierced
    return w


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = sw.scene_paths(tmp_path_factory.mktemp("segments"))
    w = {"mixed": world(paths["mixed"], ("host", "device"), 930), "tri5k": world(tri5k_path, ("device",), 931),
         "planes": world(paths["planes"], ("none",), 932)}
    dq.assert_deep(w["tri5k"].devs["device"])  # deeper than the stack window: the spill path runs
    return w


@pytest.fixture(scope="module")
def host_answers(worlds):
    """(scene, k, n_skip, ranged, limited) -> the host form's answers for all N rows, computed once"""
    cache = {}

    def get(name, query, key, limited):
        full = (name,) + key + (limited,)
        if full not in cache:
            cache[full] = query.host_form(worlds[name].hs, worlds[name], N, limited)
        return cache[full]
    return get


@pytest.mark.parametrize("n_skip", fr.N_SKIPS)
@pytest.mark.parametrize("k", KS)
def test_the_kernel_is_the_host_form(k, n_skip, worlds, host_answers):
    query = nearest_segment_k(k, n_skip)
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        free, limited = host_answers(name, query, (k, n_skip, True), False), host_answers(name, query, (k, n_skip, True), True)
        for n in BATCHES:
            dq.check_ragged_batches(query, w, n, free, limited, "%s, k = %d, n_skip = %d" % (name, k, n_skip))
        named = fr.skipped(w.n_objs, N, w.host["d_skip"][:, :n_skip], w.host["d_skip_range"])
        found = free["object"] >= 0
        assert not named[free["object"][found], np.nonzero(found)[0]].any() and found.any()
        assert (free["object"][:, 0] != w.unfiltered[:, 0]).any(), name + ": the filters changed no answer"
        # the limits keep nothing, cut a list short (a list of one cannot be) and leave one whole, all in one batch
        assert (limited["count"] == 0).any() and (k == 1 or ((limited["count"] > 0) & (limited["count"] < free["count"])).any())
        assert ((limited["count"] > 0) & (limited["count"] == free["count"])).any()


@pytest.mark.parametrize("k", KS)
def test_an_absent_filter_launches_the_kernel_without_filters(k, worlds, host_answers):
    """n_skip = 0 and no range: the unfiltered kernel, held to the host form as well; the pierce-built segments are at
    distance exactly 0, and a == b is the point query's answer at a, bit for bit"""
    query = nearest_segment_k(k, 0, ranged=False)
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        free, limited = host_answers(name, query, (k, 0, False), False), host_answers(name, query, (k, 0, False), True)
        for n in (BATCHES[0], BATCHES[3], BATCHES[-1]):
            dq.check_ragged_batches(query, w, n, free, limited, "%s, k = %d, no filter" % (name, k))
        built = w.pierced >= 0
        assert (free["dist"][built, 0] == 0).all() and (free["on_segment"][built, 0] == free["closest"][built, 0]).all()
        point = (w.host["d_a"] == w.host["d_b"]).all(1)
        assert point.sum() > N // 10
        for tree, dev, accel in w.back_ends():
            got = query.ask(dev, accel, query.inputs_of(w, N))
            at = {key: v.cpu().numpy() for key, v in p3d.nearest_k_filtered_device(dev, accel, w.dev["d_a"], k, want=("dist", "closest", "normal")).items()}
            for name_ in ("count", "object", "dist", "closest", "normal"):
                dq.assert_same_bits(got[name_][point], at[name_][point], "%s, %s tree, accel %d: a == b, %s" % (name, tree, accel, name_))
            found = got["object"][point] >= 0
            assert not got["param"][point][found].any() and not np.signbit(got["param"][point][found]).any()
            dq.assert_same_bits(got["on_segment"][point][found], np.broadcast_to(w.host["d_a"][point][:, None, :], got["on_segment"][point].shape)[found], "a == b: on_segment")
            # filters that name nothing, through the filtered kernel: the same bits
            none = p3d.nearest_segment_k_device(dev, accel, w.dev["d_a"], w.dev["d_b"], k, skip=gpu(np.full((N, 8), -1, np.int32)),
                                                skip_range=gpu(np.tile(np.array([[w.n_objs, 5]], np.int32), (N, 1))), want=query.optional)
            dq.assert_same_bits({key: v.cpu().numpy() for key, v in none.items()}, got, "%s, %s tree, accel %d: filters that name nothing" % (name, tree, accel))
            assert dev.status() == 0


def test_neighbouring_lanes_skip_each_others_answers(worlds):
    """Lane i skips what lane i ^ 1 finds without a filter, and nothing else: where the two answers differ, lane i must still find
    its own - a filter held in a wave-uniform value, or read from the neighbour's row, would take it away"""
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        n = 4098
        swap = np.arange(n) ^ 1
        nearest = w.unfiltered[:n, 0]
        skip = np.ascontiguousarray(nearest[swap][:, None].astype(np.int32))
        want = dict(zip(HOST, p3d.host_nearest_segment_k(w.hs, w.host["d_a"][:n], w.host["d_b"][:n], 1, skip=skip)))
        dev = w.devs["device"]
        for accel in w.accels("device"):
            got = p3d.nearest_segment_k_device(dev, accel, w.dev["d_a"][:n], w.dev["d_b"][:n], 1, skip=gpu(skip), want=HOST[2:])
            got = {key: v.cpu().numpy() for key, v in got.items()}
            dq.assert_answers(got, want, p3d._nearest_segment_k_outputs(1), "%s, accel %d: swapped lists" % (name, accel))
            differ = nearest != nearest[swap]
            assert differ.sum() > n // 4 and (got["object"][differ, 0] == nearest[differ]).all() and (got["object"][~differ, 0] != nearest[~differ]).all()
        assert dev.status() == 0


def test_the_contract_of_every_device_query(worlds):
    query = nearest_segment_k(K_CONTRACT, SKIP_CONTRACT)
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    outs = dq.check_buffer_refusals(query, dev, query.inputs_of(w, n, True), n, planes=worlds["planes"])
    dq.check_empty_batch(query, dev)
    # the filter's own refusals and k's, through the entry point: nothing is enqueued
    every = dict(query.inputs_of(w, n), **{"d_" + name: t for name, t in outs.items()})
    at = query.layout.index("d_skip") + 1  # n_skip stands behind its buffer
    assert query.layout[at] == SKIP_CONTRACT
    nine = dq.Query(query.name, query.layout[:at] + (9,) + query.layout[at + 1:], query.inputs, query.table, query.order, query.required, query.call)
    for rows in (n, 0):
        assert nine.raw(dev, p3d.ACCEL_BVH, rows, **every) == INVALID and b"n_skip must be" in p3d.lib().p3d_last_error()
    assert query.raw(dev, p3d.ACCEL_NONE, n, **dict(every, d_skip=None)) == INVALID and b"d_skip is needed" in p3d.lib().p3d_last_error()
    for k in (0, 17):
        bad_k = dq.Query(query.name, (k,) + query.layout[1:], query.inputs, query.table, query.order, query.required, query.call)
        assert bad_k.raw(dev, p3d.ACCEL_BVH, n, **every) == INVALID and b"k must be" in p3d.lib().p3d_last_error()
    assert query.raw(dev, p3d.ACCEL_GRID, n, **every) == UNSUPPORTED and b"grid" in p3d.lib().p3d_last_error()
    dq.assert_untouched(outs)
    whole = query.ask(dev, p3d.ACCEL_BVH, query.inputs_of(w, N, True))
    dq.check_callers_outputs(query, dev, p3d.ACCEL_BVH, query.inputs_of(w, N, True), whole, "segments", optional=("param", "closest"))
    dq.check_behind_a_refit(query, worlds["tri5k"], N, what="tri5k behind a refit")
    dq.check_behind_a_pose(query, w, N, what="mixed behind a pose")
    assert dev.status() == 0


def test_a_scene_with_a_box_is_refused(tmp_path):
    path = tmp_path / "boxed.p3f"
    path.write_text(ref.HEAD + "s 4 0 0 1\nbox -1 3 -1 1 7 2\n")
    hs = p3d.HostScene(str(path))
    dev = p3d.DeviceScene(hs, bvh=True)
    a = gpu(np.zeros((4, 3), np.float32))
    outs = {"count": gpu(np.full(4, 77, np.int32)), "object": gpu(np.full((4, 1), 77, np.int32))}
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        rc = p3d.lib().p3d_nearest_segment_k_device(dev._h, accel, 4, 1, a.data_ptr(), a.data_ptr(), None, None, 0, None, outs["count"].data_ptr(),
                                                    outs["object"].data_ptr(), None, None, None, None, None, None)
        assert rc == UNSUPPORTED and b"is a box" in p3d.lib().p3d_last_error()
        dq.assert_refused([("the wrapper", UNSUPPORTED, "box", lambda: p3d.nearest_segment_k_device(dev, accel, a, a, 1))])
    assert (outs["count"].cpu().numpy() == 77).all() and (outs["object"].cpu().numpy() == 77).all() and dev.status() == 0
