"""Overlap queries over device tensors (p3d_overlap_box_device) on the GPU.

The yardstick is exact: host_overlap_box, the brute force on the CPU that test_overlap_reference.py holds to the float64 model.
Under ACCEL_NONE and ACCEL_BVH, on uploaded and device-built trees and through the spill path of a deep tree, at every batch
size, k, list width and flag, the outputs must be the host form's bits - the tree is walked without slack, so this holds for
every box, the degenerate, the inverted and the NaN ones included, which are in every batch beyond the lone lane; an absent
filter is the kernel without filter code; and what every device query promises is device_query_contract.py's.  Every
comparison here has tolerance 0."""
import numpy as np
import pytest

import device_query_contract as dq
from device_query_contract import BATCHES, INVALID, UNSUPPORTED, Input
from frame_checks import gpu
import filter_reference as fr
import intersect_reference as ref
import overlap_reference as ov
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

N = max(BATCHES)
KS = (1, 4, 16)
K_CONTRACT, SKIP_CONTRACT = 3, 2  # (a required row of the shared refusals has at most 12 bytes)
HOST = ("total", "object")


def overlap_box(k, n_skip, ranged=True, solid=False):
    """p3d_overlap_box_device at this k, list width and flag: the list is the first n_skip columns of the world's"""
    def inputs_of(w, n, limited=False):
        i = {"d_lo": w.dev["d_lo"][:n], "d_hi": w.dev["d_hi"][:n]}
        if ranged:
            i["d_skip_range"] = w.dev["d_skip_range"][:n]
        if n_skip:
            i["d_skip"] = w.lists[n_skip][:n]
        return i

    def host_form(hs, w, n, limited):
        total, obj = p3d.host_overlap_box(hs, w.host["d_lo"][:n], w.host["d_hi"][:n], k, skip=w.host["d_skip"][:n, :n_skip] if n_skip else None,
                                          skip_range=w.host["d_skip_range"][:n] if ranged else None, solid=solid)
        return {"total": total, "object": obj} if k else {"total": total}

    return dq.Query(
        "overlap_box_device", (k, "d_lo", "d_hi", "d_skip", n_skip, "d_skip_range", p3d.OVERLAP_SOLID if solid else 0, "d_total", "d_object"),
        (Input("d_lo", 3, True), Input("d_hi", 3, True), Input("d_skip", n_skip, n_skip > 0, "int32"), Input("d_skip_range", 2, False, "int32")),
        p3d._overlap_outputs(k), HOST, HOST[:2 if k else 1], witness="total", refuses_planes=True, inputs_of=inputs_of, host_form=host_form,
        call=lambda dev, accel, i, want, stream, out: p3d.overlap_box_device(
            dev, accel, i["d_lo"], i["d_hi"], k, skip=i.get("d_skip"), skip_range=i.get("d_skip_range"),
            n_skip=n_skip if "d_skip" in i else None, solid=solid, stream=stream, out=out))


def world(path, trees, seed):
    """One scene with N boxes (overlap_reference.scene_boxes: near surfaces, every 16th degenerate, inverted ones and NaNs among
    them) and filters drawn round the unfiltered answers: the list's first columns are the objects each box would list (three
    rows in four), so that a filter changes what is found"""
    w = dq.World(path, trees)
    lo, hi = ov.scene_boxes(ref.load_objects(path), seed, N)
    dead = ~(lo <= hi).all(1)
    assert dead[:63].sum() >= 2 and np.isnan(lo[:63]).any() | np.isnan(hi[:63]).any() and ((lo[:63] == hi[:63]).all(1)).any()
    w.attach(d_lo=lo, d_hi=hi)
    total, listed = p3d.host_overlap_box(w.hs, lo, hi, 16)
    n_objs = int(w.hs.arrays()["n_prims"])
    skip, skip_range = fr.draw(N, n_objs, 8, True, seed + 3, answers=listed)
    w.attach(d_skip=skip, d_skip_range=skip_range)
    w.lists = {s: gpu(np.ascontiguousarray(skip[:, :s])) for s in (1, SKIP_CONTRACT, 8)}  # (a list is contiguous: its first columns are a copy)
    w.n_objs, w.unfiltered, w.dead = n_objs, (total, listed), dead
    return w


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = ov.scene_paths(tmp_path_factory.mktemp("overlap"))
    w = {"mixed": world(paths["boxes"], ("host", "device"), 960), "tri5k": world(tri5k_path, ("device",), 961),
         "planes": world(paths["planes"], ("none",), 962)}
    kinds = {ob["kind"] for ob in ref.load_objects(paths["boxes"])}
    assert kinds == {ov.SPHERE, ov.TRIANGLE, ov.BOX}  # mixed: spheres, triangles and boxes
    dq.assert_deep(w["tri5k"].devs["device"])  # deeper than the stack window: the spill path runs
    return w


@pytest.fixture(scope="module")
def host_answers(worlds):
    """(scene, k, n_skip, ranged, solid) -> the host form's answers for all N rows, computed once"""
    cache = {}

    def get(name, query, key):
        if (name,) + key not in cache:
            cache[(name,) + key] = query.host_form(worlds[name].hs, worlds[name], N, False)
        return cache[(name,) + key]
    return get


@pytest.mark.parametrize("solid", (False, True))
@pytest.mark.parametrize("n_skip", fr.N_SKIPS)
@pytest.mark.parametrize("k", KS)
def test_the_kernel_is_the_host_form(k, n_skip, solid, worlds, host_answers):
    query = overlap_box(k, n_skip, solid=solid)
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        want = host_answers(name, query, (k, n_skip, True, solid))
        for n in BATCHES:
            dq.check_ragged_batches(query, w, n, want, None, "%s, k = %d, n_skip = %d, solid %d" % (name, k, n_skip, solid))
        named = fr.skipped(w.n_objs, N, w.host["d_skip"][:, :n_skip], w.host["d_skip_range"])
        found = want["object"] >= 0
        assert not named[want["object"][found], np.nonzero(found)[0]].any() and found.any(), name + ": a named object is listed"
        assert (want["total"] != w.unfiltered[0]).any(), name + ": the filters changed no answer"
        assert not want["total"][w.dead].any() and (want["object"][w.dead] == -1).all()
        # nothing found, a list cut short by k and one with room left, all in one batch
        assert (want["total"] == 0).any() and ((want["total"] > 0) & (want["total"] <= k)).any() and (k == 16 or (want["total"] > k).any())


@pytest.mark.parametrize("solid", (False, True))
def test_the_count_alone(solid, worlds):
    """k = 0: total and nothing else, no list in LDS; the bits of the host form and of total at k = 16, on every back end"""
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        for n_skip, ranged in ((0, False), (8, True)):
            query = overlap_box(0, n_skip, ranged=ranged, solid=solid)
            want = query.host_form(w.hs, w, N, False)
            wide = overlap_box(16, n_skip, ranged=ranged, solid=solid)
            for tree, dev, accel in w.back_ends():
                for n in BATCHES:
                    got = query.ask(dev, accel, query.inputs_of(w, n))
                    dq.assert_same_bits(got, dq.rows_of(want, n), "%s, %s tree, accel %d, %d rows: the count alone" % (name, tree, accel, n))
                at16 = wide.ask(dev, accel, wide.inputs_of(w, N))
                dq.assert_same_bits(at16["total"], want["total"], "%s, %s tree, accel %d: total at k = 16" % (name, tree, accel))
                assert dev.status() == 0


@pytest.mark.parametrize("k", KS)
def test_an_absent_filter_launches_the_kernel_without_filters(k, worlds, host_answers):
    """n_skip = 0 and no range: the unfiltered kernel, held to the host form as well; filters that name nothing, through the
    filtered kernel, give its bytes; and the tree equals the brute force equals the host form on ALL rows"""
    query = overlap_box(k, 0, ranged=False)
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        want = host_answers(name, query, (k, 0, False, False))
        for n in (BATCHES[0], BATCHES[3], BATCHES[-1]):
            dq.check_ragged_batches(query, w, n, want, None, "%s, k = %d, no filter" % (name, k))
        dq.assert_same_bits(want["total"], w.unfiltered[0], name + ": total does not depend on k")
        for tree, dev, accel in w.back_ends():
            got = query.ask(dev, accel, query.inputs_of(w, N))
            none = p3d.overlap_box_device(dev, accel, w.dev["d_lo"], w.dev["d_hi"], k, skip=gpu(np.full((N, 8), -1, np.int32)),
                                          skip_range=gpu(np.tile(np.array([[w.n_objs, 5]], np.int32), (N, 1))))
            dq.assert_same_bits({key: v.cpu().numpy() for key, v in none.items()}, got, "%s, %s tree, accel %d: filters that name nothing" % (name, tree, accel))
            assert dev.status() == 0


def test_neighbouring_lanes_skip_each_others_answers(worlds):
    """Lane i skips the first object lane i ^ 1 lists without a filter, and nothing else: a filter held in a wave-uniform value,
    or read from the neighbour's row, would show"""
    for name in ("mixed", "tri5k"):
        w = worlds[name]
        n = 4098
        swap = np.arange(n) ^ 1
        first = w.unfiltered[1][:n, 0]
        skip = np.ascontiguousarray(first[swap][:, None].astype(np.int32))
        total, obj = p3d.host_overlap_box(w.hs, w.host["d_lo"][:n], w.host["d_hi"][:n], 4, skip=skip)
        dev = w.devs["device"]
        for accel in w.accels("device"):
            got = p3d.overlap_box_device(dev, accel, w.dev["d_lo"][:n], w.dev["d_hi"][:n], 4, skip=gpu(skip))
            dq.assert_same_bits({key: v.cpu().numpy() for key, v in got.items()}, {"total": total, "object": obj}, "%s, accel %d: swapped lists" % (name, accel))
        differ = (first != first[swap]) & (first >= 0)
        assert differ.sum() > n // 8 and (obj[differ, 0] == first[differ]).all()
        assert dev.status() == 0


def test_the_contract_of_every_device_query(worlds):
    query = overlap_box(K_CONTRACT, SKIP_CONTRACT)
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    outs = dq.check_buffer_refusals(query, dev, query.inputs_of(w, n), n, planes=worlds["planes"])
    dq.check_empty_batch(query, dev)
    # the filter's own refusals, k's and the flags', through the entry point: nothing is enqueued
    every = dict(query.inputs_of(w, n), **{"d_" + name: t for name, t in outs.items()})
    relaid = lambda layout: dq.Query(query.name, layout, query.inputs, query.table, query.order, query.required, query.call)
    at = query.layout.index("d_skip") + 1  # n_skip stands behind its buffer
    assert query.layout[at] == SKIP_CONTRACT
    for rows in (n, 0):
        assert relaid(query.layout[:at] + (9,) + query.layout[at + 1:]).raw(dev, p3d.ACCEL_BVH, rows, **every) == INVALID and b"n_skip must be" in p3d.lib().p3d_last_error()
    assert query.raw(dev, p3d.ACCEL_NONE, n, **dict(every, d_skip=None)) == INVALID and b"d_skip is needed" in p3d.lib().p3d_last_error()
    assert relaid((17,) + query.layout[1:]).raw(dev, p3d.ACCEL_BVH, n, **every) == INVALID and b"k must be" in p3d.lib().p3d_last_error()
    flag = query.layout.index("d_skip_range") + 1
    assert query.layout[flag] == 0
    for bad in (2, 3, 0x100):
        for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
            assert relaid(query.layout[:flag] + (bad,) + query.layout[flag + 1:]).raw(dev, accel, n, **every) == INVALID and b"unknown flag" in p3d.lib().p3d_last_error()
    assert query.raw(dev, p3d.ACCEL_GRID, n, **every) == UNSUPPORTED and b"grid" in p3d.lib().p3d_last_error()
    # a plane under the tree, behind the wrapper's back: a device scene that does not know its host scene's kinds
    planed = p3d.DeviceScene(worlds["planes"].hs, bvh=True)
    assert query.raw(planed, p3d.ACCEL_BVH, n, **every) == UNSUPPORTED and b"plane" in p3d.lib().p3d_last_error()
    count_alone = overlap_box(0, SKIP_CONTRACT)
    assert count_alone.raw(dev, p3d.ACCEL_BVH, n, **dict(every, d_total=None)) == INVALID and b"null argument" in p3d.lib().p3d_last_error()
    dq.assert_untouched(outs)
    assert planed.status() == 0
    whole = query.ask(dev, p3d.ACCEL_BVH, query.inputs_of(w, N))
    dq.check_callers_outputs(query, dev, p3d.ACCEL_BVH, query.inputs_of(w, N), whole, "boxes")
    dq.check_behind_a_refit(query, worlds["tri5k"], N, what="tri5k behind a refit")
    dq.check_behind_a_pose(query, w, N, limits=(False,), what="mixed behind a pose")
    assert dev.status() == 0
