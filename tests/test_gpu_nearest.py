"""Nearest-surface queries over device tensors (p3d_nearest_device) on the GPU.

The yardstick is exact: HostScene.nearest, the brute force on the CPU that test_nearest_reference.py holds to the float64
model.  Under ACCEL_NONE object, dist and closest must be its bits at every batch size, with and without limits; under
ACCEL_BVH they must be the ACCEL_NONE bits, on uploaded and on device-built trees, through the spill path of a deep tree, and
behind a refit or a pose enqueued on the same stream.  Every comparison here has tolerance 0.  What the query shares with
every other device query - stream order, refusals, batches, outputs - is device_query_contract.py's.

The library's debug hooks expose no scratch sizes, so "a second call of the same n allocates nothing" is not tested here."""
import numpy as np
import pytest

import device_query_contract as dq
from device_query_contract import BATCHES, NEAREST, UNSUPPORTED
from frame_checks import as_bytes, gpu
import intersect_reference as ref
import nearest_reference as near
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

SEED = {"mixed": 400, "mixed_planes": 401, "planes": 402, "axis_aligned": 403, "tri5k": 404}  # the CPU suite's


def world(name, path, trees):
    """max(BATCHES) points (the CPU suite's 2 000 first), their limits (drawn from the host form's distances as the CPU suite
    draws them from the model's), and the host form's answers"""
    w = dq.World(path, trees)
    objs = ref.load_objects(path)
    p = np.concatenate([near.scene_points(objs, SEED[name]), near.scene_points(objs, SEED[name] + 1000, max(BATCHES) - near.N_POINTS)])
    w.attach(d_point=p)
    w.free = NEAREST.host_form(w.hs, w, len(p), False)
    w.attach(d_max_dist=near.draw_limits(w.free["dist"].astype(np.float64), SEED[name] + 50))
    w.limited = NEAREST.host_form(w.hs, w, len(p), True)
    return w


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest")), tri5k=tri5k_path)
    trees = {"mixed": ("host", "device"), "axis_aligned": ("host",), "tri5k": ("device",), "mixed_planes": ("none",), "planes": ("none",)}
    w = {name: world(name, paths[name], trees[name]) for name in trees}
    dq.assert_deep(w["tri5k"].devs["device"])
    return w


def ask(dev, accel, d_p, d_limits=None):
    return NEAREST.ask(dev, accel, {"d_point": d_p, "d_max_dist": d_limits})


def assert_normals(dev, got, what, most=24):
    obj, q, nrm = got["object"], got["closest"], got["normal"]
    for j in np.unique(obj[obj >= 0])[:most]:
        m = obj == j
        assert as_bytes(nrm[m]) == as_bytes(dev.object_normal(int(j), q[m])), "%s: the normal of object %d" % (what, j)


@pytest.mark.parametrize("n", BATCHES)
def test_the_device_form_is_the_host_form(n, worlds):
    def also(dev, got, limited, what):
        assert_normals(dev, got, what)
        if not limited:
            assert (got["object"] >= 0).all()
        elif n >= 63:
            assert NEAREST.assert_mixed(got, n), what + ": found and not found in one batch"

    for name, w in worlds.items():
        dq.check_ragged_batches(NEAREST, w, n, w.free, w.limited, name, also)
        for tree, dev, accel in w.back_ends():
            dq.check_callers_outputs(NEAREST, dev, accel, NEAREST.inputs_of(w, n, True), dq.rows_of(w.limited, n), "%s, %s tree, accel %d, %d points" % (name, tree, accel, n), optional=("closest",))


def test_limits_that_keep_nothing_or_everything(worlds):
    for name, w in worlds.items():
        n = 515
        d_p = w.dev["d_point"][:n]
        for tree, dev, accel in w.back_ends():
            what = "%s, %s tree, accel %d" % (name, tree, accel)
            for value in (0.0, -2.0, np.nan, -np.inf):
                got = ask(dev, accel, d_p, gpu(np.full(n, value, np.float32)))
                assert (got["object"] == -1).all(), "%s: a limit of %g" % (what, value)
                dq.assert_no_answer_values(got, NEAREST.table, "%s: a limit of %g" % (what, value))
            dq.assert_answers(ask(dev, accel, d_p, gpu(np.full(n, np.inf, np.float32))), w.free, NEAREST.table, what + ", infinite limits")
            # the limit at the distance itself (d2 against the float32 square of sqrtf(d2): the host form says which way), and twice it
            d = w.free["dist"][:n]
            same = dict(zip(("object", "dist", "closest"), w.hs.nearest(w.host["d_point"][:n], max_dist=d)))
            dq.assert_answers(ask(dev, accel, d_p, gpu(d)), same, NEAREST.table, what + ", the distance as the limit")
            dq.assert_answers(ask(dev, accel, d_p, gpu(np.where(d > 0, 2 * d, np.float32(1e-3)))), w.free, NEAREST.table, what + ", twice the distance as the limit")


def test_an_empty_scene_and_an_empty_batch(tmp_path, worlds):
    path = tmp_path / "empty.p3f"
    path.write_text(ref.HEAD)
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh=False)
    got = ask(dev, p3d.ACCEL_NONE, gpu(np.zeros((65, 3), np.float32)))
    assert (got["object"] == -1).all()
    dq.assert_no_answer_values(got, NEAREST.table, "an empty scene")
    dq.check_empty_batch(NEAREST, worlds["mixed"].devs["host"])


def test_refusals_enqueue_nothing(worlds):
    w, n = worlds["mixed"], 129
    dev = w.devs["host"]
    outs = dq.check_buffer_refusals(NEAREST, dev, NEAREST.inputs_of(w, n, True), n, planes=worlds["planes"])
    dq.assert_refused([("the grid", UNSUPPORTED, "grid", lambda: NEAREST.call(dev, p3d.ACCEL_GRID, NEAREST.inputs_of(w, n), NEAREST.optional, 0, outs))])
    dq.assert_untouched(outs)
    assert dev.status() == 0


def test_behind_a_refit_on_the_same_stream(worlds):
    """refit_triangles with moved positions on a side stream, the query behind it on that stream, nothing in between: the
    answers are those of a fresh scene of the moved geometry under ACCEL_NONE, and the host form's after set_geometry."""
    dq.check_behind_a_refit(NEAREST, worlds["tri5k"], 4099, what="tri5k behind a refit", before={False: worlds["tri5k"].free, True: worlds["tri5k"].limited})


def test_behind_a_pose_on_the_same_stream(worlds):
    dq.check_behind_a_pose(NEAREST, worlds["mixed"], 4099, what="mixed behind a pose", before={False: worlds["mixed"].free, True: worlds["mixed"].limited})
