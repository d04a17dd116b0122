"""The k nearest surfaces over device tensors (p3d_nearest_k_device) on the GPU.

The yardstick is exact: HostScene.nearest_k, the brute force on the CPU that test_nearest_k_reference.py holds to the float64
model.  Under ACCEL_NONE and under ACCEL_BVH - uploaded and device-built trees, through the spill path of a deep tree, behind
a refit or a pose enqueued on the same stream - count, object, dist and closest must be its bits at every batch size and k,
with and without limits; at k = 1 the four outputs must be nearest_device's.  Every comparison here has tolerance 0.  What
the query shares with every other device query - stream order, refusals, batches, outputs - is device_query_contract.py's."""
import numpy as np
import pytest
import torch

import device_query_contract as dq
from device_query_contract import BATCHES, INVALID, NEAREST, UNSUPPORTED, nearest_k
from frame_checks import as_bytes, gpu
import intersect_reference as ref
import nearest_k_reference as nk
import nearest_reference as near
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 16)
SEED = {"mixed": 400, "mixed_planes": 401, "planes": 402, "axis_aligned": 403, "tri5k": 404}  # the CPU suite's
TREES = {"mixed": ("host", "device"), "axis_aligned": ("host",), "tri5k": ("device",), "mixed_planes": ("none",), "planes": ("none",)}


class World(dq.World):
    """max(BATCHES) points (the CPU suite's 2 000 first), the model's smallest distances to them (computed once, only to draw
    the limits from), and per k the limits and the host form's answers"""

    def __init__(self, name, path, trees):
        super().__init__(path, trees)
        self.name = name
        objs = ref.load_objects(path)
        self.n_objs = len(objs)
        self.attach(d_point=np.concatenate([near.scene_points(objs, SEED[name]), near.scene_points(objs, SEED[name] + 1000, max(BATCHES) - near.N_POINTS)]))
        self.srt = nk.sorted_table(near.table(objs, self.host["d_point"]), 2 * max(KS))
        self._limits, self._free, self._limited = {}, {}, {}

    def limits(self, k):
        """(host array, device tensor)"""
        if k not in self._limits:
            lim = nk.draw_k_limits(self.srt, k, SEED[self.name] + 50 + k)
            self._limits[k] = (lim, gpu(lim))
        return self._limits[k]

    def free(self, k):
        if k not in self._free:
            self._free[k] = nearest_k(k).host_form(self.hs, self, max(BATCHES), False)
        return self._free[k]

    def limited(self, k):
        if k not in self._limited:
            self._limited[k] = nearest_k(k).host_form(self.hs, self, max(BATCHES), True)
        return self._limited[k]


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest_k")), tri5k=tri5k_path)
    w = {name: World(name, paths[name], TREES[name]) for name in TREES}
    dq.assert_deep(w["tri5k"].devs["device"])
    return w


def assert_shapes(got, k, what):
    n = len(got["count"])
    assert got["count"].dtype == np.int32 and got["count"].shape == (n,) and got["object"].shape == (n, k), what
    assert got["dist"].shape == (n, k) and got["closest"].shape == (n, k, 3) and got["normal"].shape == (n, k, 3), what


def assert_normals(dev, got, what, most=24):
    obj, q, nrm = got["object"], got["closest"], got["normal"]
    for j in np.unique(obj[obj >= 0])[:most]:
        m = obj == j
        assert as_bytes(nrm[m]) == as_bytes(dev.object_normal(int(j), q[m])), "%s: the normal of object %d" % (what, j)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", BATCHES)
def test_the_device_form_is_the_host_form(n, k, worlds):
    query = nearest_k(k)
    for name, w in worlds.items():
        def also(dev, got, limited, what):
            assert_shapes(got, k, what)
            assert_normals(dev, got, what)
            if not limited:
                assert (got["count"] == min(k, w.n_objs)).all()
            elif n >= 63 and w.n_objs >= k:
                assert query.assert_mixed(got, n)

        dq.check_ragged_batches(query, w, n, w.free(k), w.limited(k), "%s, k = %d" % (name, k), also)
        for tree, dev, accel in w.back_ends():
            dq.check_callers_outputs(query, dev, accel, query.inputs_of(w, n, True), dq.rows_of(w.limited(k), n), "%s, %s tree, accel %d, %d points, k = %d" % (name, tree, accel, n, k), optional=("closest",))


def test_k_1_is_nearest_device(worlds):
    w = worlds["tri5k"]
    dev = w.devs["device"]
    n, one_k = max(BATCHES), nearest_k(1)
    lim, d_lim = w.limits(1)
    p = w.host["d_point"]
    host = {False: w.hs.nearest(p), True: w.hs.nearest(p, max_dist=lim)}
    for accel in w.accels("device"):
        for limited in (False, True):
            inputs = one_k.inputs_of(w, n, limited)
            one = NEAREST.ask(dev, accel, inputs)
            got = one_k.ask(dev, accel, inputs)
            what = "accel %d, %s" % (accel, "limits" if limited else "no limit")
            dq.assert_same_bits({name: got[name][:, 0] for name in one}, one, what)
            assert (got["count"] == (one["object"] >= 0)).all()
            assert not limited or 0 < got["count"].sum() < n
            # (nearest_device is the k = 1 launch of the same kernel: the independent statement is the host's k = 1 brute force)
            dq.assert_same_bits({name: got[name][:, 0] for name in ("object", "dist", "closest")}, dict(zip(("object", "dist", "closest"), host[limited])),
                                what + ": HostScene.nearest's bits")
    assert dev.status() == 0


def test_limits_that_keep_nothing_or_everything(worlds):
    n, k = 515, 5
    query = nearest_k(k)
    for name, w in worlds.items():
        d_p = w.dev["d_point"][:n]
        for tree, dev, accel in w.back_ends():
            what = "%s, %s tree, accel %d" % (name, tree, accel)
            for value in (0.0, -2.0, np.nan, -np.inf):
                got = query.ask(dev, accel, {"d_point": d_p, "d_max_dist": gpu(np.full(n, value, np.float32))})
                assert (got["count"] == 0).all() and (got["object"] == -1).all(), "%s: a limit of %g" % (what, value)
                assert_shapes(got, k, what)
                dq.assert_no_answer_values(got, query.table, "%s: a limit of %g" % (what, value))
            dq.assert_answers(query.ask(dev, accel, {"d_point": d_p, "d_max_dist": gpu(np.full(n, np.inf, np.float32))}), w.free(k), query.table, what + ", infinite limits")


def test_an_empty_scene_and_an_empty_batch(tmp_path, worlds):
    path = tmp_path / "empty.p3f"
    path.write_text(ref.HEAD)
    dev = p3d.DeviceScene(p3d.HostScene(str(path)), bvh=False)
    got = nearest_k(3).ask(dev, p3d.ACCEL_NONE, {"d_point": gpu(np.zeros((65, 3), np.float32))})
    assert (got["count"] == 0).all() and (got["object"] == -1).all()
    dq.assert_no_answer_values(got, nearest_k(3).table, "an empty scene")
    dev = worlds["mixed"].devs["host"]
    dq.check_empty_batch(nearest_k(3), dev)  # whatever the pointers, once k is valid
    for accel in (p3d.ACCEL_NONE, p3d.ACCEL_BVH):
        for k in (0, 17):
            assert nearest_k(k).raw(dev, accel, 0) == INVALID and b"k must be" in p3d.lib().p3d_last_error()


def test_refusals_enqueue_nothing(worlds):
    w, (n, k) = worlds["mixed"], (129, 2)
    dev, query = w.devs["host"], nearest_k(k)
    inputs = query.inputs_of(w, n, True)
    outs = dq.check_buffer_refusals(query, dev, inputs, n, planes=worlds["planes"])
    host = np.zeros((n, k * 3), np.float32)
    raws = {name: (v.data_ptr(), n) for name, v in outs.items()}
    q = lambda accel, kk=k, out=outs: nearest_k(kk).call(dev, accel, inputs, query.optional, 0, out)
    dq.assert_refused(
        [("the grid", UNSUPPORTED, "grid", lambda: q(p3d.ACCEL_GRID)),
         ("k = 0", INVALID, "k must be", lambda: q(p3d.ACCEL_BVH, 0, raws)),
         ("k = 17", INVALID, "k must be", lambda: q(p3d.ACCEL_NONE, 17, raws)),
         ("a misaligned count", INVALID, "aligned", lambda: q(p3d.ACCEL_BVH, out=dict(outs, count=(outs["count"].data_ptr() + 2, n))))] +
        [("a host " + name, INVALID, "d_%s is host memory" % name, lambda name=name: q(p3d.ACCEL_BVH, out=dict(outs, **{name: (host.ctypes.data, n)}))) for name in outs])
    # n rows of n k: the sizes are those of this call, not of p3d_nearest_device (the count buffer serves n * 1, not n * k)
    huge = torch.empty((dq.BIG, 3), device="cuda")  # (never read; first, so that it takes the block of this size the check above gave back to torch)
    counts = torch.empty(dq.BIG, dtype=torch.int32, device="cuda")  # (never written: an allocation of its own, of n and not n k elements)
    far = lambda t: (t.data_ptr(), dq.BIG)
    dq.assert_refused([("an object of n, not n k, elements", INVALID, "d_object ends behind its allocation",
                        lambda: query.call(dev, p3d.ACCEL_NONE, {"d_point": far(huge)}, (), 0, {"count": far(counts), "object": far(counts)}))])
    del huge, counts
    dq.assert_untouched(outs)
    assert dev.status() == 0


def test_behind_a_refit_on_the_same_stream(worlds):
    """refit_triangles with moved positions on a side stream, the query behind it on that stream, nothing in between: the
    answers are those of a fresh scene of the moved geometry under ACCEL_NONE, and the host form's after set_geometry."""
    dq.check_behind_a_refit(nearest_k(4), worlds["tri5k"], 4099, what="tri5k behind a refit", before={False: worlds["tri5k"].free(4), True: worlds["tri5k"].limited(4)})


def test_behind_a_pose_on_the_same_stream(worlds):
    dq.check_behind_a_pose(nearest_k(4), worlds["mixed"], 4099, what="mixed behind a pose", before={False: worlds["mixed"].free(4), True: worlds["mixed"].limited(4)})
