"""The per-object query kernels (object_query_kernel<0> / <1>: p3d_object_intercepts, p3d_object_normal) and the traversal
queries on the GPU, against two yardsticks: the CPU oracle bit for bit (every case, crafted edge rays included), and the
float64 model of intersect_reference.py on its well-conditioned cases, with the assertions, tolerances and 5 % cap of the CPU
suite (test_intersect_reference.py) on the same inputs.  Scenes whose BVH and grid were built on the device have no oracle
with the same tree: there the model is the only yardstick for closest hits."""
import ctypes as C

import numpy as np
import pytest

from frame_checks import ACCELS, same_bits_or_nan
import intersect_reference as ref
from oracle import binding as ob
import p3d_amd as p3d

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(123.0)
BATCHES = [1, 63, 64, 65, 129, 4099]  # kBlock is 64: a lone lane, a full wave, one lane over, a ragged last block of many

TRI, SPH, BOX_, FLAT, PLANE_, BOX0 = ref.TRI, ref.SPH, ref.BOX_, ref.FLAT, ref.PLANE_, ref.BOX0


class World:
    def __init__(self, path):
        self.hs = p3d.HostScene(path)
        self.sc = ob.Scene(path)
        self.objs = ref.load_objects(path)
        self.dev = p3d.DeviceScene(self.hs, bvh=True, grid=True)


@pytest.fixture(scope="module")
def worlds(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("queries")
    paths = ref.scene_paths(tmp)
    edges = tmp / "edges.p3f"
    edges.write_text(ref.EDGES)
    paths["edges"] = str(edges)
    return {name: World(path) for name, path in paths.items()}


@pytest.fixture(scope="module")
def objects(worlds):
    return {name: w.objs for name, w in worlds.items() if name != "edges"}


def oracle_answers(sc, i, o, d):
    """-> (hit, t, direction out, normal at the point o + t d of a hit or at the origin of a miss, those points)"""
    out = [sc.object_intercepts(i, o[k], d[k]) for k in range(len(o))]
    hit = np.array([h for h, _, _ in out], bool)
    t = np.array([tt for _, tt, _ in out], np.float32)
    d_out = np.stack([dd for _, _, dd in out]).astype(np.float32)
    with np.errstate(all="ignore"):
        p = np.where(hit[:, None], o + t[:, None] * d_out, o).astype(np.float32)
    nrm = np.stack([sc.object_normal(i, q) for q in p])
    return hit, t, d_out, nrm, p


def assert_equals_oracle(dev, i, o, d, want, what):
    hit, t, d_out, nrm, p = want
    g_hit, g_t, g_d = dev.object_intercepts(i, o, d, t_init=SENTINEL)
    assert (g_hit == hit).all(), "%s: %d decisions differ from the oracle's" % (what, int((g_hit != hit).sum()))
    assert same_bits_or_nan(g_t[hit], t[hit]).all(), what + ": t differs in some bit"
    assert (g_t[~hit].view(np.uint32) == SENTINEL.view(np.uint32)).all(), what + ": t was written on a miss"
    assert same_bits_or_nan(g_d, d_out).all(), what + ": the direction out differs in some bit"
    assert same_bits_or_nan(dev.object_normal(i, p), nrm).all(), what + ": a normal differs in some bit"
    return g_hit, g_t, g_d


# ---- per-object kernels against the oracle, bit for bit ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def per_kind(worlds, objects):
    """kind -> (world, object, origins, directions, the oracle's answers) for max(BATCHES) rays in a fixed shuffled order, so
    that every prefix holds aimed and random rays, hits and misses"""
    out = {}
    for kind in ref.KINDS:
        name, i = ref.kind_cases(objects, kind)[0]
        w = worlds[name]
        o, d = ref.object_rays(w.objs[i], 50 + kind, max(BATCHES))
        order = np.random.default_rng(60 + kind).permutation(len(o))
        o, d = np.ascontiguousarray(o[order]), np.ascontiguousarray(d[order])
        out[kind] = (w, i, o, d, oracle_answers(w.sc, i, o, d))
    return out


@pytest.mark.parametrize("n", BATCHES)
@pytest.mark.parametrize("kind", list(ref.KINDS), ids=list(ref.KINDS.values()))
def test_object_kernels_equal_the_oracle(kind, n, per_kind):
    w, i, o, d, want = per_kind[kind]
    hit = want[0]
    if n >= 63:
        assert 0 < hit[:n].sum() < n  # hits and misses in one batch
    assert_equals_oracle(w.dev, i, o[:n], d[:n], tuple(a[:n] for a in want), "%s, %d rays" % (ref.KINDS[kind], n))


# ---- crafted edges ----------------------------------------------------------------------------------------------------------------

def _f(x):
    return np.float32(x)


T4 = _f(1e-4)  # the float just below 1e-4
UP, DOWN = _f(np.inf), _f(-np.inf)

EDGE_RAYS = {
    "triangle": (TRI, [
        ([-1, 0.5, 0], [1, 0, 0]),                       # in the triangle's plane: denominator 0, NaN t reported as a hit (A10)
        ([-1, 0, 0], [1, 0, 0]),                         # in the plane along an edge
        ([0, 0, 1], [0, 0, -1]), ([2, 0, 1], [0, 0, -1]), ([0, 2, 1], [0, 0, -2]),   # through the vertices
        ([1, 0, 1], [0, 0, -1]), ([1, 1, 1], [0, 0, -1]), ([0, 1, -1], [0, 0, 1]),   # through points of the edges
        ([0.5, 0.5, T4], [0, 0, -1]), ([0.5, 0.5, np.nextafter(T4, UP)], [0, 0, -1]),  # t either side of 1e-4
        ([0.5, 0.5, np.nextafter(T4, DOWN)], [0, 0, -1]), ([0.5, 0.5, 2e-4], [0, 0, -1]), ([0.5, 0.5, -1e-4], [0, 0, 1]),
        ([0.5, 0.5, 1], [0, 0, -1]), ([0.5, 0.5, 1], [0, 0, 1]), ([3, 3, 1], [0, 0, -1]),  # a plain hit, behind, beside
    ]),
    "sphere": (SPH, [
        ([4, 1, -3], [0, 0, 1]), ([4, -1, 3], [0, 0, -2]),   # tangent
        ([5, 0, 0], [1, 0, 0]), ([5, 0, 0], [-1, 0, 0]), ([5, 0, 0], [0, 1, 0]),  # the origin on the surface (c = 0)
        ([4, 0, 0], [0, 1, 0]), ([4, 0, 0], [1, 2, 3]),      # the origin at the centre
        ([0, 0, 0], [0, 0, 0]), ([4, 0, 0], [0, 0, 0]),      # no direction: normalising gives NaN
        ([0, 0, 0], [1, 0, 0]), ([0, 0, 0], [-1, 0, 0]), ([4.5, 0, 0], [3, 0, 0]),  # plain: a hit, behind, from inside
    ]),
    "box": (BOX_, [
        ([0, 4, 0], [1, 0, 0]), ([0, 4, 0], [0.3, 0.4, -0.5]),                    # from inside
        ([1, 4, 0], [1, 0, 0]), ([1, 4, 0], [-1, 0, 0]), ([1, 4, 0], [0, 1, 0]),   # the origin on a face: out, in, along
        ([1, 5, 0], [0, 0, 1]), ([1, 5, 0], [-1, -1, 0]), ([1, 5, 0], [1, 1, 0]),  # the origin on an edge
        ([1, 2, -0.5], [0, 1, 0.1]), ([1, 2, 0], [0, 1, 0]), ([1, 4, 0], [0, 0, 0]), ([0, 4, 0], [0, 0, 0]),  # along a face: 1, 2, 3 zero components
        ([1, 5, -3], [0, 0, 1]), ([0, 2, 0], [0, 1, 0]), ([0, 2, 0], [0, -1, 0]), ([0, 4, 0], [-0.0, 1, 0]),  # along an edge; plain
    ] + [([0, 4, 0], [_f(1e4) + _f(k) * _f(0.0009765625), 0, 0]) for k in range(-8, 9)]),  # t1 = 1 / d.x at 1e-4 and the floats around it
    "flat box": (FLAT, [
        ([0, -4, 2], [0, 0, -1]), ([0, -4, 2], [0.1, 0, -1]), ([0, -4, 0.5], [1, 0, 0]), ([-3, -4, 0.5], [1, 0, 0]), ([0, -4, 0.5], [0, 0, 1]),
    ]),
    "plane": (PLANE_, [
        ([0, 0, 0], [1, -T4, 0]), ([0, 0, 0], [1, -np.nextafter(T4, DOWN), 0]), ([0, 0, 0], [1, -np.nextafter(T4, UP), 0]),  # |N.d| at 1e-4
        ([0, 0, 0], [1, T4, 0]), ([0, 0, 0], [1, 0, 0]),
        ([3, -8, 2], [0, -1, 0]), ([3, -8, 2], [0, 1, 0]), ([3, -8, 2], [1, 0, 0]),   # the origin on the plane
        ([0, -9, 0], [0, -1, 0]), ([0, -9, 0], [0, 1, 0]), ([0, 0, 0], [0, -2, 0]),   # behind it: away, through; in front
    ]),
}
EDGE_POINTS = {
    "box": (BOX_, [[0, 4, 0], [0.5, 4.5, 0.2], [0.5, 4.1, 0.5], [0.5, 4.5, 0.5], [-0.5, 3.5, -0.5], [-0.5, 4.5, 0.5], [-0.0, 4, 0],
                   [0.25, 4, -0.25], [1, 5, 1], [1, 4.25, 0.5], [0, 4, -1]]),  # the centre; ties x=y, z=x, all three; a zero among them
    "box at the origin": (BOX0, [[0, -0.0, 10], [-0.0, -0.0, 10], [0, 0, 10], [-0.0, 0.5, 10], [0.5, -0.0, 10.5], [0, -0.0, 9]]),  # -0.0 counts as positive
    "flat box": (FLAT, [[0, -4, 0.5], [0.5, -4, 0.5], [0, -4, 1]]),
}


@pytest.mark.parametrize("case", list(EDGE_RAYS))
def test_crafted_edge_rays(case, worlds):
    w = worlds["edges"]
    i, rays = EDGE_RAYS[case]
    o = np.array([r[0] for r in rays], np.float32)
    d = np.array([r[1] for r in rays], np.float32)
    want = oracle_answers(w.sc, i, o, d)
    g_hit, g_t, _ = assert_equals_oracle(w.dev, i, o, d, want, case)
    assert 0 < g_hit.sum() < len(o) or case == "flat box"
    if case == "triangle":
        assert g_hit[0] and np.isnan(g_t[0])  # A10
        assert not g_hit[8] and g_hit[9]      # 0.0001f is under the double 1e-4, the next float is over it
    if case == "box":
        assert len(set(g_hit[-17:].tolist())) == 2  # t1 on both sides of 1e-4
    # ... and the model where it is sure of itself
    hit, t, margin = ref.intercepts(w.objs[i], o, d)
    ok = margin >= ref.THRESHOLD
    assert (ok.any() or case == "flat box") and (g_hit[ok] == hit[ok]).all(), case  # (no ray is well-conditioned against a flat box)
    both = ok & hit
    if both.any():
        assert ref.rel_err(g_t[both], t[both]).max() <= ref.TOL["t_" + ref.KINDS[w.objs[i]["kind"]]], case


def test_exact_ties_against_the_model(worlds):
    """The crafted cases whose float32 arithmetic is exact: the model's answer holds at margin 0 too."""
    w = worlds["edges"]
    ref.check_exact(w.objs, w.dev.object_intercepts, w.dev.object_normal)


@pytest.mark.parametrize("case", list(EDGE_POINTS))
def test_crafted_box_normal_points(case, worlds):
    w = worlds["edges"]
    i, pts = EDGE_POINTS[case]
    p = np.array(pts, np.float32)
    got = w.dev.object_normal(i, p)
    want = np.stack([w.sc.object_normal(i, q) for q in p])
    assert same_bits_or_nan(got, want).all(), case
    model, margin = ref.normal(w.objs[i], p)
    ok = margin >= ref.THRESHOLD
    assert (got[ok] == model[ok]).all(), case
    if case == "box":
        assert got[0].tolist() == [0, 1, 0] and got[3].tolist() == [0, 1, 0]  # all equal: y; never x on a tie, z only on a strict >
    if case == "box at the origin":
        assert (got[:3] == [0, 1, 0]).all()  # a component of -0.0 is >= 0


# ---- against the float64 model ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(ref.KINDS), ids=list(ref.KINDS.values()))
def test_gpu_intercepts_and_normals_against_the_model(kind, worlds, objects):
    for name, i in ref.kind_cases(objects, kind):
        w = worlds[name]
        m = w.objs[i]
        o, d = ref.object_rays(m, ref.case_seed(name, i), ref.RAYS_PER_OBJECT)
        what = "%s %s[%d]" % (ref.KINDS[kind], name, i)
        ref.check_intercepts(m, o, d, *w.dev.object_intercepts(i, o, d), what)
        p = ref.surface_points(m, o, d)
        if kind == ref.BOX:
            p = np.concatenate([p, ref.box_points(m, ref.case_seed(name, i))])
        ref.check_normals(m, p, w.dev.object_normal(i, p), what + " normal")


TRAVERSALS = [(name, accel) for name in ref.NO_PLANES for accel in ACCELS] + [("mixed_planes", "none"), ("planes", "none")]


def gpu_closest(dev, accel, objs, o, d, what):
    hit, hp, t = dev.trace_closest(ACCELS[accel], o, d, want_t=True)
    ref.check_closest(objs, o, d, hit, t, hp, accel, what)


@pytest.mark.parametrize("name,accel", TRAVERSALS)
def test_gpu_closest_hit_is_the_true_nearest(name, accel, worlds):
    w = worlds[name]
    o, d = ref.scene_rays(w.objs, 7)
    gpu_closest(w.dev, accel, w.objs, o, d, "closest %s over %s" % (name, accel))


@pytest.mark.parametrize("name,accel", [(n, a) for n, a in TRAVERSALS if a != "bvh"])
def test_gpu_any_hit_against_the_model(name, accel, worlds):
    w = worlds[name]
    o, d = ref.scene_rays(w.objs, 8)
    ref.check_occluded(w.objs, o, d, w.dev.trace_any(ACCELS[accel], o, d), "any hit %s over %s" % (name, accel))


@pytest.mark.parametrize("name", ref.NO_PLANES)
def test_closest_hits_on_a_scene_built_on_the_device(name, worlds):
    """A linear BVH and a grid built on the GPU: no oracle has the same tree, the model says what the nearest hit is."""
    w = worlds[name]
    dev = p3d.DeviceScene(w.hs, bvh="device", grid="device")
    o, d = ref.scene_rays(w.objs, 7)
    for accel in ("bvh", "grid"):
        gpu_closest(dev, accel, w.objs, o, d, "closest %s over a device-built %s" % (name, accel))
    ref.check_occluded(w.objs, o, d, dev.trace_any(p3d.ACCEL_GRID, o, d), "any hit %s over a device-built grid" % name)
    # ... and the per-object queries answer there as on an uploaded scene
    i = 0
    a = w.dev.object_intercepts(i, o[:129], d[:129], t_init=SENTINEL)
    b = dev.object_intercepts(i, o[:129], d[:129], t_init=SENTINEL)
    assert all(same_bits_or_nan(x.astype(np.float32), y.astype(np.float32)).all() for x, y in zip(a, b))


# ---- the contract of the calls ----------------------------------------------------------------------------------------------------

def _raw_intercepts(dev, obj, n, o, d, hit, t):
    return p3d.lib().p3d_object_intercepts(dev._h, int(obj), int(n), C.c_void_p(o.ctypes.data), C.c_void_p(d.ctypes.data),
                                           C.c_void_p(hit.ctypes.data), C.c_void_p(t.ctypes.data))


def _filled(n=8):
    return (np.full((n, 3), 0.5, np.float32), np.full((n, 3), 7.0, np.float32), np.full(n, 9, np.uint8), np.full(n, SENTINEL, np.float32))


def test_an_object_out_of_range_is_refused_and_nothing_is_written(worlds):
    w = worlds["mixed"]
    n_objs = len(w.objs)
    for obj in (n_objs, n_objs + 1, 0xffffffff):
        o, d, hit, t = _filled()
        assert _raw_intercepts(w.dev, obj, len(o), o, d, hit, t) == -1  # P3D_ERR_INVALID
        assert (d == 7.0).all() and (hit == 9).all() and (t == SENTINEL).all()
        nrm = np.full((8, 3), 7.0, np.float32)
        assert p3d.lib().p3d_object_normal(w.dev._h, obj, 8, C.c_void_p(o.ctypes.data), C.c_void_p(nrm.ctypes.data)) == -1
        assert (nrm == 7.0).all()
    with pytest.raises(p3d.P3DError) as e:
        w.dev.object_normal(n_objs, np.zeros((1, 3), np.float32))
    assert e.value.code == -1


def test_an_empty_batch_is_ok_and_leaves_the_arrays(worlds):
    w = worlds["mixed"]
    o, d, hit, t = _filled()
    assert _raw_intercepts(w.dev, 0, 0, o, d, hit, t) == 0
    assert (d == 7.0).all() and (hit == 9).all() and (t == SENTINEL).all()
    nrm = np.full((8, 3), 7.0, np.float32)
    assert p3d.lib().p3d_object_normal(w.dev._h, 0, 0, C.c_void_p(o.ctypes.data), C.c_void_p(nrm.ctypes.data)) == 0
    assert (nrm == 7.0).all()


def test_skybox_colour_without_a_cubemap_is_refused(worlds):
    with pytest.raises(p3d.P3DError) as e:
        worlds["mixed"].dev.skybox_color(np.array([[0, 0, 1]], np.float32))
    assert e.value.code == -1


def test_queries_right_after_a_frame_with_a_tail_stream(worlds):
    """p3d_trace_* join the scene's tail stream themselves; the per-object queries do not, and need not: they write only
    their own staging buffers.  Both return, with a literal frame's hand-off still on the tail stream, what they returned before it."""
    import torch
    w = worlds["mixed"]
    dev = w.dev
    i = [m["kind"] for m in w.objs].index(ref.SPHERE)
    o, d = ref.object_rays(w.objs[i], 5, 4099)
    so, sd = ref.scene_rays(w.objs, 9)
    before = dev.object_intercepts(i, o, d, t_init=SENTINEL) + (dev.object_normal(i, o),) + dev.trace_closest(p3d.ACCEL_BVH, so, sd, want_t=True)
    tile = dev.full_tile()
    n = tile.w * tile.h
    buf = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    tail = torch.cuda.Stream()
    cfg = p3d.whitted_config(accel=p3d.ACCEL_BVH, max_depth=4)
    dev.set_tail_stream(tail)
    try:
        dev.render_device(cfg, tile, d_rgb=buf.data_ptr(), d_hit=buf.data_ptr() + n * 12, stream=torch.cuda.current_stream().cuda_stream)
        after = dev.object_intercepts(i, o, d, t_init=SENTINEL) + (dev.object_normal(i, o),)
        after += dev.trace_closest(p3d.ACCEL_BVH, so, sd, want_t=True)
        dev.join(host_wait=True)
        assert dev.status() == 0, p3d.lib().p3d_last_error().decode()
    finally:
        dev.set_tail_stream(None)
    for a, b in zip(before, after):
        assert same_bits_or_nan(a.astype(np.float32), b.astype(np.float32)).all()
    rgb, hit, _ = dev.render(cfg)  # and the frame was not disturbed by the queries
    host = buf.cpu().numpy()
    assert (host[n * 12:].view(np.int32).reshape(tile.h, tile.w) == hit).all()
    assert same_bits_or_nan(host[: n * 12].view(np.float32).reshape(tile.h, tile.w, 3), rgb).all()
