"""The CPU oracle's geometric core against the float64 model of intersect_reference.py, without a GPU: Object::intercepts and
getNormal per kind, closest hits over the three back ends and any-hit over two, on the fixed input sets the GPU suite
(test_gpu_object_queries.py) runs through the kernels.  Ill-conditioned cases (margin under THRESHOLD) are left out and their
share is capped at 5 % in every test; run with -s to see the shares and the measured errors behind intersect_reference.TOL."""
import numpy as np
import pytest

import intersect_reference as ref
from oracle import binding as ob

ACCELS = {"none": 0, "grid": 1, "bvh": 2}


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (oracle scene, the model's objects)"""
    paths = ref.scene_paths(tmp_path_factory.mktemp("intersect"))
    return {name: (ob.Scene(path), ref.load_objects(path)) for name, path in paths.items()}


@pytest.fixture(scope="module")
def objects(scenes):
    return {name: objs for name, (_, objs) in scenes.items()}


def oracle_intercepts(sc, i, o, d):
    out = [sc.object_intercepts(i, o[k], d[k]) for k in range(len(o))]
    return np.array([h for h, _, _ in out]), np.array([t for _, t, _ in out], np.float32), np.stack([dd for _, _, dd in out])


def oracle_normals(sc, i, p):
    return np.stack([sc.object_normal(i, q) for q in p]) if len(p) else np.zeros((0, 3), np.float32)


# ---- the model by itself ----------------------------------------------------------------------------------------------------------

def test_model_sphere_closed_form():
    s = dict(kind=ref.SPHERE, c=np.zeros(3), r=1.0)
    hit, t, margin = ref.intercepts(s, [[-3, 0, 0], [0, 0, 0], [0.5, 0, 0], [3, 0, 0], [-3, 1, 0], [-3, 2, 0]],
                                    [[2, 0, 0], [0, 5, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0], [1, 0, 0]])
    assert hit.tolist() == [True, True, True, False, True, False]
    assert np.allclose(t[[0, 1, 2, 4]], [2, 1, 0.5, 3], rtol=0, atol=1e-7)  # units of d/|d|; inside: the far root; tangent: the foot
    assert margin[4] < ref.THRESHOLD and (margin[[0, 1, 2, 3, 5]] > ref.THRESHOLD).all()
    n, m = ref.normal(s, [[0, 0, 2], [0, 0, 0]])
    assert n[0].tolist() == [0, 0, 1] and m[1] == 0


def test_model_triangle_closed_form():
    tri = dict(kind=ref.TRIANGLE, p0=np.array([0., 0, 0]), p1=np.array([3., 0, 0]), p2=np.array([0., 3, 0]))
    o = [[1, 1, 2], [1, 1, -2], [1, 1, 2], [2.5, 2.5, 2], [0, 0, 2], [1, 1, 5e-5], [1, 1, 1]]
    d = [[0, 0, -4], [0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [0, 0, -1], [1, 0, 0]]
    hit, t, margin = ref.intercepts(tri, o, d)
    assert hit.tolist() == [True, True, False, False, True, False, False]
    assert np.allclose(t[[0, 1, 4]], [0.5, 2, 2], rtol=0, atol=1e-12)  # through the centroid, in units of d; both faces
    assert margin[0] == pytest.approx(1 / 3) and margin[4] == 0 and margin[6] == 0  # a vertex; a ray parallel to the plane
    assert (ref.normal(tri, [[1, 1, 0]])[0] == [0, 0, 1]).all()


def test_model_box_closed_form():
    b = dict(kind=ref.BOX, mn=np.array([-1., -1, -1]), mx=np.array([1., 1, 3]))
    o = [[0, 0, 0], [-3, 0, 0], [-3, 0, 0], [-3, 2, 0], [-3, 1, 0], [0, 0, 5]]
    d = [[0, 0, 2], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, -1]]
    hit, t, margin = ref.intercepts(b, o, d)
    assert hit.tolist()[:4] == [True, True, False, False] and hit[5]
    assert t[[0, 1, 5]].tolist() == [1.5, 2.0, 2.0]  # from inside: the exit, in units of d
    assert margin[4] == 0 and (margin[[0, 1, 2, 3, 5]] > ref.THRESHOLD).all()  # along a face: the zero component decides
    n, m = ref.normal(b, [[1, 0.5, 1.2], [0.2, -1, 1], [0, 0, 3], [0.5, 0.5, 1], [0.5, -0.5, 1.2], [0, 0, 1], [-0.0, 0, 1]])
    # largest |p - centre| component, centre (0, 0, 1); ties: y over x, z over neither; zero counts as positive
    assert n.tolist() == [[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 1, 0], [0, -1, 0], [0, 1, 0], [0, 1, 0]]
    assert (m[3:] == 0).all() and (m[:3] > ref.THRESHOLD).all()


def test_model_plane_closed_form():
    pl = dict(kind=ref.PLANE, p0=np.array([0., 1, 0]), p1=np.array([1., 1, 0]), p2=np.array([0., 1, 1]))
    assert np.allclose(ref.unit_normal(pl), [0, -1, 0])  # (P2-P1) x (P0-P1) = (-1, 0, 1) x (-1, 0, 0)
    hit, t, margin = ref.intercepts(pl, [[0, 3, 0], [0, 3, 0], [0, 3, 0], [0, -1, 0], [0, 1, 0]],
                                    [[0, -2, 0], [0, 1, 0], [1, 0, 0], [1, 1, 0], [0, -1, 0]])
    assert hit.tolist() == [True, False, False, True, False]
    assert t[[0, 3]].tolist() == [1.0, 2.0]
    assert margin[2] == pytest.approx(1e-4) and margin[4] == 0 and margin[0] == 1.0  # parallel; the origin on the plane


def test_model_closest_and_occluded():
    objs = [dict(kind=ref.SPHERE, c=np.array([0., 0, 5]), r=1.0), dict(kind=ref.BOX, mn=np.array([-1., -1, 1]), mx=np.array([1., 1, 2])),
            dict(kind=ref.SPHERE, c=np.array([5., 0, 0]), r=1.0)]
    idx, t, gap, margin = ref.closest(objs, [[0, 0, 0], [0, 0, 0], [0, 0, 0]], [[0, 0, 1], [1, 0, 0], [0, 1, 0]])
    assert idx.tolist() == [1, 2, -1] and t[:2].tolist() == [1.0, 4.0] and gap[0] == 3.0 and np.isinf(gap[1:]).all()
    assert (margin > ref.THRESHOLD).all()
    occ, m = ref.occluded(objs, [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 3]], [[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 0, 1]])
    assert occ.tolist() == [True, False, True, True]  # the last two: along the box's face (a miss), tangent to the sphere (a hit)
    assert (m[:2] > ref.THRESHOLD).all() and m[2] == 0 and m[3] == 0


# ---- the loaders agree on the objects ---------------------------------------------------------------------------------------------

def test_the_models_objects_are_the_oracles(scenes):
    for name, (sc, objs) in scenes.items():
        assert sc.counts()["objects"] == len(objs), name
        for i, m in enumerate(objs):
            o = sc.object(i)
            assert o["type"] == m["kind"], (name, i)
            want = {ref.SPHERE: lambda: np.r_[m["c"], m["r"]], ref.BOX: lambda: np.r_[m["mn"], m["mx"]]}.get(
                m["kind"], lambda: np.r_[m["p0"], m["p1"], m["p2"]])()
            if m["kind"] == ref.PLANE:  # the oracle keeps the normal and the anchor point
                assert (o["v"][3:6] == m["p0"]).all() or (o["v"][:3] == m["p0"]).all(), (name, i)
            else:
                assert (o["v"][:len(want)] == want).all(), (name, i)


def test_oracle_exact_ties_against_the_model(tmp_path):
    """Rays and points whose float32 arithmetic is exact: the model's answer holds at margin 0, so the oracle must give it."""
    path = tmp_path / "edges.p3f"
    path.write_text(ref.EDGES)
    sc = ob.Scene(str(path))
    ref.check_exact(ref.load_objects(str(path)), lambda i, o, d: oracle_intercepts(sc, i, o, d), lambda i, p: oracle_normals(sc, i, p))


# ---- Object::intercepts and getNormal, per kind -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(ref.KINDS), ids=list(ref.KINDS.values()))
def test_oracle_intercepts_against_the_model(kind, scenes, objects):
    cases = ref.kind_cases(objects, kind)
    assert len(cases) >= 3
    worst, left, total = 0.0, 0, 0
    for name, i in cases:
        sc, objs = scenes[name]
        o, d = ref.object_rays(objs[i], ref.case_seed(name, i), ref.RAYS_PER_OBJECT)
        err, out = ref.check_intercepts(objs[i], o, d, *oracle_intercepts(sc, i, o, d), "%s %s[%d]" % (ref.KINDS[kind], name, i))
        worst, left, total = max(worst, err), left + out, total + len(o)
    print("%s: %d of %d rays left out, largest relative t error %.3g" % (ref.KINDS[kind], left, total, worst))


@pytest.mark.parametrize("kind", list(ref.KINDS), ids=list(ref.KINDS.values()))
def test_oracle_normals_against_the_model(kind, scenes, objects):
    worst = 0.0
    for name, i in ref.kind_cases(objects, kind):
        sc, objs = scenes[name]
        p = ref.surface_points(objs[i], *ref.object_rays(objs[i], ref.case_seed(name, i), ref.RAYS_PER_OBJECT))
        if kind == ref.BOX:
            p = np.concatenate([p, ref.box_points(objs[i], ref.case_seed(name, i))])
        assert len(p) >= 40
        err, _ = ref.check_normals(objs[i], p, oracle_normals(sc, i, p), "%s normal %s[%d]" % (ref.KINDS[kind], name, i))
        worst = max(worst, err)
    print("%s: largest normal error %.3g" % (ref.KINDS[kind], worst))


# ---- traversal ------------------------------------------------------------------------------------------------------------------

TRAVERSALS = [(name, accel) for name in ref.NO_PLANES for accel in ACCELS] + [("mixed_planes", "none"), ("planes", "none")]


@pytest.mark.parametrize("name,accel", TRAVERSALS)
def test_oracle_closest_hit_is_the_true_nearest(name, accel, scenes):
    sc, objs = scenes[name]
    o, d = ref.scene_rays(objs, 7)
    hit, t, hp = sc.trace_closest(ACCELS[accel], o, d)
    ref.check_closest(objs, o, d, hit, t, hp, accel, "closest %s over %s" % (name, accel))


@pytest.mark.parametrize("name,accel", [(n, a) for n, a in TRAVERSALS if a != "bvh"])
def test_oracle_any_hit_against_the_model(name, accel, scenes):
    sc, objs = scenes[name]
    o, d = ref.scene_rays(objs, 8)
    ref.check_occluded(objs, o, d, sc.trace_any(ACCELS[accel], o, d), "any hit %s over %s" % (name, accel))
