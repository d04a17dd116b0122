"""HostScene.nearest (p3d_host_scene_nearest: the brute-force statement of the nearest-surface query, on the CPU) against the
float64 model of nearest_reference.py, on the four scenes of intersect_reference.scene_paths and on the triangle mesh; and the
cases whose answer is exact."""
import numpy as np
import pytest

import intersect_reference as ref
import nearest_reference as near
import p3d_amd as p3d

SCENES = ("mixed", "mixed_planes", "planes", "axis_aligned", "tri5k")
SEED = {name: 400 + k for k, name in enumerate(SCENES)}
FLT_MAX = near.FLT_MAX


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    """name -> (host scene, model objects, points, the model's table)"""
    paths = dict(ref.scene_paths(tmp_path_factory.mktemp("nearest")), tri5k=tri5k_path)
    out = {}
    for name in SCENES:
        objs = ref.load_objects(paths[name])
        pts = near.scene_points(objs, SEED[name])
        out[name] = (p3d.HostScene(paths[name]), objs, pts, near.table(objs, pts))
    return out


@pytest.mark.parametrize("name", SCENES)
def test_the_host_form_against_the_model(name, worlds):
    hs, objs, pts, tab = worlds[name]
    assert len(pts) == near.N_POINTS and len(objs) == hs.arrays()["n_prims"]
    got = hs.nearest(pts)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].shape == (len(pts), 3)
    near.check_nearest(objs, pts, got, "nearest, " + name, tab=tab)


@pytest.mark.parametrize("name", SCENES)
def test_limits(name, worlds):
    hs, objs, pts, tab = worlds[name]
    limits = near.draw_limits(tab.min(0), SEED[name] + 50)
    free = hs.nearest(pts)
    got = hs.nearest(pts, max_dist=limits)
    left = near.check_limited(objs, pts, limits, got, free, "nearest with limits, " + name, tab=tab)
    assert left == 0  # by construction no limit lies near the distance it decides
    for k, bad in ((0, 0.0), (25, -1.5), (50, np.nan)):  # a zero, a negative and a NaN limit keep nothing
        assert (got[0][k::75] == -1).all() and (np.isnan(limits[k::75]) if np.isnan(bad) else limits[k::75] == bad).all()
    nothing = hs.nearest(pts[:64], max_dist=np.full(64, np.nan, np.float32))
    assert (nothing[0] == -1).all() and (nothing[1] == FLT_MAX).all() and not nothing[2].any()
    everything = hs.nearest(pts, max_dist=np.full(len(pts), np.inf, np.float32))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(everything, free))


# small dyadic numbers: every operation of the rule is exact on them
EXACT = ref.HEAD + """s 4 0 0 1
p 3
0 0 0
2 0 0
0 2 0
box -1 3 -1 1 7 2
s -8 0 0 1
s -4 0 0 1
p 3
0 0 8
2 0 8
0 2 8
p 3
0 0 8
0 2 8
-2 0 8
"""
SPH, TRI, BOX_, SPH_L, SPH_R, TRI_A, TRI_B = range(7)
EXACT_CASES = [  # (point, object, dist, closest)
    ([4, 0, 0], SPH, 1.0, [5, 0, 0]),           # a sphere's centre: c + (r, 0, 0)
    ([4, 0, 4], SPH, 3.0, [4, 0, 1]),           # outside
    ([4, 0.5, 0], SPH, 0.5, [4, 1, 0]),         # inside: the surface, not the solid
    ([0, 0, 0], TRI, 0.0, [0, 0, 0]),           # on a vertex
    ([2, 0, 0], TRI, 0.0, [2, 0, 0]),
    ([-1, -1, 0], TRI, 1.4142135, [0, 0, 0]),   # the vertex region (sqrtf(2))
    ([1, -1, 0.0], TRI, 1.0, [1, 0, 0]),        # an edge region
    ([0.5, 0.5, 2], TRI, 2.0, [0.5, 0.5, 0]),   # the face
    ([2, 2, 0], TRI, 1.4142135, [1, 1, 0]),     # the hypotenuse
    ([0, 5, 0.5], BOX_, 1.0, [-1, 5, 0.5]),     # a box's centre: x, y and z faces tie at ... x: 1, y: 2, z: 1.5 -> the min x face
    ([0, 5, -0.5], BOX_, 0.5, [0, 5, -1]),      # inside, the z min face is nearest
    ([0.5, 5, 0.5], BOX_, 0.5, [1, 5, 0.5]),    # inside, the x max face
    ([3, 8, 0], BOX_, 2.236068, [1, 7, 0]),     # outside: the clamp (sqrtf(5))
    ([1, 4, 0], BOX_, 0.0, [1, 4, 0]),          # on a face
    ([-6, 0, 0], SPH_L, 1.0, [-7, 0, 0]),       # equidistant from two spheres: the lower index
    ([-1, 1, 9], TRI_B, 1.0, [-1, 1, 8]),
    ([0, 1, 9], TRI_A, 1.0, [0, 1, 8]),         # above the edge two triangles share: the lower index
]


def test_exact_cases(tmp_path):
    path = tmp_path / "exact.p3f"
    path.write_text(EXACT)
    hs = p3d.HostScene(str(path))
    objs = ref.load_objects(str(path))
    assert len(objs) == 7
    p = np.array([c[0] for c in EXACT_CASES], np.float32)
    obj, dist, closest = hs.nearest(p)
    want_obj = np.array([c[1] for c in EXACT_CASES])
    want_dist = np.array([c[2] for c in EXACT_CASES], np.float32)
    want_q = np.array([c[3] for c in EXACT_CASES], np.float32)
    tab = near.table(objs, p)
    assert np.abs(tab.min(0) - want_dist).max() < 1e-7 and np.abs(tab[want_obj, np.arange(len(p))] - tab.min(0)).max() < 1e-12, "the model"
    assert obj.tolist() == want_obj.tolist()
    assert dist.tolist() == want_dist.tolist()
    assert closest.tolist() == want_q.tolist()
    # the ties are ties for the model too
    for k, other in ((14, SPH_R), (16, TRI_B)):
        assert tab[other, k] == tab[want_obj[k], k]
    # a limit is strict: the distance itself keeps nothing, the float above it does
    same = hs.nearest(p, max_dist=want_dist)
    # (the limit is squared in float32: above a distance of 0 the next float's square is 0 again, so those cases get 2^-10)
    above = hs.nearest(p, max_dist=np.where(want_dist > 0, np.nextafter(want_dist, np.float32(np.inf)), np.float32(2.0 ** -10)))
    assert (same[0] == -1).all() and (same[1] == FLT_MAX).all() and not same[2].any()
    assert above[0].tolist() == obj.tolist() and above[1].tobytes() == dist.tobytes() and above[2].tobytes() == closest.tobytes()


def test_an_empty_batch_and_an_empty_scene(tmp_path):
    path = tmp_path / "empty.p3f"
    path.write_text(ref.HEAD)
    hs = p3d.HostScene(str(path))
    obj, dist, closest = hs.nearest(np.zeros((3, 3), np.float32))
    assert obj.tolist() == [-1] * 3 and (dist == FLT_MAX).all() and not closest.any()
    obj, dist, closest = hs.nearest(np.zeros((0, 3), np.float32))
    assert len(obj) == 0 and len(dist) == 0 and closest.shape == (0, 3)
    with pytest.raises(ValueError):
        hs.nearest(np.zeros((3, 3), np.float32), max_dist=np.ones(2, np.float32))
