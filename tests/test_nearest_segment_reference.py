"""host_nearest_segment_k (p3d_host_scene_nearest_segment_k: the brute-force statement of the nearest-surfaces-to-a-segment
query, on the CPU) against the float64 model of nearest_segment_reference.py, on the scenes of sweep_reference.scene_paths (no
boxes; spheres, triangles, planes and their mixtures) and on the triangle mesh; and the three properties of the contract, which
are exact: a == b is the point query, a smaller k is a prefix, a filtered query is the query over the thinned scene."""
import numpy as np
import pytest

import filter_reference as fr
import intersect_reference as ref
import nearest_reference as near
import nearest_segment_reference as seg
import p3d_amd as p3d
import sweep_reference as sw

SCENES = ("spheres", "triangles", "planes", "mixed", "mixed_planes", "tri5k")
SEED = {name: 900 + k for k, name in enumerate(SCENES)}
FLT_MAX = near.FLT_MAX


@pytest.fixture(scope="module")
def worlds(tmp_path_factory, tri5k_path):
    """name -> (host scene, model objects, a, b, pierced)"""
    paths = dict(sw.scene_paths(tmp_path_factory.mktemp("segments")), tri5k=tri5k_path)
    out = {}
    for name in SCENES:
        objs = ref.load_objects(paths[name])
        out[name] = (p3d.HostScene(paths[name]), objs) + seg.scene_segments(objs, SEED[name])
    return out


@pytest.mark.parametrize("name", SCENES)
def test_the_host_form_against_the_model(name, worlds):
    hs, objs, a, b, pierced = worlds[name]
    assert len(a) == seg.N_SEGMENTS and len(objs) == hs.arrays()["n_prims"]
    got = p3d.host_nearest_segment_k(hs, a, b, 1)
    assert got[0].dtype == np.int32 and got[2].dtype == np.float32 and got[4].shape == (len(a), 1, 3)
    seg.check_segments(objs, a, b, pierced, got, "segments, " + name)


@pytest.mark.parametrize("name", ("mixed", "mixed_planes"))
def test_limits(name, worlds):
    hs, objs, a, b, _ = worlds[name]
    d_min, _ = seg.scene_minimum(objs, a, b)
    limits = near.draw_limits(d_min, SEED[name] + 50)
    free = p3d.host_nearest_segment_k(hs, a, b, 1)
    got = p3d.host_nearest_segment_k(hs, a, b, 1, max_dist=limits)
    found, margin = near.decide(d_min, limits)
    assert (margin >= near.THRESHOLD).all()  # by construction no limit lies near the distance it decides
    assert ((got[0] == 1) == found).all() and 0 < found.sum() < len(found)
    hit = got[0] == 1
    assert all(g[hit].tobytes() == f[hit].tobytes() for g, f in zip(got[1:], free[1:])), "a limit changed an answer"
    assert (got[1][~hit] == -1).all() and (got[2][~hit] == FLT_MAX).all() and (got[3][~hit] == FLT_MAX).all()
    assert not got[4][~hit].any() and not got[5][~hit].any()
    for k, bad in ((0, 0.0), (25, -1.5), (50, np.nan)):  # a zero, a negative and a NaN limit keep nothing
        assert (got[0][k::75] == 0).all() and (np.isnan(limits[k::75]) if np.isnan(bad) else limits[k::75] == bad).all()


@pytest.mark.parametrize("name", ("mixed", "mixed_planes", "tri5k"))
def test_a_degenerate_segment_is_the_point_query(name, worlds):
    hs, _, a, _, _ = worlds[name]
    n_objs = int(hs.arrays()["n_prims"])
    skip, skip_range = fr.draw(len(a), n_objs, 8, True, SEED[name] + 1)
    lim = np.full(len(a), np.inf, np.float32)
    lim[::3] = np.float32(0.25 * np.linalg.norm(a.max(0) - a.min(0)))
    for k in (1, 4, 16):
        for filt in (dict(), dict(skip=skip, skip_range=skip_range)):
            want = p3d.host_nearest_k_filtered(hs, a, k, max_dist=lim, **filt)
            count, obj, dist, param, on_segment, closest = p3d.host_nearest_segment_k(hs, a, a.copy(), k, max_dist=lim, **filt)
            for g, w, what in zip((count, obj, dist, closest), want, ("count", "object", "dist", "closest")):
                assert g.tobytes() == w.tobytes() and g.dtype == w.dtype and g.shape == w.shape, "%s, k = %d: %s" % (name, k, what)
            found = obj >= 0
            assert found.any()
            assert param[found].tobytes() == np.zeros(int(found.sum()), np.float32).tobytes()  # +0.0
            assert on_segment[found].tobytes() == np.broadcast_to(a[:, None, :], on_segment.shape)[found].tobytes()


@pytest.mark.parametrize("name", ("mixed", "mixed_planes", "tri5k"))
def test_a_smaller_k_is_a_prefix(name, worlds):
    hs, _, a, b, _ = worlds[name]
    wide = p3d.host_nearest_segment_k(hs, a, b, 16)
    assert (wide[2][:, :-1] <= wide[2][:, 1:]).all()  # ascending; FLT_MAX behind count
    for k in (1, 4):
        got = p3d.host_nearest_segment_k(hs, a, b, k)
        assert got[0].tobytes() == np.minimum(wide[0], k).astype(np.int32).tobytes()
        for g, w in zip(got[1:], wide[1:]):
            assert g.tobytes() == np.ascontiguousarray(w[:, :k]).tobytes()


@pytest.mark.parametrize("name", ("mixed", "tri5k"))
@pytest.mark.parametrize("n_skip", fr.N_SKIPS)
def test_a_filter_is_the_thinned_scene(name, n_skip, worlds):
    """A filtered query equals the unfiltered query over the scene without the named objects: here the unfiltered rows at a k
    wide enough to hold the k smallest survivors, with the listed objects taken out (filter_reference.without)"""
    hs, objs, a, b, _ = worlds[name]
    k = 4
    wide = p3d.host_nearest_segment_k(hs, a, b, 16)
    skip, _ = fr.draw(len(a), len(objs), n_skip, False, SEED[name] + 2, answers=wide[1])
    got = p3d.host_nearest_segment_k(hs, a, b, k, skip=skip)
    want = fr.without((wide[0], wide[1], wide[2], wide[5]), skip, k)
    for g, w, what in zip((got[0], got[1], got[2], got[5]), want, ("count", "object", "dist", "closest")):
        assert g.tobytes() == w.tobytes(), "%s, n_skip = %d: %s" % (name, n_skip, what)
    if n_skip:
        assert (got[1] != wide[1][:, :k]).any(), "the filters changed nothing"
        named = fr.skipped(len(objs), len(a), skip)
        found = got[1] >= 0
        assert not named[got[1][found], np.nonzero(found)[0]].any()
    # a range: against the model of the thinned scene, at the measured tolerance
    _, skip_range = fr.draw(len(a), len(objs), 0, True, SEED[name] + 3)
    ranged = p3d.host_nearest_segment_k(hs, a, b, 1, skip_range=skip_range)
    named = fr.skipped(len(objs), len(a), None, skip_range)
    found = ranged[1][:, 0] >= 0
    assert found.all() and not named[ranged[1][:, 0], np.arange(len(a))].any()
    d_min, _ = seg.scene_minimum(objs, a, b, leave_out=named)
    assert ref.rel_err(ranged[2][:, 0], d_min).max() <= seg.TOL["dist"]


def test_exact_cases(tmp_path):
    """small dyadic numbers: every operation of the rule is exact on them"""
    path = tmp_path / "exact.p3f"
    path.write_text(ref.HEAD + "s 4 0 0 1\np 3\n0 0 0\n2 0 0\n0 2 0\ns -8 0 0 2\n")
    hs = p3d.HostScene(str(path))
    SPH, TRI, BIG = range(3)
    cases = [  # (a, b, object, dist, param, on_segment, closest)
        ([0.5, 0.5, 1], [0.5, 0.5, -1], TRI, 0.0, 0.5, [0.5, 0.5, 0], [0.5, 0.5, 0]),   # pierces the face
        ([0.5, 0.5, 2], [0.5, 0.5, 1], TRI, 1.0, 1.0, [0.5, 0.5, 1], [0.5, 0.5, 0]),    # stops short: the endpoint b
        ([1, -1, 1], [1, -1, -1], TRI, 1.0, 0.5, [1, -1, 0], [1, 0, 0]),                # crossed with the edge A B
        ([4, 0, 3], [4, 0, -3], SPH, 0.0, 0.33333334, [4, 0, 1], [4, 0, 1]),            # enters the shell
        ([4, 0, 0], [4, 0.5, 0], SPH, 0.5, 1.0, [4, 0.5, 0], [4, 1, 0]),                # inside: the endpoint farthest from the centre
        ([4, -0.5, 0], [4, 0.5, 0], SPH, 0.5, 0.0, [4, -0.5, 0], [4, -1, 0]),           # inside, a tie: a
        ([4, -2, 2], [4, 2, 2], SPH, 1.0, 0.5, [4, 0, 2], [4, 0, 1]),                   # outside: the foot of the centre
        ([-8, 0, 1], [-8, 0, 4], BIG, 0.0, 0.33333334, [-8, 0, 2], [-8, 0, 2]),         # leaves the shell
    ]
    a, b = (np.array([c[i] for c in cases], np.float32) for i in (0, 1))
    count, obj, dist, param, on_segment, closest = p3d.host_nearest_segment_k(hs, a, b, 1)
    assert count.tolist() == [1] * len(cases) and obj[:, 0].tolist() == [c[2] for c in cases]
    assert dist[:, 0].tolist() == [c[3] for c in cases]
    assert param[:, 0].tolist() == np.array([c[4] for c in cases], np.float32).tolist()
    assert on_segment[:, 0].tolist() == [c[5] for c in cases] and closest[:, 0].tolist() == [c[6] for c in cases]
    assert not np.signbit(dist).any()
    d, _ = seg.scene_minimum(ref.load_objects(str(path)), a, b)
    assert np.abs(d - [c[3] for c in cases]).max() < 1e-9, "the model"
