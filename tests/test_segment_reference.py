"""The segment query's float64 model (segment_reference.py) against the exact brute force over the CPU oracle's per-object test,
without a GPU: any(hit_j and t_j < t_max) over Object::intercepts on a fresh copy of the ray, on the scene rays and seeded
limits the GPU suite (test_gpu_ray_query.py) runs through the kernels.  Ill-conditioned rays (margin under
intersect_reference.THRESHOLD) are left out, and their share is capped at 5 %; run with -s to see the counts."""
import numpy as np
import pytest

import intersect_reference as ref
from oracle import binding as ob
import segment_reference as seg


def test_model_on_a_closed_form_case():
    objs = [dict(kind=ref.SPHERE, c=np.array([0., 0, 5]), r=1.0), dict(kind=ref.BOX, mn=np.array([-1., -1, 1]), mx=np.array([1., 1, 2])),
            dict(kind=ref.TRIANGLE, p0=np.array([4., -1, -1]), p1=np.array([4., 1, -1]), p2=np.array([4., 0, 2]))]
    o = np.zeros((8, 3))
    d = np.array([[0, 0, 1]] * 5 + [[1, 0, 0]] * 2 + [[-np.sqrt(0.5), np.sqrt(0.5), 0]], float)
    t_max = np.array([0.5, 1.0, 1.5, np.inf, np.nan, 4.0, 4.5, np.inf])
    occ, m = seg.occluded_within(objs, o, d, t_max)
    # the box at t = 1, the sphere at 4 behind it; the triangle at t = 4; nothing along (-1, 1, 0)
    assert occ.tolist() == [False, False, True, True, False, False, True, False]
    assert m[1] == 0 and m[4] == 0 and m[5] == 0  # a limit on the hit it decides (strict: free); a NaN limit
    # ray 0 is free and runs parallel to the triangle's plane, but four units from its bounding sphere: a miss whatever the
    # bits; the least sure object left is the sphere behind the limit, 1 / 49 from a tangent
    assert m[0] == pytest.approx(1 / 49)
    assert (m[[2, 3, 6, 7]] > ref.THRESHOLD).all()
    assert m[6] == pytest.approx(0.5 / 4)  # the triangle is hit squarely: the limit, an eighth behind it, is what is nearest
    # without a limit the answer is intersect_reference.occluded's; the margin can only be better: a miss whose bounding sphere
    # the ray's line clearly passes is no longer held against a free ray
    occ_inf, m_inf = seg.occluded_within(objs, o, d, np.full(8, np.inf))
    want, m_want = ref.occluded(objs, o, d)
    assert (occ_inf == want).all() and (m_inf >= m_want).all() and (m_inf[want] == m_want[want]).all()
    # ... and is held against it where the line does meet the sphere: the same triangle in the ray's own plane
    flat = objs[:2] + [dict(kind=ref.TRIANGLE, p0=np.array([0., -1, 0.2]), p1=np.array([0., 1, 0.2]), p2=np.array([0., 0, 0.8]))]
    occ_flat, m_flat = seg.occluded_within(flat, o[:1], d[:1], np.array([0.9]))
    assert not occ_flat[0] and m_flat[0] == 0


def test_tie_limits_are_the_neighbouring_floats():
    t = np.array([1.0, 0.25, 3.0], np.float32)
    same, up, down = seg.tie_limits(t)
    assert (same == t).all() and (up > t).all() and (down < t).all()
    assert (np.nextafter(down, np.float32(np.inf)) == t).all() and (np.nextafter(up, np.float32(-np.inf)) == t).all()


@pytest.mark.parametrize("name", ref.NO_PLANES)
def test_oracle_brute_force_against_the_model(name, tmp_path):
    path = ref.scene_paths(tmp_path)[name]
    sc, objs = ob.Scene(path), ref.load_objects(path)
    o, d = ref.scene_rays(objs, 8)
    t_max = seg.draw_limits(objs, o, d, 18)
    got = seg.brute_force(seg.per_object(sc.object_intercepts, len(objs), o, d), t_max)
    left = seg.check_segment(objs, o, d, t_max, got, "segment any-hit %s, the oracle's brute force" % name)
    # the limits take part: neither the unlimited answer nor "free" is what the model says
    unlimited, _ = ref.occluded(objs, o, d)
    occ, _ = seg.occluded_within(objs, o, d, t_max)
    assert (unlimited & ~occ).sum() > len(o) // 10 and occ.sum() > len(o) // 10
    assert left <= ref.MAX_LEFT_OUT * len(o)
